"""spectrogram() (R/spectrogram.R:94-276): the numpy restatement pinned by hand,
sg_spectrogram_size against it, and the GPU (sg_spectrogram.hip) against it.

No R is installed: soundgen_beta_amd/spectrogram.py restates the reference
statement by statement with line citations, the CPU tests below pin its parts on
cases worked by hand, and the GPU tests compare the device with it.

Bars. 'processed' lies in [0, 1] and is compared absolutely; 'original' relative
to the matrix maximum. The project's bar for an fp64 path is 1e-9
(tests/test_matchpars.py); the bars held here are 10x the maxima measured on an
MI355X over every case of their class (TOL_PLAIN / TOL_QTIME below), both under 1e-9.

Measured maxima (MI355X): 'original' 3.5e-16 of the matrix maximum; plain
'processed' cases 8.9e-12 (44.1 kHz, contrast = 1; defaults 5.2e-14 / 1.2e-13 /
1.5e-12 at the three rates, the seven windows <= 1.2e-13, zp = 1024 and 4096
2.7e-14, 64 bins 8.7e-14, the scale() branch 7.2e-13, the rolling-median edges <= 1.6e-13); qTime cases 1.22e-11
(44.1 kHz, every pass on; qTime = .5 alone 1.1e-12 / 1.3e-12 / 1.1e-11).
spectrogram_batch equals spectrogram() bit for bit on all 22 non-empty calls of 24.
"""
import math
import os
from functools import lru_cache

import numpy as np
import pytest

from soundgen_beta_amd import spectrogram as SP

# Measured on an MI355X (max over the cases of the class): plain cases MEASURED_PLAIN,
# qTime cases MEASURED_QTIME (their smallest x - q sets the log floor, so their
# error scales with 1 / (the smallest relative gap), >= 1e-6 here).
MEASURED_PLAIN = 8.9e-12  # 44.1 kHz, contrast = 1 (the power e^3 multiplies the logs' round-off)
MEASURED_QTIME = 1.22e-11  # 44.1 kHz, every pass on
TOL_PLAIN = 10 * MEASURED_PLAIN
TOL_QTIME = 10 * MEASURED_QTIME

RATES = (16000, 22050, 44100)  # M = 400, 551 (odd: 19 x 29), 1102 (fft64's specialised branch)
SEEDS = {16000: 5, 22050: 4, 44100: 4}  # keep the conditioning margins below


# ------------------------------------------------------------ CPU: parts by hand
def test_roll_median_by_hand():
    x = np.array([5.0, 1.0, 4.0, 2.0, 3.0])
    assert np.array_equal(SP.roll_median(x, 3), [0, 4, 2, 3, 0])
    assert np.array_equal(SP.roll_median(x, 5), [0, 0, 3, 0, 0])  # k = n: one interior point
    with pytest.raises(ValueError):
        SP.roll_median(x, 7)  # zoo stops for k > length
    with pytest.raises(ValueError):
        SP.roll_median(x, 4)  # even k: not restated
    for k in (1, 0, -3):
        assert np.array_equal(SP.roll_median(x, k), x)  # the callers' `> 1` tests


def test_r_quantile_by_hand():
    x = np.array([0.1, 0.7, 0.3, 0.9, 0.5])
    q = SP.r_quantile(x, 0.5)  # index = 3: the element itself
    assert q == 0.5 and np.count_nonzero(x - q == 0) == 1
    assert SP.r_quantile(x, 1.0) == 0.9 and SP.r_quantile(x, 0.0) == 0.1
    y = np.array([8.0, 1.0, 4.0, 2.0])
    assert SP.r_quantile(y, 0.5) == 3.0    # index 2.5: .5 * 2 + .5 * 4
    assert SP.r_quantile(y, 0.25) == 1.75  # index 1.75: .25 * 1 + .75 * 2
    # np.quantile's formula differs in its last bits in general; this one is R's
    z = np.array([0.3, 0.3, 0.5, 0.7])
    assert SP.r_quantile(z, 0.3) == 0.3    # index 1.9, x[hi] == x[lo]: no interpolation
    w = np.array([1.0, math.inf, math.inf])
    assert SP.r_quantile(w, 0.75) == math.inf  # index 2.5 between equal infinities


def test_frame_starts_fractional_step():
    # 22.05 kHz, step 15 ms: by = 330.75; floor(1 + i by) - 1 = floor(i by)
    s = SP.frame_starts(1102 + 1400, 22050, 1102, 15)
    assert list(s) == [0, 330, 661, 992, 1323]
    # 48 kHz, step 1.1 ms: by = 52.800000000000004, to = 793: (to - 1) / by =
    # 14.999999999999998 and seq's 1e-10 makes n = 15, i.e. 16 frames, not 15
    by = 1.1 / 1000 * 48000
    assert math.floor(792 / by) == 14 and math.floor(792 / by + 1e-10) == 15
    s = SP.frame_starts(240 + 793, 48000, 240, 1.1)
    assert len(s) == 16 and s[-1] == 792  # pmin(x, to) clamps 793.0000000000001
    assert SP.spectrogram_size(240 + 793, 48000, windowLength=5, step=1.1) == (240, 240, 120, 16)
    assert len(SP.frame_starts(240 + 792, 48000, 240, 1.1)) == 15
    # a sound as long as the window, or one sample longer: one frame
    assert list(SP.frame_starts(800, 16000, 800, 15)) == [0]
    assert list(SP.frame_starts(801, 16000, 800, 15)) == [0]


def test_zero_padding_rule():
    x = np.sin(np.arange(2000) * 0.1)
    for zp, N in ((0, 800), (801, 800), (802, 802), (803, 802), (1024, 1024)):
        assert SP.spectrogram_size(2000, 16000, zp=zp)[1:3] == (N, N // 2)
        bank = SP.get_frame_bank(x, 16000, 800, "gaussian", 15, zp)
        assert bank.shape[0] == N
        h = (N - 800) // 2
        assert np.all(bank[:h] == 0) and np.all(bank[N - h:] == 0) and np.all(bank[h + 1:N - h - 1, 0] != 0)
        assert SP.spectrogram_numpy(x, 16000, zp=zp, output="original").shape[0] == N // 2


def test_windows_by_hand():
    c = math.cos
    pi = math.pi
    e12 = math.exp(-12)
    want = {  # first, index 3, last of wl = 6 (n = 5)
        "bartlett": (0.0, 2 - 6 / 5, 0.0),  # m = 2: c(0, .4, 1.2, .8, .4, 0)
        "blackman": (0.42 - 0.5 + 0.08, 0.42 - 0.5 * c(6 * pi / 5) + 0.08 * c(12 * pi / 5),
                     0.42 - 0.5 * c(2 * pi) + 0.08 * c(4 * pi)),
        "flattop": (0.2156 - 0.4160 + 0.2781, 0.2156 - 0.4160 * c(6 * pi / 5) + 0.2781 * c(12 * pi / 5),
                    0.2156 - 0.4160 * c(2 * pi) + 0.2781 * c(4 * pi)),
        "hamming": (0.54 - 0.46, 0.54 - 0.46 * c(6 * pi / 5), 0.54 - 0.46 * c(2 * pi)),
        "hanning": (0.0, 0.5 - 0.5 * c(6 * pi / 5), 0.5 - 0.5 * c(2 * pi)),
        "rectangle": (1.0, 1.0, 1.0),
        "gaussian": ((math.exp(-12 * (1 / 6 - 0.5) ** 2) - e12) / (1 - e12),
                     (math.exp(-12 * (4 / 6 - 0.5) ** 2) - e12) / (1 - e12), (math.exp(-3) - e12) / (1 - e12)),
    }
    assert set(want) == set(SP.WINDOWS)
    for wn, (a, m, z) in want.items():
        w = SP.ft_window(6, wn)
        assert len(w) == 6
        assert w[0] == pytest.approx(a, abs=1e-15) and w[3] == pytest.approx(m, abs=1e-15), wn
        assert w[5] == pytest.approx(z, abs=1e-15), wn
    assert np.allclose(SP.ft_window(6, "bartlett"), [0, .4, 1.2, .8, .4, 0], atol=1e-15)
    assert SP.ft_window(6, "gaussian")[2] == 1.0  # (3 / 6 - .5) = 0
    with pytest.raises(ValueError):
        SP.ft_window(6, "rectangular")  # the roxygen text's name is not what the code accepts


Z34 = np.array([[1.0, 9.0, 2.0, 8.0],
                [7.0, 3.0, 6.0, 4.0],
                [5.0, 10.0, 0.0, 11.0]])  # 3 frames x 4 bins


def test_orientation_by_hand():
    """Z is frames x bins: the statements run along the other axis than their
    comments say. Each expectation differs from the 'as commented' reading."""
    # smoothTime = 3: the median runs along the 4 bins of each frame
    assert np.array_equal(SP.smooth_time(Z34, 3), [[0, 2, 8, 0], [0, 6, 4, 0], [0, 5, 10, 0]])
    # smoothFreq = 3: along the 3 frames of each bin (the 'as commented' smoothTime)
    along_frames = [[0, 0, 0, 0], [5, 9, 2, 8], [0, 0, 0, 0]]
    assert np.array_equal(SP.smooth_freq(Z34, 3), along_frames)
    assert not np.array_equal(SP.smooth_time(Z34, 3), along_frames)
    with pytest.raises(ValueError):
        SP.smooth_freq(Z34, 5)  # 5 > 3 frames
    # qTime = .5: each frame minus the median of ITS bins (5, 5, 7.5)
    assert np.array_equal(SP.subtract_qtime(Z34, 0.5),
                          [[-4, 4, -3, 3], [2, -2, 1, -1], [-2.5, 2.5, -7.5, 3.5]])
    per_bin = Z34 - np.array([5.0, 9.0, 2.0, 8.0])  # 'for each freq bin, subtract median'
    assert not np.array_equal(SP.subtract_qtime(Z34, 0.5), per_bin)
    # noise subtraction: cell (f, b) takes noise[(f + 3 b) mod 4]
    noise = np.array([10.0, 20.0, 30.0, 40.0])
    rec = np.array([[10.0, 40.0, 30.0, 20.0], [20.0, 10.0, 40.0, 30.0], [30.0, 20.0, 10.0, 40.0]])
    assert np.array_equal(SP.subtract_noise(Z34, noise, 1.0), Z34 - rec)
    assert np.array_equal(SP.subtract_noise(Z34, noise, 0.5), Z34 - 0.5 * rec)
    assert not np.array_equal(SP.subtract_noise(Z34, noise, 1.0), Z34 - noise)
    # spectralDerivative: dZ_dt along bins, dZ_df along frames, first column / row 0
    d = SP.spectral_derivative(Z34)
    assert d[0, 0] == 0 and d[0, 1] == 8 and d[1, 0] == 6 and d[1, 1] == math.sqrt(4 * 4 + 6 * 6)


def test_renormalize_and_contrast_by_hand():
    Z = np.array([[math.e ** 2, 0.0], [-1.0, 1.0]])
    r = SP.renormalize(Z)  # logs: 2, 0; the nonpositives at the smallest log, 0; minus 0
    assert np.allclose(r, [[2, 0], [0, 0]], atol=1e-15)
    out = SP.denoise(Z, contrast=0, brightness=0)
    assert np.allclose(out, [[1, 0], [0, 0]], atol=1e-15)
    out = SP.denoise(np.array([[math.e ** 2, math.e]]), contrast=1, brightness=-1)
    # (log - min log) = (1, 0); ^ e^3; / max; / e^-3, clamped at 1 since e^-3 < 1
    assert np.allclose(out, [[1, 0]])
    out = SP.denoise(np.array([[math.e ** 4, math.e ** 2, math.e]]), contrast=0, brightness=1)
    assert np.allclose(out, [[math.exp(-3), math.exp(-3) / 3, 0]])


def test_get_entropy_by_hand():
    assert math.isnan(SP.get_entropy(np.zeros(4)))  # NA: an empty frame
    e = SP.get_entropy(np.array([0.0, 1.0, 1.0, 1.0]))  # the 0 becomes 1e-10
    assert e == pytest.approx(10 ** -2.5 / ((3 + 1e-10) / 4), rel=1e-12)
    assert SP.get_entropy(np.ones(9)) == pytest.approx(1.0, abs=1e-15)
    entr, q, idx = SP.noise_frames(np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 3.0], [1.0, 9.0]]), 50)
    assert math.isnan(entr[0]) and list(idx) == [1, 2]  # quantile(na.rm), which() drops NA
    assert q == entr[2]  # 3 valid values, p = .5: index 2, an element


def test_all_zero_sound_is_nan():
    for output in ("original", "processed"):
        z = SP.spectrogram_numpy(np.zeros(2000), 16000, output=output)
        assert z.shape == (400, 5) and np.isnan(z).all()


def test_arguments():
    x = np.sin(np.arange(3000) * 0.05)
    with pytest.raises(NotImplementedError):
        SP.spectrogram_numpy(x, 16000, plot=True)
    with pytest.raises(NotImplementedError):
        SP.spectrogram(x, 16000, osc=True)
    with pytest.raises(NotImplementedError):
        SP.spectrogram(x, 16000, output="none")
    with pytest.raises(ValueError):
        SP.spectrogram_numpy(x)  # no samplingRate
    with pytest.raises(ValueError):
        SP.spectrogram_numpy(x, 16000, wn="rectangular")
    with pytest.raises(ValueError):
        SP.spectrogram_numpy(x, 16000, smoothTime=4)
    with pytest.raises(ValueError):
        SP.spectrogram_numpy(x[:700], 16000)  # shorter than the 800-point window
    with pytest.raises(ValueError):
        SP.spectrogram_numpy(x, 16000, smoothFreq=11)  # 10 frames
    both = SP.spectrogram_numpy(x + 2, 16000)  # min > 0: scale() first
    c = x - x.mean()
    assert np.allclose(both, SP.spectrogram_numpy(c / c.std(ddof=1), 16000), atol=1e-12)


# ------------------------------------------------------------ CPU: sg_spectrogram_size
def _supported(bins):
    r = bins
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while r % p == 0:
            r //= p
    return r == 1 and bins <= 2048


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 48000])
def test_sg_spectrogram_size_equals_restatement(sr):
    """sg_spectrogram_size (host only) makes spectrogram_size's decisions, at lengths
    around the frame-count boundaries."""
    from soundgen_beta_amd import native
    n = refused = 0
    for wlen in (50, 25, 40, 10.5, 5):
        for step in (None, 15, 5, 7.3, 1.1, 0.013):
            for zp in (0, 512, 1024, 4096):
                wl, N, bins, _ = SP.spectrogram_size(0, sr, wlen, step, 70, zp)
                if not _supported(bins):
                    with pytest.raises(native.SoundgenError) as e:
                        SP.spectrogram_size_native(wl + 10, sr, wlen, step, 70, zp)
                    assert e.value.code == -4
                    refused += 1
                    continue
                by = (wlen * 0.3 if step is None else step) / 1000 * sr
                lens = {0, 1, 2, wl - 1, wl, wl + 1, wl + 2}
                for k in (1, 2, 7, 200):
                    for d in (-1, 0, 1, 2):
                        lens.add(wl + int(math.floor(k * by)) + d)
                for length in sorted(lens):
                    assert SP.spectrogram_size_native(length, sr, wlen, step, 70, zp) == \
                        SP.spectrogram_size(length, sr, wlen, step, 70, zp), (wlen, step, zp, length)
                    n += 1
    assert n > 500
    if sr == 48000:  # the case where seq's 1e-10 decides
        assert SP.spectrogram_size_native(240 + 793, 48000, 5, 1.1) == (240, 240, 120, 16)


def test_sg_spectrogram_size_unsupported():
    from soundgen_beta_amd import native
    assert SP.spectrogram_size(1000, 16000, windowLength=4.625)[:3] == (74, 74, 37)
    with pytest.raises(native.SoundgenError) as e:
        SP.spectrogram_size_native(1000, 16000, windowLength=4.625)  # M = 37: a prime above 31
    assert e.value.code == -4 and "zp" in str(e.value)
    assert SP.spectrogram_size_native(1000, 16000, windowLength=4.625, zp=128) == (74, 128, 64, 42)
    assert SP.spectrogram_size(1000, 16000, windowLength=4.625, zp=128) == (74, 128, 64, 42)
    with pytest.raises(native.SoundgenError) as e:
        SP.spectrogram_size_native(10000, 44100, windowLength=100)  # 4410 points > 4096
    assert e.value.code == -4
    with pytest.raises(native.SoundgenError) as e:
        SP.spectrogram_size_native(10000, 16000, step=0)
    assert e.value.code == -1


# ------------------------------------------------------------ the GPU cases' inputs
def _signal(sr, seed=None, dur=0.6):
    """A vibrato harmonic complex that fades in and out, plus a noise floor."""
    rng = np.random.default_rng(SEEDS[sr] if seed is None else seed)
    n = int(dur * sr)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(220 * (1 + 0.1 * np.sin(2 * np.pi * 3 * t))) / sr
    x = sum(np.sin(h * ph) / h for h in range(1, 9))
    return x * np.sin(np.pi * t / dur) ** 2 + 0.01 * rng.standard_normal(n)


CASES = {
    "original": dict(output="original"),
    "defaults": dict(),
    "derivative": dict(method="spectralDerivative"),
    "medians": dict(smoothTime=5, smoothFreq=3),
    "qtime": dict(qTime=0.5),
    "qtime95": dict(qTime=0.95),
    "noise": dict(noiseReduction=1.1, percentNoise=10),
    "dark": dict(contrast=1, brightness=-1),
    "bright": dict(brightness=1),
    "step": dict(step=7.3),
    "all": dict(method="spectralDerivative", smoothTime=3, smoothFreq=3, qTime=0.5, noiseReduction=1.1,
                contrast=0.5, brightness=-0.3),
}
QTIME_CASES = ("qtime", "qtime95", "all")
BINS64 = dict(windowLength=4.625, zp=128, smoothTime=3, noiseReduction=1.1)  # 64 bins < a workgroup, 430 frames
# zp = 4096: 2048 bins, the largest frame (its two LDS buffers pass 64 KB: the opt-in path)
EXTRA = [(16000, "zp1024", dict(zp=1024)), (16000, "zp4096", dict(zp=4096, smoothTime=3)),
         (16000, "bins64", BINS64)] + \
    [(22050, "wn_" + wn, dict(wn=wn)) for wn in SP.WINDOWS]
ALL_CASES = [(sr, name, kw) for sr in RATES for name, kw in CASES.items()] + EXTRA


@lru_cache(maxsize=None)
def _reference(sr, name):
    kw = dict(CASES[name]) if name in CASES else dict([c for c in EXTRA if c[1] == name][0][2])
    ref = SP.spectrogram_numpy(_signal(sr), sr, **kw)
    ref.setflags(write=False)
    return ref


def _chain_inputs(sr, kw):
    """Z1 (frames x bins) as it reaches the qTime step / the entropy step of case kw."""
    Z = SP.spectrogram_numpy(_signal(sr), sr, step=kw.get("step"), output="original").T
    Z1 = SP.spectral_derivative(Z) if kw.get("method") == "spectralDerivative" else Z
    if kw.get("smoothTime", 0) > 1:
        Z1 = SP.smooth_time(Z1, kw["smoothTime"])
    if kw.get("smoothFreq", 0) > 1:
        Z1 = SP.smooth_freq(Z1, kw["smoothFreq"])
    return Z1


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("name", QTIME_CASES)
def test_reference_is_well_conditioned_qtime(sr, name):
    """The inputs of the GPU qTime cases: the smallest non-zero |x - q| / max(x, q)
    over all frames is >= 1e-6 (it sets the log floor; measured 1.1e-5 .. 1.4e-4
    for q = .5 on the plain spectrum), and no NaN."""
    kw = CASES[name]
    Z1 = _chain_inputs(sr, kw)
    gap = math.inf
    for row in Z1:
        q = SP.r_quantile(row, kw["qTime"])
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.abs(row - q) / np.maximum(row, q)
        d = d[(row - q) != 0]
        if d.size:  # a frame the rolling median along frames filled with 0 has no other cell
            gap = min(gap, float(d.min()))
    print("conditioning %d %s: smallest relative |x - q| %.3g" % (sr, name, gap))
    assert gap >= 1e-6
    assert not np.isnan(_reference(sr, name)).any()


@pytest.mark.parametrize("sr", RATES)
@pytest.mark.parametrize("name", ("noise", "all"))
def test_reference_is_well_conditioned_noise(sr, name):
    """The inputs of the GPU noiseReduction cases: the entropy quantile lies >= 1e-9
    from the nearest frame entropy, at least one frame and fewer than all are
    selected, the frame count is no multiple of the bins (the recycling shows), no NaN."""
    kw = CASES[name]
    Z1 = _chain_inputs(sr, kw)
    if kw.get("qTime", 0) > 0:
        Z1 = SP.subtract_qtime(Z1, kw["qTime"])
    Z1 = SP.renormalize(Z1)
    entr, q, idx = SP.noise_frames(Z1, kw.get("percentNoise", 10))
    ok = entr[~np.isnan(entr)]  # 'all': the two frames smoothFreq = 3 zeroes are NA and dropped
    assert len(ok) == len(entr) - (2 if name == "all" else 0)
    dist = float(np.min(np.abs(ok - q)))
    print("conditioning %d %s: entropy quantile distance %.3g, %d of %d frames" % (sr, name, dist, len(idx), len(ok)))
    assert dist >= 1e-9
    assert 1 <= len(idx) < len(ok)
    assert len(entr) % Z1.shape[1] != 0
    assert not np.isnan(_reference(sr, name)).any()


def test_reference_is_well_conditioned_bins64():
    """The 'bins64' case: more frames (430) than bins (64), no multiple of them, so
    the recycled index wraps many times; the entropy quantile keeps its distance."""
    sr = 16000
    Z = SP.spectrogram_numpy(_signal(sr), sr, windowLength=4.625, zp=128, output="original").T
    assert Z.shape == (430, 64)
    entr, q, idx = SP.noise_frames(SP.renormalize(SP.smooth_time(Z, 3)), 10)
    assert not np.isnan(entr).any()
    dist = float(np.min(np.abs(entr - q)))
    print("conditioning bins64: entropy quantile distance %.3g, %d of %d frames" % (dist, len(idx), len(entr)))
    assert dist >= 1e-9 and 1 <= len(idx) < len(entr)
    assert not np.isnan(_reference(sr, "bins64")).any()


# ------------------------------------------------------------ GPU vs restatement
def _err(got, want, output="processed"):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert not np.isnan(got).any()
    e = float(np.max(np.abs(got - want)))
    return e / float(want.max()) if output == "original" else e


@pytest.mark.gpu
@pytest.mark.parametrize("sr,name,kw", ALL_CASES, ids=["%d-%s" % (c[0], c[1]) for c in ALL_CASES])
def test_spectrogram_gpu_equals_numpy(sr, name, kw):
    want = _reference(sr, name)
    got = SP.spectrogram(_signal(sr), sr, **kw)
    e = _err(got, want, kw.get("output", "processed"))
    print("spectrogram parity %d %s: %.3g" % (sr, name, e))
    assert e <= (TOL_QTIME if name in QTIME_CASES else TOL_PLAIN)
    if name == "qtime" and sr == 22050:
        # 551 bins: the median is an element, x - q is exactly 0 for it and the
        # nonpositives rule puts it on the floor -- the same cells on both sides
        assert want.shape[0] == 551
        assert np.array_equal(got == got.min(), want == want.min())
        # per frame the median and the 275 bins below it; and the matrix's smallest
        # positive x - q, whose log is the floor itself
        n_floor = np.sum(want == want.min(), axis=0)
        assert (n_floor >= 276).all() and n_floor.sum() == 37 * 276 + 1
    if name == "noise":
        assert want.shape[1] % want.shape[0] != 0


@pytest.mark.gpu
def test_spectrogram_scale_branch_gpu():
    """min(sound) > 0: scale() (mean and sd on the device) before / max|x|."""
    sr = 16000
    x = _signal(sr)[:4000] + 7.5
    for output in ("original", "processed"):
        e = _err(SP.spectrogram(x, sr, output=output), SP.spectrogram_numpy(x, sr, output=output), output)
        print("spectrogram parity scale %s: %.3g" % (output, e))
        assert e <= TOL_PLAIN


# Frames whose half holds the radices no case above runs (7, 11, 13, 17, 23, 31), at the
# transform's own accuracy: tests/test_fft64.py derives TOL64; the frame kernel adds the
# untangling of the packed real transform (one more radix-2 stage in the sum) and the
# fp64 reference (numpy's FFT of the N-point frame) its own 2 * 2^-52.
FFT64_CASES = [("zp2002", dict(zp=2002), 1001), ("zp1426", dict(zp=1426), 713), ("zp3844", dict(zp=3844), 1922),
               ("zp4046", dict(zp=4046), 2023), ("zp4092", dict(zp=4092), 2046),
               ("wl9.625", dict(windowLength=9.625), 77)]


@lru_cache(maxsize=None)
def _short_signal():
    x = _signal(16000, dur=0.15)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("name,kw,M", FFT64_CASES, ids=[c[0] for c in FFT64_CASES])
def test_fft64_cases_reach_their_sizes(name, kw, M):
    from test_fft64 import stages
    wl, N, bins, frames = SP.spectrogram_size(len(_short_signal()), 16000, **kw)
    assert (N, bins) == (2 * M, M) and 4 <= frames <= 64
    assert set(stages(M)) & {7, 11, 13, 17, 23, 31}


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,M", FFT64_CASES, ids=[c[0] for c in FFT64_CASES])
def test_spectrogram_original_at_fft64_accuracy(name, kw, M):
    from test_fft64 import tol64
    x = _short_signal()
    want = SP.spectrogram_numpy(x, 16000, output="original", **kw)
    got = SP.spectrogram(x, 16000, output="original", **kw)
    assert got.shape == want.shape == (M, want.shape[1]) and not np.isnan(got).any()
    e = np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)
    tol = tol64(M, extra=(2,)) + 2 * 2.0 ** -52
    print("spectrogram original %s: M %d, %d frames, worst frame %.3g, bound %.3g" % (name, M, len(e), e.max(), tol))
    assert (e <= tol).all(), (name, float(e.max()), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(smoothFreq=3), dict(smoothFreq=7), dict(smoothTime=3), dict(smoothTime=399)],
                         ids=["freq3", "freq7", "time3", "time399"])
def test_rolling_median_edges_gpu(kw):
    """A 7-frame sound: k = 3 and k equal to the extent along frames (7) and the
    largest odd k along the 400 bins (399: two interior points per frame)."""
    sr = 16000
    x = _signal(sr)[2000:2000 + 800 + 6 * 240 + 1]
    want = SP.spectrogram_numpy(x, sr, **kw)
    assert want.shape == (400, 7)
    got = SP.spectrogram(x, sr, **kw)
    e = _err(got, want)
    print("spectrogram parity median %s: %.3g" % (kw, e))
    assert e <= TOL_PLAIN
    assert np.array_equal(got == got.min(), want == want.min())  # the zero fill, on the floor


@pytest.mark.gpu
def test_all_zero_sound_is_nan_gpu():
    for output in ("original", "processed"):
        z = SP.spectrogram(np.zeros(2000), 16000, output=output)
        assert z.shape == (400, 5) and np.isnan(z).all()


def _batch_calls(sr, n, seed):
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(n):
        f0 = float(np.exp(rng.uniform(np.log(100), np.log(400))))
        v1, v2 = rng.choice(list("aoieu"), size=2, replace=False)
        calls.append({"kind": "soundgen", "args": {
            "sylLen": float(rng.uniform(150, 500)), "samplingRate": sr, "temperature": 0, "addSilence": 0,
            "pitchAnchors": {"time": [0, .5, 1], "value": [f0, f0 * 1.3, f0 * 0.8]},
            "formants": str(v1) + str(v2), "rolloff": float(rng.uniform(-18, -6)),
            "noiseAnchors": {"time": [0, 300], "value": [float(rng.uniform(-40, -10))] * 2}},
            "uniforms": rng.uniform(size=200000)})
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(method="spectralDerivative", smoothTime=3, smoothFreq=3, qTime=0.5,
                                             noiseReduction=1.1)], ids=["defaults", "all"])
def test_spectrogram_batch_equals_single(kw):
    """spectrogram_batch over 24 synthesized calls of mixed length in HBM (one launch
    sequence, to_host=False, then copied back) vs spectrogram() per call on the same
    samples: EVERY non-empty call is compared, at the bar of the GPU cases. One call
    is refused by the planner (length -1), one is cut shorter than the window and
    one to the window exactly (one frame); those without frames come back empty."""
    import torch
    from soundgen_beta_amd import batch
    sr = 16000
    calls = _batch_calls(sr, 24, 7)
    calls[4] = {"kind": "harmonics", "pitch": np.full(1, 150.0), "params": dict(samplingRate=sr)}  # refused
    data, offs, lens = batch.synthesize_packed(calls, 0)
    assert lens[4] == -1 and (np.delete(lens, 4) > 2000).all() and len(set(lens.tolist())) > 10
    lens = lens.copy()
    lens[9] = 500   # shorter than the 800-point window
    lens[13] = 800  # the window exactly: one frame
    if kw:
        lens[13] = 800 + 2 * 240 + 1  # smoothFreq = 3 needs 3 frames
    out, ooff, shapes = SP.spectrogram_batch(data, offs, lens, sr, **kw)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    h = out.cpu().numpy()
    host = data.cpu().numpy()
    compared = nonempty = 0
    worst = 0.0
    for i in range(len(calls)):
        bins, frames = shapes[i]
        assert (bins, frames) == SP.spectrogram_size(int(lens[i]), sr)[2:]
        if i in (4, 9):
            assert frames == 0
            continue
        nonempty += 1
        got = h[ooff[i]:ooff[i] + bins * frames].reshape(frames, bins).T
        y = host[offs[i]:offs[i] + lens[i]].astype(np.float64)
        worst = max(worst, _err(got, SP.spectrogram(y, sr, **kw)))
        compared += 1
    print("spectrogram_batch: %d of %d non-empty calls compared, worst %.3g" % (compared, nonempty, worst))
    assert compared == nonempty == 22
    assert worst <= (TOL_QTIME if kw else TOL_PLAIN)
    lst = SP.spectrogram_batch(data, offs, lens, sr, to_host=True, **kw)
    assert lst[4].shape == (400, 0) and lst[9].shape == (400, 0)
    assert np.array_equal(lst[0], h[ooff[0]:ooff[0] + 400 * shapes[0][1]].reshape(shapes[0][1], 400).T)
    if not kw:  # against the restatement as well, on one call
        assert _err(lst[2], SP.spectrogram_numpy(host[offs[2]:offs[2] + lens[2]].astype(np.float64), sr)) <= TOL_PLAIN


@pytest.mark.gpu
def test_spectrogram_file_path(tmp_path):
    """A 16-bit file is normalized like a vector (unlike ssm()): spectrogram(path)
    equals the numeric call on the same samples, and the restatement."""
    from soundgen_beta_amd import api
    sr = 16000
    s = _signal(sr)[:6000]
    pcm = np.round(20000 * s / np.max(np.abs(s))).astype(np.int16)
    path = os.path.join(str(tmp_path), "s.wav")
    api.write_wav(path, pcm, sr)
    got = SP.spectrogram(path)
    assert np.array_equal(got, SP.spectrogram(pcm.astype(np.float64), sr))
    assert _err(got, SP.spectrogram_numpy(path)) <= TOL_PLAIN


@pytest.mark.gpu
def test_spectrogram_errors_gpu():
    from soundgen_beta_amd import native
    x = _signal(16000)[:4000]
    with pytest.raises(native.SoundgenError) as e:
        SP.spectrogram(x, 16000, windowLength=4.625)  # 37 bins
    assert e.value.code == -4 and "zp" in str(e.value)
    with pytest.raises(ValueError):
        SP.spectrogram(x, 16000, smoothTime=4)
    with pytest.raises(ValueError):
        SP.spectrogram(x, 16000, smoothFreq=15)  # 14 frames
    with pytest.raises(ValueError):
        SP.spectrogram(x, 16000, smoothTime=401)  # 400 bins
    with pytest.raises(ValueError):
        SP.spectrogram(x, 16000, wn="rectangular")
    with pytest.raises(NotImplementedError):
        SP.spectrogram(x, 16000, plot=True)
    with pytest.raises(ValueError):
        SP.spectrogram(x[:700], 16000)
    assert SP.spectrogram(x, 16000, smoothFreq=13).shape == (400, 14)
