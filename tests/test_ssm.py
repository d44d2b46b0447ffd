"""ssm() (R/SSM.R:63-360): the numpy restatement against hand-worked cases (CPU),
sg_ssm_size against the restatement's integer decisions (CPU), and the GPU path
(sg_ssm / sg_ssm_batch, sg_ssm.hip) against the restatement."""
import math
import os

import numpy as np
import pytest

from soundgen_beta_amd import ssm as S

# GPU vs numpy, absolute, on SSM cells and novelty points. The bar started at 1e-6
# (what test_compare_sounds_batch_gpu_equals_numpy sets for statistics derived from
# the fp64 mel path); the maxima measured on an MI355X came out below 1e-7, so it is
# 10 x the measured maximum: 2.02e-14 over the eight cases of
# test_ssm_gpu_equals_numpy (a novelty point; SSM cells 7.3e-15), 6.63e-14 over every
# other comparison of this file (a novelty point of test_ssm_file_path, whose
# samples are 32767 times larger; SSM cells 2.6e-14).
TOL_MAIN = 2.02e-13
TOL = 6.63e-13


# ------------------------------------------------------------------ CPU
def test_checkerboard_kernel_small():
    """size 4 (the dnorm branch): x = -1, -1/3, 1/3, 1 and sd = .5 give dnorm ratios
    exp(-(1 - 1/9) / (2 * .25)) = exp(-16/9) between the outer and inner points."""
    k = S.get_checkerboard_kernel(4, kernelSD=.5)
    e = math.exp(-16 / 9)
    want = np.array([[e * e, e, -e, -e * e],
                     [e, 1, -1, -e],
                     [-e, -1, 1, e],
                     [-e * e, -e, e, e * e]])
    np.testing.assert_allclose(k, want, rtol=1e-14, atol=0)
    assert (np.sign(k) == np.array([[1, 1, -1, -1], [1, 1, -1, -1], [-1, -1, 1, 1], [-1, -1, 1, 1]])).all()
    assert k.max() == 1.0


def test_checkerboard_kernel_dmvnorm_branch():
    """size 50 takes mvtnorm::dmvnorm with sigma = diag(2) * kernelSD: kernelSD is a
    variance there, kernel[i, j] ~ exp(-(x_i^2 + x_j^2) / (2 kernelSD))."""
    sd = .2
    k = S.get_checkerboard_kernel(50, kernelSD=sd)
    x = np.linspace(-1, 1, 50)
    mag = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2 * sd))
    np.testing.assert_allclose(np.abs(k), mag / mag.max(), rtol=1e-12, atol=0)
    assert k.max() == 1.0
    assert (k[:25, :25] > 0).all() and (k[25:, 25:] > 0).all() and (k[:25, 25:] < 0).all() and (k[25:, :25] < 0).all()
    # the dnorm branch with the same sd is a different (narrower) kernel
    k49 = S.get_checkerboard_kernel(48, kernelSD=sd)
    assert abs(k49[0, 0]) < 1e-9 < abs(k[0, 0])


def _selfsim_loops(m, simil, win, idx):
    """The double loop of selfsim() over given windows (1-based starts), then zeroOne."""
    n = len(idx)
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            mi = np.concatenate([m[:, c] for c in range(idx[i] - 1, idx[i] - 1 + win)])
            mj = np.concatenate([m[:, c] for c in range(idx[j] - 1, idx[j] - 1 + win)])
            if simil == "cosine":
                out[i, j] = (mi @ mj) / math.sqrt((mi @ mi) * (mj @ mj))
            else:
                out[i, j] = np.corrcoef(mi, mj)[0, 1]
    out = out - out.min()
    return out / out.max()


M26 = np.array([[1., 2, 3, 4, 5, 6],
                [3., 0, 1, 0, 2, 0]])


def test_selfsim_by_hand():
    # win = 1: numWins = 6, seq(1, 5, length.out = 6) = 1, 1.8, 2.6, 3.4, 4.2, 5 -> 1 2 3 3 4 5
    assert S.win_idx(6, 1) == (1, [1, 2, 3, 3, 4, 5])
    got = S.selfsim(M26, simil="cosine", win=1)
    assert got.shape == (6, 6)
    # raw cosine of frames 1 = (1, 3) and 2 = (2, 0) is 2 / (sqrt(10) 2); of frames 2 and 4
    # (both on the first axis) 1; the whole matrix through the reference's double loop
    np.testing.assert_allclose(got, _selfsim_loops(M26, "cosine", 1, [1, 2, 3, 3, 4, 5]), rtol=0, atol=1e-14)
    raw = S.selfsim_raw(M26, simil="cosine", win=1)
    assert abs(raw[0, 1] - 1 / math.sqrt(10)) < 1e-15 and abs(raw[1, 4] - 1) < 1e-15
    assert abs(raw[2, 3] - 1) < 1e-15  # winIdx repeats frame 3
    # win = 3: numWins = 2, winIdx = 1, 3; the vectors are frames 1-3 and 3-5 stacked
    assert S.win_idx(6, 3) == (3, [1, 3])
    got = S.selfsim(M26, simil="cosine", win=3)
    a, b = np.array([1., 3, 2, 0, 3, 1]), np.array([3., 1, 4, 0, 5, 2])
    c = (a @ b) / math.sqrt((a @ a) * (b @ b))
    assert abs(S.selfsim_raw(M26, simil="cosine", win=3)[0, 1] - c) < 1e-15
    np.testing.assert_allclose(got, [[1, 0], [0, 1]], atol=1e-15)  # zeroOne of [[1, c], [c, 1]]
    # cor
    np.testing.assert_allclose(S.selfsim(M26, simil="cor", win=3), [[1, 0], [0, 1]], atol=1e-15)
    r = np.corrcoef(a, b)[0, 1]
    assert abs(S.selfsim_raw(M26, simil="cor", win=3)[0, 1] - r) < 1e-15
    got = S.selfsim(M26, simil="cor", win=1)
    np.testing.assert_allclose(got, _selfsim_loops(M26, "cor", 1, [1, 2, 3, 3, 4, 5]), rtol=0, atol=1e-14)
    # two-point vectors correlate at +-1: frames 1 = (1, 3) and 2 = (2, 0) at -1, 2 and 3 = (3, 1) at +1
    assert got[0, 1] == 0 and got[1, 2] == 1
    # cor of (1, 1) with anything is NA (zero variance): zeroOne has no na.rm
    assert np.isnan(S.selfsim(np.array([[1., 2, 3, 4], [1., 0, 1, 0]]), simil="cor", win=1)).all()


def test_selfsim_window_rules():
    # a half-even tie: seq(1, 4, length.out = 3) = 1, 2.5, 4 and R's round(2.5) is 2
    assert S.win_idx(7, 3) == (3, [1, 2, 4])
    assert S.win_idx(9, 3) == (3, [1, 4, 6])  # round(3.5) = 4
    # an even win becomes ceiling(win / 2) * 2 - 1
    assert S.win_idx(20, 4)[0] == 3 and S.win_idx(20, 2)[0] == 1 and S.win_idx(40, 6)[0] == 5
    # the clamp to floor(ncol / 2), then the even rule
    assert S.win_idx(6, 5)[0] == 3 and S.win_idx(9, 7)[0] == 3 and S.win_idx(3, 3) == (1, [1, 2, 2])
    assert S.win_idx(2, 3) == (1, [1, 1])
    # one frame: floor(1 / 2) = 0 is even -> 1; a 1 x 1 matrix whose zeroOne is 0 / 0
    assert S.win_idx(1, 3) == (1, [1])
    s = S.selfsim(np.array([[1.], [2.]]), win=3)
    assert s.shape == (1, 1) and np.isnan(s).all()
    assert (S.get_novelty(s, 4, .2) == 0).all()


def test_nan_rule():
    """One all-zero column: its cosine is 0 / 0, and zeroOne (min / max without na.rm)
    makes the whole matrix NaN; getNovelty's NA become 0."""
    m = np.abs(np.random.default_rng(0).normal(size=(5, 12))) + .1
    m[:, 7] = 0
    s = S.selfsim(m, win=1)
    assert s.shape == (12, 12) and np.isnan(s).all()
    assert (S.get_novelty(s, 4, .2) == 0).all()


def test_novelty():
    n, K = 12, 4
    assert (S.get_novelty(np.zeros((n, n)), K, .2) == 0).all()
    # a constant matrix: every patch inside it is constant (cor is NA -> 0); only the
    # patches that reach into the zero padding see an edge
    nov = S.get_novelty(np.ones((n, n)), K, .2)
    assert (nov[K // 2:n - K // 2 + 1] == 0).all() and nov[0] > 0
    # two blocks: the patch centred on the boundary is the checkerboard itself
    s = np.zeros((n, n))
    s[:6, :6] = 1
    s[6:, 6:] = 1
    # with sd = .5 the kernel is e^2, e, 1 (e = exp(-16/9)) times the signs: cor = 0.664
    nov = S.get_novelty(s, K, .5)
    assert int(np.argmax(nov)) == 6 and abs(nov[6] - 0.6643) < 1e-3
    assert nov[6] > 2 * max(nov[3], nov[9])
    # K > n: every patch holds the whole matrix
    assert S.get_novelty(s, 50, .2).shape == (n,)


def test_melfcc_cepstra():
    nb = 40
    d = S.dctm2(nb, nb)
    np.testing.assert_allclose(d @ d.T, np.eye(nb), atol=1e-13)
    np.testing.assert_allclose(S.dctm2(nb, 13), d[:13], rtol=0, atol=0)
    w = S.lifter_weights(13)
    assert w[0] == 1 and w[1] == 1
    np.testing.assert_allclose(w[1:], np.arange(1, 13) ** 0.6, rtol=1e-15)
    with pytest.raises(ValueError):
        S.lifter_weights(1)
    # a spectrum scaled by c^2 (the wave by c): cepstrum 1 moves by sqrt(nbands) 2 log(c),
    # the others do not -- what the file path (no normalize) changes against the numeric path
    A = np.abs(np.random.default_rng(1).normal(size=(nb, 7))) + .5
    c = 32767.0
    c1, c2 = S.cepstra(A, 13), S.cepstra(A * c * c, 13)
    np.testing.assert_allclose(c2[0] - c1[0], math.sqrt(nb) * 2 * math.log(c), rtol=1e-12)
    np.testing.assert_allclose(c2[1:], c1[1:], rtol=0, atol=1e-11)


def test_ssm_arguments():
    x = np.sin(np.arange(8000) * .05)
    with pytest.raises(NotImplementedError):
        S.ssm_numpy(x, 16000, plot=True)
    with pytest.raises(NotImplementedError):
        S.ssm(x, 16000, plot=True)
    with pytest.raises(ValueError):
        S.ssm_numpy(x)  # no samplingRate
    with pytest.raises(ValueError):
        S.ssm_numpy(x, 16000, MFCC=[0, 3])
    with pytest.raises(ValueError):
        S.ssm_numpy(x, 16000, MFCC=[2, 201])
    with pytest.raises(ValueError):
        S.ssm_numpy(x, 16000, kernelLen=20)  # kernelSize 0


SIZE_SETTINGS = [dict(), dict(windowLength=25, overlap=50, ssmWin=10, kernelLen=150),
                 dict(windowLength=40, overlap=75, ssmWin=50, kernelLen=600),
                 dict(windowLength=25, overlap=50, kernelLen=2500), dict(windowLength=30, step=7, ssmWin=35, kernelLen=90),
                 dict(windowLength=20, overlap=0, ssmWin=200, kernelLen=300)]


@pytest.mark.parametrize("sr", [16000, 22050, 44100])
def test_sg_ssm_size_equals_restatement(sr):
    """sg_ssm_size (host only) makes the restatement's integer decisions: frames, n,
    win after the clamp, kernelSize; around the one- and two-frame boundaries too."""
    for kw in SIZE_SETTINGS:
        wl = kw.get("windowLength", 40)
        step = kw.get("step", wl * (1 - kw.get("overlap", 75) / 100))
        winpts, steppts = int(np.round(wl / 1000 * sr)), int(np.round(step / 1000 * sr))
        lens = [0, 1, 2, winpts - 1, winpts, winpts + 1, winpts + 2, winpts + steppts, winpts + steppts + 1,
                winpts + steppts + 2, winpts + 2 * steppts + 1, winpts + 5 * steppts + 3, sr // 3, sr, 3 * sr + 17]
        for n in lens:
            want = S.ssm_size(n, sr, **kw)
            assert S.ssm_size_native(n, sr, **kw) == want, (sr, kw, n)
    assert S.ssm_size(1, sr)[:2] == (0, 0)
    wp = int(np.round(.04 * sr))
    st = int(np.round(.01 * sr))
    assert S.ssm_size(wp + 1, sr)[:3] == (1, 1, 1)         # one frame
    assert S.ssm_size(wp + st + 1, sr)[:3] == (2, 2, 1)    # two frames: winIdx 1, 1
    assert S.ssm_size(sr, sr)[2:] == (3, 4)                # round(2.5) * 2 = 4: half to even


def test_sg_ssm_size_errors():
    from soundgen_beta_amd import native
    with pytest.raises(native.SoundgenError):
        S.ssm_size_native(1000, 16000, windowLength=0)
    with pytest.raises(native.SoundgenError):
        S.ssm_size_native(1000, 16000, step=0)


# ------------------------------------------------------------------ GPU
def _signal(sr, dur=1.2, seed=11):
    """A 19-harmonic glide 120 -> 200 Hz with a formant bump that jumps from 700 to
    1600 Hz at the midpoint, a 20 dB dip around the midpoint, white noise over the
    last fifth and a 1e-3 noise floor."""
    rng = np.random.default_rng(seed)
    n = int(round(dur * sr))
    t = np.arange(n) / sr
    f0 = 120 + 80 * t / dur
    ph = 2 * np.pi * np.cumsum(f0) / sr
    fc = np.where(t < dur / 2, 700.0, 1600.0)
    y = np.zeros(n)
    for h in range(1, 20):
        y += (1 + 4 * np.exp(-0.5 * ((h * f0 - fc) / 150) ** 2)) / h * np.sin(h * ph)
    y *= 10 ** (-np.exp(-0.5 * ((t - dur / 2) / 0.05) ** 2))
    tail = t >= 0.8 * dur
    y[tail] += 0.7 * rng.standard_normal(int(tail.sum()))
    return y + 1e-3 * rng.standard_normal(n)


SETTINGS = [dict(),
            dict(input="audiogram", simil="cor", ssmWin=10, kernelLen=150),
            dict(input="mfcc", norm=True, ssmWin=50, kernelLen=600),
            dict(input="spectrum", windowLength=25, overlap=50, kernelLen=2500)]

_REF = {}


def _reference(sr, k):
    """The numpy side of one (sr, setting) case, computed once and shared."""
    if (sr, k) not in _REF:
        r = S.ssm_numpy(_signal(sr), sr, returnSSM="raw", **SETTINGS[k])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[(sr, k)] = r
    return _REF[(sr, k)]


@pytest.mark.parametrize("k", range(len(SETTINGS)))
@pytest.mark.parametrize("sr", [16000, 44100])
def test_ssm_reference_is_well_conditioned(sr, k):
    """What makes the comparison below fair, asserted on the reference alone (CPU):
    no NaN cell, a raw similarity range >= 0.1 before zeroOne, and every novelty
    patch with a standard deviation >= 1e-3 (a correlation of a near-constant patch
    is round-off noise)."""
    r = _reference(sr, k)
    assert not np.isnan(r["ssm"]).any() and not np.isnan(r["novelty"]).any()
    assert r["raw"].max() - r["raw"].min() >= 0.1
    assert S.novelty_patch_sd(r["ssm"], r["kernelSize"]).min() >= 1e-3
    if k == 3:
        assert r["kernelSize"] == 100 and r["kernelSize"] > r["ssm"].shape[0]  # dmvnorm branch, K > n


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SETTINGS)))
@pytest.mark.parametrize("sr", [16000, 44100])
def test_ssm_gpu_equals_numpy(sr, k):
    """ssm() on the GPU vs the numpy restatement: equal shapes, every SSM cell and
    every novelty point within TOL_MAIN absolute, nothing left out."""
    r = _reference(sr, k)
    got = S.ssm(_signal(sr), sr, **SETTINGS[k])
    assert got["ssm"].shape == r["ssm"].shape and got["novelty"].shape == r["novelty"].shape
    es = float(np.max(np.abs(got["ssm"] - r["ssm"])))
    en = float(np.max(np.abs(got["novelty"] - r["novelty"])))
    print("ssm parity sr=%d setting=%d n=%d: max |dSSM| = %.3g, max |dnovelty| = %.3g" % (sr, k, len(r["novelty"]),
                                                                                         es, en))
    assert not np.isnan(got["ssm"]).any() and not np.isnan(got["novelty"]).any()
    assert es <= TOL_MAIN and en <= TOL_MAIN


def _close(got, want, what, mask=None):
    """Both within TOL, the maximum printed first (nothing but `mask` left out)."""
    g, w = (got, want) if mask is None else (got[mask], want[mask])
    err = float(np.max(np.abs(g - w))) if w.size else 0.0
    print("%s: max |d| = %.3g over %d values" % (what, err, w.size))
    assert not np.isnan(g).any() and err <= TOL, (what, err)


def _cut(sr, n, win, wl=40, step=10):
    """A length whose ssm() has exactly n windows of `win` frames."""
    winpts, steppts = int(np.round(wl / 1000 * sr)), int(np.round(step / 1000 * sr))
    for nf in range(1, 400):
        length = winpts + 1 + (nf - 1) * steppts
        got = S.ssm_size(length, sr, wl, ssmWin=step * win if win > 1 else 1, step=step)
        if got[1] == n and got[2] == win:
            return length
    raise AssertionError("no length gives n = %d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("win", [1, 3])
@pytest.mark.parametrize("n", [15, 16, 17, 33])
def test_ssm_tile_edges(n, win):
    """n around the 16 x 16 tile and over more than one tile, with D win = 11 or 33
    (no multiple of the MFMA's k = 4)."""
    sr = 16000
    x = _signal(sr)[:_cut(sr, n, win)]
    kw = dict(MFCC=range(2, 13), ssmWin=10 * win if win > 1 else 1, step=10, kernelLen=200)
    want = S.ssm_numpy(x, sr, **kw)
    got = S.ssm(x, sr, **kw)
    assert want["ssm"].shape == (n, n) == got["ssm"].shape
    assert not np.isnan(want["ssm"]).any()
    assert (S.novelty_patch_sd(want["ssm"], 4) >= 1e-3).all()  # every point is compared
    _close(got["ssm"], want["ssm"], "tile edges n=%d win=%d ssm" % (n, win))
    _close(got["novelty"], want["novelty"], "tile edges n=%d win=%d novelty" % (n, win))


@pytest.mark.gpu
def test_ssm_single_coefficient():
    """MFCC = 13 alone: D = 1, and with win = 1 a dot product of length 1 (cosine +-1)."""
    sr = 16000
    x = _signal(sr)[:9000]
    for win_ms in (1, 30):
        kw = dict(MFCC=[13], ssmWin=win_ms, kernelLen=200)
        want, got = S.ssm_numpy(x, sr, **kw), S.ssm(x, sr, **kw)
        assert got["ssm"].shape == want["ssm"].shape
        _close(got["ssm"], want["ssm"], "D = 1 ssmWin=%d ssm" % win_ms)
        # with win = 1 the cells are +-1 up to round-off and most patches near-constant
        ok = S.novelty_patch_sd(want["ssm"], 4) >= 1e-3
        _close(got["novelty"], want["novelty"], "D = 1 ssmWin=%d novelty" % win_ms, ok)


@pytest.mark.gpu
@pytest.mark.parametrize("n,L", [(15, 11), (16, 4), (17, 33), (33, 1), (50, 36)])
def test_gram_tile_map_exact(n, L):
    """The tile map of sg_ssm_gram (sg_debug_ssm_gram): small integers through the
    fp64 MFMA give the unnormalised Gram matrix bit for bit (every sum is exact), so a
    result written to a wrong row or column cannot hide."""
    import ctypes as C
    from soundgen_beta_amd import native
    rng = np.random.default_rng(n * 100 + L)
    F = rng.integers(-9, 10, size=(n, L)).astype(np.float64)
    F += np.arange(n)[:, None] * 16  # rows differ by more than any in-tile permutation could hide
    out = np.zeros(n * n)
    ctx = native.default_context(0)
    dp = C.POINTER(C.c_double)
    native.check(native.lib().sg_debug_ssm_gram(ctx.ptr, np.ascontiguousarray(F).ctypes.data_as(dp), L, n,
                                                out.ctypes.data_as(dp)), ctx.ptr)
    assert np.array_equal(out.reshape(n, n).T, F @ F.T)


@pytest.mark.gpu
def test_ssm_nan_rule_gpu():
    """An integer-valued wave with an exact zero sum and a zero stretch longer than
    two windows: the mean is exactly 0, the silent frames are exactly 0, their
    audiogram columns have norm 0, and one NaN cell makes the matrix NaN and the
    novelty 0 -- on both sides."""
    sr = 16000
    a = np.round(3000 * _signal(sr)[:6000])
    x = np.concatenate([a, np.zeros(2500), -a[::-1]])
    assert x.sum() == 0 and (x == np.round(x)).all()
    want = S.ssm_numpy(x, sr, input="audiogram")
    got = S.ssm(x, sr, input="audiogram")
    assert want["ssm"].shape == got["ssm"].shape and want["ssm"].shape[0] > 16
    assert np.isnan(want["ssm"]).all() and np.isnan(got["ssm"]).all()
    assert (want["novelty"] == 0).all() and (got["novelty"] == 0).all()


def _batch_calls(sr, n, seed):
    """Calls whose pitch and formants move within each call (structure for the SSM)."""
    rng = np.random.default_rng(seed)
    calls = []
    for i in range(n):
        f0 = float(np.exp(rng.uniform(np.log(100), np.log(400))))
        v1, v2 = rng.choice(list("aoieu"), size=2, replace=False)
        calls.append({"kind": "soundgen", "args": {
            "sylLen": float(rng.uniform(250, 900)), "samplingRate": sr, "temperature": 0, "addSilence": 0,
            "pitchAnchors": {"time": [0, .5, 1], "value": [f0, f0 * float(rng.uniform(1.2, 1.6)),
                                                           f0 * float(rng.uniform(0.6, 0.9))]},
            "formants": str(v1) + str(v2), "rolloff": float(rng.uniform(-18, -6)),
            "noiseAnchors": {"time": [0, 300], "value": [float(rng.uniform(-40, -10))] * 2}},
            "uniforms": rng.uniform(size=200000)})
    return calls


@pytest.mark.gpu
def test_ssm_batch_equals_single():
    """ssm_batch over 24 synthesized calls in HBM (one launch sequence) vs ssm_numpy
    per call: n_out equals sg_ssm_size, every SSM cell within TOL, and every novelty
    point whose reference patch has a standard deviation >= 1e-3 (at least 90 % of
    all points). Mixed lengths: calls with fewer frames than 2 win, a one-frame call
    and a call of length 0 (skipped)."""
    from soundgen_beta_amd import batch
    sr = 16000
    calls = _batch_calls(sr, 24, 3)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    assert (lens > 2000).all()
    lens = lens.copy()
    lens[5] = 0        # skipped: R's length(x) > 1 test
    lens[9] = 500      # shorter than one window: one frame
    lens[13] = 1120    # 3 frames < 2 win
    lens[17] = 1440    # 5 frames < 2 win
    novs, mats = S.ssm_batch(data, offs, lens, sr, returnSSM=True)
    novs2 = S.ssm_batch(data, offs, lens, sr)
    host = data.cpu().numpy()
    tot = cmp = 0
    seen = set()
    for i in range(len(calls)):
        nf, n, win, K = S.ssm_size_native(int(lens[i]), sr)
        assert (nf, n, win, K) == S.ssm_size(int(lens[i]), sr)
        assert novs[i].shape == (n,) and mats[i].shape == (n, n)
        assert np.array_equal(novs[i], novs2[i])
        seen.add(min(nf, 7))
        if n == 0:
            continue
        y = host[offs[i]:offs[i] + lens[i]].astype(np.float64)
        want = S.ssm_numpy(y, sr)
        assert want["ssm"].shape == (n, n)
        if n == 1:
            assert np.isnan(want["ssm"]).all() and np.isnan(mats[i]).all() and novs[i][0] == 0
            continue
        assert not np.isnan(want["ssm"]).any()
        _close(mats[i], want["ssm"], "batch call %d ssm" % i)
        ok = S.novelty_patch_sd(want["ssm"], K) >= 1e-3
        tot += n
        cmp += int(ok.sum())
        _close(novs[i], want["novelty"], "batch call %d novelty" % i, ok)
    assert {0, 1, 3, 5, 7} <= seen
    print("ssm_batch: %d of %d novelty points compared" % (cmp, tot))
    assert cmp >= 0.9 * tot


@pytest.mark.gpu
def test_ssm_file_path(tmp_path):
    """A 16-bit file is used raw (no normalize): ssm(path) equals ssm_numpy(path), and
    with cepstrum 1 among the features it differs from the numeric-vector call on the
    same samples (the normalize quirk)."""
    from soundgen_beta_amd import api
    sr = 16000
    pcm = np.round(20000 * _signal(sr)[:12000] / np.max(np.abs(_signal(sr)))).astype(np.int16)
    path = os.path.join(str(tmp_path), "s.wav")
    api.write_wav(path, pcm, sr)
    x, sr2 = S.read_wave(path)
    assert sr2 == sr and np.array_equal(x, pcm.astype(np.float64))
    kw = dict(MFCC=range(1, 14))
    want, got = S.ssm_numpy(path, **kw), S.ssm(path, **kw)
    assert got["ssm"].shape == want["ssm"].shape
    _close(got["ssm"], want["ssm"], "file ssm")
    assert (S.novelty_patch_sd(want["ssm"], 4) >= 1e-3).all()
    _close(got["novelty"], want["novelty"], "file novelty")
    vec = S.ssm(x, sr, **kw)
    assert np.max(np.abs(vec["ssm"] - got["ssm"])) > 1e-3


@pytest.mark.gpu
def test_ssm_errors_gpu():
    from soundgen_beta_amd import native
    x = _signal(16000)[:8000]
    with pytest.raises(native.SoundgenError) as e:
        S.ssm(x, 16000, windowLength=300)  # 4800 points: above the 4096-point FFT
    assert e.value.code == -4 and "4096" in str(e.value)
    with pytest.raises(native.SoundgenError) as e:
        S.ssm(x, 16000, kernelLen=30)
    assert e.value.code == -1
