"""time_stretch(), shift_pitch() and resample() (soundgen_beta_amd/stretch.py, csrc/sg_stretch.h,
csrc/sg_stretch.hip): a phase vocoder between the operator pair (A, A+) and a band-limited
resampler.

The rule of every comparison with the GPU, the one tests/test_invert.py, tests/test_fft64.py and
tests/test_sine_bank.py use: the measure is the relative 2-norm against the numpy restatement
run in long double, and the bound is 8 times the deviation of the SAME restatement run in fp64
from the long-double one on the same inputs. Nothing is taken from the code under test. Every
figure is printed before it is asserted (pytest -s shows them; DESIGN.md section 5 records
them). Inputs are a tone on noise a fifth as large: no bin is empty, no phase arbitrary.

CPU: the integer side (sg_stretch.h) as a stand-alone program, plain and with
-fsanitize=address,undefined, against brute force; the restatements on tones (the resampler
against the ideal tone, the vocoder's pitch and level); the identity q_j = j; the refusals.
"""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from soundgen_beta_amd import invert as IV
from soundgen_beta_amd import native
from soundgen_beta_amd import spectrogram as SP
from soundgen_beta_amd import stretch as ST

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundgen_beta_amd", "csrc")
LD = np.longdouble
SR = 16000

# The smallest shapes that reach every branch (tests/test_invert.py's, restated): windows of 8, 44
# (a fractional step), 62 ('hanning': zero denominators), 96 (zero padding; a step longer than the
# window: uncovered samples) and 2204 points (fft64's folded branch, 1103 bins: 18 walking waves a
# sound, the last one partly idle); an odd pad; a sound of wl + 1 samples (one frame: i1 = i, h = 0
# everywhere), a few hundred, 6000.
CASES = {
    "w8": dict(n=400, kw=dict(windowLength=0.5)),
    "w8_pad3": dict(n=400, kw=dict(windowLength=0.5, zp=14)),
    "w8_one_frame": dict(n=9, kw=dict(windowLength=0.5)),
    "w44_fractional": dict(n=300, kw=dict(windowLength=2.75, step=1.3)),
    "w62_hanning": dict(n=500, kw=dict(windowLength=3.9, wn="hanning")),
    "w96_gap": dict(n=700, kw=dict(windowLength=6, step=7.5)),
    "w96_zp": dict(n=6000, kw=dict(windowLength=6, zp=128)),
    "w2204": dict(n=6000, kw=dict(windowLength=137.75, step=60)),
}
FACTORS = (1, 0.5, 1.37, 2)
POSITION_CASES = ("w8_pad3", "w44_fractional", "w62_hanning", "w96_gap")
MODES = ("reversed", "freeze", "last_run")


def rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    cd = np.clongdouble
    return float(np.sqrt((np.abs(got.astype(cd) - want.astype(cd)) ** 2).sum() / (np.abs(want.astype(cd)) ** 2).sum()))


def _tone_noise(n, seed):
    """A tone on noise a fifth as large: no bin of a frame is empty."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return np.sin(2 * np.pi * 1234.5 * t + 0.3) + 0.2 * rng.standard_normal(n)


def _frames(n, kw):
    return len(IV._setup(n, SR, IV._args(kw), np.float64)[3])


def _covered(n, kw):
    wl, pad, N, starts, w = IV._setup(n, SR, IV._args(kw), np.float64)
    den = np.zeros(n)
    for s in starts:
        den[s:s + wl] += w * w
    return den != 0


def _mode_positions(mode, f_in):
    """Explicit positions for an output as long as the input (F_out = F_in): the frames backwards;
    one position between two frames throughout (a freeze); twice the speed, then a run of
    F_in - 1 exactly (i1 = i, h = 0)."""
    j = np.arange(f_in, dtype=np.float64)
    if mode == "reversed":
        return f_in - 1 - j
    if mode == "freeze":
        return np.full(f_in, min((f_in - 1) / 2 + 0.25, f_in - 1))
    return np.minimum(2 * j, f_in - 1)


@functools.lru_cache(maxsize=None)
def sound_of(name):
    x = _tone_noise(CASES[name]["n"], sum(map(ord, name)))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def vocoder_case(name, how):
    """The restatement of one stretch in long double and in fp64, computed once and never written
    to: how is a factor, or one of MODES."""
    c = CASES[name]
    n, kw = c["n"], c["kw"]
    args = dict(factor=how) if how in FACTORS else dict(positions=_mode_positions(how, _frames(n, kw)), length=n)
    out = dict(n=n, kw=kw, args=args)
    out["y_ld"], out["X_ld"] = ST.time_stretch_numpy(sound_of(name), SR, dtype=LD, return_spectrum=True, **args, **kw)
    out["y_64"], out["X_64"] = ST.time_stretch_numpy(sound_of(name), SR, return_spectrum=True, **args, **kw)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ratio (up, down) and length: every ratio of the issue at 1, 33 and 1000 samples, the extremes at
# 200, and n : n_s as shift_pitch forms it (1000 samples by 1.37: 1000 : 1370 = 100 : 137)
RESAMPLE = [(u, d, n) for (u, d) in ((3, 2), (2, 3), (160, 147)) for n in (1, 33, 1000)] + \
           [(1, 64, 200), (64, 1, 200), (1000, 1370, 1000), (1370, 1000, 1370), (1, 4, 33)]


@functools.lru_cache(maxsize=None)
def resample_cases(f32):
    """Every (ratio, length) of RESAMPLE on its own tone-plus-noise sound (rounded to fp32 first
    when f32), restated in long double and in fp64."""
    out = []
    for k, (u, d, n) in enumerate(RESAMPLE):
        x = _tone_noise(n, 300 + k)
        if f32:
            x = x.astype(np.float32)
        ld, f64 = ST.resample_numpy(x, up=u, down=d, dtype=LD), ST.resample_numpy(x, up=u, down=d)
        for v in (x, ld, f64):
            v.setflags(write=False)
        out.append(dict(up=u, down=d, n=n, x=x, ld=ld, f64=f64))
    return out


# ---- CPU -------------------------------------------------------------------------------------

def _build_pins(tmp_path, sanitize):
    exe = str(tmp_path / ("stretch_pins_san" if sanitize else "stretch_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "stretch_pins.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_integer_side_on_the_host_equals_brute_force(tmp_path):
    """tests/cpp/stretch_pins.cpp: n_out, the taps of every output sample, the reduction mod 2 D and
    the position split of sg_stretch.h against brute force over 7 ratios x 4 lengths; its own
    program, plain and with -fsanitize=address,undefined."""
    exes = [_build_pins(tmp_path, False)]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(_build_pins(tmp_path, True))
    for exe in exes:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert r.stdout.split()[:2] == ["ok", "28"]


def test_library_and_restatement_agree_on_sizes():
    """sg_stretch_size (host only) against the restatement: frames of both lengths and the
    workspace by hand; n_out and the most taps of a ratio."""
    for name, c in CASES.items():
        n, kw = c["n"], c["kw"]
        wl, pad, N, starts, _ = IV._setup(n, SR, IV._args(kw), np.float64)
        n_out = ST._out_length(n, 1.37)
        z = ST.stretch_size(n, SR, out_length=n_out, **kw)
        f_out = _frames(n_out, kw)
        assert (z["frames_in"], z["frames_out"]) == (len(starts), f_out), name
        assert z["workspace_bytes"] == len(starts) * (N // 2 + 1) * 16 + f_out * ((N // 2 + 1) * 16 + wl * 8 + 48)
    for u, d, n in RESAMPLE:
        z = ST.stretch_size(n, up=u, down=d)
        assert z["n_out"] == -((-n * u) // d) == len(ST.resample_numpy(np.zeros(n), up=u, down=d))
    assert ST.stretch_size(200, up=1, down=64) == dict(n_out=4, taps=2048)
    assert ST.stretch_size(200, up=128, down=2) == dict(n_out=12800, taps=32)
    assert ST.stretch_size(1000, up=160, down=147)["taps"] == 32


def test_resample_numpy_of_equal_rates_is_the_input_bit_for_bit():
    x = _tone_noise(1000, 3)
    for u, d in ((1, 1), (7, 7), (44100, 44100)):
        for dt in (np.float64, LD):
            y = ST.resample_numpy(x, up=u, down=d, dtype=dt)
            assert y.dtype == dt and np.array_equal(y, x.astype(dt))
    assert np.array_equal(ST.resample_numpy(x, 16000, 16000), x)


def test_resample_numpy_of_a_tone_is_the_tone():
    """1 kHz at 16 kHz, 4000 samples, by 3:2 and 2:3: the middle 60 % of the output against the
    ideal tone at the new rate, 1e-4 maximum error (measured 4.1e-5 and 3.3e-5: the ripple of a
    Hann-windowed sinc of 16 zero crossings). 3 kHz by 1:4 lies above the new Nyquist rate (2 kHz)
    and is removed: below 1e-3 RMS over the same middle (measured 6.9e-5)."""
    t = np.arange(4000) / SR
    for (u, d), seen in (((3, 2), 4.1e-5), ((2, 3), 3.3e-5)):
        y = ST.resample_numpy(np.sin(2 * np.pi * 1000 * t), up=u, down=d)
        assert len(y) == -((-4000 * u) // d)
        ideal = np.sin(2 * np.pi * 1000 * np.arange(len(y)) * d / u / SR)
        a, b = int(0.2 * len(y)), int(0.8 * len(y))
        err = float(np.abs(y - ideal)[a:b].max())
        print("resample %d:%d of a 1 kHz tone: max error %.3g (recorded %.3g)" % (u, d, err, seen))
        assert err <= 1e-4
    y = ST.resample_numpy(np.sin(2 * np.pi * 3000 * t), SR, SR // 4)
    assert len(y) == 1000
    rms = float(np.sqrt(np.mean(y[200:800] ** 2)))
    print("resample 1:4 of a 3 kHz tone: RMS %.3g" % rms)
    assert rms <= 1e-3


@pytest.mark.parametrize("name", [k for k in CASES if k != "w8_one_frame"] + ["w8_one_frame"])
def test_stretch_numpy_at_its_own_positions_is_the_identity(name):
    """q_j = j and n_out = n: X' = X up to rounding, so y = x on covered samples -- in long double
    within 1e-15 relative (measured 6e-19 .. 6e-18); the fp64 figure is printed. Uncovered
    samples are 0."""
    c = CASES[name]
    n, kw = c["n"], c["kw"]
    x, cov = sound_of(name), _covered(n, kw)
    q = np.arange(_frames(n, kw), dtype=np.float64)
    y_ld = ST.time_stretch_numpy(x, SR, positions=q, length=n, dtype=LD, **kw)
    y_64 = ST.time_stretch_numpy(x, SR, positions=q, length=n, **kw)
    d_ld, d_64 = rel(y_ld[cov], x[cov]), rel(y_64[cov], x[cov])
    print("identity %s: long double %.3g, fp64 %.3g" % (name, d_ld, d_64))
    assert d_ld <= 1e-15
    assert np.all(y_ld[~cov] == 0) and np.all(y_64[~cov] == 0)
    # factor = 1 forms the same positions and length
    assert np.array_equal(ST.time_stretch_numpy(x, SR, factor=1, **kw), y_64)


def _peak_hz(y):
    """The spectral peak of the middle 3200 samples (5 Hz bins at 16 kHz) and their RMS."""
    a = (len(y) - 3200) // 2
    mid = y[a:a + 3200]
    sp = np.abs(np.fft.rfft(mid * np.hanning(3200)))
    return float(np.argmax(sp) * SR / 3200), float(np.sqrt(np.mean(mid ** 2)))


def test_stretch_and_shift_numpy_of_a_tone():
    """1 kHz at 16 kHz, 8000 samples, windowLength = 25: 1.5 times as long, the middle still peaks at
    1000 Hz with an RMS within 1 % of 1 / sqrt 2 (measured 0.70711); shifted by 1.25 it has its n
    samples and peaks at 1250 Hz."""
    tone = np.sin(2 * np.pi * 1000 * np.arange(8000) / SR)
    y = ST.time_stretch_numpy(tone, SR, factor=1.5, windowLength=25)
    hz, rms = _peak_hz(y)
    print("time_stretch_numpy(1.5): %d samples, peak %g Hz, RMS %.5f" % (len(y), hz, rms))
    assert len(y) == 12000 and hz == 1000 and abs(rms * np.sqrt(2) - 1) <= 0.01
    z = ST.shift_pitch_numpy(tone, SR, 1.25, windowLength=25)
    hz, rms = _peak_hz(z)
    print("shift_pitch_numpy(1.25): %d samples, peak %g Hz, RMS %.5f" % (len(z), hz, rms))
    assert len(z) == 8000 and hz == 1250 and abs(rms * np.sqrt(2) - 1) <= 0.01


REFUSALS = [dict(windowLength=4.7), dict(windowLength=300), dict(windowLength=6, zp=10000), dict(windowLength=0.1)]


@pytest.mark.parametrize("kw", REFUSALS, ids=["half_37", "window_4800", "zp_10000", "window_2"])
def test_refusals_are_spectrograms(kw):
    """spectrogram()'s code and text from sg_stretch_size, and the code from the entry point with
    ctx = NULL and no buffers: raised before the context is looked at."""
    with pytest.raises(native.SoundgenError) as want:
        SP.spectrogram_size_native(1000, SR, **kw)
    with pytest.raises(native.SoundgenError) as got:
        ST.stretch_size(1000, SR, out_length=1370, **kw)
    assert got.value.code == want.value.code == -4 and str(got.value) == str(want.value)
    P = IV._params(SR, IV._args(kw))
    assert native.lib().sg_time_stretch_batch(None, None, 0, None, None, 1, C.byref(P), None, None, None, None, None, None, 0,
                                              None, None) == -4


def test_own_refusals():
    x = _tone_noise(700, 9)
    kw = dict(windowLength=6)  # 96 points
    f_in = _frames(700, kw)
    good = np.arange(f_in, dtype=np.float64)
    for bad in (np.where(good == 3, np.nan, good), good - 1e-9, np.where(good == 2, f_in - 1 + 1e-9, good), good[:-1],
                np.concatenate([good, [0.0]])):
        with pytest.raises(ValueError):
            ST.time_stretch_numpy(x, SR, positions=bad, length=700, **kw)
    with pytest.raises(ValueError):  # the sound is shorter than the window, as stft() has it
        ST.time_stretch_numpy(x[:95], SR, factor=2, **kw)
    with pytest.raises(ValueError):  # the output is
        ST.time_stretch_numpy(x, SR, factor=0.1, **kw)
    with pytest.raises(ValueError):
        ST.time_stretch_numpy(x, SR, factor=0, **kw)
    with pytest.raises(TypeError):
        ST.time_stretch_numpy(x, SR, factor=2, windowLenght=6)
    for u, d in ((1, 65), (65, 1), (130, 2), (0, 1), (1, -1), (1.5, 1), (1 << 31, 1 << 31)):
        with pytest.raises(ValueError):
            ST.resample_numpy(x, up=u, down=d)
    with pytest.raises(ValueError):
        ST.resample_numpy(x, 16000.5, 8000)
    with pytest.raises(ValueError):
        ST.resample_numpy(x, 16000)
    # the library's own: SG_E_ARG with a text
    for u, d in ((1, 65), (0, 1), (1 << 31, 1)):
        with pytest.raises(native.SoundgenError) as e:
            ST.stretch_size(200, up=u, down=d)
        assert e.value.code == -1
    with pytest.raises(native.SoundgenError) as e:
        ST.stretch_size(1431655765, up=3, down=2)  # ceil(1.5 n) = 2^31
    assert e.value.code == -1 and "2^31" in str(e.value)
    assert ST.stretch_size(1431655764, up=3, down=2)["n_out"] == 2147483646
    # the entry points with ctx = NULL: the ratio, a NaN position, a count and a short output are refused
    # before the context is looked at (a missing context has the same code: the texts are checked on the GPU)
    L = native.lib()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)  # noqa: E731
    assert L.sg_resample_batch(None, None, 0, None, i64(200), 1, i64(1), i64(65), None, None) == -1
    P = IV._params(SR, IV._args(kw))
    q = (C.c_double * f_in)(*good)
    assert L.sg_time_stretch_batch(None, None, 0, None, i64(700), 1, C.byref(P), i64(50), q, i64(0), i64(f_in), None, None, 0,
                                   None, None) == -1


# ---- GPU -------------------------------------------------------------------------------------

def _check(what, got, want_ld, fp64):
    dev = rel(fp64, want_ld)
    err = rel(got, want_ld)
    print("%s: GPU %.3g, fp64 restatement %.3g, bound %.3g" % (what, err, dev, 8 * dev))
    assert err <= 8 * dev, what


def _stretch(name, how):
    """The sound and X' of one stretch, each by the rule."""
    c = vocoder_case(name, how)
    y, X = ST.time_stretch(sound_of(name), SR, return_spectrum=True, **c["args"], **c["kw"])
    assert y.shape == c["y_ld"].shape and X.shape == c["X_ld"].shape and X.dtype == np.complex128
    _check("X' %s %s" % (name, how), X, c["X_ld"], c["X_64"])
    _check("sound %s %s" % (name, how), y, c["y_ld"], c["y_64"])
    assert np.array_equal(ST.time_stretch(sound_of(name), SR, **c["args"], **c["kw"]), y)  # without the spectrum's copy
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("name", list(CASES))
def test_time_stretch_by_a_factor(name, factor):
    c = CASES[name]
    if name == "w8_one_frame" and factor == 0.5:  # 5 samples: shorter than the window
        with pytest.raises(ValueError):
            ST.time_stretch(sound_of(name), SR, factor=factor, **c["kw"])
        return
    y = _stretch(name, factor)
    if factor == 1:  # the identity, on the GPU: the input wherever a frame covers it, by the rule
        cov = _covered(c["n"], c["kw"])
        v = vocoder_case(name, factor)
        _check("identity " + name, y[cov], sound_of(name)[cov].astype(LD), v["y_64"][cov])
        assert np.all(y[~cov] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", POSITION_CASES)
def test_time_stretch_at_explicit_positions(name, mode):
    _stretch(name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_resample_against_restatement(f32):
    """Every ratio and length of RESAMPLE in one batch, fp64 and fp32 inputs; 1:1 (given as 7:7)
    returns the input bit for bit. 2:3 of one sample is a single product, x[0] * (2 / 3), which the
    fp64 and the long-double restatement round to the same number: its bound by the rule is 0, and
    the GPU returns that number (measured 0)."""
    import torch
    cases = resample_cases(f32)
    xs = [c["x"] for c in cases] + [cases[2]["x"]]
    lens = [len(x) for x in xs]
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    data = torch.from_numpy(np.concatenate(xs)).cuda()
    out, ooff, olen = ST.resample_batch(data, offs, lens, up=[c["up"] for c in cases] + [7], down=[c["down"] for c in cases] + [7])
    assert out.is_cuda and out.dtype == torch.float64
    h = out.cpu().numpy()
    for k, c in enumerate(cases):
        assert olen[k] == len(c["ld"])
        _check("resample %d:%d of %d %s samples" % (c["up"], c["down"], c["n"], "fp32" if f32 else "fp64"),
               h[ooff[k]:ooff[k] + olen[k]], c["ld"], c["f64"])
    assert olen[-1] == lens[-1] and np.array_equal(h[ooff[-1]:ooff[-1] + olen[-1]], xs[-1].astype(np.float64))
    # one sound from the host, by its rates
    one = ST.resample(cases[2]["x"], 16000, 24000)
    assert np.array_equal(one, h[ooff[2]:ooff[2] + olen[2]])


@pytest.mark.gpu
@pytest.mark.parametrize("multiplier", [0.8, 1.25])
@pytest.mark.parametrize("name", ["w62_hanning", "w96_zp"])
def test_shift_pitch(name, multiplier):
    c = CASES[name]
    x = sound_of(name)
    ld = ST.shift_pitch_numpy(x, SR, multiplier, dtype=LD, **c["kw"])
    f64 = ST.shift_pitch_numpy(x, SR, multiplier, **c["kw"])
    y = ST.shift_pitch(x, SR, multiplier, **c["kw"])
    assert y.shape == (c["n"],)
    _check("shift_pitch %s by %g" % (name, multiplier), y, ld, f64)


def _batch():
    """Mixed lengths under one setting (96 points): one frame and an uncovered sample, several
    frames, shorter than the window (no frames: refused per call, as stft_batch has it), exactly the
    window, long, odd."""
    kw = dict(windowLength=6, step=2.3)
    lens = [97, 700, 50, 96, 1500, 333]
    return kw, lens, [_tone_noise(n, 60 + i) for i, n in enumerate(lens)]


@pytest.mark.gpu
def test_batch_equals_singles_bit_for_bit():
    """A sound's samples alone, in a batch, in the reversed batch and under three workspace caps from
    sg_stretch_size (one sound a chunk, two of the largest, no cap); time_stretch, then shift_pitch
    with the stretched sounds kept in HBM."""
    import torch
    kw, lens, xs = _batch()
    f = 1.37
    single = [ST.time_stretch(x, SR, factor=f, **kw) if n >= 96 else None for x, n in zip(xs, lens)]
    shifted = [ST.shift_pitch(x, SR, f, **kw) if n >= 96 else None for x, n in zip(xs, lens)]
    with pytest.raises(ValueError):
        ST.time_stretch(xs[2], SR, factor=f, **kw)
    need = [ST.stretch_size(n, SR, out_length=ST._out_length(n, f), **kw)["workspace_bytes"] for n in lens]
    for order in (list(range(6)), list(range(5, -1, -1))):
        data = torch.from_numpy(np.concatenate([xs[i] for i in order])).cuda()
        ls = [lens[i] for i in order]
        offs = np.concatenate([[0], np.cumsum(ls)])[:-1]
        for cap in (1, 2 * max(need), 0):
            out, ooff, olen = ST.time_stretch_batch(data, offs, ls, SR, factor=f, workspace_cap=cap, **kw)
            assert out.is_cuda and out.dtype == torch.float64
            h = out.cpu().numpy()
            sh = ST.shift_pitch_batch(data, offs, ls, SR, f, workspace_cap=cap, to_host=True, **kw)
            for k, i in enumerate(order):
                assert olen[k] == ST._out_length(lens[i], f) and len(sh[k]) == lens[i]
                got = h[ooff[k]:ooff[k] + olen[k]]
                if single[i] is None:
                    assert np.all(got == 0) and np.all(sh[k] == 0)
                else:
                    assert np.array_equal(got, single[i]), (order, cap, i)
                    assert np.array_equal(sh[k], shifted[i]), (order, cap, i)


GUARD = 12345.678


@pytest.mark.gpu
def test_nothing_is_written_around_an_output():
    """The entry points on a caller's buffer with 64 guard cells before, between and behind the
    outputs (sounds and X'), fp32 input: the guards are untouched and the outputs are the wrappers'.
    Then the refusals that need a context to read their text."""
    import torch
    kw, lens, xs = _batch()
    L, ctx = native.lib(), native.default_context(0)
    P = IV._params(SR, IV._args(kw))
    f, G = 1.37, 64
    x32 = [x.astype(np.float32) for x in xs]
    data = torch.from_numpy(np.concatenate(x32)).cuda()
    offs, ls, nc, p_offs, p_lens = native.batch_layout(np.concatenate([[0], np.cumsum(lens)])[:-1], lens)
    i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    arr = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.int64))  # noqa: E731
    outl = arr([ST._out_length(n, f) for n in lens])
    z = [ST.stretch_size(n, SR, out_length=int(o), **kw) for n, o in zip(lens, outl)]
    qs = [ST._positions(None, f, s["frames_in"], s["frames_out"]) if s["frames_in"] else np.zeros(0) for s in z]
    pcnt = arr([len(q) for q in qs])
    poff = arr(np.concatenate([[0], np.cumsum(pcnt)])[:-1])
    flat = np.ascontiguousarray(np.concatenate(qs))
    ooff = arr(G + np.concatenate([[0], np.cumsum(outl + G)])[:-1])
    cells = pcnt * 49
    soff = arr(G + np.concatenate([[0], np.cumsum(cells + G)])[:-1])
    out = torch.full((int(ooff[-1] + outl[-1] + G),), GUARD, dtype=torch.float64, device="cuda")
    spec = torch.full((int(soff[-1] + cells[-1] + G),), GUARD, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()

    def call(q=flat, cnt=pcnt, ol=outl):
        return L.sg_time_stretch_batch(ctx.ptr, C.c_void_p(data.data_ptr()), 0, p_offs, p_lens, nc, C.byref(P),
                                       ol.ctypes.data_as(i64p), q.ctypes.data_as(dp), poff.ctypes.data_as(i64p),
                                       cnt.ctypes.data_as(i64p), C.c_void_p(out.data_ptr()), ooff.ctypes.data_as(i64p), 0,
                                       C.c_void_p(spec.data_ptr()), soff.ctypes.data_as(i64p))
    native.check(call(), ctx.ptr)
    h, hs = out.cpu().numpy(), spec.cpu().numpy()
    want, (wspec, woff, _) = ST.time_stretch_batch(data, offs, ls, SR, factor=f, return_spectrum=True, **kw)
    want, wspec = want[0].cpu().numpy(), wspec.cpu().numpy()
    keep, keep_s, at = np.ones(len(h), bool), np.ones(len(hs), bool), 0
    for k in range(nc):
        keep[ooff[k]:ooff[k] + outl[k]] = False
        keep_s[soff[k]:soff[k] + cells[k]] = False
        assert np.array_equal(h[ooff[k]:ooff[k] + outl[k]], want[at:at + outl[k]])
        assert np.array_equal(hs[soff[k]:soff[k] + cells[k]], wspec[woff[k]:woff[k] + cells[k]])
        at += outl[k]
    assert keep.sum() == G * (nc + 1) and np.all(h[keep] == GUARD) and np.all(hs[keep_s] == GUARD)
    # the resampler, the same way
    ups, downs = arr([3, 2, 160, 1, 64, 7]), arr([2, 3, 147, 64, 1, 7])
    rl = arr([ST.stretch_size(n, up=int(u), down=int(d))["n_out"] for n, u, d in zip(lens, ups, downs)])
    roff = arr(G + np.concatenate([[0], np.cumsum(rl + G)])[:-1])
    rout = torch.full((int(roff[-1] + rl[-1] + G),), GUARD, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    native.check(L.sg_resample_batch(ctx.ptr, C.c_void_p(data.data_ptr()), 0, p_offs, p_lens, nc, ups.ctypes.data_as(i64p),
                                     downs.ctypes.data_as(i64p), C.c_void_p(rout.data_ptr()), roff.ctypes.data_as(i64p)), ctx.ptr)
    hr = rout.cpu().numpy()
    rw = ST.resample_batch(data, offs, ls, up=ups, down=downs, to_host=True)
    keep = np.ones(len(hr), bool)
    for k in range(nc):
        keep[roff[k]:roff[k] + rl[k]] = False
        assert np.array_equal(hr[roff[k]:roff[k] + rl[k]], rw[k])
    assert keep.sum() == G * (nc + 1) and np.all(hr[keep] == GUARD)
    # SG_E_ARG with its text: a NaN position, a position past the last frame, a wrong count, a short output
    nan_q = flat.copy()
    nan_q[poff[1] + 3] = np.nan
    past = flat.copy()
    past[poff[4]] = z[4]["frames_in"] - 1 + 1e-9
    fewer = pcnt.copy()
    fewer[1] -= 1
    short = outl.copy()
    short[3] = 95
    for kwargs, word in ((dict(q=nan_q), "position 3"), (dict(q=past), "position 0"), (dict(cnt=fewer), "positions"),
                         (dict(ol=short), "shorter than the window")):
        with pytest.raises(native.SoundgenError) as e:
            native.check(call(**kwargs), ctx.ptr)
        assert e.value.code == -1 and word in str(e.value), str(e.value)
    bad_down = arr([2, 3, 147, 65, 1, 7])
    rc = L.sg_resample_batch(ctx.ptr, C.c_void_p(data.data_ptr()), 0, p_offs, p_lens, nc, ups.ctypes.data_as(i64p),
                             bad_down.ctypes.data_as(i64p), C.c_void_p(rout.data_ptr()), roff.ctypes.data_as(i64p))
    with pytest.raises(native.SoundgenError) as e:
        native.check(rc, ctx.ptr)
    assert e.value.code == -1 and "call 3" in str(e.value) and "2,048" in str(e.value)
    with pytest.raises(ValueError):
        ST.resample_batch(data, offs, ls, up=ups, down=bad_down, to_host=True)


@pytest.mark.gpu
def test_stage_clock_reports_every_stage():
    import torch
    kw, lens, xs = _batch()
    L, ctx = native.lib(), native.default_context(0)
    data = torch.from_numpy(np.concatenate(xs)).cuda()
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    L.sg_set_profiling(ctx.ptr, 1)
    try:
        ST.time_stretch_batch(data, offs, lens, SR, factor=1.37, **kw)
        st = ST.kernel_ms()
        ST.resample_batch(data, offs, lens, up=3, down=2)
        rs = ST.kernel_ms()
    finally:
        L.sg_set_profiling(ctx.ptr, 0)
    print(st, rs)
    assert st["resample"] == 0 and all(st[k] > 0 for k in ("forward", "vocoder", "inverse", "overlap-add"))
    assert rs["resample"] > 0 and all(rs[k] == 0 for k in ("forward", "vocoder", "inverse", "overlap-add"))
