"""stft(), istft() and invert_spectrogram() (soundgen_beta_amd/invert.py, csrc/sg_invert.h,
csrc/sg_invert.hip): the operator pair (A, A+) and the alternating projections on top.

The rule of every comparison with the GPU, the one tests/test_sine_bank.py and
tests/test_fft64.py use: the measure is the relative 2-norm against the numpy restatement
run in long double, and the bound is 8 times the deviation of the SAME restatement run in
fp64 from the long-double one on the same inputs. The margin covers a different but equally
valid summation order; nothing is taken from the code under test. Every figure is printed
before it is asserted (pytest -s shows them; DESIGN.md section 5 records them).

CPU: the coverage arithmetic of sg_invert.h as a stand-alone program (plain and with
-fsanitize=address,undefined) against brute force; A+ A = I on covered samples in long
double (measured: at most 5.8e-18, 'hanning'); the error of the iteration does not increase;
the refusals, with spectrogram()'s code and text.
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

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundgen_beta_amd", "csrc")
LD = np.longdouble
SR = 16000

# The smallest shapes that reach every branch: windows of 8, 44 (half 2 x 11), 62 (half 2 x 31),
# 96 and 2204 points (half 1102 = 2 x 19 x 29, fft64's folded branch); a sound of wl + 1 samples
# (one frame and an uncovered sample), a few hundred, 6000; a fractional step (20.8 points); a
# step longer than the window (uncovered samples); zero padding; 'hanning' (zero denominators);
# the smallest frame spectrogram() accepts (4 points, half 2); an odd pad, where a packed pair
# (2n - pad, 2n + 1 - pad) straddles the frame's edge, one half a sample and the other a zero:
# pad 1 around 4 points (half 3) and pad 3 around 8 (half 7).
CASES = {
    "w4": dict(n=400, kw=dict(windowLength=0.25)),
    "w4_pad1": dict(n=400, kw=dict(windowLength=0.25, zp=6)),
    "w8_pad3": dict(n=400, kw=dict(windowLength=0.5, zp=14)),
    "w8_one_frame": dict(n=9, kw=dict(windowLength=0.5)),
    "w44_fractional": dict(n=300, kw=dict(windowLength=2.75, step=1.3)),
    "w62_hanning": dict(n=500, kw=dict(windowLength=3.9, wn="hanning")),
    "w96_gap": dict(n=700, kw=dict(windowLength=6, step=7.5)),
    "w96_zp": dict(n=6000, kw=dict(windowLength=6, zp=128)),
    "w2204": dict(n=6000, kw=dict(windowLength=137.75, step=60)),
}
ITER_CASES = ("w44_fractional", "w62_hanning", "w96_zp_short")
CASES_ITER = dict(CASES, w96_zp_short=dict(n=800, kw=dict(windowLength=6, zp=128)))


def rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    cd = np.clongdouble
    return float(np.sqrt((np.abs(got.astype(cd) - want.astype(cd)) ** 2).sum() / (np.abs(want.astype(cd)) ** 2).sum()))


def _tone_noise(n, seed):
    """A tone on noise a fifth as large: no bin of a frame is empty."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return np.sin(2 * np.pi * 1234.5 * t + 0.3) + 0.2 * rng.standard_normal(n)


def _covered(n, kw):
    wl, pad, N, starts, w = IV._setup(n, SR, IV._args(kw), np.float64)
    den = np.zeros(n)
    for s in starts:
        den[s:s + wl] += w * w
    return den != 0


@functools.lru_cache(maxsize=None)
def operator_case(name):
    """The inputs of a case and their restatements, computed once and never written to: the sound, A of
    it (long double and fp64), a random complex matrix with A+ of it (both), the round trip (both)."""
    c = CASES[name]
    n, kw = c["n"], c["kw"]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = _tone_noise(n, rng.integers(1 << 30))
    out = dict(n=n, kw=kw, x=x, covered=_covered(n, kw))
    out["A_ld"] = IV.stft_numpy(x, SR, dtype=LD, **kw)
    out["A_64"] = IV.stft_numpy(x, SR, **kw)
    rows, frames = out["A_ld"].shape
    out["Y"] = rng.standard_normal((rows, frames)) + 1j * rng.standard_normal((rows, frames))
    for r, tag in ((rows, "full"), (rows - 1, "ref")):  # M + 1 rows, and the reference's M
        out["Ainv_ld_" + tag] = IV.istft_numpy(out["Y"][:r], SR, length=n, dtype=LD, **kw)
        out["Ainv_64_" + tag] = IV.istft_numpy(out["Y"][:r], SR, length=n, **kw)
    out["xn_ld"] = IV._normalize(x, LD)
    out["round_64"] = IV.istft_numpy(out["A_64"], SR, length=n, **kw)
    out["round_ld"] = IV.istft_numpy(out["A_ld"], SR, length=n, dtype=LD, **kw)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def iteration_case(name, full, n_iter):
    """Magnitudes (M + 1 rows if full), random initial phases, and the restatement of n_iter
    iterations in long double and in fp64 with the conditioning either met."""
    c = CASES_ITER[name]
    n, kw = c["n"], c["kw"]
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    S = np.abs(IV.stft_numpy(_tone_noise(n, rng.integers(1 << 30)), SR, nyquist=bool(full), **kw))
    ph = rng.uniform(-np.pi, np.pi, S.shape)
    x_ld, e_ld, worst_ld = IV.invert_spectrogram_numpy(S, SR, length=n, nIter=n_iter, phase0=ph, dtype=LD, details=True, **kw)
    x_64, e_64, worst_64 = IV.invert_spectrogram_numpy(S, SR, length=n, nIter=n_iter, phase0=ph, details=True, **kw)
    for v in (S, ph, x_ld, e_ld, x_64, e_64):
        v.setflags(write=False)
    return dict(n=n, kw=kw, S=S, ph=ph, x_ld=x_ld, e_ld=e_ld, x_64=x_64, e_64=e_64, worst=min(worst_ld, worst_64))


# ---- CPU -------------------------------------------------------------------------------------

def _build_pins(tmp_path, sanitize):
    exe = str(tmp_path / ("ola_pins_san" if sanitize else "ola_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "ola_pins.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_coverage_header_on_the_host_equals_brute_force(tmp_path):
    """tests/cpp/ola_pins.cpp: sg_invert.h's first and last covering frame of every sample against
    brute force over wl x len x by (72 geometries), and the sizes by hand; its own program, plain
    and with -fsanitize=address,undefined."""
    exes = [_build_pins(tmp_path, False)]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(_build_pins(tmp_path, True))
    for exe in exes:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert r.stdout.split()[:2] == ["ok", "72"]


# the frame grid alone (sizes only): a step under one point (0.32: equal consecutive starts), and a
# length whose last start is clamped at len - wl (1 + 25 * 17.6 = 441.00000000000006 > 537 - 96);
# the fractional step is w44_fractional's
GRID_CASES = {
    "w44_equal_starts": dict(n=300, kw=dict(windowLength=2.75, step=0.02)),
    "w96_clamped": dict(n=537, kw=dict(windowLength=6, step=1.1)),
}


def test_header_and_restatement_agree_on_frames():
    """sg_invert_size (host only) against the restatement's frame count and sizes."""
    st = IV._starts(300, SR, 44, 0.02)
    assert len(st) == 797 and np.all(np.diff(st) >= 0) and (np.diff(st) == 0).sum() > 500
    st = IV._starts(537, SR, 96, 1.1)
    assert st[-1] == 537 - 96 - 1 and 1.0 + (len(st) - 1) * (1.1 / 1000 * SR) > 537 - 96
    for name, c in dict(CASES, **GRID_CASES).items():
        z = IV.invert_size(c["n"], SR, **c["kw"])
        wl, pad, N, starts, _ = IV._setup(c["n"], SR, IV._args(c["kw"]), np.float64)
        assert (z["wl"], z["N"], z["bins"], z["frames"], z["samples"]) == (wl, N, N // 2, len(starts), c["n"]), name
        assert z["workspace_bytes"] == len(starts) * ((N // 2 + 1) * 16 + wl * 8 + 16)
        assert IV.min_length(len(starts), SR, **c["kw"]) <= c["n"]
        assert len(IV._starts(IV.min_length(len(starts), SR, **c["kw"]), SR, wl, IV._geometry(SR, IV._args(c["kw"]))[3])) == len(starts)


@pytest.mark.parametrize("name", list(CASES))
def test_synthesis_left_inverts_analysis_in_long_double(name):
    """A+ A = I on covered samples: nothing but long-double rounding is left (measured: 2.0e-19
    .. 5.8e-18, the largest with 'hanning', whose smallest non-zero denominator is w[1]^2 = 7e-6).
    The bound, 2^-52 / 4, is a quarter of what one fp64 rounding would leave: an operator that is
    a left inverse only to fp64 accuracy cannot pass. Uncovered samples are 0."""
    c = operator_case(name)
    cov = c["covered"]
    d = rel(c["round_ld"][cov], c["xn_ld"][cov])
    print("A+ A - I, long double, %s: %.3g (%d of %d samples uncovered)" % (name, d, int((~cov).sum()), c["n"]))
    assert d <= 2.0 ** -52 / 4
    assert np.all(c["round_ld"][~cov] == 0) and np.all(c["round_64"][~cov] == 0)
    if name in ("w8_one_frame", "w96_gap", "w62_hanning"):
        assert (~cov).sum() > 0
    # the fp64 restatement of A is spectrogram_numpy's matrix under the modulus
    assert rel(np.abs(c["A_64"])[:-1], SP.spectrogram_numpy(c["x"], SR, output="original", **c["kw"])) <= 8 * rel(c["A_64"], c["A_ld"])


def test_restatement_error_does_not_increase():
    """M rows and random phases, 20 iterations: e_k of the long-double restatement does not
    increase beyond 8 times the largest increase the fp64 one shows (none: 0), and falls."""
    for name in ITER_CASES:
        c = iteration_case(name, False, 20)
        slack = 8 * max(0.0, float(np.diff(c["e_64"]).max()))
        print("restatement, %s: e_1 %.4g e_20 %.4g, largest step %.3g (fp64 %.3g)"
              % (name, c["e_ld"][0], c["e_ld"][-1], float(np.diff(c["e_ld"]).max()), float(np.diff(c["e_64"]).max())))
        assert np.all(np.diff(c["e_ld"]) <= slack) and c["e_ld"][-1] < c["e_ld"][0]
        assert np.all(np.diff(c["e_64"]) <= slack)


REFUSALS = [dict(windowLength=4.7), dict(windowLength=300), dict(windowLength=6, zp=10000), dict(windowLength=0.1)]


@pytest.mark.parametrize("kw", REFUSALS, ids=["half_37", "window_4800", "zp_10000", "window_2"])
def test_refusals_are_spectrograms(kw):
    """A window whose half is not 31-smooth or is above 2048, zp past 4096, a window under 4 points:
    spectrogram()'s code and text from sg_invert_size, and the code from the three entry points with
    ctx = NULL and no buffers -- raised before the context is looked at, let alone a launch."""
    with pytest.raises(native.SoundgenError) as want:
        SP.spectrogram_size_native(1000, SR, **kw)
    with pytest.raises(native.SoundgenError) as got:
        IV.invert_size(1000, SR, **kw)
    assert got.value.code == want.value.code == -4 and str(got.value) == str(want.value)
    L = native.lib()
    P = IV._params(SR, IV._args(kw))
    assert L.sg_spg_stft_batch(None, None, 0, None, None, 1, C.byref(P), 48, None, None) == -4
    assert L.sg_spg_istft_batch(None, None, None, None, 1, C.byref(P), 48, None, None) == -4
    assert L.sg_invert_spectrogram_batch(None, None, None, None, None, 1, C.byref(P), 48, 3, 0, None, None, None) == -4


def test_own_refusals_without_a_context():
    L = native.lib()
    P = IV._params(SR, IV._args(dict(windowLength=6)))  # 96 points, 48 bins
    for rows in (47, 50):  # SG_E_ARG (a good row count would be refused for its missing context with the same code)
        assert L.sg_spg_istft_batch(None, None, None, None, 1, C.byref(P), rows, None, None) == -1
    with pytest.raises(native.SoundgenError) as e:
        IV.invert_size(1000, SR, rows=50, windowLength=6)
    assert e.value.code == -1 and "48" in str(e.value) and "49" in str(e.value)
    assert IV.invert_size(1000, SR, rows=49, windowLength=6)["frames"] == IV.invert_size(1000, SR, windowLength=6)["frames"]
    with pytest.raises(TypeError):
        IV.invert_size(1000, SR, windowLenght=6)
    with pytest.raises(ValueError):
        IV.invert_spectrogram_numpy(-np.ones((48, 3)), SR, windowLength=6)
    with pytest.raises(ValueError):
        IV.istft_numpy(np.ones((50, 3)), SR, windowLength=6)


def test_size_error_text_lasts_until_the_next_host_only_call():
    """The readers of the host-only entry points share one text per thread: a refused sg_invert_size
    leaves its text, and the next host-only call (a sg_spectrogram_size that succeeds) clears it."""
    L = native.lib()
    with pytest.raises(native.SoundgenError):
        IV.invert_size(1000, SR, windowLength=4.7)
    text = L.sg_invert_size_error().decode()
    assert "37" in text and text.startswith("spectrogram: a frame of")
    assert SP.spectrogram_size_native(1000, SR, windowLength=6)[0] == 96
    assert L.sg_invert_size_error() == b"" and L.sg_spectrogram_size_error() == b""


# ---- GPU -------------------------------------------------------------------------------------

def _check(what, got, want_ld, fp64):
    dev = rel(fp64, want_ld)
    err = rel(got, want_ld)
    print("%s: GPU %.3g, fp64 restatement %.3g, bound %.3g" % (what, err, dev, 8 * dev))
    assert err <= 8 * dev, what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_stft_istft_and_round_trip(name):
    c = operator_case(name)
    n, kw, cov = c["n"], c["kw"], c["covered"]
    X = IV.stft(c["x"], SR, **kw)
    assert X.shape == c["A_ld"].shape and X.dtype == np.complex128
    _check("stft " + name, X, c["A_ld"], c["A_64"])
    M = X.shape[0] - 1
    assert np.array_equal(IV.stft(c["x"], SR, nyquist=False, **kw), X[:M])
    dev = rel(np.abs(c["A_64"])[:M], np.abs(c["A_ld"])[:M])
    err = rel(np.abs(X)[:M], SP.spectrogram(c["x"], SR, output="original", **kw))
    print("|stft| against spectrogram(output = 'original') %s: %.3g, bound %.3g" % (name, err, 8 * dev))
    assert err <= 8 * dev
    for r, tag in ((M + 1, "full"), (M, "ref")):
        y = IV.istft(c["Y"][:r], SR, length=n, **kw)
        assert y.shape == (n,)
        _check("istft (%d rows) %s" % (r, name), y, c["Ainv_ld_" + tag], c["Ainv_64_" + tag])
        assert np.all(y[~cov] == 0)  # uncovered, or under window zeros only: 0 exactly
    back = IV.istft(X, SR, length=n, **kw)
    _check("round trip " + name, back[cov], c["xn_ld"][cov], c["round_64"][cov])
    assert np.all(back[~cov] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("name", ITER_CASES)
def test_iterations_against_restatement(name, n_iter):
    """The sound and e_1 .. e_k after one and after three iterations, M rows and M + 1, on tone-plus-
    noise magnitudes whose conditioning is asserted here, not skipped: every constrained |Z| met
    is at least 1e-6 of its iteration's largest (tests/test_analyze_sweep.py's margin convention)."""
    for full in (False, True):
        c = iteration_case(name, full, n_iter)
        assert c["worst"] >= 1e-6, c["worst"]
        x, e = IV.invert_spectrogram(c["S"], SR, length=c["n"], nIter=n_iter, phase0=c["ph"], return_error=True, **c["kw"])
        tag = "%s, %d iteration(s), %s rows" % (name, n_iter, "M + 1" if full else "M")
        _check("sound " + tag, x, c["x_ld"], c["x_64"])
        _check("errors " + tag, e, c["e_ld"], c["e_64"])


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["M", "M+1"])
def test_error_is_monotone_over_30_iterations(full):
    for name in ITER_CASES:
        c = iteration_case(name, full, 30)
        slack = 8 * max(0.0, float(np.diff(c["e_64"]).max()))
        _, e = IV.invert_spectrogram(c["S"], SR, length=c["n"], nIter=30, phase0=c["ph"], return_error=True, **c["kw"])
        print("%s, %s rows: e_1 %.6g e_30 %.6g, largest step %.3g, slack %.3g (restatement e_30 %.6g)"
              % (name, "M + 1" if full else "M", e[0], e[-1], float(np.diff(e).max()), slack, c["e_64"][-1]))
        assert np.all(np.diff(e) <= slack)
        assert e[-1] < e[0]


def _batch():
    """Five matrices of three geometries' worth of lengths under one setting, on the host."""
    kw = dict(windowLength=6, step=2.3)
    lens = [97, 700, 96, 1500, 333]
    rng = np.random.default_rng(11)
    mats = [np.abs(IV.stft_numpy(_tone_noise(n, 100 + i), SR, nyquist=False, **kw)) for i, n in enumerate(lens)]
    phs = [rng.uniform(-np.pi, np.pi, m.shape) for m in mats]
    return kw, lens, mats, phs


def _pack(mats):
    import torch
    flat = np.concatenate([np.ascontiguousarray(m.T).ravel() for m in mats])
    offs = np.concatenate([[0], np.cumsum([m.size for m in mats])])[:-1]
    return torch.from_numpy(flat).cuda(), offs, [m.shape for m in mats]


@pytest.mark.gpu
def test_batch_equals_singles_bit_for_bit():
    """A sound's samples and errors alone, in a batch, in the reversed batch, and under three
    workspace caps from sg_invert_size: one sound a chunk, two of the largest, no cap."""
    kw, lens, mats, phs = _batch()
    single = [IV.invert_spectrogram(m, SR, length=n, nIter=4, phase0=p, return_error=True, **kw)
              for m, n, p in zip(mats, lens, phs)]
    need = [IV.invert_size(n, SR, **kw)["workspace_bytes"] for n in lens]
    for order in (list(range(5)), list(range(4, -1, -1))):
        d_mag, offs, shapes = _pack([mats[i] for i in order])
        d_ph, _, _ = _pack([phs[i] for i in order])
        for cap in (1, 2 * max(need), 0):
            out, err = IV.invert_spectrogram_batch(d_mag, offs, shapes, SR, lengths=[lens[i] for i in order], nIter=4,
                                                   phase0=d_ph, workspace_cap=cap, to_host=True, **kw)
            for k, i in enumerate(order):
                assert np.array_equal(out[k], single[i][0]), (order, cap, i)
                assert np.array_equal(err[k], single[i][1]), (order, cap, i)


@pytest.mark.gpu
def test_spectrogram_batch_hands_over_in_hbm():
    """spectrogram_batch's (out, offsets, shapes) go into invert_spectrogram_batch as they are:
    no host copy in between, and the same bits as the single call on the copied matrix. One sound
    is shorter than the window: no frames, a silent result. rng draws R's runif() phases."""
    import torch
    from soundgen_beta_amd.rrng import RRng
    kw = dict(windowLength=6, step=2.3)
    lens = [1200, 50, 801]
    x = np.concatenate([_tone_noise(n, 40 + i) for i, n in enumerate(lens)]).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    data = torch.from_numpy(x).cuda()
    mag, moff, shapes = SP.spectrogram_batch(data, offs, lens, SR, output="original", **kw)
    assert mag.is_cuda and shapes[1] == (48, 0)
    out, ooff, err = IV.invert_spectrogram_batch(mag, moff, shapes, SR, lengths=lens, nIter=3, rng=RRng(1), **kw)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64 and err.shape == (3, 3)
    h, hm = out.cpu().numpy(), mag.cpu().numpy()
    ph = IV.r_phases(RRng(1), shapes)
    assert np.all((ph >= -np.pi) & (ph <= np.pi)) and len(ph) == sum(r * f for r, f in shapes)
    k = 0
    for i, (r, f) in enumerate(shapes):
        if f == 0:
            assert np.all(h[ooff[i]:ooff[i] + lens[i]] == 0) and np.all(np.isnan(err[i]))
            continue
        S = hm[moff[i]:moff[i] + r * f].reshape(f, r).T
        want, e = IV.invert_spectrogram(S, SR, length=lens[i], nIter=3, phase0=ph[k:k + r * f].reshape(f, r).T,
                                        return_error=True, **kw)
        k += r * f
        assert np.array_equal(h[ooff[i]:ooff[i] + lens[i]], want) and np.array_equal(err[i], e)
    # stft_batch and istft_batch the same way: fp32 sounds in, spectra and sounds stay in HBM
    spec, soff, sshapes = IV.stft_batch(data, offs, lens, SR, **kw)
    assert spec.is_cuda and spec.dtype == torch.complex128 and sshapes == [(49, s[1]) for s in shapes]
    back, boff = IV.istft_batch(spec, soff, sshapes, SR, lengths=lens, **kw)
    hb = back.cpu().numpy()
    x0 = x[:1200].astype(np.float64)
    assert np.array_equal(hb[boff[0]:boff[0] + 1200], IV.istft(IV.stft(x0, SR, **kw), SR, length=1200, **kw))
    assert np.all(hb[boff[1]:boff[1] + 50] == 0)
    with pytest.raises(native.SoundgenError) as bad:
        IV.invert_spectrogram_batch(-mag, moff, shapes, SR, lengths=lens, nIter=1, **kw)
    assert bad.value.code == -1


@pytest.mark.gpu
def test_stage_clock_reports_every_stage():
    kw, lens, mats, phs = _batch()
    L = native.lib()
    ctx = native.default_context(0)
    d_mag, offs, shapes = _pack(mats)
    L.sg_set_profiling(ctx.ptr, 1)
    try:
        IV.invert_spectrogram_batch(d_mag, offs, shapes, SR, lengths=lens, nIter=2, **kw)
        few = IV.kernel_ms()
        IV.invert_spectrogram_batch(d_mag, offs, shapes, SR, lengths=lens, nIter=40, **kw)
        many = IV.kernel_ms()
        IV.stft(_tone_noise(700, 1), SR, **kw)
        fwd = IV.kernel_ms()
    finally:
        L.sg_set_profiling(ctx.ptr, 0)
    print(few, many, fwd)
    for k in ("forward", "start", "inverse", "overlap-add", "error fold"):
        assert few[k] > 0 and many[k] > 0, k
    assert few["statistics"] == 0 and fwd["statistics"] > 0 and fwd["forward"] > 0 and fwd["inverse"] == 0
    for k in ("forward", "inverse", "overlap-add", "error fold"):  # 40 (41) launches against 2 (3)
        assert many[k] > 4 * few[k], k
