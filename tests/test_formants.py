"""analyze()'s formant tracks (soundgen_beta_amd/formants.py, csrc/sg_formants.h, sg_formants.hip):
phonTools::findformants restated (unpinned against R), on the host in fp64 and long double and on the
GPU. The long-double restatement is the reference of every comparison; the bound of the GPU tests is
measured from the fp64 restatement's own deviation from it (test_bound_is_measured)."""
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from soundgen_beta_amd import analyze as A
from soundgen_beta_amd import formants as F
from soundgen_beta_amd import native
from soundgen_beta_amd.spectrogram import ft_window

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
LD = np.longdouble

# (fs, frame length): the orders 11, 19, 47, 51 and 63 (the last that leaves a lane idle; 60400 Hz gives 63 too:
# round(60.4) is 60), 64 (no idle lane: 61000 Hz), and a length that is no multiple of 4 or 256 for the lag kernel's
# tails
FRAME_CASES = ((8000, 160), (16000, 320), (44100, 442), (48000, 480), (60000, 600), (60400, 604), (61000, 610),
               (16000, 333))
# seeds for which the long-double restatement finds the margins of test_gpu_inputs_are_well_conditioned
FRAME_SEEDS = {(60000, 600): 1}
N_FRAMES = 7
# end to end: (samplingRate, seed); windowLength = 20 ms
SOUND_CASES = ((16000, 5), (44100, 2), (16000, 11))
SOUND_KW = dict(windowLength=20)
GPU_FACTOR = 8  # the GPU may deviate from the long-double restatement by 8 x the fp64 restatement's deviation


def resonate(x, fs, freq, bw):
    """x through the two-pole resonator with a pole pair at (freq, bw)."""
    r = math.exp(-math.pi * bw / fs)
    c1, c2 = 2 * r * math.cos(2 * math.pi * freq / fs), -r * r
    y = np.zeros(len(x))
    for i in range(len(x)):
        y[i] = x[i] + c1 * (y[i - 1] if i > 0 else 0.0) + c2 * (y[i - 2] if i > 1 else 0.0)
    return y


def voiced(fs, n, rng, wide=False):
    """A harmonic source through three resonances, peak 1, plus noise at 1e-2 of the peak. wide: the
    resonances' bandwidths lie around phonTools' 600 Hz limit, so that fewer roots are kept."""
    lead = 256
    t = np.arange(n + lead) / fs
    f0 = rng.uniform(90, 220)
    src = np.zeros(n + lead)
    for k in range(1, int(0.45 * fs / f0) + 1):
        src += np.cos(2 * math.pi * k * f0 * t + rng.uniform(0, 2 * math.pi)) / k
    top = min(0.42 * fs, 3600.0)
    for lo, hi in ((0.08, 0.25), (0.33, 0.62), (0.72, 1.0)):
        bw = rng.uniform(450, 900) if wide else rng.uniform(50, 150)
        src = resonate(src, fs, rng.uniform(lo * top, hi * top), bw)
    x = src[lead:]
    x = x / np.abs(x).max()
    return x + 1e-2 * rng.standard_normal(n)


def hum(fs, n, rng):
    """A loud 100 Hz hum in noise: its only narrow root lies below phonTools' 200 Hz floor."""
    return 0.8 * np.cos(2 * math.pi * 100 * np.arange(n) / fs + 1.0) + 1e-2 * rng.standard_normal(n)


def onset(fs, n, rng):
    """The hum setting in halfway through a quiet frame, as in the sounds of the end-to-end cases: few roots or
    none are kept."""
    return np.concatenate([1e-3 * rng.standard_normal(n // 2), hum(fs, n - n // 2, rng)])


@functools.lru_cache(maxsize=None)
def frame_case(fs, n):
    """N_FRAMES frames, Gaussian-windowed as getFrameBank does: voiced ones, the last but one with wide
    resonances, the last an onset, which keeps fewer rows than the others."""
    rng = np.random.default_rng(1000 + fs + n + FRAME_SEEDS.get((fs, n), 0))
    w = ft_window(n, "gaussian")
    fr = np.stack([voiced(fs, n, rng, wide=i == N_FRAMES - 2) * w for i in range(N_FRAMES - 1)] + [onset(fs, n, rng) * w])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def frame_reference(fs, n):
    """Per frame of the case, the long-double restatement (raw) and the fp64 one."""
    fr = frame_case(fs, n)
    return tuple((F.find_formants_numpy(x, fs, dtype=LD, raw=True), F.find_formants_numpy(x, fs, raw=True)) for x in fr)


def case_nformants(refs):
    """nFormants of a case, decided by the reference alone: the largest kept count over its frames (at most 8),
    so that one frame fills the row and, where the counts differ, another leaves NA."""
    return min(F.MAX_FORMANTS, max(len(ld["kept"]) for ld, _ in refs))


@functools.lru_cache(maxsize=None)
def sound_case(sr, seed):
    """About 0.15 s: a voiced stretch, a quiet one (its frames fail cond_silence), and a loud 100 Hz hum in noise,
    whose only narrow root lies below phonTools' 200 Hz floor."""
    rng = np.random.default_rng(seed)
    n1, n2, n3 = int(0.07 * sr), int(0.035 * sr), int(0.045 * sr)
    x = np.concatenate([voiced(sr, n1, rng), 1e-3 * rng.standard_normal(n2), hum(sr, n3, rng)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sound_reference(sr, seed):
    """formants_numpy's frames and gate, and per analysed frame the two restatements (raw)."""
    probe = {}
    F.formants_numpy(sound_case(sr, seed), sr, nFormants=8, _probe=probe, **SOUND_KW)
    fr = probe["frames"]
    refs = {int(f): (F.find_formants_numpy(fr[:, f], sr, dtype=LD, raw=True), F.find_formants_numpy(fr[:, f], sr, raw=True))
            for f in probe["analysed"]}
    return fr.shape[1], refs


def table_from(refs, frames, nFormants, which):
    """The frames x 2 nFormants table of a sound from the per-frame restatements (0: long double, 1: fp64)."""
    m = np.full((frames, 2 * nFormants), math.nan)
    for f, pair in refs.items():
        m[f] = F._rows(pair[which]["kept"], nFormants)
    return m


def all_reference_pairs():
    for fs, n in FRAME_CASES:
        yield ("frames", fs, n), list(frame_reference(fs, n))
    for sr, seed in SOUND_CASES:
        yield ("sound", sr, seed), list(sound_reference(sr, seed)[1].values())


def deviation(ld, other):
    """(Hz in the unrounded frequencies, Hz in the bandwidths) between two raw restatements of a frame, over the
    roots the long-double one keeps, matched by rank."""
    if ld["failed"] or other["failed"] or len(ld["keep"]) != len(other["keep"]):
        return math.inf, math.inf
    df = np.abs(other["freq"][other["keep"]].astype(LD) - ld["freq"][ld["keep"]])
    db = np.abs(other["bandwidth"][other["keep"]].astype(LD) - ld["bandwidth"][ld["keep"]])
    return (float(df.max()), float(db.max())) if len(df) else (0.0, 0.0)


@functools.lru_cache(maxsize=None)
def measured_bound():
    """The largest deviation of the fp64 restatement from the long-double one over every analysed frame of
    every GPU case: (Hz in frequency, Hz in bandwidth)."""
    df = db = 0.0
    for _, pairs in all_reference_pairs():
        for ld, d in pairs:
            a, b = deviation(ld, d)
            df, db = max(df, a), max(db, b)
    return df, db


def assert_table_within(got, ref_ld, what):
    """got against the long-double table: the same NaN pattern, rounded frequencies equal exactly, bandwidths within
    GPU_FACTOR x the measured fp64 deviation. The frequency bound holds with them: a rounded frequency is a
    function of the unrounded one, whose margin test_gpu_inputs_are_well_conditioned checks."""
    _, bb = measured_bound()
    assert got.shape == ref_ld.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref_ld)), what
    ok = ~np.isnan(ref_ld)
    fcols = np.zeros(got.shape, bool)
    fcols[:, 0::2] = True
    assert np.array_equal(got[ok & fcols], ref_ld[ok & fcols]), what
    dev = np.abs(got[ok & ~fcols] - ref_ld[ok & ~fcols])
    print("%s: largest bandwidth deviation %.3g Hz (bound %.3g Hz)" % (what, dev.max() if len(dev) else 0.0, GPU_FACTOR * bb))
    assert np.all(dev <= GPU_FACTOR * bb), (what, float(dev.max()), GPU_FACTOR * bb)


# ---------------------------------------------------------------- CPU
def poly_from_pairs(pairs, fs, extra_real=()):
    """a1..ap of the monic polynomial with a conjugate pole pair per (frequency, bandwidth) and the real roots."""
    roots = []
    for f, bw in pairs:
        z = math.exp(-math.pi * bw / fs) * np.exp(1j * 2 * math.pi * f / fs)
        roots += [z, np.conj(z)]
    roots += list(extra_real)
    return np.real(np.poly(roots))[1:]


def test_by_hand():
    """Two chosen pole pairs come back as (frequency, bandwidth) to 1e-12 relative; a pair with bandwidth 700,
    a pair at 150 Hz and a real root are dropped. Then the 150 Hz case at 10 kHz, where the pair lies so close to
    its conjugate that the corrections stay at the rounding noise of P / P', above 4 eps |z|: the rule
    |w| <= 4 eps |z| alone passed only by chance, after 112 steps in fp64 and not within 300 in long double; with
    the noise rule of fmt_aberth_step the roots settle in 11 and 12 steps."""
    for dtype in (np.float64, LD):
        got = F.formants_from_coeffs(poly_from_pairs([(700.0, 80.0), (150.0, 60.0)], 10000.0), 10000.0, dtype=dtype, raw=True,
                                     max_iter=F.MAX_ITER)
        assert not got["failed"] and got["iterations"] <= 16, got["iterations"]
        assert got["kept"].shape == (1, 2) and got["kept"][0, 0] == 700.0 and abs(got["kept"][0, 1] - 80.0) <= 1e-12 * 80.0
    fs = 4000.0
    a = poly_from_pairs([(700.0, 80.0), (1800.0, 120.0)], fs)
    assert len(a) == 4
    got = F.formants_from_coeffs(a, fs, raw=True)
    assert not got["failed"]
    want = np.array([[700.0, 80.0], [1800.0, 120.0]])
    assert got["kept"].shape == (2, 2)
    assert np.all(np.abs(got["freq"][got["keep"]] - want[:, 0]) <= 1e-12 * want[:, 0])
    assert np.all(np.abs(got["kept"][:, 1] - want[:, 1]) <= 1e-12 * want[:, 1])
    assert np.array_equal(got["kept"][:, 0], want[:, 0])  # round(f, 2)
    for pairs, real in (([(700.0, 80.0), (1800.0, 700.0)], ()),      # bandwidth 700 >= maxbw
                        ([(700.0, 80.0), (150.0, 60.0)], ()),        # 150 Hz <= minformant
                        ([(700.0, 80.0)], (0.9, -0.8))):             # real roots: 0 Hz and fs / 2
        got = F.formants_from_coeffs(poly_from_pairs(pairs, fs, real), fs)
        assert got.shape == (1, 2)
        assert got[0, 0] == 700.0 and abs(got[0, 1] - 80.0) <= 1e-12 * 80.0
    # the long-double route agrees
    got = F.formants_from_coeffs(a, fs, dtype=LD)
    assert np.all(np.abs(got - want) <= 1e-12 * want)


def test_levinson_against_solve():
    """'LU and Levinson-Durbin agree far below everything else in the chain': on the lags of every frame of
    the frame cases, each one's deviation from the long-double Levinson-Durbin (the largest over a frame's
    coefficients, relative to the largest coefficient), the largest over all frames: one value each.
    Levinson's must lie within 4 x the solve's.
    Measured here: Levinson 8.3e-14, solve 2.1e-14. Frame by frame the ratio of the two varies more: in
    its worst frame (48 kHz) Levinson deviates by 4.3e-14 and the solve by 8.3e-15."""
    worst_lev = worst_lu = 0.0
    for fs, n in FRAME_CASES:
        order = F.formant_order(fs)
        for x in frame_case(fs, n):
            r = F.lpc_lags(x, fs, order)
            ref = F.levinson(r.astype(LD), LD)
            scale = float(np.abs(ref).max())
            lev = float(np.abs(F.levinson(r) - ref).max()) / scale
            lu = float(np.abs(F.toeplitz_solve(r) - ref).max()) / scale
            print("%d/%d: Levinson %.3g, solve %.3g" % (fs, n, lev, lu))
            worst_lev, worst_lu = max(worst_lev, lev), max(worst_lu, lu)
    print("Levinson %.3g, solve %.3g" % (worst_lev, worst_lu))
    assert worst_lev <= 4 * worst_lu, (worst_lev, worst_lu)


def test_gpu_inputs_are_well_conditioned():
    """Every analysed frame of every GPU case (the share left out is 0), in the long-double restatement alone:
    the iteration converges; every root's bandwidth is 1e-6 relative away from 600 and its frequency from 200
    and fs / 2, or the root is far outside; 100 f is 1e-4 away from every half-integer; the kept roots'
    rounded frequencies are pairwise distinct; and every case has a frame with at least nFormants kept rows and
    one with fewer. Far outside: dropped by another of the three criteria with that margin, or a real root
    (|Im z| <= 1e-12 |z|, which an odd order always has): the polynomial is real, so whatever rounding leaves in
    Im z, its frequency rounds to 0 or +-fs / 2 and it is dropped; the half-integer margin covers that rounding."""
    for case, pairs in all_reference_pairs():
        counts = []
        fs = case[1]
        for ld, _ in pairs:
            assert not ld["failed"], case
            f, bw, z = ld["freq"], ld["bandwidth"], ld["roots"]
            m_bw, m_lo, m_hi = np.abs(bw - 600) >= 1e-6 * 600, np.abs(f - 200) >= 1e-6 * 200, np.abs(f - fs / LD(2)) >= 1e-6 * fs / 2
            out_bw, out_lo, real = (bw > 600) & m_bw, (f < 200) & m_lo, np.abs(z.imag) <= 1e-12 * np.abs(z)
            assert np.all(real | ((m_bw | out_lo) & (m_lo | out_bw) & (m_hi | out_bw | out_lo))), case
            h = 100 * f - LD(0.5)
            assert np.all(np.abs(h - np.rint(h)) >= 1e-4), case
            kept = ld["kept"][:, 0]
            assert len(set(kept.tolist())) == len(kept), case
            counts.append(len(kept))
        nF = (case_nformants(pairs),) if case[0] == "frames" else (1, 3, 8)
        for k in nF:
            assert max(counts) >= k and min(counts) < k, (case, k, counts)


def test_bound_is_measured():
    """The bound of the GPU tests: the largest deviation of the fp64 restatement from the long-double one over
    every analysed frame of every GPU case. Measured here: 6.1e-11 Hz in frequency, 8.4e-11 Hz in bandwidth (see
    DESIGN.md section 5 for the GPU's). The fp64 restatement itself must keep the same roots."""
    df, db = measured_bound()
    print("fp64 against long double: %.3g Hz in frequency, %.3g Hz in bandwidth" % (df, db))
    assert math.isfinite(df) and math.isfinite(db)
    assert 0 < df < 1e-6 and 0 < db < 1e-6  # far below round(f, 2)'s step: the inputs' own sensitivity


def _dump(path, frames, fs, nFormants):
    head = np.array([frames.shape[0], frames.shape[1], fs, nFormants], dtype=np.float64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(np.ascontiguousarray(frames, dtype=np.float64).tobytes())


def _run_pins(exe, path, nFormants):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [line.split() for line in r.stdout.strip().splitlines()]
    return np.array([int(v[0]) for v in rows]), np.array([[float(x) for x in v[1:]] for v in rows]).reshape(len(rows), 2 * nFormants)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_host_pins(tmp_path, flags):
    """The host build of sg_formants.h (a stand-alone program, run directly) on the frame cases' frames against
    the long-double restatement, held to the bound of the GPU tests; built once more with the address and
    undefined-behaviour sanitizers."""
    exe = str(tmp_path / "formant_pins")
    subprocess.run(["g++", "-std=c++17", *flags, "-I" + CSRC, os.path.join(HERE, "cpp", "formant_pins.cpp"), "-o", exe],
                   check=True, timeout=300)
    for fs, n in FRAME_CASES:
        refs = frame_reference(fs, n)
        nF = case_nformants(refs)
        path = str(tmp_path / ("frames_%d_%d.bin" % (fs, n)))
        _dump(path, frame_case(fs, n), fs, nF)
        it, got = _run_pins(exe, path, nF)
        assert np.all(it > 0) and np.all(it < F.MAX_ITER), (fs, n, it)
        want = np.stack([F._rows(ld["kept"], nF) for ld, _ in refs])
        assert_table_within(got, want, "host pins %d/%d" % (fs, n))


def test_refusals_on_the_host():
    for fs in (61600, 96000):  # orders 65 and 99
        with pytest.raises(native.SoundgenError) as e:
            F.formants_size(A.repair(fs), 3)
        assert e.value.code == -4
    assert F.formants_size(A.repair(61000, windowLength=21), 3) == (64, 6)  # 1280 points: a window the gate can transform
    assert F.formants_size(A.repair(44100), 8) == (47, 16)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            F.formants_size(A.repair(44100), bad)
        with pytest.raises(ValueError):
            F.formants_numpy(np.zeros(4000), 16000, nFormants=bad)
    with pytest.raises(native.SoundgenError):
        F.formants_numpy(np.zeros(8000), 61600)


def test_half_even_order():
    assert [F.formant_order(fs) for fs in (8000, 16000, 22050, 44100, 48000, 60000, 60400, 60500, 61000, 61500, 62500)] == \
        [11, 19, 25, 47, 51, 63, 63, 63, 64, 65, 65]


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("fs,n", FRAME_CASES)
def test_frames_hook(fs, n):
    """sg_formants_frames against the long-double restatement: the same NaN pattern, every rounded frequency
    equal, bandwidths within 8 x the fp64 restatement's own deviation (8.4e-11 Hz, so 6.7e-10 Hz), no frame
    at the iteration cap. Measured on the MI355X: at most 6.7e-11 Hz (48 kHz, order 51); 7.4 (order 11) to
    11.0 (order 63) Aberth steps per frame."""
    refs = frame_reference(fs, n)
    nF = case_nformants(refs)
    got = F.find_formants_frames(frame_case(fs, n), fs, nF)
    capped, analysed, iters = F.formants_counts()
    print("order %d: %d frames, %.1f iterations per frame" % (F.formant_order(fs), analysed, iters / max(analysed, 1)))
    assert capped == 0 and analysed == N_FRAMES
    assert_table_within(got, np.stack([F._rows(ld["kept"], nF) for ld, _ in refs]), "frames hook %d/%d" % (fs, n))


@pytest.mark.gpu
@pytest.mark.parametrize("nFormants", [1, 3, 8])
@pytest.mark.parametrize("sr,seed", SOUND_CASES)
def test_end_to_end(sr, seed, nFormants):
    """formants() against formants_numpy(): the same NaN pattern (frames that fail cond_silence, rows past the
    kept count), values within the bound of test_frames_hook. Measured on the MI355X: at most 7.0e-11 Hz."""
    x = sound_case(sr, seed)
    frames, refs = sound_reference(sr, seed)
    assert 0 < len(refs) < frames  # some frames fail the gate
    got = F.formants(x, sr, nFormants=nFormants, **SOUND_KW)
    assert F.formants_counts()[0] == 0
    m = np.stack([got[k] for k in F.formant_columns(nFormants)], axis=1)
    host = F.formants_numpy(x, sr, nFormants=nFormants, **SOUND_KW)
    h = np.stack([host[k] for k in F.formant_columns(nFormants)], axis=1)
    assert np.array_equal(np.isnan(m), np.isnan(h))
    assert_table_within(m, table_from(refs, frames, nFormants, 0), "end to end %d/%d/%d" % (sr, seed, nFormants))
    assert_table_within(h, table_from(refs, frames, nFormants, 0), "formants_numpy %d/%d/%d" % (sr, seed, nFormants))


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [16000, 44100])
def test_batch_equals_single(sr):
    """Every sound's table in a batch equals its single-sound table bit for bit, at two different positions (call
    index and sample offset) of the batch, next to a sound not longer than the window (no rows) and a failed
    call (length < 0), which move too."""
    import torch
    sounds = [sound_case(s, seed) for s, seed in SOUND_CASES if s == sr]
    # the batch reads float32 samples: compare against the single sound of the same samples
    single = [F.formants(x.astype(np.float32).astype(np.float64), sr, nFormants=3, **SOUND_KW) for x in sounds]
    assert all(len(t["f1_freq"]) > 0 for t in single)
    short = np.full(int(0.02 * sr), 0.5)
    rev = list(reversed(range(len(sounds))))
    # a layout: sound indices, "short" and "failed" in call order
    layouts = (["short"] + list(range(len(sounds))) + ["failed"], [rev[0], "failed"] + rev[1:] + ["short"])
    seen = {i: set() for i in range(len(sounds))}
    for layout in layouts:
        parts, offs, lens = [], [], []
        for what in layout:
            offs.append(sum(len(q) for q in parts))
            if what == "failed":
                lens.append(-1)
                continue
            parts.append(short if what == "short" else sounds[what])
            lens.append(len(parts[-1]))
        data = torch.from_numpy(np.concatenate(parts).astype(np.float32)).cuda()
        got = F.formants_batch(data, offs, lens, sr, nFormants=3, to_host=True, **SOUND_KW)
        assert len(got) == len(layout)
        for j, what in enumerate(layout):
            if isinstance(what, str):
                assert len(got[j]["f1_freq"]) == 0, (layout, what)
                continue
            seen[what].add((j, offs[j]))
            for k in F.formant_columns(3):
                assert np.array_equal(got[j][k], single[what][k], equal_nan=True), (layout, what, k)
    for i, where in seen.items():
        (j0, o0), (j1, o1) = sorted(where)
        assert j0 != j1 and o0 != o1, (i, where)


@pytest.mark.gpu
def test_analyze_with_formants():
    sr, seed = SOUND_CASES[0]
    x = sound_case(sr, seed)
    base = A.analyze(x, sr, **SOUND_KW)
    both = A.analyze(x, sr, formants=True, nFormants=3, **SOUND_KW)
    fm = F.formants(x, sr, nFormants=3, **SOUND_KW)
    assert set(both) == set(base) | set(F.formant_columns(3))
    for k in base:
        assert np.array_equal(both[k], base[k], equal_nan=True), k
    for k in fm:
        assert np.array_equal(both[k], fm[k], equal_nan=True), k
    assert np.any(~np.isnan(fm["f1_freq"])) and np.any(np.isnan(fm["f1_freq"]))
    row = A.analyze(x, sr, summary=True, **SOUND_KW)
    row2 = A.analyze(x, sr, summary=True, formants=True, nFormants=3, **SOUND_KW)
    assert list(row2)[:44] == list(A.SUMMARY_COLUMNS) and len(row2) == 44 + 18
    for k in row:
        assert np.array_equal(row2[k], row[k], equal_nan=True), k
    want = F.formant_summary(fm, 3)
    assert list(row2)[44:] == list(want)
    for k, v in want.items():
        assert np.array_equal(row2[k], v, equal_nan=True), k
    assert math.isfinite(row2["f1_freq_mean"])


@pytest.mark.gpu
def test_analyze_batch_with_formants():
    import torch
    sr = 16000
    sounds = [sound_case(s, seed).astype(np.float32) for s, seed in SOUND_CASES if s == sr]
    lens = [len(p) for p in sounds]
    offs = np.concatenate([[0], np.cumsum(lens[:-1])])
    data = torch.from_numpy(np.concatenate(sounds)).cuda()
    plain = A.analyze_batch(data, offs, lens, sr, to_host=True, **SOUND_KW)
    got = A.analyze_batch(data, offs, lens, sr, to_host=True, formants=True, nFormants=2, **SOUND_KW)
    dev = A.analyze_batch(data, offs, lens, sr, formants=True, nFormants=2, **SOUND_KW)
    assert dev["formants"]["cols"] == 4 and dev["formants"]["columns"] == F.formant_columns(2)
    for i, x in enumerate(sounds):
        fm = F.formants(x.astype(np.float64), sr, nFormants=2, **SOUND_KW)
        for k in plain[i]:
            assert np.array_equal(got[i][k], plain[i][k], equal_nan=True), k
        for k in fm:
            assert np.array_equal(got[i][k], fm[k], equal_nan=True), k
    rows = A.analyze_batch(data, offs, lens, sr, to_host=True, summary=True, formants=True, nFormants=2, **SOUND_KW)
    for i, x in enumerate(sounds):
        one = A.analyze(x.astype(np.float64), sr, summary=True, formants=True, nFormants=2, **SOUND_KW)
        assert list(rows[i]) == list(one)
        for k in one:
            assert np.array_equal(rows[i][k], one[k], equal_nan=True), k


@pytest.mark.gpu
def test_analyze_folder_with_formants(tmp_path):
    """analyze_folder(formants=True): every row is analyze(path, summary=True, formants=True), every table
    analyze(path, formants=True); without the keyword the rows have the 44 cells."""
    import wave
    for name, (sr, seed) in zip(("b.wav", "a.wav"), SOUND_CASES[:2]):
        with wave.open(str(tmp_path / name), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            x = sound_case(sr, seed)
            w.writeframes(np.round(x / np.max(np.abs(x)) * 20000).astype("<i2").tobytes())
    rows = A.analyze_folder(str(tmp_path), formants=True, nFormants=2, **SOUND_KW)
    assert [r["sound"] for r in rows] == ["a.wav", "b.wav"]
    for r in rows:
        one = A.analyze(str(tmp_path / r["sound"]), summary=True, formants=True, nFormants=2, **SOUND_KW)
        assert list(r) == ["sound"] + list(one) and len(one) == 44 + 12
        for k in one:
            assert np.array_equal(r[k], one[k], equal_nan=True), (r["sound"], k)
        assert math.isfinite(r["f1_freq_mean"])
    tables = A.analyze_folder(str(tmp_path), summary=False, formants=True, nFormants=2, **SOUND_KW)
    for path, t in tables.items():
        one = A.analyze(path, formants=True, nFormants=2, **SOUND_KW)
        assert set(t) == set(one) and "f2_width" in t
        for k in one:
            assert np.array_equal(t[k], one[k], equal_nan=True), (path, k)
    assert all(len(r) == 45 for r in A.analyze_folder(str(tmp_path), **SOUND_KW))


def test_window_not_longer_than_the_order_is_refused():
    """windowLength = 1 ms at 44.1 kHz gives frames of 44 samples for an order of 47: refused as an argument error
    that names both, on the host, before any launch; the restatement refuses such a frame too."""
    with pytest.raises(ValueError, match="windowLength.*44.*47"):
        F.formants_size(A.repair(44100, windowLength=1), 3)
    assert F.formants_size(A.repair(44100, windowLength=2), 3) == (47, 6)  # 88 samples
    with pytest.raises(ValueError):
        F.find_formants_numpy(np.ones(47), 44100)


def test_analyze_without_formants_is_unchanged():
    """analyze(formants=False) takes the path it took: the keyword defaults to off and the formant code is not
    reached (on the GPU, test_analyze_with_formants compares the keys and the values)."""
    import inspect
    for fn in (A.analyze, A.analyze_batch, A.analyze_folder):
        assert inspect.signature(fn).parameters["formants"].default is False
    assert A.formants_numpy is F.formants_numpy and A.find_formants_numpy is F.find_formants_numpy
    assert A.formants_batch is F.formants_batch and A.find_formants_frames is F.find_formants_frames


@pytest.mark.gpu
def test_analyze_default_keys_are_unchanged():
    sr, seed = SOUND_CASES[0]
    t = A.analyze(sound_case(sr, seed), sr, **SOUND_KW)
    assert not any(k.startswith("f1_") for k in t)
    assert set(t) == set(A.COLUMNS) | {"autocorCand", "autocorCert", "time", "duration"} | set(A.PITCH_KEYS) | set(A.TRACK_COLUMNS)
