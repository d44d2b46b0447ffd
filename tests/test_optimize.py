"""optimize_pars(), segment_folder(), segment_sweep() and sweep_fitness()
(soundgen_beta_amd/optimize.py; sg_segment_sweep and sg_sweep_fitness in sg_segment.hip).

On the CPU: nelder_mead (every branch, maxit, speculative against one evaluation at a
time), evaluatePars' bounds rule, the reference's formal-order quirk, the refusals, the
ordering of the result, the starts against matchpars' draws, the fitness restatement by
hand, sg_segment.h's seg_sound_at as a stand-alone program (plain and with
-fsanitize=address,undefined), and the conditioning of the GPU inputs.

On the GPU the reference for values is segment_numpy(summary=True) looped over rows and
sounds, and _fitness below: the pairwise-complete Pearson correlation in np.longdouble.
Counts and the NaN pattern are compared exactly (every decision of the restatement on
these inputs has a relative margin >= MARGIN); times and lengths in ms with BOUND, the
bound tests/test_segment.py derived for the same arithmetic. FIT_BOUND, for the fitness, is
the next power of ten above 8 x the largest deviation measured on an MI355X over the
cases of test_sweep_fitness_equals_restatement (1.7e-16, so 1e-14), below its
ceiling of 1e-12: 64 terms at 1.1e-16 with well-separated values.
"""
import math
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from soundgen_beta_amd import optimize as OP
from soundgen_beta_amd import segment as SG

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
MARGIN = 1e-6
BOUND = 1e-14
FIT_BOUND = 1e-14
SR = 16000
nan = math.nan
_LD = np.longdouble


# ----------------------------------------------------------------------- Nelder-Mead
def _quadratic(p):
    return (p[0] - 1) ** 2 + 3 * (p[1] + 2) ** 2


def _rosenbrock(p):
    return sum(100 * (p[i + 1] - p[i] ** 2) ** 2 + (1 - p[i]) ** 2 for i in range(len(p) - 1))


def _checkerboard(p):  # contractions that fail: the simplex has to shrink
    return abs(p[0]) + abs(p[1]) + (5 if (int(math.floor(p[0] * 7)) + int(math.floor(p[1] * 7))) % 2 else 0)


NM_CASES = {"quadratic": (_quadratic, [0.0, 0.0], [1.0, -2.0]), "rosenbrock 2": (_rosenbrock, [-1.2, 1.0], [1.0, 1.0]),
            "rosenbrock 3": (_rosenbrock, [-1.2, 1.0, 0.5], [1.0, 1.0, 1.0]), "checkerboard": (_checkerboard, [1.5, 2.5], None)}


def _run_nm(name, speculate, **kw):
    f, start, _ = NM_CASES[name]
    events, calls = [], []

    def fn_many(vs):
        calls.append(len(vs))
        return [f(v) for v in vs]
    res = OP.nelder_mead(fn_many, start, speculate=speculate, trace=lambda k, x, v: events.append((k, tuple(x), v)), **kw)
    return res, events, calls


@pytest.mark.parametrize("name", list(NM_CASES))
def test_nelder_mead_converges_and_speculation_changes_nothing(name):
    """Convergence within maxit, the count of evaluations, and the same vertices and values
    whether the candidates of a step are evaluated together or one at a time."""
    res, events, calls = _run_nm(name, True, maxit=3000)
    assert res["convergence"] == 0 and res["counts"] <= 3000
    evals = [e for e in events if e[0] == "eval"]
    assert len(evals) == res["counts"]
    want = NM_CASES[name][2]
    if want is not None:
        assert np.allclose(res["par"], want, atol=2e-3) and res["value"] < 1e-5
    else:
        assert res["value"] < 1e-5
    assert max(calls) <= 4 and sum(calls) >= res["counts"] and len(calls) < res["counts"]
    one, events1, calls1 = _run_nm(name, False, maxit=3000)
    assert set(calls1) == {1} and len(calls1) == one["counts"]
    assert events1 == events and one == res


def test_nelder_mead_takes_every_branch():
    kinds = set()
    for name in NM_CASES:
        kinds |= {e[0] for e in _run_nm(name, True, maxit=3000)[1]}
    assert kinds == {"eval", "REFLECTION", "EXTENSION", "HI-REDUCTION", "LO-REDUCTION", "SHRINK"}
    assert "SHRINK" in {e[0] for e in _run_nm("checkerboard", True, maxit=3000)[1]}


@pytest.mark.parametrize("name,maxit", [("rosenbrock 2", 30), ("rosenbrock 3", 40), ("checkerboard", 25), ("quadratic", 0)])
def test_nelder_mead_obeys_maxit(name, maxit):
    """The loop runs while the count is <= maxit: the last pass adds at most the re-evaluation
    of the n other vertices after a shrink and the two evaluations of a step."""
    res, events, _ = _run_nm(name, True, maxit=maxit)
    n = len(NM_CASES[name][1])
    if maxit == 0:
        assert res["counts"] == 0 and res["convergence"] == 0 and res["par"] == NM_CASES[name][1]
        return
    assert res["convergence"] == 1 and maxit < res["counts"] <= maxit + n + 2
    assert len([e for e in events if e[0] == "eval"]) == res["counts"]
    assert _run_nm(name, False, maxit=maxit)[0] == res


def test_nelder_mead_values_that_are_not_finite():
    with pytest.raises(ValueError, match="initial parameters"):
        OP.nelder_mead(lambda vs: [nan for _ in vs], [1.0, 1.0])
    res = OP.nelder_mead(lambda vs: [nan if v[0] > 1.05 else _quadratic(v) for v in vs], [1.0, 1.0], maxit=200)
    assert res["convergence"] == 0 and res["par"][0] <= 1.05 and math.isfinite(res["value"])


def test_nelder_mead_many_equals_single_runs():
    f = _rosenbrock
    starts = [[-1.2, 1.0], [0.5, 0.5], [2.0, -1.0]]
    sizes = []

    def fn_many(vs):
        sizes.append(len(vs))
        return [f(v) for v in vs]
    many = OP.nelder_mead_many(fn_many, starts, maxit=60, reltol=1e-3)
    assert max(sizes) > 4 and max(sizes) <= 4 * len(starts)
    assert many == [OP.nelder_mead(lambda vs: [f(v) for v in vs], s, maxit=60, reltol=1e-3, speculate=False) for s in starts]


# ------------------------------------------------------------- optimizePars' host side
def test_bounds_rule_scores_one_without_evaluating():
    seen = []

    def evaluate(vs):
        seen.extend(vs)
        return [0.25] * len(vs)
    fn = OP.bounded(evaluate, [0, 0], [1, math.inf])
    assert fn([[0.5, 3], [-0.1, 3], [0.5, -1], [1.5, 2], [1, 0]]) == [0.25, 1.0, 1.0, 1.0, 0.25]
    assert seen == [[0.5, 3], [1, 0]]
    seen.clear()
    assert fn([[2, 2]]) == [1.0] and seen == []


def test_formal_order_quirk():
    """Without init the starting values come in the order of the formals, and the names are
    given by position in `pars`: out of formal order the two mismatch, as in the reference."""
    assert OP.start_means("segmentFolder", ["shortestSyl", "sylThres"]) == [40.0, 0.9]
    means = OP.start_means("segmentFolder", ["sylThres", "shortestSyl"])
    assert means == [40.0, 0.9]
    assert OP.name_values(["sylThres", "shortestSyl"], means) == {"sylThres": 40.0, "shortestSyl": 0.9}
    assert OP.start_means("segmentFolder", ["overlap", "troughLeft", "windowLength"]) == [1.0, 40.0, 80.0]
    assert OP.start_means("analyzeFolder", ["specThres", "silence"]) == [0.04, 0.3]
    assert OP.start_means("segmentFolder", ["sylThres", "shortestSyl"], init=[0.8, 30]) == [0.8, 30.0]


def test_null_default_is_refused():
    with pytest.raises(ValueError, match="NULL"):
        OP.start_means("segmentFolder", ["shortestSyl", "interburst"])
    with pytest.raises(ValueError, match="NULL"):
        OP.start_means("analyzeFolder", ["step"])
    with pytest.raises(ValueError, match="NULL"):
        OP.optimize_pars("/nowhere", [1, 2], "segmentFolder", ["interburst"], fitnessPar="nBursts")
    assert OP.start_means("segmentFolder", ["interburst"], init=[120]) == [120.0]
    with pytest.raises(ValueError, match="myfun"):
        OP.start_means("segment", ["sylThres"])


def test_mygrid_column_check():
    grid = {"sylThres": [0.5, 0.9], "shortestSyl": [20, 40]}
    with pytest.raises(ValueError, match="mygrid should be either NULL or a dataframe with one column per parameter"):
        OP.optimize_pars("/nowhere", [1, 2], "segmentFolder", ["shortestSyl", "sylThres"], fitnessPar="nBursts", mygrid=grid)
    with pytest.raises(ValueError, match="mygrid should be"):
        OP.optimize_pars("/nowhere", [1, 2], "segmentFolder", ["sylThres", "shortestSyl", "overlap"], fitnessPar="nBursts",
                         mygrid=grid)


def test_result_ordering_with_ties_and_nan():
    assert OP.order_decreasing([0.2, nan, 0.9, 0.2, nan, 0.9, -1.0]) == [2, 5, 0, 3, 6, 1, 4]
    assert OP.order_decreasing([]) == [] and OP.order_decreasing([nan]) == [0]


def test_starts_equal_matchpars_draws():
    from soundgen_beta_amd import matchpars as MP
    from soundgen_beta_amd.rrng import RRng
    means, low, high = [40.0, 0.9], [30.0, 0.0], [50.0, 1.0]
    got = OP.draw_starts(means, 0.2, low, high, 5, RRng(42))
    D = MP._Draws(RRng(42))
    assert got == [MP.rnorm_bounded(D, 2, means, [8.0, 0.9 * 0.2], low, high) for _ in range(5)]
    assert all(low[i] <= p[i] <= high[i] for p in got for i in range(2)) and len({tuple(p) for p in got}) == 5
    free = OP.draw_starts(means, 0.2, [-math.inf] * 2, [math.inf] * 2, 3, RRng(7))
    z = RRng(7)
    assert free == [[40.0 + 8.0 * float(z.standard_normal()), 0.9 + 0.9 * 0.2 * float(z.standard_normal())] for _ in range(3)]
    assert MP.rnorm_bounded(MP._Draws(RRng(1)), 3, [10, 50, 100], [0, 0, 0], 0, 60) == [10, 50, 60]  # a number for all


def _fitness(x, key):
    """1 - cor(x, key, use = 'pairwise.complete.obs') in long double: the complete pairs, the
    means refined once, the sums about them; NaN for fewer than two pairs or a side without
    variance; clamped to [-1, 1]."""
    x, key = np.asarray(x, dtype=np.float64), np.asarray(key, dtype=np.float64)
    ok = ~(np.isnan(x) | np.isnan(key))
    a, b = x[ok].astype(_LD), key[ok].astype(_LD)
    n = len(a)
    if n < 2 or a.min() == a.max() or b.min() == b.max():
        return nan
    ma, mb = a.sum() / n, b.sum() / n
    ma, mb = ma + (a - ma).sum() / n, mb + (b - mb).sum() / n
    r = ((a - ma) * (b - mb)).sum() / (np.sqrt(((a - ma) ** 2).sum()) * np.sqrt(((b - mb) ** 2).sum()))
    return float(1 - min(max(r, _LD(-1)), _LD(1)))


def test_fitness_restatement_by_hand():
    key = np.array([1.0, 2.0, 3.0, 4.0])
    assert _fitness(3 * key + 5, key) == 0.0
    assert _fitness(-2 * key + 1, key) == 2.0
    assert _fitness([1, 2, 3, 100], [1, 2, 3, nan]) == 0.0 and _fitness([1, nan, 3, 4], [2, 7, 6, 8]) == 0.0
    assert abs(_fitness([1, 2, 3], [1, 3, 2]) - 0.5) < 1e-15
    assert math.isnan(_fitness([5, 5, 5, 5], key)) and math.isnan(_fitness(key, [2, 2, 2, 2]))
    assert math.isnan(_fitness([1, nan, nan, nan], key)) and math.isnan(_fitness([nan] * 4, key))


# -------------------------------------------------- sg_segment.h's variant on the host
def _hx(v):
    return "nan" if v != v else float(v).hex()


def _pin_cases():
    rng = np.random.default_rng(11)
    out = []
    for k in range(200):
        m = int(rng.integers(0, 90)) if k else 0
        kind = int(rng.integers(0, 3))
        if kind == 0:
            v = rng.random(m)
        elif kind == 1:
            v = np.round(rng.random(m) * 4) / 4 + 0.25
        else:
            v = np.repeat(rng.random(m // 4 + 1) > 0.5, 4)[:m] * 1.0 + 0.01 * rng.random(m)
        timestep = float(rng.choice([7.3, 8.0, 12.5]))
        syl = float(rng.choice([0, 20, 40, 56]))
        head = [m, timestep, math.ceil(syl / timestep), float(rng.choice([0.9, 0.5])), syl,
                rng.choice([nan, 15.0, 40.0]).item(), rng.choice([nan, 0.0, 25.0, 2000.0]).item(), float(rng.choice([1, 0.5])),
                0.075, float(rng.choice([3, 1.05])), int(rng.integers(0, 2)), int(rng.integers(0, 2))]
        out.append((head, v))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_sweep_header_on_the_host(tmp_path):
    """tests/cpp/sweep_pins.cpp: seg_sound_at with the envelope apart and exactly the cells the
    sweep gives a pair writes what seg_sound writes, bit for bit, and seg_min_count is the
    planner's ceiling; plain and under the address and undefined-behaviour sanitizers."""
    cases = _pin_cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for head, v in cases:
            f.write(" ".join(_hx(h) for h in head) + " " + " ".join(_hx(x) for x in v) + "\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "sweep_pins.cpp")]
    exes = [str(tmp_path / "sweep_pins")]
    subprocess.run(base + ["-o", exes[0]], check=True, timeout=300)
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(str(tmp_path / "sweep_pins_san"))
        subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + base[1:] +
                       ["-o", exes[1]], check=True, timeout=300)
    outs = []
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(cases)
        outs.append(lines)
    assert all(o == outs[0] for o in outs)
    first = [float.fromhex(x) if "nan" not in x else nan for x in outs[0][0].split()]
    assert first[0] == 0 and first[7] == 0 and all(math.isnan(v) for i, v in enumerate(first) if i not in (0, 7))


# -------------------------------------------------------------------- the GPU inputs
def _signal(n, seed):
    """Bursts of a decaying 440 Hz tone, four a second with three amplitudes in turn, on low
    noise (the signal of tests/test_segment.py)."""
    rng = np.random.default_rng(seed)
    period = SR // 4
    d = np.arange(period) / SR
    tone = np.exp(-d / 0.04) * np.sin(2 * np.pi * 440 * d)
    k = n // period + 2
    x = np.concatenate([np.zeros(SR // 20), ((0.6 + 0.1 * (np.arange(k) % 3))[:, None] * tone[None, :]).ravel()])
    return x[:n] + 0.01 * rng.standard_normal(n)


def _flutter(n, seed):
    """20 ms of tone every 60 ms: the smoothed envelope crosses the threshold too often for a
    run to last longer than the default shortest syllable."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    return ((t % 0.06) < 0.02) * np.sin(2 * np.pi * 440 * t) * 0.7 + 0.01 * rng.standard_normal(n)


def _pcm(x, add=0):
    return (np.round(x * 12000) + add).astype(np.int16)


@lru_cache(maxsize=None)
def _sounds():
    """(file name, int16 samples, rate) in sorted order of the names; the first five at 16 kHz."""
    return (("a_onepass_1500.wav", _pcm(_signal(1500, 1)), SR), ("b_padded_4097.wav", _pcm(_signal(4097, 2)), SR),
            ("c_positive_6000.wav", _pcm(_signal(6000, 3), 15000), SR), ("d_flutter_8192.wav", _pcm(_flutter(8192, 4)), SR),
            ("e_two.wav", np.array([6000, -3000], dtype=np.int16), SR), ("f_other_rate.wav", _pcm(_signal(5000, 5)), 22050))


# seven rows in two envelope groups; the last one runs with the sweep's troughRight flag
ROWS = (dict(windowLength=40, overlap=80),
        dict(windowLength=40, overlap=80, shortestSyl=20, sylThres=0.7),
        dict(windowLength=40, overlap=80, burstThres=0.15, peakToTrough=2),
        dict(windowLength=40, overlap=80, shortestPause=None),
        dict(windowLength=25, overlap=50),
        dict(windowLength=25, overlap=50, interburst=100),
        dict(windowLength=25, overlap=50, shortestSyl=60, sylThres=1.1, peakToTrough=1.5))
FLAGS = (False,) * 6 + (True,)
DEFAULTS = dict(windowLength=40, overlap=80, shortestSyl=40, shortestPause=40, sylThres=0.9, interburst=None,
                interburstMult=1, burstThres=0.075, peakToTrough=3)


def _grid(idx):
    return {k: [ROWS[r].get(k, DEFAULTS[k]) for r in idx] for k in
            sorted({k for r in idx for k in ROWS[r]} | {"shortestSyl"})}


@lru_cache(maxsize=None)
def _reference():
    """segment_numpy(summary=True) of the first four sounds under every row, with the traces."""
    out = {}
    for s, (_, pcm, _) in enumerate(_sounds()[:4]):
        for r, kw in enumerate(ROWS):
            tr = {}
            out[r, s] = (SG.segment_numpy(pcm.astype(np.float64), SR, troughRight=FLAGS[r], summary=True, _trace=tr, **kw), tr)
    return out


def test_gpu_inputs_are_well_conditioned():
    """Every decision of the restatement on every (sound, row) of the GPU tests has a relative
    margin >= MARGIN, so a deviation within BOUND cannot flip one; and the sounds are what
    their names say."""
    ref = _reference()
    for (r, s), (row, tr) in ref.items():
        margins = {k: tr[k] for k in ("threshold", "count", "merge", "cond2", "cond3") if k in tr}
        assert "threshold" in margins and "cond2" in margins
        assert min(margins.values()) >= MARGIN, (r, s, margins)
    snd = _sounds()
    assert [len(v) for _, v, _ in snd] == [1500, 4097, 6000, 8192, 2, 5000] and snd[2][1].min() > 0
    assert [n for n, _, _ in snd] == sorted(n for n, _, _ in snd)
    assert math.isnan(ref[0, 3][0]["sylLen_mean"]) and ref[0, 3][0]["nSyl"] == 1  # no syllable: the one row of NA
    assert ref[1, 3][0]["nSyl"] >= 2 and ref[0, 2][0]["nSyl"] >= 2
    rows = [tuple(tuple(ref[r, s][0].values()) for s in range(4)) for r in range(len(ROWS))]
    assert len({repr(v) for v in rows}) >= 5  # the rows do change the summaries


# ---------------------------------------------------------------------- GPU: the sweep
@lru_cache(maxsize=None)
def _device_batch():
    import torch
    parts = [v.astype(np.float32) for _, v, _ in _sounds()[:5]]
    lens = np.array([len(v) for v in parts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    host = np.zeros(int(offs[-1] + lens[-1]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    return torch.from_numpy(host).cuda(), offs, lens


def _sweep(idx=tuple(range(7)), **kw):
    """Rows idx: those without the flag as one sweep, the one with it as another."""
    data, offs, lens = _device_batch()
    out = np.zeros((len(idx), len(lens), 11))
    for flag in (False, True):
        at = [i for i, r in enumerate(idx) if FLAGS[r] == flag]
        if at:
            out[at] = OP.segment_sweep(data, offs, lens, SR, _grid([idx[i] for i in at]), troughRight=flag, **kw)
    return out


@lru_cache(maxsize=None)
def _swept():
    return _sweep()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.gpu
def test_sweep_equals_segment_batch():
    """Row g of the sweep is segment_batch(summary=True) under row g's parameters bit for bit,
    NaN pattern included; the two-sample sound has the row of a sound the reference stops on."""
    import torch
    data, offs, lens = _device_batch()
    got = _swept()
    assert got.shape == (7, 5, 11)
    for r, kw in enumerate(ROWS):
        ref = SG.segment_batch(data, offs, lens, SR, summary=True, troughRight=FLAGS[r], **kw)
        assert ref[4] is None
        for s in range(4):
            want = np.array([ref[s][k] for k in SG.SUMMARY_COLUMNS], dtype=np.float64)
            assert np.array_equal(_bits(got[r, s]), _bits(want)), (r, s, got[r, s], want)
        assert got[r, 4, 0] == 0 and got[r, 4, 7] == 0 and np.isnan(np.delete(got[r, 4], [0, 7])).all()
    dev = OP.segment_sweep(data, offs, lens, SR, _grid(range(6)), to_host=False)
    assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == (6, 5, 11)
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(got[:6]))
    assert OP.segment_sweep(data, offs, lens, SR, {}).shape == (0, 5, 11)


def _chunking_caps():
    """Workspace caps that split the sweep, from sg_segment_size's cells: the transform of a
    sound of 2^p >= 4096 points takes 16 x 2^p bytes; a (sound, row) pair keeps its cells less
    the 11 of the summary and the m of the envelope, 8 bytes each."""
    lens = _device_batch()[2]
    sizes = {}
    for g, (wl, ov) in enumerate(((40, 80), (25, 50))):
        d = [SG.segment_size_native(int(n), SG._params(SR, windowLength=wl, overlap=ov)) for n in lens[:4]]
        sizes[g] = (8 * sum(v["cells"] - 11 - v["n_env"] for v in d) + 8 * 8, [16 << v["log2n"] for v in d if v["log2n"] >= 12])
    row_bytes = max(v[0] for v in sizes.values())
    work = sizes[0][1]
    assert len(work) == 3 and 7 * row_bytes <= max(work)  # under the first cap all rows are one chunk
    return dict(sounds=max(work), one_row=row_bytes, two_rows=2 * row_bytes + 8)


@pytest.mark.gpu
def test_sweep_does_not_depend_on_the_launch():
    """The same bits with the rows reversed, one row at a time, and under caps that split the
    sounds into three chunks of transforms (all rows in one chunk), the rows into seven
    chunks, and into chunks of two."""
    want = _bits(_swept())
    assert np.array_equal(_bits(_sweep(tuple(range(6, -1, -1)))[::-1]), want)
    for r in range(7):
        assert np.array_equal(_bits(_sweep((r,))[0]), want[r]), r
    for name, cap in _chunking_caps().items():
        assert np.array_equal(_bits(_sweep(workspace_cap=int(cap))), want), name


@pytest.mark.gpu
def test_sweep_equals_restatement():
    got, ref = _swept(), _reference()
    dev = 0.0
    for (r, s), (row, _) in ref.items():
        want = np.array([row[k] for k in SG.SUMMARY_COLUMNS], dtype=np.float64)
        assert got[r, s, 0] == want[0] and got[r, s, 7] == want[7], (r, s)
        assert np.array_equal(np.isnan(got[r, s]), np.isnan(want)), (r, s, got[r, s], want)
        ok = ~np.isnan(want)
        dev = max(dev, float(np.max(np.abs(got[r, s][ok] - want[ok]))))
    print("sweep deviation: %.3e ms" % dev)
    assert dev <= BOUND


@pytest.mark.gpu
def test_sweep_refusals():
    """A row the planner refuses for one sound refuses the sweep and names both; rows that
    differ in samplingRate are not one sweep."""
    import ctypes as C
    import torch
    from soundgen_beta_amd import _abi, native
    data, offs, lens = _device_batch()
    with pytest.raises(ValueError, match="row 1, sound 0.*cannot be equal to 0 or 1"):
        OP.segment_sweep(data, offs, lens, SR, dict(windowLength=[40, 0.05]))
    with pytest.raises(ValueError, match="interburst"):
        OP.segment_sweep(data, offs, lens, SR, dict(interburst=[None, -1]))
    with pytest.raises(ValueError, match="not a parameter"):
        OP.segment_sweep(data, offs, lens, SR, dict(troughLeft=[True]))
    P = (_abi.sg_segment_params * 2)(SG._params(SR), SG._params(22050))
    _, _, nc, p_offs, p_lens = native.batch_layout(offs, lens)
    out = torch.zeros(2 * nc * 11, dtype=torch.float64, device="cuda")
    ctx = native.default_context(0)
    rc = native.lib().sg_segment_sweep(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, P, 2,
                                       C.c_void_p(out.data_ptr()))
    assert rc == -1 and b"row 1" in native.lib().sg_last_error(ctx.ptr)
    assert not out.cpu().numpy().any()  # nothing was launched


# -------------------------------------------------------------------- GPU: the fitness
def _synthetic():
    rng = np.random.default_rng(3)
    m = rng.normal(50, 20, size=(5, 64, 11))
    key = np.round(rng.normal(5, 2, size=64))
    m[0, :, 2] = 3 * key + rng.normal(0, 1, 64)
    m[1, rng.random(64) < 0.3, 2] = nan
    m[2, :, 2] = 7.25            # a constant row
    m[3, 1:, 2] = nan            # a single complete pair
    m[4, :, 2] = -key
    key[[5, 17]] = nan
    return m, key


@pytest.mark.gpu
def test_sweep_fitness_equals_restatement():
    import torch
    dev = 0.0
    cases = []
    sw = _swept()
    for col in ("nBursts", "sylLen_mean"):
        c = SG.SUMMARY_COLUMNS.index(col)
        cases.append((sw, c, col, np.array([1.0, 2.0, 2.0, 8.0, 0.0])))
    m, key = _synthetic()
    cases.append((m, 2, 2, key))
    for m, c, col, key in cases:
        got = OP.sweep_fitness(torch.from_numpy(m).cuda(), col, key)
        want = np.array([_fitness(m[r, :, c], key) for r in range(len(m))])
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (col, got, want)
        ok = ~np.isnan(want)
        if ok.any():
            dev = max(dev, float(np.max(np.abs(got[ok] - want[ok]))))
        if col == 2:
            assert np.isnan(want[[2, 3]]).all() and ok.sum() == 3 and got[4] == 2.0
            one = OP.sweep_fitness(torch.from_numpy(m[1]).cuda(), 2, key)  # a row alone: the same bits
            assert np.array_equal(_bits(one), _bits(got[1:2]))
    print("fitness deviation: %.3e" % dev)
    assert dev <= FIT_BOUND
    with pytest.raises(ValueError, match="key has"):
        OP.sweep_fitness(torch.from_numpy(sw).cuda(), 0, [1.0, 2.0])


# ------------------------------------------------------- GPU: the folder and optimizePars
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from soundgen_beta_amd import api
    d = tmp_path_factory.mktemp("sounds")
    for name, pcm, sr in reversed(_sounds()):
        api.write_wav(str(d / name), pcm, sr)
    (d / "notes.txt").write_text("not a sound")
    return str(d)


KEY = [1.0, 2.0, 2.0, 8.0, 0.0, 3.0]


@pytest.mark.gpu
def test_segment_folder(folder):
    rows = OP.segment_folder(folder, verbose=True)
    snd = _sounds()
    assert [r["sound"] for r in rows] == [n for n, _, _ in snd]
    for row, (name, pcm, sr) in zip(rows, snd):
        assert list(row) == ["sound"] + list(SG.SUMMARY_COLUMNS)
        if len(pcm) < 3:
            assert row["nSyl"] == 0 and row["nBursts"] == 0 and all(math.isnan(row[k]) for k in SG.SUMMARY_COLUMNS[1:7])
            continue
        one = SG.segment(pcm.astype(np.float64), sr, summary=True)
        assert np.array_equal(_bits([row[k] for k in SG.SUMMARY_COLUMNS]), _bits([one[k] for k in SG.SUMMARY_COLUMNS])), name
    full = OP.segment_folder(folder, summary=False, sylThres=0.7)
    assert list(full) == [os.path.join(folder, n) for n, _, _ in snd] and full[os.path.join(folder, "e_two.wav")] is None
    one = SG.segment(snd[1][1].astype(np.float64), SR, sylThres=0.7)
    got = full[os.path.join(folder, snd[1][0])]
    assert all(np.array_equal(got[p][k], one[p][k], equal_nan=True) for p in one for k in one[p])
    with pytest.raises(NotImplementedError):
        OP.segment_folder("/nowhere", plot=True)
    with pytest.raises(NotImplementedError):
        OP.segment_folder("/nowhere", savePath="/tmp")


@pytest.mark.gpu
def test_optimize_pars_grid(folder):
    import torch
    from soundgen_beta_amd import analyze as AN
    pars = ["shortestSyl", "sylThres"]
    grid = {"shortestSyl": [40, 20, 60, 40], "sylThres": [0.9, 0.7, 1.1, 0.5], "label": list("abcd")}
    res = OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="nBursts", mygrid=grid, verbose=False,
                           otherPars=dict(plot=False, verbose=False, windowLength=25, overlap=50),
                           bounds=dict(low=[100, 100], high=[200, 200]))  # a grid is evaluated without bounds
    assert list(res) == ["shortestSyl", "sylThres", "label", "fit"] and res["label"] == list("abcd")
    host = []
    for syl, thr in zip(grid["shortestSyl"], grid["sylThres"]):
        rows = OP.segment_folder(folder, shortestSyl=syl, sylThres=thr, windowLength=25, overlap=50)
        host.append([[r[k] for k in SG.SUMMARY_COLUMNS] for r in rows])
    host = np.array(host, dtype=np.float64)
    c = SG.SUMMARY_COLUMNS.index("nBursts")
    assert np.array_equal(_bits(res["fit"]), _bits(OP.sweep_fitness(torch.from_numpy(host).cuda(), "nBursts", KEY)))
    want = np.array([_fitness(host[r, :, c], KEY) for r in range(4)])
    assert np.array_equal(np.isnan(res["fit"]), np.isnan(want)) and not np.isnan(want).all()
    assert np.nanmax(np.abs(res["fit"] - want)) <= FIT_BOUND
    seen = []

    def fun(x):
        seen.append(x)
        return float(np.nansum(x)) / 7
    res2 = OP.optimize_pars(folder, None, "segmentFolder", pars, fitnessPar="sylLen_mean", fitnessFun=fun, mygrid=grid,
                            verbose=False, otherPars=dict(windowLength=25, overlap=50))
    c2 = SG.SUMMARY_COLUMNS.index("sylLen_mean")
    assert all(isinstance(x, np.ndarray) and x.shape == (6,) for x in seen) and len(seen) == 4
    assert np.array_equal(_bits(res2["fit"]), _bits([float(np.nansum(host[r, :, c2])) / 7 for r in range(4)]))
    agrid = {"specThres": [0.3, 0.05]}
    res3 = OP.optimize_pars(folder, KEY, "analyzeFolder", ["specThres"], fitnessPar="pitch_median", mygrid=agrid,
                            verbose=False, otherPars=dict(plot=False, verbose=False, pitchMethods=("spec",)))
    rows = [AN.analyze_folder(folder, specThres=v, pitchMethods=("spec",)) for v in agrid["specThres"]]
    m = np.array([[[r[k] for k in AN.SUMMARY_COLUMNS] for r in rr] for rr in rows], dtype=np.float64)
    assert m.shape == (2, 6, 44)
    assert np.array_equal(_bits(res3["fit"]), _bits(OP.sweep_fitness(torch.from_numpy(m).cuda(), "pitch_median", KEY)))
    print("analyzeFolder fit:", res3["fit"])
    with pytest.raises(ValueError, match="fitnessPar"):
        OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="pitch_median", mygrid=grid, verbose=False)
    with pytest.raises(NotImplementedError):
        OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="nBursts", mygrid=grid, otherPars=dict(plot=True))


@pytest.mark.gpu
def test_optimize_pars_simplex(folder):
    """nIter = 2 restarts whose candidates share sweeps equal, bit for bit, the same optimizer
    driven through one-row sweeps, one evaluation at a time; a returned vector evaluated
    again through mygrid gives exactly 1 - r."""
    from soundgen_beta_amd.rrng import RRng
    pars = ("shortestSyl", "sylThres")
    ctl = dict(maxit=12, reltol=.01)
    other = dict(plot=False, verbose=False)
    res = OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="nBursts", nIter=2, control=ctl,
                           otherPars=other, verbose=False, rng=RRng(5))
    assert len(res) == 2 and all(list(r) == ["r", "shortestSyl", "sylThres"] for r in res)
    assert not (res[0]["r"] < res[1]["r"])

    def one(p):
        g = OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="nBursts", verbose=False, otherPars=other,
                             mygrid={"shortestSyl": [p[0]], "sylThres": [p[1]]})
        return float(g["fit"][0])
    starts = OP.draw_starts(OP.start_means("segmentFolder", pars), .2, [-math.inf] * 2, [math.inf] * 2, 2, RRng(5))
    runs = [OP.nelder_mead(lambda vs: [one(v) for v in vs], s, speculate=False, **ctl) for s in starts]
    rows = [[1 - r["value"]] + r["par"] for r in runs]
    rows = [rows[i] for i in OP.order_decreasing([r[0] for r in rows])]
    assert all(12 < r["counts"] <= 16 or r["convergence"] == 0 for r in runs)
    assert np.array_equal(_bits([list(r.values()) for r in res]), _bits(rows)), (res, rows)
    for r in res:  # r = 1 - fit is the same operation again; fit against 1 - r has the two roundings, 2^-53 each
        fit = one([r["shortestSyl"], r["sylThres"]])
        assert np.array_equal(_bits(1 - fit), _bits(r["r"])) and abs(fit - (1 - r["r"])) <= 2.0 ** -52
    lazy = OP.optimize_pars(folder, KEY, "segmentFolder", pars, fitnessPar="nBursts", nIter=2, control=ctl,
                            otherPars=other, verbose=False, rng=RRng(5), speculate=False)
    assert np.array_equal(_bits([list(r.values()) for r in lazy]), _bits(rows))
