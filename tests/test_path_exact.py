"""pathfinding = 'exact': the path through a voiced segment's pitch candidates that minimises
the reference's own costPerPath() (R/utilities_pitch_postprocessing.R:347-372), which the
refused 'slow' approximates by annealing, found by dynamic programming; and path_costs(),
which reports what any pathfinder's choice cost. 'exact' is not in the reference.

CPU: the numpy restatement (analyze.pathfinding_exact, cost_per_path) against the enumeration
of every path in long double, on hand cases and on the cases of analyze_numpy; the names and
refusals; the sizes of the other modes at the values recorded before 'exact' existed; sg_path.h
compiled for the host (tests/cpp/path_exact_pins.cpp) against the restatement, plainly and
under AddressSanitizer and UBSan. GPU: analyze(), analyze_batch(), pitch_path(), path_costs()
and analyze_sweep() with 'exact' against the restatement and against each other.

Bars. A pick is a discrete decision: it must equal the restatement's wherever every minimum
the restatement takes has a relative margin >= 1e-6 (MARGIN, as tests/test_analyze.py). The
cost of the recursion's path may exceed the enumerated minimum by a relative 8 * 2n * 2^-52 for
n frames: the cost has at most 2n terms and each term of the recursion carries a few ulp. A
cost from sg_path.h (host or device) is held to 1e-12 relative of cost_per_path: both are sums
of at most a few hundred positive terms of an exp() good to a few ulp, orders below that. pitch
on the GPU: tests/test_analyze.py's _compare (1e-9).
"""
import inspect
import itertools
import math
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
import test_analyze as TA
from test_pitch_candidates import _margins as _tracker_margins
from test_pitch_candidates import _signal

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import native

MARGIN = TA.MARGIN
nan = math.nan
_hz = TA._hz
TRACE_KEYS = ("band", "start", "choice", "fb", "maxiter", "delta", "force", "exact")


def _cog(C):
    return [AN._mean(f) if f else nan for f in C]


def _cost_ld(C, cog, picks, cw):
    """costPerPath() in long double, written out independently of the module."""
    L = np.longdouble
    v = [None if k is None else L(C[f][k]) for f, k in enumerate(picks)]
    cert = [abs(v[f] - L(cog[f])) for f in range(len(C)) if v[f] is not None]
    jump = [1 / (1 + 10 * np.exp(3 - 7 * abs(v[f] - v[f + 1]))) for f in range(len(C) - 1)
            if v[f] is not None and v[f + 1] is not None]
    if not cert or not jump:
        return L(nan)
    return L(cw) * (sum(cert, L(0)) / len(cert)) + (1 - L(cw)) * (sum(jump, L(0)) / len(jump))


def _enumerate(C, cog, cw):
    """(cost, picks) of the cheapest of all paths (the first in lexicographic order of equal ones), in long double."""
    best = None
    for q in itertools.product(*[range(len(f)) if f else [None] for f in C]):
        c = _cost_ld(C, cog, q, cw)
        if not np.isnan(c) and (best is None or c < best[0]):
            best = (c, list(q))
    return best


def _exact_margin(tr):
    return TA._pairs(tr["exact"])


def _margin(p):
    """tests/test_analyze.py's _track_margin with the minima of 'exact' included."""
    return min([TA._track_margin(p)] + [_exact_margin(s) for s in p["segments"]])


# ------------------------------------------------------------ CPU: the recursion against every path
def test_exact_equals_brute_force():
    rng = np.random.default_rng(2024)
    total = compared = skipped = degenerate = with_gap = 0
    worst = 0.0
    for t in range(2600):
        n = int(rng.integers(2, 7))
        C = [sorted(set(np.round(rng.uniform(7, 10, int(rng.integers(1, 5))), 3).tolist())) for _ in range(n)]
        if t % 7 == 0 and n > 2:
            C[int(rng.integers(1, n - 1))] = []  # an empty inner frame
        cog = _cog(C)
        cw = float(rng.choice([0.2, 0.5, 0.8]))
        tr = {"choice": []}
        picks = AN.pathfinding_exact(C, cog, cw, tr)
        best = _enumerate(C, cog, cw)
        if best is None:  # no two neighbouring frames: every path costs NaN, the picks are 'none''s
            degenerate += 1
            assert picks == AN._pick_none(C, cog, {"choice": []}) and math.isnan(AN.cost_per_path(C, cog, picks, cw))
            continue
        total += 1
        with_gap += any(not f for f in C)
        assert [k is None for k in picks] == [not f for f in C]
        got = _cost_ld(C, cog, picks, cw)
        excess = float((got - best[0]) / best[0])
        worst = max(worst, excess)
        assert excess <= 8 * 2 * n * 2.0 ** -52, (C, cw, picks, best)
        assert AN.cost_per_path(C, cog, picks, cw) == pytest.approx(float(got), rel=1e-14)
        if _exact_margin(tr) >= MARGIN:
            compared += 1
            assert picks == best[1], (C, cw)
        else:
            skipped += 1
    print("segments %d (with an empty frame %d, without neighbours %d), picks compared %d, skipped %d, largest excess %.2e"
          % (total, with_gap, degenerate, compared, skipped, worst))
    assert total >= 2000 and with_gap >= 100 and degenerate >= 10
    assert skipped <= 0.05 * total


PIN_C = [[7.011, 8.726, 8.946], [7.196], [7.048, 7.149, 9.608, 9.744]]
PIN_A = [[.1, .1, .1], [.5], [.1, .1, .9, .1]]


def test_pinned_case():
    cog = _cog(PIN_C)
    tr = {}
    picks = AN.pathfinding_exact(PIN_C, cog, 0.2, tr)
    assert picks == [0, 0, 1] == _enumerate(PIN_C, cog, 0.2)[1]
    assert AN.cost_per_path(PIN_C, cog, picks, 0.2) == pytest.approx(0.17355050795414312, rel=1e-12)
    assert min(abs(a - b) for a, b in tr["exact"]) == pytest.approx(9.5e-3, rel=0.01)  # the smallest decision margin
    ftr = {k: [] for k in TRACE_KEYS}
    fast = AN._picks_of(PIN_C, AN.pathfinding_fast(PIN_C, PIN_A, cog, 0.2, ftr))
    assert fast == [2, 0, 2]  # 8.946, 7.196, 9.608
    assert AN.cost_per_path(PIN_C, cog, fast, 0.2) == pytest.approx(0.9288844095787764, rel=1e-12)
    # by hand: two means, then the weights
    cert = (abs(7.011 - cog[0]) + 0 + abs(7.149 - cog[2])) / 3
    jump = (TA._jump(7.011, 7.196) + TA._jump(7.196, 7.149)) / 2
    assert AN.cost_per_path(PIN_C, cog, picks, 0.2) == pytest.approx(.2 * cert + .8 * jump, rel=1e-14)
    # through the pathfinder: the path and its cost in the trace
    tr = {}
    hz = [[2.0 ** v for v in f] for f in PIN_C]
    p = AN.pathfinder_numpy(hz, PIN_A, certWeight=.2, pathfinding="exact", interpolWin=0, snakeStep=0, _trace=tr)
    assert p == pytest.approx([2.0 ** 7.011, 2.0 ** 7.196, 2.0 ** 7.149], rel=1e-14) and tr["picks"] == [0, 0, 1]
    assert tr["cost"] == pytest.approx(0.17355050795414312, rel=1e-12) and tr["direction"] is None and tr["fb"] == []
    tr = {}
    AN.pathfinder_numpy(hz, PIN_A, certWeight=.2, pathfinding="fast", interpolWin=0, snakeStep=0, _trace=tr)
    assert tr["picks"] == [2, 0, 2] and tr["cost"] == pytest.approx(0.9288844095787764, rel=1e-12)


def test_ties_take_the_lowest_index():
    # both candidates of frame 1 are equally far from their mean and from 8.5: k = 0 wins the inner minimum
    C = [[8.0, 9.0], [8.5]]
    tr = {}
    assert AN.pathfinding_exact(C, _cog(C), .5, tr) == [0, 0] and (tr["exact"][0][0] == tr["exact"][0][1])
    # the mirror image: the tie is at the end of the run, i = 0 wins
    C = [[8.5], [8.0, 9.0]]
    tr = {}
    assert AN.pathfinding_exact(C, _cog(C), .5, tr) == [0, 0] and (tr["exact"][-1][0] == tr["exact"][-1][1])
    # three frames tied throughout: all lowest
    C = [[8.0, 9.0], [8.0, 9.0], [8.0, 9.0]]
    assert AN.pathfinding_exact(C, _cog(C), .5, {}) == [0, 0, 0]


def test_empty_frame_splits_two_runs():
    C = [[8.0, 9.0], [8.0, 8.1], [], [9.0, 9.2], [8.0, 9.05]]
    cog = _cog(C)
    tr = {}
    picks = AN.pathfinding_exact(C, cog, .5, tr)
    assert picks == _enumerate(C, cog, .5)[1] == [0, 0, None, 0, 1] and _exact_margin(tr) >= MARGIN
    # n_c = 4 frames, n_j = 2 pairs: the pair across the gap does not count
    want = .5 * (.5 + .05 + .1 + abs(9.05 - 8.525)) / 4 + .5 * (TA._jump(8, 8) + TA._jump(9, 9.05)) / 2
    assert AN.cost_per_path(C, cog, picks, .5) == pytest.approx(want, rel=1e-14)
    tr = {}
    p = AN.pathfinder_numpy([[2.0 ** v for v in f] for f in C], [[.5] * len(f) for f in C], pathfinding="exact", interpolWin=0,
                            snakeStep=0.05, _trace=tr)
    assert math.isnan(p[2]) and p[:2] == [256.0, 256.0] and p[3] == 512.0 and tr["iterations"] == 0 and tr["maxiter"] == []  # no snake
    # with interpolation the gap is filled and the snake runs
    tr = {}
    p = AN.pathfinder_numpy([[2.0 ** v for v in f] for f in C], [[.5] * len(f) for f in C], pathfinding="exact", interpolWin=3,
                            interpolTol=0.3, _trace=tr)
    assert not np.isnan(p).any() and tr["interpolated"] >= 1 and tr["maxiter"] and None not in tr["picks"]


def test_no_neighbouring_frames_takes_none():
    cands, cert = [_hz(8, 8.1, 9), [], _hz(8, 8.8, 9)], [[.5] * 3, [], [.5] * 3]
    tr = {}
    p = AN.pathfinder_numpy(cands, cert, pathfinding="exact", interpolWin=0, _trace=tr)
    q = AN.pathfinder_numpy(cands, cert, pathfinding="none", interpolWin=0)
    assert p[::2] == q[::2] == pytest.approx([2.0 ** 8.1, 2.0 ** 8.8], rel=1e-14) and math.isnan(p[1])
    assert tr["exact"] == [] and tr["picks"] == [1, None, 1] and math.isnan(tr["cost"])  # mean of no jump: NaN, as in the reference


def test_early_exits_are_unchanged():
    # a one-row segment: returned as 2 ^ pitchCands whatever the pathfinder (:87-89)
    for pf in ("exact", "fast", "none"):
        tr = {}
        p = AN.pathfinder_numpy([_hz(8), [], [], _hz(9)], [[.5], [], [], [.5]], pathfinding=pf, interpolWin=1, interpolTol=0.05,
                                _trace=tr)
        assert p == [256.0, 256.0, 2.0 ** 8.5, 512.0] and tr["rows"] == 1 and tr["exact"] == [] and tr["picks"] == [0] * 4
    # a segment of one frame takes 'none' (:93)
    tr = {}
    p = AN.pathfinder_numpy([_hz(8, 8.1, 9)], [[.5] * 3], pathfinding="exact", interpolWin=0, snakeStep=0, _trace=tr)
    assert p == pytest.approx([2.0 ** 8.1], rel=1e-14) and tr["exact"] == [] and tr["choice"] and math.isnan(tr["cost"])


# ------------------------------------------------------------ the names, the refusals, the sizes
def test_exact_name_is_accepted():
    import ctypes as C
    assert AN.PATHFINDING[:3] == ("none", "fast", "slow") and AN.PATHFINDING.index("exact") == 3
    base = AN.repair_pitch(16000, None)
    s = AN.repair_track(base, pathfinding="exact")
    assert s["pathfinding"] == "exact" and AN._track_params(s).pathfinding == 3
    want, got = AN.track_decisions(9600, s), AN.track_decisions_native(9600, s)
    keys = AN.TRACK_SIZE_KEYS + ("frames", "cols")
    assert {k: got[k] for k in keys} == {k: want[k] for k in keys}
    P = AN._track_params(s)
    fr, cl = C.c_int32(), C.c_int32()
    L = native.lib()
    assert L.sg_analyze_size(9600, C.byref(P), C.byref(fr), C.byref(cl), None) == 0 and (fr.value, cl.value) == (22, 25)
    for v, code in ((2, -4), (4, -1), (-1, -1), (7, -1)):
        Q = type(P).from_buffer_copy(P)
        Q.pathfinding = v
        assert L.sg_analyze_size(9600, C.byref(Q), C.byref(fr), C.byref(cl), None) == code, v
    assert hasattr(L, "sg_pitch_path_costs")
    x = _signal(16000, 1)
    r = AN.analyze_numpy(x, 16000, pathfinding="exact")
    assert r["voiced"].sum() >= 8
    assert "pathfinding" in inspect.signature(AN.path_costs).parameters


def test_slow_and_unknown_names_still_raise():
    base = AN.repair_pitch(16000, None)
    with pytest.raises(ValueError):
        AN.repair_track(base, pathfinding="quick")
    for dec in (AN.track_decisions, AN.track_decisions_native):
        with pytest.raises(native.SoundgenError, match="slow") as e:
            dec(9600, AN.repair_track(base, pathfinding="slow"))
        assert e.value.code == -4
    with pytest.raises(NotImplementedError):
        AN.pathfinder_numpy([_hz(8, 9)], [[.5, .5]], pathfinding="slow")
    with pytest.raises(NotImplementedError):
        AN.analyze_numpy(np.zeros(4000), 16000, pathfinding="slow")
    with pytest.raises(NotImplementedError, match="row 1"):
        AN.sweep_plan(16000, [dict(pathfinding="exact"), dict(pathfinding="slow")])
    with pytest.raises(ValueError, match="row 0"):
        AN.sweep_plan(16000, [dict(pathfinding="quick")])


# sg_analyze_size (minVoicedCands, noRequired, nToleratedNA, hw, interpolWin, frames, cols) and sg_analyze_sweep_size
# (frame group, store, row bytes; sounds of `length` and 3 * length samples) before 'exact' existed
SIZE_CASES = dict(defaults=(16000, dict(), 9600), step5_ncands3=(16000, dict(step=5, nCands=3, pitchMethods=TA.ALL4), 16000),
                  sr44100=(44100, dict(), 50000))
RECORDED = dict(defaults=([2, 1, 2, 2, 3, 22, 25], [309856, 0, 30912]),
                step5_ncands3=([2, 4, 12, 9, 3, 190, 37], [2701920, 0, 411840]),
                sr44100=([2, 1, 2, 2, 3, 44, 25], [1608136, 0, 60144]))


@pytest.mark.parametrize("name", sorted(SIZE_CASES))
def test_sizes_of_the_other_modes_are_unchanged(name):
    sr, kw, length = SIZE_CASES[name]
    frames = None
    for pf in ("none", "fast", "exact"):
        s = AN.repair_track(AN.repair_pitch(sr, None, **kw), pathfinding=pf)
        d = AN.track_decisions_native(length, s)
        z = AN.sweep_size([length, 3 * length], sr, [dict(kw, pathfinding=pf)])
        got = ([d[k] for k in AN.TRACK_SIZE_KEYS + ("frames", "cols")], [z["frame_group"], z["store"], z["row"]])
        if pf != "exact":
            assert got == RECORDED[name], pf
            continue
        # 'exact': 2 + 3 nCands back-pointers more per frame of the two sounds, nothing else
        s3 = AN.repair_track(AN.repair_pitch(sr, None, **kw), pathfinding="fast")
        frames = d["frames"] + AN.track_decisions_native(3 * length, s3)["frames"]
        assert got[0] == RECORDED[name][0] and got[1][:2] == RECORDED[name][1][:2]
        assert got[1][2] == RECORDED[name][1][2] + 8 * frames * (2 + 3 * s["nCands"])


def test_sweep_rows_share_everything_before_the_path():
    f, st, c = AN.sweep_plan(16000, [dict(), dict(pathfinding="exact"), dict(pathfinding="exact", certWeight=.2)])
    assert f.tolist() == [0, 0, 0] and st.tolist() == [0, 0, 0] and c.tolist() == [0, 0, 0]


# ------------------------------------------------------------ the GPU cases' inputs, checked on the CPU
# tests/test_pitch_candidates.py's _signal(16000, 1) (22 frames, two segments), under 'exact'
CASES = [
    (16000, "defaults", dict()),
    (16000, "step5", dict(step=5, snakeStep=0.1)),  # 110 frames: more frames than lanes (snakeStep: see tests/test_analyze.py)
    (16000, "all4-ncands3", dict(pitchMethods=TA.ALL4, nCands=3, cepThres=0.1, specPeak=0.2)),  # rows >= 5
    # an empty inner frame: no interpolation, and a pause long enough to keep the gap inside one segment. The snake is
    # not run on such a segment, so pitch is a candidate itself: at 16 kHz dom = 240 Hz then puts 1.25 * pitch on the
    # label 0.3 kHz exactly (tests/test_analyze.py, snakeStep0). The same samples read at 18.4 kHz (920-point frames,
    # a 253 -> 306 Hz glide) have no such label, and keep 'spec', so three rows
    (18400, "interpolWin0", dict(interpolWin=0, shortestPause=100)),
]
IDS = [c[1] for c in CASES]
MODES = ("exact", "fast", "none")


@lru_cache(maxsize=None)
def _reference(i, pathfinding="exact", plain=False):
    """analyze_numpy() of case i and its probe; plain: without the snake and the smoother (path_costs' setting)."""
    sr, _, kw = CASES[i]
    probe = {}
    kw = dict(kw, pathfinding=pathfinding, **(dict(snakeStep=0, smooth=0) if plain else {}))
    ref = AN.analyze_numpy(_signal(16000, 1), sr, _probe=probe, **kw)
    for v in ref.values():
        v.setflags(write=False)
    return ref, probe


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gpu_inputs_are_well_conditioned(i):
    """Every traced decision, the minima of 'exact' included, holds in the restatement alone
    with a relative margin >= 1e-6 on every GPU case; the cases are what they are meant to be."""
    ref, p = _reference(i)
    m = _margin(p)
    print(CASES[i][:2], "margin %.2e" % m, [(s["start_frame"], s["end_frame"], s["rows"], s["picks"], s["cost"]) for s in p["segments"]])
    assert m >= MARGIN and min(_tracker_margins(p).values()) >= MARGIN
    assert sum(len(s["exact"]) for s in p["segments"]) >= 8 and ref["voiced"].sum() >= 8
    pk = _pitch_kw(CASES[i][2])
    s = AN.repair_track(AN.repair_pitch(CASES[i][0], None, **pk), pathfinding="exact", **{k: v for k, v in CASES[i][2].items() if k not in pk})
    assert AN.track_decisions_native(len(_x()), s)["frames"] == len(ref["pitch"])  # the library takes the setting
    name = CASES[i][1]
    if name == "defaults":
        assert len(ref["pitch"]) == 22 and len(p["segments"]) == 2
    if name == "step5":
        assert len(ref["pitch"]) == 110 and max(s["end_frame"] - s["start_frame"] for s in p["segments"]) >= 30
    if name == "all4-ncands3":
        assert max(s["rows"] for s in p["segments"]) >= 5
    if name == "interpolWin0":  # a gap inside the segment, candidates on either side
        k = p["segments"][0]["picks"]
        assert len(p["segments"]) == 1 and None in k and k[0] is not None and k[-1] is not None and p["segments"][0]["rows"] >= 3
        assert np.isnan(ref["pitch"][p["segments"][0]["start_frame"] - 1:p["segments"][0]["end_frame"]]).any()
    # the run without snake and smoother, whose costs path_costs() is compared with
    for pf in MODES:
        q = _reference(i, pf, True)[1]
        assert [(s["start_frame"], s["end_frame"]) for s in q["segments"]] == [(s["start_frame"], s["end_frame"]) for s in p["segments"]]


@pytest.mark.parametrize("i", [0, 1], ids=IDS[:2])
def test_exact_is_never_dearer(i):
    """cost(exact) <= cost(fast) and cost(exact) <= cost(none) on every voiced segment of
    analyze_numpy (every frame of these segments has a candidate, so the three costs have
    the same denominators)."""
    costs = {pf: [s["cost"] for s in _reference(i, pf)[1]["segments"]] for pf in MODES}
    picks = {pf: [s["picks"] for s in _reference(i, pf)[1]["segments"]] for pf in MODES}
    print(CASES[i][1], costs)
    assert len(costs["exact"]) >= 2 and not any(None in k for pf in MODES for k in picks[pf])
    for e, f, n in zip(costs["exact"], costs["fast"], costs["none"]):
        assert e <= f and e <= n
    if CASES[i][1] == "defaults":
        assert costs["exact"][0] < costs["fast"][0]  # 'fast' leaves something on the table here


# ------------------------------------------------------------ sg_path.h on the host
SETTINGS = dict(TA.PATH_KW, pitchFloor=75, pitchCeiling=3500, priorMean="default", priorSD=6, interpolWin=3, interpolTol=0.3,
                interpolCert=0.3, pathfinding="exact", certWeight=.5, snakeStep=0.05, smooth=1, smoothVars=AN.SMOOTH_VARS)


def _pin_table():
    return TA._table([[2.0 ** v for v in f] for f in PIN_C], PIN_A)


@lru_cache(maxsize=None)
def _host_cases():
    """(table, settings, reference, probe): 400 segments of tests/test_analyze.py's generator under 'exact' (every fourth
    without interpolation, every fifth with certWeight 0.2) and 100 under 'fast' (the segment list and its costs are
    for every mode), the hand tables in their own mode and under 'exact', and the pinned case; kept where every
    traced decision has a margin >= MARGIN. Many are not: in a frame with two candidates both are equally far from
    their mean, so two tracks through the same pairs of candidates tie by construction ('none' on such frames
    decides by the last bit, which is why it is left to the hand tables here)."""
    rng = np.random.default_rng(7)
    out = []
    todo = []
    for i in range(500):
        t = TA._segment_table(rng)
        kw = dict(pathfinding="exact" if i < 400 else "fast")
        if i % 4 == 3:
            kw["interpolWin"] = 0
        if i % 5 == 4:
            kw["certWeight"] = 0.2
        todo.append((t, kw))
    for t, kw in TA._hand_tables():
        todo += [(t, dict(dict(pathfinding="fast"), **kw)), (t, dict(kw, pathfinding="exact"))]
    todo.append((_pin_table(), dict(pathfinding="exact", certWeight=.2, interpolWin=0, snakeStep=0, smooth=0, priorMean=None)))
    todo.append((_pin_table(), dict(pathfinding="fast", certWeight=.2, interpolWin=0, snakeStep=0, smooth=0, priorMean=None)))
    for t, kw in todo:
        kw = dict(TA.PATH_KW, **kw)
        p = {}
        r = AN.pitch_path_numpy(t, 25, 16000, _probe=p, **kw)
        if _margin(p) >= MARGIN:
            out.append((t, AN._path_settings(t, 25, 16000, dict(SETTINGS, **kw)), r, p))
    return out, len(todo)


def test_host_cases_cover_the_recursion():
    cases, n = _host_cases()
    print("kept %d of %d" % (len(cases), n))
    assert sum(ss["pathfinding"] == "exact" for _, ss, _, _ in cases) >= 200
    assert sum(ss["pathfinding"] == "fast" for _, ss, _, _ in cases) >= 50 and any(ss["pathfinding"] == "none" for _, ss, _, _ in cases)
    segs = [s for _, ss, _, p in cases if ss["pathfinding"] == "exact" for s in p["segments"]]
    assert sum(len(s["exact"]) >= 10 for s in segs) >= 100 and sum(None in s["picks"] for s in segs) >= 20
    assert sum(s["iterations"] > 3 for s in segs) >= 20 and sum(s["rows"] == 1 for s in segs) >= 1
    assert sum(math.isnan(s["cost"]) for s in segs) >= 1


def _build(tmp_path, sanitize):
    exe = str(tmp_path / ("path_exact_pins_san" if sanitize else "path_exact_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + TA.CSRC, os.path.join(TA.HERE, "cpp", "path_exact_pins.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_path_header_on_the_host_equals_restatement(tmp_path):
    """sg_path.h with 'exact' and the segment list compiled in, built for the host as a
    stand-alone program, plainly and under AddressSanitizer and UBSan: pitch within 1e-9,
    the segments' frames and rows equal, their costs within 1e-12, everything else exact.
    With the snake off, pitch is the picked candidate itself: the picks are then equal."""
    cases, _ = _host_cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for t, ss, _, _ in cases:
            n = len(t["ampl"])
            f.write(TA._pins_case(t, ss, AN.smoothing_hw(ss["smooth"], n, AN._path_length(t, 16000), 16000)) + "\n")
    exes = [_build(tmp_path, False)]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(_build(tmp_path, True))
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.split("\n")
        assert len(lines) == 2 * len(cases) + 1
        worst = worst_cost = 0.0
        for k, (t, ss, ref, p) in enumerate(cases):
            v = np.array([float.fromhex(x) for x in lines[2 * k].split()]).reshape(-1, 6)
            assert np.array_equal(np.isnan(v[:, 0]), np.isnan(ref["pitch"]))
            ok = ~np.isnan(ref["pitch"])
            if ok.any():
                worst = max(worst, float(np.max(np.abs(v[ok, 0] - ref["pitch"][ok]) / ref["pitch"][ok])))
            assert np.array_equal(v[:, 1], ref["dom"], equal_nan=True)
            assert np.allclose(v[:, 2], ref["HNR"], rtol=0, atol=1e-12, equal_nan=True)
            assert np.array_equal(v[:, 3], ref["amplVoiced"], equal_nan=True) and np.array_equal(v[:, 4] == 1, ref["voiced"])
            g = np.array([float.fromhex(x) for x in lines[2 * k + 1].split()]).reshape(-1, 4)
            assert len(g) == len(p["segments"])
            for row, s in zip(g, p["segments"]):
                assert (row[0], row[1], row[2]) == (s["start_frame"], s["end_frame"], s["rows"])
                assert math.isnan(row[3]) == math.isnan(s["cost"])
                if not math.isnan(s["cost"]):
                    worst_cost = max(worst_cost, abs(row[3] - s["cost"]) / s["cost"])
                if ss["snakeStep"] == 0 and ss["smooth"] == 0:  # the picks themselves
                    a, b = s["start_frame"] - 1, s["end_frame"]
                    want = [nan if q is None else 2.0 ** s["C"][f][q] for f, q in enumerate(s["picks"])]
                    assert v[a:b, 0] == pytest.approx(want, rel=1e-14, nan_ok=True)
        print(os.path.basename(exe), "cases", len(cases), "worst relative pitch error %.2e, cost error %.2e" % (worst, worst_cost))
        assert worst <= 1e-9 and worst_cost <= 1e-12


# ------------------------------------------------------------ GPU
def _x():
    return _signal(16000, 1)


def _pitch_kw(kw):
    return {k: v for k, v in kw.items() if k in inspect.signature(AN.pitch_candidates).parameters}


def _path_kw(kw):
    return {k: v for k, v in kw.items() if k in inspect.signature(AN.pitch_path).parameters and k != "step"}


def _step(sr, kw):
    return AN.repair_pitch(sr, len(_x()) / sr, **_pitch_kw(kw))["step"]


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_exact_gpu_equals_numpy(i):
    sr, _, kw = CASES[i]
    ref, _ = _reference(i)
    got = AN.analyze(_x(), sr, pathfinding="exact", **kw)
    TA._compare(got, ref, AN.pitch_candidates(_x(), sr, **_pitch_kw(kw)))


def _batch():
    """(host buffer, offsets, lengths): the signal, a silent sound and one too short for a frame."""
    parts = [_x().astype(np.float32), np.zeros(5000, np.float32), _signal(16000, 3, 0.41)[:700].astype(np.float32)]
    lens = np.array([len(v) for v in parts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    host = np.zeros(int(offs[-1] + lens[-1]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    return host, offs, lens


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_batch_exact_equals_single(i):
    import torch
    sr, _, kw = CASES[i]
    host, offs, lens = _batch()
    kw = dict(kw, pathfinding="exact")
    r = AN.analyze_batch(torch.from_numpy(host).cuda(), offs, lens, sr, **kw)
    h = r["out"].cpu().numpy()
    cols = r["cols"]
    assert r["frames"][2] == 0 and r["frames"][0] > 0 and r["frames"][1] > 0
    for c in (0, 1):
        f = r["frames"][c]
        got = h[r["offsets"][c]:r["offsets"][c] + f * cols].reshape(f, cols)
        one = AN.analyze(host[offs[c]:offs[c] + lens[c]].astype(np.float64), sr, **kw)
        want = np.column_stack([one[k] for k in AN.COLUMNS] + [one["autocorCand"], one["autocorCert"]] +
                               [one[k] for k in AN.PITCH_KEYS] + [one[k].astype(float) for k in AN.TRACK_COLUMNS])
        assert np.array_equal(got, want, equal_nan=True), c
        assert (one["voiced"].sum() >= 8) if c == 0 else (one["voiced"].sum() == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pitch_path_exact_equals_the_tail_of_analyze(i):
    """pitch_path() on the candidates the device made equals analyze()'s own tail bit for bit."""
    sr, _, kw = CASES[i]
    x = _signal(16000, 1).astype(np.float32).astype(np.float64)
    full = AN.analyze(x, sr, pathfinding="exact", **kw)
    pc = AN.pitch_candidates(x, sr, **_pitch_kw(kw))
    got = AN.pitch_path(pc, _step(sr, kw), sr, pathfinding="exact", **_path_kw(kw))
    assert got["voiced"].sum() >= 8
    for k in ("pitch", "voiced", "amplVoiced", "dom", "HNR", "quartile25", "quartile50", "quartile75", "ampl", "domCand", "specCand"):
        assert np.array_equal(got[k], full[k], equal_nan=True), k


def _device_picks(seg, pitch):
    """The candidate each frame's pitch is (snake and smoother off: pitch = 2 ^ candidate)."""
    out = []
    for f, c in enumerate(seg["C"]):
        v = pitch[seg["start_frame"] - 1 + f]
        if math.isnan(v):
            out.append(None)
            continue
        k = int(np.argmin([abs(2.0 ** u - v) for u in c]))
        assert abs(2.0 ** c[k] - v) <= 1e-12 * v
        out.append(k)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_path_costs_gpu(i):
    """path_costs() without snake and smoother under 'exact', 'fast' and 'none' on the device's
    own candidates: every cost within 1e-12 of cost_per_path on the restatement's picks, and
    'exact' never dearer than 'fast' or 'none'.

    Two conditions, both properties of the input and not of the code. (1) Where the
    restatement's own choice in a segment has a margin below 1e-6 (with two candidates in a
    frame both are equally far from their mean, and 'none' decides by the last bit of a log2:
    tests/test_analyze.py's 'none' case), its picks are no reference; the cost is then
    cost_per_path on the picks read from the device's pitch, which must be candidates. (2)
    'fast' may leave a frame that has candidates without a value (no backward start next to an
    empty frame); its mean then has other denominators and is not the function 'exact'
    minimises, so the order is asserted where both paths have a value in the same frames."""
    sr, _, kw = CASES[i]
    x = _x()
    pc = AN.pitch_candidates(x, sr, **_pitch_kw(kw))
    step = _step(sr, kw)
    pkw = dict(_path_kw(kw), snakeStep=0, smooth=0)
    cost, picks = {}, {}
    for pf in MODES:
        got, segs = AN.path_costs(pc, step, sr, pathfinding=pf, **pkw)
        p = {}
        ref = AN.pitch_path_numpy(pc, step, sr, pathfinding=pf, _probe=p, **pkw)
        assert np.array_equal(got["voiced"], ref["voiced"]) and len(segs) == len(p["segments"]) >= 1
        plain = AN.pitch_path(pc, step, sr, pathfinding=pf, **pkw)
        assert np.array_equal(got["pitch"], plain["pitch"], equal_nan=True)  # the table is pitch_path()'s
        cost[pf], picks[pf] = [], []
        for g, s in zip(segs, p["segments"]):
            assert (g["start_frame"], g["end_frame"], g["rows"]) == (s["start_frame"], s["end_frame"], s["rows"])
            sure = min(TA._pairs(s[k]) for k in ("start", "choice", "fb", "exact")) >= MARGIN
            k = s["picks"] if sure else _device_picks(s, got["pitch"])
            assert pf != "exact" or sure
            want = AN.cost_per_path(s["C"], s["cog"], k, kw.get("certWeight", .5))
            print(CASES[i][1], pf, g, "want %r" % want, "restatement's picks" if sure else "device's picks")
            assert math.isnan(g["cost"]) == math.isnan(want)
            assert math.isnan(want) or abs(g["cost"] - want) <= 1e-12 * want
            cost[pf].append(g["cost"])
            picks[pf].append([q is None for q in k])
    for j, e in enumerate(cost["exact"]):
        for pf in ("fast", "none"):
            if picks[pf][j] == picks["exact"][j]:
                assert e <= cost[pf][j], (pf, j)
    # 'none' always has a value where a frame has candidates; so has 'fast' unless a frame is empty
    assert picks["none"] == picks["exact"] and (picks["fast"] == picks["exact"] or CASES[i][1] == "interpolWin0")


@pytest.mark.gpu
def test_path_costs_hand_tables_gpu():
    """The pinned case and the hand tables (empty frames, a one-row table, two segments) through
    pitch_path() and path_costs() under 'exact' against the restatement."""
    t = _pin_table()
    kw = dict(TA.PATH_KW, certWeight=.2, interpolWin=0, snakeStep=0, smooth=0, priorMean=None)
    got, segs = AN.path_costs(t, 25, 16000, pathfinding="exact", **kw)
    assert got["pitch"] == pytest.approx([2.0 ** 7.011, 2.0 ** 7.196, 2.0 ** 7.149], rel=1e-12)
    assert len(segs) == 1 and (segs[0]["start_frame"], segs[0]["end_frame"], segs[0]["rows"]) == (1, 3, 4)
    assert segs[0]["cost"] == pytest.approx(0.17355050795414312, rel=1e-12)
    _, segs = AN.path_costs(t, 25, 16000, pathfinding="fast", **kw)
    assert segs[0]["cost"] == pytest.approx(0.9288844095787764, rel=1e-12)
    worst, kept = 0.0, 0
    split = [[8.0, 9.0], [8.0, 8.1], [], [9.0, 9.2], [8.0, 9.05]]  # test_empty_frame_splits_two_runs: two runs in one segment
    split = (TA._table([[2.0 ** v for v in f] for f in split], [[.5] * len(f) for f in split]), dict(interpolWin=0, priorMean=None))
    for t, hkw in TA._hand_tables() + [split]:
        kw = dict(TA.PATH_KW, **dict(hkw, pathfinding="exact"))
        p = {}
        ref = AN.pitch_path_numpy(t, 25, 16000, _probe=p, **kw)
        if _margin(p) < MARGIN:  # [8, 9] around their mean 8.5 with no neighbour: a tie by construction
            continue
        kept += 1
        got, segs = AN.path_costs(t, 25, 16000, **kw)
        worst = max(worst, TA._compare_path(got, ref))
        assert np.array_equal(AN.pitch_path(t, 25, 16000, **kw)["pitch"], got["pitch"], equal_nan=True)
        assert len(segs) == len(p["segments"])
        for g, s in zip(segs, p["segments"]):
            assert (g["start_frame"], g["end_frame"], g["rows"]) == (s["start_frame"], s["end_frame"], s["rows"])
            assert math.isnan(g["cost"]) == math.isnan(s["cost"])
            assert math.isnan(s["cost"]) or abs(g["cost"] - s["cost"]) <= 1e-12 * s["cost"]
    print("hand tables under 'exact': %d, worst relative pitch error %.2e" % (kept, worst))
    assert kept >= 4  # the tables without a tie: no neighbours, one row, the smoother's outliers, the two runs
    empty = dict(TA._table([], []), duration=np.zeros(0))
    got, segs = AN.path_costs(empty, 25, 16000, pathfinding="exact")
    assert len(got["pitch"]) == 0 and segs == []


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_sweep_exact_equals_batch(i):
    """Rows with 'fast' and 'exact' in one sweep: every pair's 44 cells equal
    analyze_batch(summary=True) under that row bit for bit."""
    import torch
    sr, _, kw = CASES[i]
    host, offs, lens = _batch()
    data = torch.from_numpy(host).cuda()
    rows = [dict(kw), dict(kw, pathfinding="exact"), dict(kw, pathfinding="exact", certWeight=.2)]
    f, st, c = AN.sweep_plan(sr, rows)
    assert f.tolist() == [0, 0, 0] and len(set(st.tolist())) == 1 and c.tolist() == [0, 0, 0]
    got = AN.analyze_sweep(data, offs, lens, sr, rows).cpu().numpy()
    assert got.shape == (3, 3, 44)
    for r, row in enumerate(rows):
        want = AN.analyze_batch(data, offs, lens, sr, summary=True, **row)["out"].cpu().numpy()
        assert np.array_equal(got[r], want, equal_nan=True), r
    assert not np.isnan(got[:, 0, :2]).any() and np.isnan(got[:, 2]).all()
    # a small workspace cap puts every row in a chunk of its own: the same cells
    capped = AN.analyze_sweep(data, offs, lens, sr, rows, workspace_cap=1).cpu().numpy()
    assert np.array_equal(capped, got, equal_nan=True)
