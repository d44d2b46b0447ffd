"""analyze(): the tail behind the pitch candidates (R/analyze.R:576-707,
R/utilities_pitch_postprocessing.R: the prior, findVoicedSegments, pathfinder, medianSmoother,
the final columns): the numpy restatement pinned by hand, sg_analyze_size against it,
sg_path.h compiled for the host against it, and the GPU (sg_anl_path, sg_anl_harm in
sg_analyze.hip) against it.

No R is installed: soundgen_beta_amd/analyze.py restates the reference statement by
statement with line citations, the CPU tests pin its parts on cases worked by hand, and
the host build of sg_path.h and the GPU are compared with it.

Bars. voiced, the NaN patterns, amplVoiced, the quartiles, the smoothed dom and every
column analyze() does not rewrite must match exactly (the untouched columns bit for bit
with pitch_candidates()); test_gpu_inputs_are_well_conditioned shows that every discrete
decision behind them holds in the restatement alone with a relative margin >= 1e-6
(MARGIN). pitch: 1e-9 relative (fp64 rounding through at most a few hundred
non-amplifying snake steps is orders below that; the smallest real error, one snake step
or a neighbouring candidate, is above 1e-4). HNR and harmonics in dB: |delta| <= 4.35 *
d / (x (1 - x)) for the reference's ratio x, to_dB's derivative times a ratio error d:
d = 1e-12 for harmonics (at most 2048 positive terms), 1e-13 for HNR (about twice the HNR
bar of tests/test_pitch_candidates.py).

Measured on an MI355X, the maxima over the GPU cases below: see DESIGN.md section 5.
"""
import inspect
import math
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
from test_pitch_candidates import _margins as _tracker_margins
from test_pitch_candidates import _signal

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
MARGIN = 1e-6
ALL4 = ("autocor", "cep", "spec", "dom")
nan = math.nan


def _hz(*log2s):
    return [2.0 ** v for v in log2s]


def _jump(a, b):
    """costJumps(), written out independently of the module."""
    return 1 / (1 + 10 * math.exp(3 - 7 * abs(a - b)))


# ------------------------------------------------------------ CPU: the routines by hand
def test_find_voiced_segments_by_hand():
    # noRequired = 2, one tolerated NA: the gap at frame 3 is bridged; frames 6-7 end the segment at i - 1 = 5;
    # frames 9-10 are voiced but i stops below n - noRequired + 1 = 9: the tail cannot start a segment
    assert AN.find_voiced_segments([2, 2, 0, 2, 2, 0, 0, 0, 2, 2], 2, 2, 1) == [(1, 5)]
    # the same tail with one more frame behind it does start one, ended by the last voiced frame
    assert AN.find_voiced_segments([2, 2, 0, 2, 2, 0, 0, 0, 2, 2, 0], 2, 2, 1) == [(1, 5), (9, 10)]
    # no window of nToleratedNA + 1 frames fits behind i: the end is the last voiced frame
    assert AN.find_voiced_segments([0, 2, 2, 2, 0], 2, 1, 3) == [(2, 4)]
    # nToleratedNA = 0: every NA ends a segment; the last frame never starts one (i < n)
    assert AN.find_voiced_segments([1, 0, 1, 1, 0, 1], 1, 1, 0) == [(1, 1), (3, 4)]
    # minVoicedCands counts candidates
    assert AN.find_voiced_segments([1, 2, 3, 1, 1], 2, 1, 0) == [(2, 3)]
    assert AN.find_voiced_segments([], 1, 1, 2) == [] and AN.find_voiced_segments([0, 0, 0], 1, 1, 2) == []
    assert AN.find_voiced_segments([1, 1], 1, 3, 2) == []  # shorter than noRequired


def test_repair_track_settings():
    s = AN.repair_track(AN.repair_pitch(16000, None))
    assert (s["minVoicedCands"], s["noRequired"], s["nToleratedNA"]) == (2, 1, 2)  # 20 / 25 -> 1; 60 / 25 -> 2
    assert s["priorMean"] == AN.hz_to_semitones(300) and s["interpolTol"] == 0.3
    assert AN.repair_track(AN.repair_pitch(16000, None, pitchMethods=("dom",)))["minVoicedCands"] == 1
    assert AN.repair_track(AN.repair_pitch(16000, None, pitchMethods=("autocor", "cep")))["minVoicedCands"] == 1
    assert AN.repair_track(AN.repair_pitch(16000, None), minVoicedCands=4)["minVoicedCands"] == 2  # above 3 methods
    assert AN.repair_track(AN.repair_pitch(16000, None), minVoicedCands=3)["minVoicedCands"] == 3
    s = AN.repair_track(AN.repair_pitch(16000, None, step=7), shortestSyl=20, shortestPause=60)
    assert (s["noRequired"], s["nToleratedNA"]) == (3, 8)
    assert AN.repair_track(AN.repair_pitch(16000, None), priorMean=None)["priorMean"] is None
    assert AN.repair_track(AN.repair_pitch(16000, None), priorSD="a")["priorSD"] is None
    for kw in (dict(plot=True), dict(priorPlot=True), dict(snakePlot=True), dict(smoothVars=("pitch", "HNR"))):
        with pytest.raises(NotImplementedError):
            AN.repair_track(AN.repair_pitch(16000, None), **kw)
    for kw in (dict(interpolWin=2.5), dict(certWeight=1.5), dict(certWeight=-0.1), dict(pathfinding="quick"),
               dict(priorSD=0)):
        with pytest.raises(ValueError):
            AN.repair_track(AN.repair_pitch(16000, None), **kw)
    # half-even rounding of smoothing_ww: 2.5 -> 2, 3.5 -> 4
    assert AN.smoothing_hw(1, 25, 16000, 16000) == 1 and AN.smoothing_hw(1, 35, 16000, 16000) == 2
    assert AN.smoothing_hw(0, 25, 16000, 16000) == 0 and AN.smoothing_hw(1, 40, 16000, 16000) == 2


def test_interpolated_frame_enters_the_next_median():
    # log2 candidates 8, -, -, 9 with interpolWin = 1. Frame 2: median(8, NA, NA) = 8 is added and its centre of
    # gravity becomes 8; frame 3 then sees median(8, NA, 9) = 8.5 (without the update: 9). One candidate per
    # frame: a one-row segment, returned as 2 ^ pitchCands without pathfinding or snake.
    tr = {}
    p = AN.pathfinder_numpy([_hz(8), [], [], _hz(9)], [[.5], [], [], [.5]], interpolWin=1, interpolTol=0.05, _trace=tr)
    assert p == [256.0, 256.0, 2.0 ** 8.5, 512.0]
    assert tr["interpolated"] == 2 and tr["rows"] == 1 and tr["iterations"] == 0 and tr["direction"] is None
    # frame 4: median(8.5, 9) = 8.75, the band 8.75 * (1 -+ 0.05) holds 9: nothing added; the tolerance multiplies a log2
    assert (9.0, 8.75 * 1.05) in tr["band"] and (9.0, 8.75 * 0.95) in tr["band"]
    # with the tolerance at 0.01 the band (8.6625, 8.8375) misses 9: 8.75 is added, two rows, 'none' picks the nearer
    p = AN.pathfinder_numpy([_hz(8), [], [], _hz(9)], [[.5], [], [], [.5]], pathfinding="none", interpolWin=1,
                            interpolTol=0.01, snakeStep=0)
    assert p[:3] == [256.0, 256.0, 2.0 ** 8.5] and p[3] == 2.0 ** 8.75  # |8.75 - 8.875| = |9 - 8.875|: the first (lowest)
    # a one-row segment with an NA frame and no interpolation
    p = AN.pathfinder_numpy([[300.0], [], [310.0]], [[.4], [], [.4]], interpolWin=0)
    assert math.isnan(p[1]) and p[::2] == pytest.approx([300.0, 310.0], rel=1e-15)


def test_fast_backward_wins():
    # frames {8 (.9), 9 (.1)}, {8, 9}, {9}: forward starts at 8 (.9 / .5 > .1 / .5 around the median 8.5), keeps 8 in
    # frame 2 and must jump to 9 in frame 3; backward starts at 9 and stays: cheaper
    tr = {}
    p = AN.pathfinder_numpy([_hz(8, 9), _hz(8, 9), _hz(9)], [[.9, .1], [.5, .5], [.5]], certWeight=.5, pathfinding="fast",
                            interpolWin=0, snakeStep=0, _trace=tr)
    assert p == [512.0, 512.0, 512.0] and tr["direction"] == "backward"
    costF = (.5 * .5 + .5 * _jump(8, 8)) + (.5 * 0 + .5 * _jump(8, 9))
    costB = 2 * (.5 * .5 + .5 * _jump(9, 9))
    assert tr["fb"] == [pytest.approx((costF, costB), rel=1e-14)] and costB < costF
    # point_current is never updated: with a third step to 10 the forward cost still measures jumps from the start
    tr = {}
    AN.pathfinder_numpy([_hz(8, 8.5), _hz(9), _hz(10)], [[.9, .1], [.5], [.5]], interpolWin=0, snakeStep=0, _trace=tr)
    assert tr["fb"][0][0] == pytest.approx(.5 * _jump(8, 9) + .5 * _jump(8, 10), rel=1e-14)
    # forward wins on the mirror image
    tr = {}
    p = AN.pathfinder_numpy([_hz(9), _hz(8, 9), _hz(8, 9)], [[.5], [.5, .5], [.9, .1]], interpolWin=0, snakeStep=0, _trace=tr)
    assert p == [512.0] * 3 and tr["direction"] == "forward"
    with pytest.raises(NotImplementedError):
        AN.pathfinder_numpy([_hz(8, 9)], [[.5, .5]], pathfinding="slow")


def test_find_grad_by_hand():
    assert AN.find_grad([5.0]) == [0.0]  # interpol = 1: the ends repeated
    assert AN.find_grad([1.0, 3.0]) == [0.0, 0.0]  # slope 2 either side: a line
    # slopes (1 - 0) / 2 and (0 - 1) / 2: -1, -.5, 0, 0, 1, 0, 0, -.5, -1
    assert AN.find_grad([0.0, 0, 1, 0, 0]) == [2.0, -4.5, 6.0, -4.5, 2.0]
    # three points: both slopes (4 - 0) / 2: -4, -2, 0, 1, 4, 6, 8
    assert AN.find_grad([0.0, 1, 4]) == [-4 + 8 + 0 - 4 + 4, -2 - 0 + 6 - 16 + 6, 0 - 4 + 24 - 24 + 8]


def test_one_snake_iteration_by_hand():
    cands = [[8.0, 8.1, 8.6], [8.0, 8.2, 8.72]]
    cert = [[.5, .3, .2], [.6, .4, .7]]
    pitch = [8.1, 8.2]  # two points: findGrad gives 0
    f = AN.force_per_path(pitch, cands, cert, 0.5)
    e0 = -.5 / math.exp(.1 ** 2) - .3 + .2 / math.exp(.5 ** 2)  # 8.1 == pitch: cands > pitch is false, it pushes with -cert
    e1 = -.6 / math.exp(.2 ** 2) - .4 + .7 / math.exp(.52 ** 2)
    assert f == pytest.approx([.5 * e0, .5 * e1], rel=1e-12)
    # pathfinder: 'none' picks 8.1 and 8.2 (nearest the means 8.2333 and 8.3067); maxIter = floor(.72 / .05 * 2 = 28.8);
    # the first force_delta is (1e10 - force_new) / 1e10, nearly 1: the snake moves by snakeStep * force
    tr = {}
    hz = [[2.0 ** v for v in fr] for fr in cands]
    p = AN.pathfinder_numpy(hz, cert, certWeight=.5, pathfinding="none", interpolWin=0, snakeStep=0.05, _trace=tr)
    assert tr["maxiter"] == [(pytest.approx(28.8, abs=1e-9), 29.0)] and tr["iterations"] >= 1
    assert tr["delta"][0] == (pytest.approx(1 - (abs(f[0]) + abs(f[1])) / 2 / 1e10, rel=1e-12), 0.05)
    want = [math.log2(hz[0][1]), math.log2(hz[1][1])]
    force_old = 1e10
    for _ in range(27):  # i = 1 .. 27 < maxIter
        f = AN.force_per_path(want, [[math.log2(v) for v in fr] for fr in hz], cert, 0.5)
        new = (abs(f[0]) + abs(f[1])) / 2
        delta, force_old = (force_old - new) / force_old, new
        if delta < 0.05:
            break
        want = [want[0] + 0.05 * f[0], want[1] + 0.05 * f[1]]
    assert p == pytest.approx([2.0 ** want[0], 2.0 ** want[1]], rel=1e-13)
    # maxIter = 2: one iteration at most
    tr = {}
    AN.pathfinder_numpy(hz, cert, certWeight=.5, pathfinding="none", interpolWin=0, snakeStep=0.7, _trace=tr)
    assert tr["maxiter"][0][1] == 2.0 and tr["iterations"] == 1 and len(tr["delta"]) == 1


def test_smoother_subtracts_one():
    up, down = 100 * 2 ** (4.5 / 12), 100 * 2 ** (-3.5 / 12)
    # +4.5 semitones: |4.5 - 1| = 3.5 is not above 4: kept (abs(deviance) would replace it)
    assert AN.median_smoother([100, 100, up, 100, 100], 5, 4.0)[2] == up
    # -3.5 semitones: |-3.5 - 1| = 4.5 is above 4: replaced (abs(deviance) would keep it)
    assert AN.median_smoother([100, 100, down, 100, 100], 5, 4.0)[2] == 100
    # NaN stays NaN and is left out of the medians (na.rm = TRUE)
    x = AN.median_smoother([nan, 100, 30, 100, nan], 5, 4.0)
    assert math.isnan(x[0]) and math.isnan(x[4]) and x[2] == 100
    assert AN.median_smoother([100.0, 30, 100], 0, 4.0).tolist() == [100.0, 30, 100]  # hw = 0: its own median


def test_empty_frame_keeps_nan_and_its_neighbours():
    """The one stated difference from the reference (see analyze_numpy)."""
    tr = {}
    p = AN.pathfinder_numpy([_hz(8, 9), [], _hz(8)], [[.9, .2], [], [.5]], interpolWin=0, snakeStep=0.05, _trace=tr)
    # forward: median(8.5, 8) = 8.25, start 8 (.9 / .25 > .2 / .75), frame 3 costs .5 * costJumps(8, 8); backward: the
    # median of (8, NA, 8.5) is NA: no start, no jump cost, frame 1 costs .5 * .5: forward wins
    assert p[0] == 256.0 and math.isnan(p[1]) and p[2] == 256.0
    assert tr["direction"] == "forward" and tr["iterations"] == 0 and tr["maxiter"] == []  # no snake
    assert tr["fb"] == [pytest.approx((.5 * _jump(8, 8), .25), rel=1e-14)]
    # the mirror image: backward (from no start, all its jump costs 0) wins and its first frame, the segment's
    # last, has no choice either
    tr = {}
    p = AN.pathfinder_numpy([_hz(8), [], _hz(8, 9)], [[.5], [], [.9, .2]], interpolWin=0, snakeStep=0.05, _trace=tr)
    assert p[0] == 256.0 and math.isnan(p[1]) and math.isnan(p[2]) and tr["direction"] == "backward"
    # 'none' likewise; the other frames are the nearest to their centre of gravity
    p = AN.pathfinder_numpy([_hz(8, 8.1, 9), [], _hz(8, 8.8, 9)], [[.5] * 3, [], [.5] * 3], pathfinding="none", interpolWin=0)
    assert p[::2] == pytest.approx([2.0 ** 8.1, 2.0 ** 8.8], rel=1e-14) and math.isnan(p[1])
    # with interpolation the gap is filled and the snake runs
    tr = {}
    p = AN.pathfinder_numpy([_hz(8, 8.1, 9), [], _hz(8, 8.8, 9)], [[.5] * 3, [], [.5] * 3], interpolWin=3, interpolTol=0.3, _trace=tr)
    assert not np.isnan(p).any() and tr["interpolated"] == 1 and tr["maxiter"]


def test_prior_multiplier_equals_scipy():
    stats = pytest.importorskip("scipy.stats")
    for mean, sd, lo, hi in ((AN.hz_to_semitones(300), 6, 75, 3500), (AN.hz_to_semitones(150), 2.5, 50, 1000), (40.0, 20, 30, 8000)):
        prior = AN.prior_setup(mean, sd, lo, hi)
        shape, rate = mean ** 2 / sd ** 2, mean / sd ** 2
        grid = np.linspace(AN.hz_to_semitones(lo), AN.hz_to_semitones(hi), 100)
        norm = stats.gamma.pdf(grid, a=shape, scale=1 / rate).max()
        for hz in np.exp(np.linspace(np.log(lo), np.log(hi), 40)):
            want = stats.gamma.pdf(AN.hz_to_semitones(hz), a=shape, scale=1 / rate) / norm
            assert AN.prior_multiplier(hz, prior) == pytest.approx(want, rel=1e-12)
    assert AN.prior_multiplier(10.0, prior) == 0.0  # below C0: a negative semitone value
    assert AN.prior_multiplier(300.0, AN.prior_setup(AN.hz_to_semitones(300), 6, 75, 3500)) > 0.99


def test_to_dB():
    v = AN.to_dB([0.5, 0.9, 0.0, -0.2, nan, 0.9999])
    assert v[0] == 0 and v[1] == pytest.approx(10 * math.log10(9), rel=1e-15) and v[2] == -math.inf
    assert math.isnan(v[3]) and math.isnan(v[4]) and v[5] == pytest.approx(39.9996, abs=1e-3)


def test_pitch_path_numpy_by_hand():
    # five frames, nCands = 1, the default methods: dom + spec agree around 256 in frames 2-4, frame 1 has dom alone
    # (one candidate: not voiced with minVoicedCands 2), frame 5 nothing
    n = 5
    t = dict(ampl=np.full(n, .5), HNR=np.full(n, .5), dom=np.array([250.0, 256, 256, 256, nan]),
             quartile25=np.arange(n) + 1.0, quartile50=np.arange(n) + 2.0, quartile75=np.arange(n) + 3.0,
             domCand=np.array([250.0, 256, 256, 256, nan]), domCert=np.array([.5, .5, .5, .5, nan]),
             specCand=np.array([[nan], [256.0], [256.0], [256.0], [nan]]), specCert=np.array([[nan], [.6], [.6], [.6], [nan]]),
             duration=np.full(n, n * 0.025))
    p = {}
    r = AN.pitch_path_numpy(t, 25, 16000, priorMean=None, _probe=p)
    assert [(s["start_frame"], s["end_frame"]) for s in p["segments"]] == [(2, 4)]
    assert r["voiced"].tolist() == [False, True, True, True, False]
    assert r["pitch"][1:4] == pytest.approx([256.0] * 3, rel=1e-12) and np.isnan(r["pitch"][[0, 4]]).all()
    assert np.array_equal(r["amplVoiced"], [nan, .5, .5, .5, nan], equal_nan=True)
    assert np.array_equal(r["quartile50"], [nan, 3, 4, 5, nan], equal_nan=True) and np.all(r["HNR"] == 0)
    assert np.all(np.isnan(r["harmonics"])) and t["HNR"][0] == .5  # the caller's table is not changed
    with pytest.raises(NotImplementedError):
        AN.pitch_path_numpy(t, 25, 16000, pathfinding="slow")


# ------------------------------------------------------------ sg_analyze_size
@pytest.mark.parametrize("sr", [16000, 22050, 44100, 48000])
def test_sg_analyze_size_equals_restatement(sr):
    n = 0
    for step in (None, 5, 10, 12.5, 25):
        for smooth, syl, pause in ((1, 20, 60), (0, 0, 0), (2.5, 33, 61), (6, 20, 59.9), (1, 101, 12)):
            s = AN.repair_track(AN.repair_pitch(sr, None, step=step), smooth=smooth, shortestSyl=syl, shortestPause=pause)
            wl = AN.pitch_decisions(0, s)["wl"]
            for length in (wl, wl + 1, 3 * wl + 17, int(0.6 * sr), int(2.5 * sr) + 3):
                want, got = AN.track_decisions(length, s), AN.track_decisions_native(length, s)
                keys = AN.TRACK_SIZE_KEYS + ("frames", "cols")
                assert {k: got[k] for k in keys} == {k: want[k] for k in keys}, (step, smooth, syl, pause, length)
                assert want["cols"] == 15 + 6 + 4
                n += 1
    assert n == 125
    d = AN.track_decisions_native(9600, AN.repair_track(AN.repair_pitch(16000, None)))
    assert [d[k] for k in AN.TRACK_SIZE_KEYS] == [2, 1, 2, 2, 3]


def test_track_refusals_on_the_host():
    base = AN.repair_pitch(16000, None)
    for dec in (AN.track_decisions, AN.track_decisions_native):
        with pytest.raises(native.SoundgenError, match="slow") as e:
            dec(9600, AN.repair_track(base, pathfinding="slow"))
        assert e.value.code == -4
        with pytest.raises(native.SoundgenError, match="at most 64") as e:
            dec(9600, AN.repair_track(base, interpolWin=65))
        assert e.value.code == -4
        with pytest.raises(native.SoundgenError, match="at most 64"):  # 200 frames / s: smoothing_ww = 140, hw = 70
            dec(96000, AN.repair_track(AN.repair_pitch(16000, None, step=5), smooth=7))
        assert 60 <= dec(96000, AN.repair_track(AN.repair_pitch(16000, None, step=5), smooth=6.4))["hw"] <= 64
        with pytest.raises(native.SoundgenError, match="snakeStep"):
            dec(9600, AN.repair_track(base, snakeStep=0.001))
        assert dec(9600, AN.repair_track(base, interpolWin=64, snakeStep=0.005))["interpolWin"] == 64
    P = AN._track_params(AN.repair_track(base))
    for field, v in (("interpolWin", 2.5), ("certWeight", 1.01), ("certWeight", -0.01), ("priorSD", -1.0)):
        Q = type(P).from_buffer_copy(P)
        setattr(Q, field, v)
        import ctypes as C
        fr, cl = C.c_int32(), C.c_int32()
        assert native.lib().sg_analyze_size(9600, C.byref(Q), C.byref(fr), C.byref(cl), None) == -1, field
    with pytest.raises(NotImplementedError):
        AN.analyze_numpy(np.zeros(4000), 16000, pathfinding="slow")
    with pytest.raises(NotImplementedError):
        AN.analyze_numpy(np.zeros(4000), 16000, plot=True)
    with pytest.raises(ValueError, match="not longer than the window"):
        AN.analyze_numpy(np.sin(np.arange(800.0)), 16000)


# ------------------------------------------------------------ sg_path.h on the host
PATH_KW = dict(pitchMethods=ALL4, minVoicedCands=1, shortestSyl=0, shortestPause=25 * 50)  # a table is one segment
SLOTS = ("domCand", "autocorCand", "cepCand", "specCand")


def _segment_table(rng):
    """A random voiced segment as a pitch_candidates()-shaped table: 2-40 frames, a wobbling
    contour, 0-4 candidates per frame (both ends non-empty) with octave errors of both signs
    and random certainties."""
    n = int(rng.integers(2, 41))
    x = np.arange(n)
    contour = math.log2(rng.uniform(120, 600)) + 0.15 * np.sin(2 * np.pi * x / n * rng.uniform(0.5, 2) + rng.uniform(0, 6)) \
        + np.cumsum(rng.normal(0, 0.01, n))
    t = dict(ampl=rng.uniform(0.05, 0.9, n), HNR=rng.uniform(0.05, 0.95, n), quartile25=rng.uniform(300, 900, n),
             quartile50=rng.uniform(900, 1500, n), quartile75=rng.uniform(1500, 3000, n), duration=np.full(n, n * 0.025))
    for k in SLOTS:
        t[k], t[k.replace("Cand", "Cert")] = np.full((n, 1), nan), np.full((n, 1), nan)
    for f in range(n):
        k = int(rng.choice(5, p=[.12, .25, .3, .2, .13]))
        if f in (0, n - 1):
            k = max(k, 1)
        for slot in rng.permutation(4)[:k]:
            octave = rng.choice([0, 1, -1], p=[.75, .125, .125])
            t[SLOTS[slot]][f, 0] = 2.0 ** (contour[f] + rng.normal(0, 0.02) + octave)
            t[SLOTS[slot].replace("Cand", "Cert")][f, 0] = rng.uniform(0.05, 1)
    t["dom"] = t["domCand"][:, 0].copy()
    t["domCand"], t["domCert"] = t["domCand"][:, 0], t["domCert"][:, 0]
    return t


def _rel(a, b):
    if a == b:
        return 0.0
    if math.isinf(a) or math.isinf(b):
        return 1.0
    return abs(a - b) / max(abs(a), abs(b))


def _pairs(pairs):
    return min([_rel(a, b) for a, b in pairs] + [math.inf])


def _track_margin(p):
    """The smallest relative margin of every traced decision of the tail in a restatement run."""
    m = min(_pairs(p["smooth"]), _pairs(p["harm"]))
    for s in p["segments"]:
        m = min([m] + [_pairs(s[k]) for k in ("band", "start", "choice", "fb", "maxiter", "delta", "force")])
    return m


@lru_cache(maxsize=None)
def _generated():
    """(tables, references, probes) of the generator's 2000 segments, and the indices kept
    (smallest traced margin >= MARGIN)."""
    rng = np.random.default_rng(7)
    tabs, refs, probes, kept = [], [], [], []
    for i in range(2000):
        t = _segment_table(rng)
        p = {}
        r = AN.pitch_path_numpy(t, 25, 16000, _probe=p, **PATH_KW)
        tabs.append(t)
        refs.append(r)
        probes.append(p)
        if _track_margin(p) >= MARGIN:
            kept.append(i)
    return tabs, refs, probes, kept


def _rows(t, nC=1):
    m = np.column_stack([t[k] if k in t else np.full(len(t["ampl"]), nan) for k in AN.COLUMNS] +
                        [t[k] for k in ("autocorCand", "autocorCert") + AN.PITCH_KEYS])
    assert m.shape[1] == 15 + 6 * nC
    return m


def _pins_case(t, s, hw):
    prior = AN.prior_setup(s["priorMean"], s["priorSD"], s["pitchFloor"], s["pitchCeiling"]) if s["priorMean"] is not None \
        else (0.0, 0.0, 0.0, 1.0)
    head = [s["nCands"], len(t["ampl"]), hw, s["minVoicedCands"], s["noRequired"], s["nToleratedNA"], s["interpolWin"],
            AN.PATHFINDING.index(s["pathfinding"]), int(s["priorMean"] is not None), int("pitch" in s["smoothVars"] and s["smooth"] > 0),
            int("dom" in s["smoothVars"] and s["smooth"] > 0)] + list(prior) + \
           [s["interpolTol"], s["interpolCert"], s["certWeight"], s["snakeStep"], 4 / s["smooth"] if s["smooth"] > 0 else 0.0]
    return " ".join(float(v).hex() for v in head + _rows(t).ravel().tolist())


def test_generated_segments_cover_the_tail():
    tabs, refs, probes, kept = _generated()
    print("kept %d of %d" % (len(kept), len(tabs)))
    assert len(kept) >= 0.9 * len(tabs)  # at most 10 % dropped
    segs = [probes[i]["segments"][0] for i in kept]
    assert all(len(probes[i]["segments"]) == 1 for i in kept)
    assert sum(s["interpolated"] for s in segs) >= 100
    assert sum(s["direction"] == "forward" for s in segs) >= 20 and sum(s["direction"] == "backward" for s in segs) >= 20
    assert sum(s["iterations"] > 3 for s in segs) >= 20
    assert sum(s["rows"] == 1 for s in segs) >= 1
    # interpolate() fills every gap of a segment when interpolWin >= 1 (a filled frame enters the next median)
    assert not any(np.isnan(refs[i]["pitch"]).any() for i in kept)


def _build_pins(tmp_path, sanitize):
    exe = str(tmp_path / ("path_pins_san" if sanitize else "path_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "path_pins.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_path_header_on_the_host_equals_restatement(tmp_path):
    """sg_path.h (what the lanes of sg_anl_path run) built for the host as a stand-alone
    program, plainly and under AddressSanitizer and UBSan, on the kept generated segments
    and the hand-worked empty-frame tables: pitch within 1e-9, everything else exact."""
    tabs, refs, probes, kept = _generated()
    s = AN._path_settings(tabs[0], 25, 16000, dict(PATH_KW, pitchFloor=75, pitchCeiling=3500, priorMean="default", priorSD=6,
                                                  interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast",
                                                  certWeight=.5, snakeStep=0.05, smooth=1, smoothVars=AN.SMOOTH_VARS))
    cases = [(tabs[i], refs[i], s) for i in kept]
    for t, kw in _hand_tables():
        ss = AN._path_settings(t, 25, 16000, dict(dict(PATH_KW, pitchFloor=75, pitchCeiling=3500, priorMean="default", priorSD=6,
                                                       interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast",
                                                       certWeight=.5, snakeStep=0.05, smooth=1, smoothVars=AN.SMOOTH_VARS), **kw))
        cases.append((t, AN.pitch_path_numpy(t, 25, 16000, **dict(PATH_KW, **kw)), ss))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for t, _, ss in cases:
            n = len(t["ampl"])
            f.write(_pins_case(t, ss, AN.smoothing_hw(ss["smooth"], n, AN._path_length(t, 16000), 16000)) + "\n")
    exes = [_build_pins(tmp_path, False)]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(_build_pins(tmp_path, True))
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(cases)
        worst = 0.0
        for line, (t, ref, _) in zip(lines, cases):
            v = np.array([float.fromhex(x) for x in line.split()]).reshape(-1, 6)
            assert np.array_equal(np.isnan(v[:, 0]), np.isnan(ref["pitch"]))
            ok = ~np.isnan(ref["pitch"])
            if ok.any():
                worst = max(worst, float(np.max(np.abs(v[ok, 0] - ref["pitch"][ok]) / ref["pitch"][ok])))
            assert np.array_equal(v[:, 1], ref["dom"], equal_nan=True)
            assert np.allclose(v[:, 2], ref["HNR"], rtol=0, atol=1e-12, equal_nan=True)
            assert np.array_equal(v[:, 3], ref["amplVoiced"], equal_nan=True) and np.array_equal(v[:, 4] == 1, ref["voiced"])
            assert np.array_equal(v[:, 5], ref["quartile25"], equal_nan=True)
        print(os.path.basename(exe), "cases", len(cases), "worst relative pitch error %.2e" % worst)
        assert worst <= 1e-9


def _table(cands, certs, dom=None):
    """A table from per-frame lists of up to four candidates (slots dom, autocor, cep, spec in order)."""
    n = len(cands)
    t = dict(ampl=np.linspace(.2, .8, n), HNR=np.linspace(.3, .9, n), quartile25=np.full(n, 500.0), quartile50=np.full(n, 1000.0),
             quartile75=np.full(n, 2000.0), duration=np.full(n, n * 0.025))
    for k in SLOTS:
        t[k], t[k.replace("Cand", "Cert")] = np.full((n, 1), nan), np.full((n, 1), nan)
    for f in range(n):
        for j, (c, a) in enumerate(zip(cands[f], certs[f])):
            t[SLOTS[j]][f, 0], t[SLOTS[j].replace("Cand", "Cert")][f, 0] = c, a
    t["dom"] = t["domCand"][:, 0].copy() if dom is None else np.array(dom, float)
    t["domCand"], t["domCert"] = t["domCand"][:, 0], t["domCert"][:, 0]
    return t


def _hand_tables():
    """The explicit empty-frame cases (interpolWin = 0), a nine-frame gap that interpolate()
    fills frame after frame (each filled frame enters the next median), a one-row table, two
    segments with an unvoiced gap, and smoother outliers."""
    out = [(_table([_hz(8, 9), [], _hz(8)], [[.9, .2], [], [.5]]), dict(interpolWin=0, priorMean=None)),
           (_table([_hz(8), [], _hz(8, 9)], [[.5], [], [.9, .2]]), dict(interpolWin=0, priorMean=None)),
           (_table([_hz(8, 8.1, 9), [], _hz(8, 8.8, 9)], [[.5] * 3, [], [.5] * 3]), dict(interpolWin=0, pathfinding="none")),
           (_table([_hz(8, 8.3)] + [[]] * 9 + [_hz(8.1, 8.2)], [[.5, .4]] + [[]] * 9 + [[.3, .6]]), dict(interpolWin=3)),
           (_table([_hz(8), [], [], _hz(9)], [[.5], [], [], [.5]]), dict(interpolWin=1, interpolTol=0.05)),
           (_table([_hz(8, 8.1), _hz(8.05, 8.2), [], [], [], _hz(9, 9.1), _hz(9.05, 9.3), _hz(9)],
                   [[.5, .6], [.4, .7], [], [], [], [.5, .6], [.4, .7], [.5]]), dict(shortestPause=50, minVoicedCands=2)),
           (_table([_hz(8, 8.01), _hz(8, 8.02), _hz(9, 9.01), _hz(8, 8.01), _hz(8, 8.03), _hz(7.5, 7.52), _hz(8, 8.04)],
                   [[.5, .5]] * 7, dom=[300, 300, 300 * 2 ** (4.5 / 12), 300, 300 * 2 ** (-3.5 / 12), 300, 300]),
            dict(snakeStep=0, smooth=1.3))]
    return out


# ------------------------------------------------------------ the GPU cases' inputs
# the signal is tests/test_pitch_candidates.py's _signal: a gliding eight-harmonic tone (220 -> 280 Hz) over
# 2 % noise, with a near-silent onset, a gap, and a noise-only tail
CASES = [
    (16000, "defaults", dict()),  # 22 frames, two segments of 8 and 4 voiced frames
    (16000, "all4-ncands3", dict(pitchMethods=ALL4, nCands=3, cepThres=0.1, specPeak=0.2)),  # 5 candidates per frame
    # 110 frames: more than one wave's lanes. At snakeStep 0.05 the steady middle of the tone moves a snake point by
    # less than 1e-6 of its value in one step (a force near 1e-4), so `cands > pitch[i]` has no margin: 0.1 here
    (16000, "step5", dict(step=5, snakeStep=0.1)),
    (44100, "step10", dict(step=10)),
    # with two candidates in a frame both are equally far from their mean: 'none' then decides by the last bit in
    # the reference too. Three candidates per voiced frame, and no tolerated gap inside a segment
    (16000, "none", dict(pathfinding="none", minVoicedCands=3, shortestPause=0)),
    # without the snake the pitch is a candidate itself: with 20 Hz bins dom = 240 Hz puts 1.25 * pitch on the label
    # 0.3 kHz exactly. 25 Hz bins (a 40 ms window) have no such label between 215 and 285 Hz; 'spec' is not run
    # with them (tests/test_pitch_candidates.py); shortestPause = 40 keeps the two segments apart at step 20
    (16000, "snakeStep0", dict(snakeStep=0, windowLength=40, pitchMethods=("autocor", "dom"), shortestPause=40)),
    (16000, "noprior", dict(priorMean=None)),
    (16000, "smooth0", dict(smooth=0)),
    (16000, "interpolWin0", dict(interpolWin=0)),
]
SEEDS = {}
IDS = ["%d-%s" % (c[0], c[1]) for c in CASES]


def _seed(sr, name):
    return SEEDS.get((sr, name), 1)


@lru_cache(maxsize=None)
def _reference(i):
    sr, name, kw = CASES[i]
    probe = {}
    ref = AN.analyze_numpy(_signal(sr, _seed(sr, name)), sr, _probe=probe, **kw)
    for v in ref.values():
        v.setflags(write=False)
    return ref, probe


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_gpu_inputs_are_well_conditioned(i):
    """Every traced decision of the tail holds in the restatement alone with a relative
    margin >= 1e-6 on every GPU case, and each case has at least two voiced segments."""
    ref, p = _reference(i)
    m = _track_margin(p)
    print(CASES[i][:2], "margin %.2e" % m, [(s["start_frame"], s["end_frame"], s["rows"], s["direction"], s["iterations"],
                                             s["interpolated"]) for s in p["segments"]])
    assert m >= MARGIN
    assert min(_tracker_margins(p).values()) >= MARGIN  # the candidates' own decisions, as tests/test_pitch_candidates.py
    assert len(p["segments"]) >= 2 and ref["voiced"].sum() >= 8
    if CASES[i][1] == "defaults":
        assert len(ref["pitch"]) == 22 and [s["end_frame"] - s["start_frame"] + 1 for s in p["segments"]] == [8, 4]
    if CASES[i][1] == "step5":
        assert len(ref["pitch"]) == 110
    if CASES[i][1] == "all4-ncands3":
        assert max(s["rows"] for s in p["segments"]) >= 5


def test_analyze_numpy_leaves_the_other_columns_alone():
    ref, p = _reference(0)
    pc = AN.pitch_candidates_numpy(_signal(16000, 1), 16000)
    rewritten = ("HNR", "dom", "quartile25", "quartile50", "quartile75")
    assert set(ref) == set(pc) | {"pitch", "voiced", "amplVoiced", "harmonics"}
    assert all(np.array_equal(ref[k], pc[k], equal_nan=True) for k in pc if k not in rewritten)
    assert np.array_equal(ref["HNR"], AN.to_dB(pc["HNR"]), equal_nan=True)
    v = ref["voiced"]
    assert np.array_equal(ref["quartile50"][v], pc["quartile50"][v]) and np.all(np.isnan(ref["quartile50"][~v]))
    assert np.array_equal(np.isnan(ref["harmonics"]), ~v) and np.all(ref["harmonics"][v] > 0)  # most energy above 1.25 f0
    assert 225 < ref["pitch"][v].min() and ref["pitch"][v].max() < 270  # the 220 -> 280 Hz glide


# ------------------------------------------------------------ GPU
UNTOUCHED = tuple(k for k in AN.COLUMNS if k not in ("HNR", "dom", "quartile25", "quartile50", "quartile75")) + \
    ("autocorCand", "autocorCert") + AN.PITCH_KEYS + ("time", "duration")


def _ratio(db):
    return 1 / (1 + 10 ** (-db / 10))


def _compare(got, ref, pc):
    """got: analyze() on the GPU; ref: analyze_numpy(); pc: pitch_candidates() on the GPU."""
    assert got.keys() == ref.keys()
    for k in UNTOUCHED:
        assert np.array_equal(got[k], pc[k], equal_nan=True), k
    assert np.array_equal(got["voiced"], ref["voiced"]) and got["voiced"].dtype == bool
    for k in ("pitch", "harmonics", "HNR", "dom", "quartile25", "quartile50", "quartile75", "amplVoiced"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    v = ref["voiced"]
    assert np.array_equal(got["amplVoiced"][v], pc["ampl"][v])
    for k in ("dom", "quartile25", "quartile50", "quartile75"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    err = dict(pitch=float(np.max(np.abs(got["pitch"][v] - ref["pitch"][v]) / ref["pitch"][v])))
    for k, d in (("HNR", 1e-13), ("harmonics", 1e-12)):
        ok = ~np.isnan(ref[k]) & ~np.isinf(ref[k])
        x = _ratio(ref[k][ok])
        delta = np.abs(got[k][ok] - ref[k][ok])
        err[k] = float(delta.max()) if ok.any() else 0.0
        err[k + "_bound_used"] = float(np.max(delta / (4.35 * d / (x * (1 - x))))) if ok.any() else 0.0
    print("analyze errors:", {k: "%.2e" % e for k, e in err.items()})
    assert err["pitch"] <= 1e-9 and err["HNR_bound_used"] <= 1 and err["harmonics_bound_used"] <= 1
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_gpu_equals_numpy(i):
    sr, name, kw = CASES[i]
    ref, _ = _reference(i)
    x = _signal(sr, _seed(sr, name))
    pkw = {k: v for k, v in kw.items() if k in inspect.signature(AN.pitch_candidates).parameters}
    _compare(AN.analyze(x, sr, **kw), ref, AN.pitch_candidates(x, sr, **pkw))


def _stitched():
    """50 kept generated segments stitched into tables of five, with unvoiced gaps of six
    frames (nToleratedNA = 2) between them."""
    tabs, _, _, kept = _generated()
    out = []
    for g in range(10):
        parts = [tabs[i] for i in kept[5 * g:5 * g + 5]]
        n = sum(len(t["ampl"]) for t in parts) + 6 * 4
        big = {k: (np.full((n,) + np.shape(v)[1:], nan)) for k, v in parts[0].items()}
        at = 0
        for t in parts:
            m = len(t["ampl"])
            for k in t:
                big[k][at:at + m] = t[k]
            at += m + 6
        for k in ("ampl", "HNR", "quartile25", "quartile50", "quartile75"):
            big[k] = np.where(np.isnan(big[k]), 0.5, big[k])
        big["duration"] = np.full(n, n * 0.025)
        out.append(big)
    return out


STITCH_KW = dict(pitchMethods=ALL4, minVoicedCands=1, shortestSyl=0, shortestPause=60)


def test_stitched_tables_are_well_conditioned():
    for t in _stitched():
        p = {}
        AN.pitch_path_numpy(t, 25, 16000, _probe=p, **STITCH_KW)
        assert _track_margin(p) >= MARGIN and len(p["segments"]) >= 5


def _compare_path(got, ref):
    assert np.array_equal(np.isnan(got["pitch"]), np.isnan(ref["pitch"])) and np.array_equal(got["voiced"], ref["voiced"])
    v = ref["voiced"]
    err = float(np.max(np.abs(got["pitch"][v] - ref["pitch"][v]) / ref["pitch"][v])) if v.any() else 0.0
    assert err <= 1e-9, err
    for k in ("dom", "amplVoiced", "quartile25", "quartile50", "quartile75", "ampl", "domCand", "specCand"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    assert np.allclose(got["HNR"], ref["HNR"], rtol=0, atol=1e-11, equal_nan=True) and np.all(np.isnan(got["harmonics"]))
    return err


@pytest.mark.gpu
def test_pitch_path_gpu_equals_numpy():
    worst = 0.0
    for t in _stitched():
        worst = max(worst, _compare_path(AN.pitch_path(t, 25, 16000, **STITCH_KW), AN.pitch_path_numpy(t, 25, 16000, **STITCH_KW)))
    for t, kw in _hand_tables():  # the explicit empty-frame cases among them
        kw = dict(PATH_KW, **kw)
        worst = max(worst, _compare_path(AN.pitch_path(t, 25, 16000, **kw), AN.pitch_path_numpy(t, 25, 16000, **kw)))
    print("pitch_path: worst relative pitch error %.2e" % worst)
    empty = dict(_table([], []), duration=np.zeros(0))
    assert len(AN.pitch_path(empty, 25, 16000)["pitch"]) == 0


@pytest.mark.gpu
def test_analyze_batch_equals_single():
    """analyze_batch over five packed calls (one not longer than the window, the others of
    different lengths) equals analyze() per call bit for bit."""
    import torch
    sr = 16000
    parts = [_signal(sr, 1), _signal(sr, 3, 0.41)[:800], _signal(sr, 4, 0.33), _signal(sr, 5, 0.6)[1500:7777],
             _signal(sr, 6, 0.2)[1700:2501]]
    lens = np.array([len(v) for v in parts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    host = np.zeros(int(offs[-1] + lens[-1]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    data = torch.from_numpy(host).cuda()
    kw = dict(pitchMethods=ALL4, nCands=2, cepThres=0.1, specPeak=0.2)
    r = AN.analyze_batch(data, offs, lens, sr, **kw)
    assert r["out"].is_cuda and r["out"].dtype == torch.float64 and r["cols"] == 31 == len(r["columns"])
    assert r["columns"][27:] == ("pitch", "amplVoiced", "voiced", "harmonics") and r["columns"][:15] == AN.COLUMNS
    assert r["frames"][1] == 0 and r["frames"][4] == 1 and len(set(r["frames"])) == 5
    h = r["out"].cpu().numpy()
    voiced = 0
    for i in range(5):
        f = r["frames"][i]
        if f == 0:
            continue
        got = h[r["offsets"][i]:r["offsets"][i] + f * 31].reshape(f, 31)
        one = AN.analyze(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr, **kw)
        want = np.column_stack([one[k] for k in AN.COLUMNS] + [one["autocorCand"], one["autocorCert"]] +
                               [one[k] for k in AN.PITCH_KEYS] + [one[k].astype(float) for k in AN.TRACK_COLUMNS])
        assert np.array_equal(got, want, equal_nan=True), i
        voiced += int(one["voiced"].sum())
    assert voiced >= 12
    lst = AN.analyze_batch(data, offs, lens, sr, to_host=True, **kw)
    assert lst[1]["pitch"].shape == (0,) and lst[1]["voiced"].dtype == bool
    assert np.array_equal(lst[0]["pitch"], h[:r["frames"][0] * 31].reshape(-1, 31)[:, 27], equal_nan=True)
    assert np.array_equal(lst[3]["harmonics"], h[r["offsets"][3]:r["offsets"][3] + r["frames"][3] * 31].reshape(-1, 31)[:, 30],
                          equal_nan=True)


@pytest.mark.gpu
def test_analyze_refusals_gpu():
    import ctypes as C
    import torch
    x = _signal(16000, 1)[:4000]
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    AN.analyze(x, 16000)
    ms = (C.c_double * 8)()
    L.sg_debug_track_kernel_ms(ms)
    assert ms[0] > 0 and ms[6] > 0
    with pytest.raises(native.SoundgenError, match="slow") as e:
        AN.analyze(x, 16000, pathfinding="slow")  # refused by the setup: nothing is launched
    assert e.value.code == -4
    L.sg_debug_track_kernel_ms(ms)
    assert ms[0] > 0  # the stage clocks of the run before are untouched
    L.sg_set_profiling(ctx.ptr, 0)
    d = torch.zeros(4000, dtype=torch.float32, device="cuda")
    with pytest.raises(native.SoundgenError) as e:
        AN.analyze_batch(d, [0], [4000], 16000, pathfinding="slow")
    assert e.value.code == -4
    with pytest.raises(NotImplementedError):
        AN.analyze(x, 16000, plot=True)
    with pytest.raises(NotImplementedError):
        AN.analyze(x, 16000, smoothVars=("pitch", "ampl"))
    with pytest.raises(ValueError, match="not longer than the window"):
        AN.analyze(x[:800], 16000)
    with pytest.raises(ValueError, match="certWeight"):
        AN.analyze(x, 16000, certWeight=2)
    r = AN.analyze_batch(d, [0, 0], [300, 800], 16000)  # nothing longer than the window: nothing launched
    assert r["frames"] == [0, 0] and r["cols"] == 25
