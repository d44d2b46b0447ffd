"""analyze_sweep(), sweep_plan() and sweep_size() (soundgen_beta_amd/analyze.py; sg_analyze_sweep,
sg_analyze_sweep_plan and sg_analyze_sweep_size in sg_analyze.hip / sg_analyze.cpp) and optimize_pars()
for analyzeFolder on top of them.

On the CPU: the planner's three groupings (by resolved decisions, first-appearance numbering), the
refusals and the row they name, sg_path.h's path_sound_at against path_sound as a stand-alone
program (plain and with -fsanitize=address,undefined), and the conditioning of the GPU inputs.

On the GPU the sweep is compared bit for bit with one analyze_batch(summary=True) per row, in the
settings that must not change a bit (row order, sound order, one row at a time, the store off,
three workspace caps), and with the restatement summarize_table_numpy(analyze_numpy()) under the
bound of tests/test_analyze_summary.py (_check_row with _cell_tolerances: no constant of its own).
The inputs keep, under every row, the margin tests/test_analyze.py demands of its own
(test_gpu_inputs_are_well_conditioned below), so a deviation within the bound flips no decision.
"""
import ctypes as C
import math
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest
from test_analyze import MARGIN, _track_margin
from test_analyze_summary import NAMES, _cell_tolerances, _check_row
from test_pitch_candidates import _margins as _tracker_margins

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import native
from soundgen_beta_amd import optimize as OP

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
SR = 16000
nan = math.nan

# the eleven rows, as changes from analyze()'s defaults: two frame groups (the last but one has its own window
# and step), three stores (the defaults' gates, row 9's, row 10's) and seven candidate groups
ROWS = (dict(),
        dict(certWeight=.9),
        dict(priorMean=None, pathfinding="none"),
        dict(smooth=0, interpolWin=0, snakeStep=0),
        dict(shortestSyl=60, shortestPause=20, minVoicedCands=2),
        dict(specThres=.1, specSmooth=100),
        dict(autocorThres=.5, autocorSmooth=5, nCands=3),
        dict(pitchMethods=("autocor", "cep", "dom"), cepThres=.2),
        dict(silence=.1, entropyThres=.4),
        dict(windowLength=25, step=5),
        dict(pitchMethods=("spec",)))


# ------------------------------------------------------------------------ CPU: the planner
def _renamed(a, b):
    """Two group vectors are the same partition under a renaming of the groups."""
    return len(set(zip(a, b))) == len(set(a)) == len(set(b))


def test_sweep_plan_groups_by_resolved_decisions():
    f, s, c = AN.sweep_plan(SR, list(ROWS))
    assert list(f) == [0] * 9 + [1, 0]
    assert list(s) == [0] * 8 + [1, 2, -1]
    assert list(c) == [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 6]
    # NULL step is windowLength * (1 - overlap / 100); NULL autocorSmooth is 2 * ceiling(7 * 16000 / 44100 / 2) - 1 = 3
    f, s, c = AN.sweep_plan(SR, [dict(step=None, overlap=50, windowLength=50), dict(step=25), dict(autocorSmooth=None),
                                 dict(autocorSmooth=3)])
    assert list(f) == list(s) == list(c) == [0, 0, 0, 0]
    pairs = {"certWeight": (dict(certWeight=.2), (True, True, True)), "specThres": (dict(specThres=.2), (True, True, False)),
             "autocorThres": (dict(autocorThres=.6), (True, True, False)), "silence": (dict(silence=.05), (True, False, False)),
             "windowLength": (dict(windowLength=40), (False, False, False))}
    for name, (kw, shared) in pairs.items():
        groups = AN.sweep_plan(SR, [dict(), kw])
        assert tuple(int(g[0]) == int(g[1]) for g in groups) == shared, name
    f, s, c = AN.sweep_plan(SR, [dict(pitchMethods=("spec",)), dict(), dict(pitchMethods=("spec",), certWeight=.1)])
    assert list(s) == [-1, 0, -1] and list(f) == [0, 0, 0] and list(c) == [0, 1, 0]
    assert all(len(g) == 0 for g in AN.sweep_plan(SR, []))


def test_sweep_plan_numbering_under_permutation():
    rng = np.random.default_rng(5)
    base = [np.asarray(g) for g in AN.sweep_plan(SR, list(ROWS))]
    for _ in range(6):
        perm = rng.permutation(len(ROWS))
        got = AN.sweep_plan(SR, [ROWS[i] for i in perm])
        for g, b in zip(got, base):
            assert _renamed(list(g), list(b[perm]))
            seen = [v for i, v in enumerate(g) if v >= 0 and v not in list(g[:i])]
            assert seen == list(range(len(seen)))  # first appearance: 0, 1, 2, ...
            assert [v < 0 for v in g] == [v < 0 for v in b[perm]]


def test_sweep_refusals_name_the_row():
    with pytest.raises(NotImplementedError, match="row 1: .*slow"):
        AN.sweep_plan(SR, [dict(), dict(pathfinding="slow")])
    with pytest.raises(native.SoundgenError, match="row 2: .*nCands = 9") as e:
        AN.sweep_plan(SR, [dict(), dict(), dict(nCands=9)])
    assert e.value.code == -4
    with pytest.raises(ValueError, match="row 1: samplingRate"):
        AN.sweep_plan(SR, [dict(), dict(samplingRate=22050)])
    # 200 frames a second: smoothing_ww = round(7 * 200 / 10) = 140, half of it 70 frames
    with pytest.raises(native.SoundgenError, match="row 1, sound 2: .*at most 64"):
        AN.sweep_size([2, 801, 96000], SR, [dict(), dict(step=5, smooth=7)])
    for kw, err in ((dict(formants=True), NotImplementedError), (dict(plot=True), NotImplementedError),
                    (dict(summary=False), ValueError), (dict(nosuch=1), ValueError)):
        with pytest.raises(err, match="row 1"):
            AN.sweep_plan(SR, [dict(), kw])
    # the C entry points alone: a raw pathfinding = 2 and a second rate, both named
    P = AN._sweep_params(SR, [dict(), dict()])
    P[1].pathfinding = 2
    g = [(C.c_int32 * 2)() for _ in range(3)]
    assert native.lib().sg_analyze_sweep_plan(P, 2, *g) == -4
    assert b"row 1: " in native.lib().sg_analyze_frames_size_error() and b"slow" in native.lib().sg_analyze_frames_size_error()


def test_sweep_size_reports_the_three_workspaces():
    lens = [2, 800, 801, 6000, 16000, 30000]
    frames50 = sum(AN.track_decisions_native(n, AN.repair_track(AN.repair_pitch(SR, None)))["frames"] for n in lens)
    s10 = AN.repair_track(AN.repair_pitch(SR, None, windowLength=25, step=5))
    frames25 = sum(AN.track_decisions_native(n, s10)["frames"] for n in lens)
    assert frames50 == 1 + 13 + 38 + 73 and frames25 > 64 * 6
    b = AN.sweep_size(lens, SR, list(ROWS))
    # the first frame group: 400 bins, and candidate tables of 15 + 6 nCands columns: five with nCands 1, one with 3;
    # the second: 200 bins and one table, over five times the frames
    assert b["frame_group"] == 8 * max(frames50 * (400 + 5 * 21 + 33), frames25 * (200 + 21)) == 8 * frames25 * 221
    assert b["store"] == 8 * frames50 * 209  # the lags 5 .. 213 (75 < 16000 / j < 3500); only the first store is shared
    assert b["row"] == 8 * frames25 * (25 + 2 * 5 + 7)  # row 10: 15 + 6 + 4 columns and path_stride(1)
    assert AN.sweep_size(lens, SR, [dict(), dict(silence=.1)])["store"] == 0  # nothing to share


# ------------------------------------------------------- CPU: sg_path.h's variant on the host
def _at_case(rng, nC, frames, kw):
    """A candidate table of `frames` rows with voiced stretches, gaps and octave errors, and the settings of a
    row, in tests/cpp/path_pins.cpp's format."""
    cols = 15 + 6 * nC
    m = np.full((frames, cols), nan)
    m[:, 0] = rng.uniform(0.05, 0.9, frames)                      # ampl
    m[:, 1] = rng.uniform(0.1, 0.9, frames)                       # entropy
    m[:, 2] = rng.uniform(0.05, 0.95, frames)                     # HNR
    m[:, 4:11] = rng.uniform(300, 3000, (frames, 7))
    contour = math.log2(220) + 0.2 * np.sin(np.arange(frames) / 9.0) + np.cumsum(rng.normal(0, 0.01, frames))
    for f in range(frames):
        if (f // 13) % 3 == 2 and rng.random() < 0.9:              # an unvoiced stretch
            continue
        if rng.random() < 0.8:                                     # dom
            m[f, 3] = m[f, 11] = 2.0 ** (contour[f] + rng.normal(0, 0.02))
            m[f, 12] = rng.uniform(0.05, 1)
        for g in range(3):                                         # autocor, cep, spec
            for k in range(int(rng.integers(0, nC + 1))):
                m[f, 15 + 2 * g * nC + k] = 2.0 ** (contour[f] + rng.normal(0, 0.03) + rng.choice([0, 1, -1], p=[.8, .1, .1]))
                m[f, 15 + (2 * g + 1) * nC + k] = rng.uniform(0.05, 1)
    prior = AN.prior_setup(AN.hz_to_semitones(300), 6, 75, 3500) if kw["prior"] else (0.0, 0.0, 0.0, 1.0)
    head = [nC, frames, kw["hw"], kw["minVoiced"], kw["noRequired"], kw["nTolerated"], kw["interpolWin"], kw["pathfinding"],
            int(kw["prior"]), int(kw["hw"] > 0), int(kw["hw"] > 0)] + list(prior) + \
           [0.3, 0.3, kw["certWeight"], kw["snakeStep"], 4.0 if kw["hw"] > 0 else 0.0]
    return " ".join(float(v).hex() for v in head + m.ravel().tolist())


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_path_at_header_on_the_host(tmp_path):
    """tests/cpp/path_at_pins.cpp: path_sound_at from a table apart, with exactly the cells the sweep gives a
    pair, writes what path_sound writes in place, bit for bit, and leaves the source untouched: tables of 130
    frames (more than the 64 lanes of the device's workgroup), nCands 1 and 3, under the tails of the GPU rows;
    plain and under the address and undefined-behaviour sanitizers."""
    rng = np.random.default_rng(21)
    settings = [dict(hw=2, minVoiced=2, noRequired=1, nTolerated=2, interpolWin=3, pathfinding=1, prior=True, certWeight=.5,
                     snakeStep=.05),
                dict(hw=2, minVoiced=2, noRequired=1, nTolerated=2, interpolWin=3, pathfinding=1, prior=True, certWeight=.9,
                     snakeStep=.05),
                dict(hw=2, minVoiced=2, noRequired=1, nTolerated=2, interpolWin=3, pathfinding=0, prior=False, certWeight=.5,
                     snakeStep=.05),
                dict(hw=0, minVoiced=2, noRequired=1, nTolerated=2, interpolWin=0, pathfinding=1, prior=True, certWeight=.5,
                     snakeStep=0),
                dict(hw=10, minVoiced=1, noRequired=12, nTolerated=4, interpolWin=3, pathfinding=1, prior=True, certWeight=.5,
                     snakeStep=.05)]
    cases = [_at_case(rng, nC, frames, kw) for nC in (1, 3) for kw in settings for frames in (130,)]
    cases += [_at_case(rng, 1, 0, settings[0]), _at_case(rng, 3, 1, settings[0])]
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(cases) + "\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "path_at_pins.cpp")]
    exes = [str(tmp_path / "path_at_pins")]
    subprocess.run(base + ["-o", exes[0]], check=True, timeout=300)
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(str(tmp_path / "path_at_pins_san"))
        subprocess.run(base[:1] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + base[1:] +
                       ["-o", exes[1]], check=True, timeout=300)
    outs = []
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        outs.append(lines)
    assert all(o == outs[0] for o in outs)
    voiced = [np.array([float.fromhex(x) if "nan" not in x else nan for x in line.split()]).reshape(-1, 4)[:, 3] for line in outs[0][:10]]
    assert all(20 < v.sum() < 130 for v in voiced)  # the tables do have voiced and unvoiced frames


# ---------------------------------------------------------------------- the GPU inputs
LENGTHS = (2, 800, 801, 6000, 16000, 30000)
# per sound: the tone's frequency (Hz), the depth of its vibrato, its harmonics, the seed of its noise, `rich`
# (found by scanning 240 .. 300 Hz in steps of 1 Hz for the margin below: at most frequencies the autocorrelation's
# and the cepstrum's candidate of one period, or a spectral peak ratio and a border of the BaNa table, coincide)
TONES = ((251, .004, 6, 2, False), (256, .004, 6, 800, False), (259, .004, 6, 801, False), (267, .004, 6, 6000, False),
         (286, .004, 6, 16000, True), (281, .004, 6, 30000, False))


def _tone(n, f0, depth, harmonics, seed, rich):
    """A harmonic tone with a 5.5 Hz vibrato, sounding over two stretches of the sound, on low noise with a
    near-silent onset and a noise burst near the end; float32, as the device gets it. rich: a 45 ms gap in the first
    stretch, a 35 ms blip between the two and the octave below added in the second, so that the rows of the tail
    (shortestSyl, shortestPause, interpolWin, certWeight, pathfinding, the prior) come to different tracks."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    ph = 2 * np.pi * np.cumsum(f0 * (1 + depth * np.sin(2 * np.pi * 5.5 * t))) / SR
    x = sum(np.sin(h * ph) / h for h in range(1, harmonics + 1))
    u = np.arange(n) / max(n, 1)
    env = ((u > 0.08) & (u < 0.5)) | ((u > 0.6) & (u < 0.82))
    level = np.where(u < 0.06, 0.002, np.where((u > 0.88) & (u < 0.96), 0.3, 0.02))
    if rich:
        x2 = sum(np.sin(h * ph / 2) / h for h in range(1, harmonics + 1))
        env = ((u > 0.08) & (u < 0.5) & ~((u > 0.27) & (u < 0.315))) | ((u > 0.6) & (u < 0.82)) | ((u > 0.53) & (u < 0.565))
        return ((0.5 * (x + np.where(u > 0.6, 0.6 * x2, 0.0)) * env + level * rng.standard_normal(n)) / 2).astype(np.float32)
    return ((0.5 * x * env + level * rng.standard_normal(n)) / 2).astype(np.float32)


@lru_cache(maxsize=None)
def _sounds():
    return tuple(_tone(n, *TONES[i]) for i, n in enumerate(LENGTHS))


@lru_cache(maxsize=None)
def _reference():
    """analyze_numpy() of every (row, sound) that has frames, with its probe."""
    out = {}
    for s, x in enumerate(_sounds()):
        for r, kw in enumerate(ROWS):
            if len(x) <= (400 if r == 9 else 800):
                continue
            p = {}
            ref = AN.analyze_numpy(x.astype(np.float64), SR, _probe=p, **kw)
            for v in ref.values():
                v.setflags(write=False)
            out[r, s] = (ref, p)
    return out


def test_gpu_inputs_are_well_conditioned():
    """Under the restatement alone every traced decision of the tail and of the two trackers, on every (row,
    sound) of the GPU tests, keeps the relative margin tests/test_analyze.py demands; and the inputs are not
    degenerate: every row has a sound with a pitch, and at least half of the pairs have voiced frames."""
    ref = _reference()
    assert len(ref) == 11 * 4 + 1  # 801, 6000, 16000 and 30000 samples under every row; 800 under the 25 ms window
    voiced = {}
    for (r, s), (t, p) in ref.items():
        m = min(_track_margin(p), min(_tracker_margins(p).values()))
        assert m >= MARGIN, (r, s, m)
        voiced[r, s] = AN.summarize_table_numpy(t)
    for r in range(len(ROWS)):
        assert any(math.isfinite(v["pitch_median"]) for (q, _), v in voiced.items() if q == r), r
    assert sum(v["voiced"] > 0 for v in voiced.values()) >= len(voiced) / 2
    assert len(ref[9, 5][0]["pitch"]) > 64 * 5  # the lanes of sg_anl_sweep_path stride
    assert len({repr(sorted(voiced[r, 4].items())) for r in range(len(ROWS))}) >= 7  # the rows do change the summaries


# ---------------------------------------------------------------------- GPU: the sweep
@lru_cache(maxsize=None)
def _device_batch():
    import torch
    parts = _sounds()
    lens = np.array([len(v) for v in parts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    host = np.zeros(int(offs[-1] + lens[-1]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    return torch.from_numpy(host).cuda(), offs, lens


def _sweep(rows=tuple(range(11)), sounds=tuple(range(6)), **kw):
    data, offs, lens = _device_batch()
    at = list(sounds)
    return AN.analyze_sweep(data, offs[at], lens[at], SR, [ROWS[r] for r in rows], **kw).cpu().numpy()


@lru_cache(maxsize=None)
def _swept():
    return _sweep()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.gpu
def test_sweep_equals_analyze_batch():
    """Row r of the sweep is analyze_batch(summary=True) under row r's parameters bit for bit, NaN pattern
    included; a sound without frames has a row of NaN."""
    import torch
    data, offs, lens = _device_batch()
    got = _swept()
    assert got.shape == (11, 6, 44)
    for r, kw in enumerate(ROWS):
        want = AN.analyze_batch(data, offs, lens, SR, summary=True, **kw)["out"].cpu().numpy()
        assert np.array_equal(_bits(got[r]), _bits(want)), (r, np.argwhere(_bits(got[r]) != _bits(want))[:5])
        assert np.isnan(got[r, 0]).all() and np.isnan(got[r, 1]).all() == (r != 9) and not np.isnan(got[r, 2]).all()
    dev = AN.analyze_sweep(data, offs, lens, SR, [ROWS[0], ROWS[6]])
    assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == (2, 6, 44)
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(got[[0, 6]]))
    lst = AN.analyze_sweep(data, offs, lens, SR, [ROWS[6]], to_host=True)
    assert len(lst) == 1 and len(lst[0]) == 6 and tuple(lst[0][4]) == NAMES
    assert np.array_equal(_bits([lst[0][4][k] for k in NAMES]), _bits(got[6, 4]))
    assert tuple(AN.analyze_sweep(data, offs, lens, SR, []).shape) == (0, 6, 44)


def _caps():
    """Workspace caps from sg_analyze_sweep_size: everything fits; the shared store does not (its groups run
    the plain kernel); one row per chunk (no row fits, and at least one runs)."""
    b = AN.sweep_size(LENGTHS, SR, list(ROWS))
    assert 0 < b["store"] and 8 < b["row"]
    return dict(everything=b["store"] + len(ROWS) * b["row"], no_store=b["store"] - 8, one_row=8)


@pytest.mark.gpu
def test_sweep_does_not_depend_on_the_launch():
    """The same bits with the rows reversed, row by row, with the sounds reversed, with the store off, and under
    the three caps. sg_set_analyze_sweep_store refuses every mode but 0 and 1 and then leaves the mode as it was."""
    want = _bits(_swept())
    assert np.array_equal(_bits(_sweep(tuple(range(10, -1, -1)))[::-1]), want)
    for r in range(11):
        assert np.array_equal(_bits(_sweep((r,))[0]), want[r]), r
    assert np.array_equal(_bits(_sweep(sounds=tuple(range(5, -1, -1)))[:, ::-1]), want)
    L = native.lib()
    try:
        assert L.sg_set_analyze_sweep_store(0) == 0  # the store off
        assert np.array_equal(_bits(_sweep()), want)
        assert L.sg_set_analyze_sweep_store(1) == 0
        for mode in (2, 3, 5, 8):  # SG_E_ARG, and mode 1 stays in force
            assert L.sg_set_analyze_sweep_store(mode) == -1, mode
        ctx = native.default_context(0)
        L.sg_set_profiling(ctx.ptr, 1)
        try:
            _sweep()
        finally:
            L.sg_set_profiling(ctx.ptr, 0)
        assert AN.sweep_kernel_ms()["autocorrelation (peaks only)"] > 0
    finally:
        L.sg_set_analyze_sweep_store(1)
    for name, cap in _caps().items():
        assert np.array_equal(_bits(_sweep(workspace_cap=int(cap))), want), name


def _tolerances(ref):
    """tests/test_analyze_summary.py's per-cell tolerances. It scales by the largest pitch and specSlope of the
    table: a table without a voiced frame, or with one frame below the silence gate, has none (and no cell of that
    variable to compare), so a zero stands in."""
    t = dict(ref)
    for k in ("pitch", "specSlope"):
        if not np.isfinite(t[k]).any():
            t[k] = np.zeros(1)
    return _cell_tolerances(t)


@pytest.mark.gpu
def test_sweep_equals_restatement():
    """Against summarize_table_numpy(analyze_numpy()): duration, voiced and the NaN pattern exact, the values
    within the bound tests/test_analyze_summary.py applies to the same cells."""
    got = _swept()
    worst = 0.0
    for (r, s), (ref, _) in _reference().items():
        want = AN.summarize_table_numpy(ref)
        row = dict(zip(NAMES, (float(v) for v in got[r, s])))
        assert [math.isnan(row[k]) for k in NAMES] == [math.isnan(want[k]) for k in NAMES], (r, s)
        worst = max(worst, _check_row(row, want, ref, _tolerances(ref)))
    print("sweep against the restatement: worst error / bound %.2e" % worst)


@pytest.mark.gpu
def test_sweep_stage_clock():
    """sg_debug_analyze_sweep_kernel_ms: the peak picker runs from the store when it is on and not when it is off
    or does not fit."""
    data, offs, lens = _device_batch()
    L = native.lib()
    ctx = native.default_context(0)

    def stages(mode, cap=0):
        L.sg_set_analyze_sweep_store(mode)
        L.sg_set_profiling(ctx.ptr, 1)
        try:
            AN.analyze_sweep(data, offs, lens, SR, list(ROWS), workspace_cap=cap)
        finally:
            L.sg_set_profiling(ctx.ptr, 0)
            L.sg_set_analyze_sweep_store(1)
        return AN.sweep_kernel_ms()
    on, off, small = stages(1), stages(0), stages(1, _caps()["no_store"])
    print("stages, store on:", {k: round(v, 4) for k, v in on.items()})
    assert tuple(on) == AN.SWEEP_STAGES and len(on) == 10
    assert on["autocorrelation (peaks only)"] > 0 and off["autocorrelation (peaks only)"] == 0
    assert small["autocorrelation (peaks only)"] == 0
    assert all(v > 0 for k, v in on.items() if k != "autocorrelation (peaks only)") and all(v >= 0 for v in off.values())


# ------------------------------------------------------------- GPU: optimizePars on a folder
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from soundgen_beta_amd import api
    d = tmp_path_factory.mktemp("sweep_sounds")
    for name, i in (("a_801.wav", 2), ("b_6000.wav", 3), ("c_16000.wav", 4), ("d_30000.wav", 5)):
        api.write_wav(str(d / name), np.round(_sounds()[i].astype(np.float64) * 24000).astype(np.int16), SR)
    return str(d)


@pytest.mark.gpu
def test_optimize_pars_runs_the_sweep(folder):
    """optimize_pars(myfun='analyzeFolder', mygrid=...) over rows 1, 2, 6 and 7: its fit column equals, bit for
    bit, the fitness of one analyze_batch(summary=True) per row."""
    import torch
    pars = ["certWeight", "specThres", "specSmooth", "autocorThres", "autocorSmooth", "nCands"]
    defaults = dict(certWeight=.5, specThres=.3, specSmooth=150, autocorThres=.7, autocorSmooth=3, nCands=1)
    rows = [dict(defaults, **ROWS[r]) for r in (0, 1, 5, 6)]
    grid = {k: [row[k] for row in rows] for k in pars}
    key = [1.0, 2.0, 4.0, 3.0]
    res = OP.optimize_pars(folder, key, "analyzeFolder", pars, fitnessPar="ampl_mean", mygrid=grid, verbose=False,
                           otherPars=dict(plot=False, verbose=False))
    names, _, groups = AN.folder_groups(folder)
    assert len(names) == 4 and len(groups) == 1
    g = groups[0]
    m = torch.stack([AN.analyze_batch(g["data"], g["offsets"], g["lengths"], g["samplingRate"], summary=True,
                                      **{k: float(v) for k, v in row.items()})["out"] for row in rows])
    want = OP.sweep_fitness(m, "ampl_mean", key)
    print("analyzeFolder fit:", res["fit"], want)
    assert np.array_equal(_bits(res["fit"]), _bits(want)) and not np.isnan(want).any()
    res2 = OP.optimize_pars(folder, key, "analyzeFolder", pars, fitnessPar="pitch_median", mygrid=grid, verbose=False)
    assert np.array_equal(_bits(res2["fit"]), _bits(OP.sweep_fitness(m, "pitch_median", key)))
