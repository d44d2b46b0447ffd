"""analyze(summary = TRUE) and analyzeFolder() (R/analyze.R:770-796, :831-930):
summarize_table_numpy (the host restatement), sg_summary.h on the host (tests/cpp/summary_pins.cpp)
and sg_anl_summary on the GPU (summarize_table, analyze(summary=True), analyze_batch(summary=True),
analyze_folder).

The summation tolerance. For a column whose finite values have the largest magnitude M, a mean,
median or sd computed in fp64 in any fixed order differs from R's long-double value by at most
about n * eps * M (eps = 1.1e-16): |got - ref| <= 1e-9 * max(1, M) covers n up to 1e6 with a
decade to spare. The median of an odd count of values is one of them and must be equal; NaN and
+-Inf must agree in position and sign."""
import math
import os
import shutil
import subprocess
import wave
from functools import lru_cache

import numpy as np
import pytest
from test_analyze import CASES, IDS, _ratio, _reference, _seed
from test_pitch_candidates import RELATIVE as PC_RELATIVE
from test_pitch_candidates import TOL as PC_TOL
from test_pitch_candidates import _signal

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
nan, inf = math.nan, math.inf
STATS = ("mean", "median", "sd")
NAMES = ("duration", "voiced",
         "ampl_mean", "ampl_median", "ampl_sd", "amplVoiced_mean", "amplVoiced_median", "amplVoiced_sd",
         "dom_mean", "dom_median", "dom_sd", "entropy_mean", "entropy_median", "entropy_sd",
         "harmonics_mean", "harmonics_median", "harmonics_sd", "HNR_mean", "HNR_median", "HNR_sd",
         "meanFreq_mean", "meanFreq_median", "meanFreq_sd", "peakFreq_mean", "peakFreq_median", "peakFreq_sd",
         "peakFreqCut_mean", "peakFreqCut_median", "peakFreqCut_sd", "pitch_mean", "pitch_median", "pitch_sd",
         "quartile25_mean", "quartile25_median", "quartile25_sd", "quartile50_mean", "quartile50_median", "quartile50_sd",
         "quartile75_mean", "quartile75_median", "quartile75_sd", "specSlope_mean", "specSlope_median", "specSlope_sd")


def _blank(n, nC=1):
    """An analyze()-shaped table of n frames, every cell NaN, nobody voiced."""
    t = {k: np.full(n, nan) for k in AN.COLUMNS + AN.TRACK_COLUMNS}
    for k in ("autocorCand", "autocorCert") + AN.PITCH_KEYS:
        t[k] = np.full((n, nC), nan)
    t["voiced"] = np.zeros(n, dtype=bool)
    t["time"], t["duration"] = np.arange(n, dtype=float), np.full(n, nan)
    return t


# ------------------------------------------------------------ CPU
def test_summary_by_hand():
    assert AN.SUMMARY_COLUMNS == NAMES and len(NAMES) == 44 and len(AN.SUMMARY_VARS) == 14
    t = _blank(4)
    t["duration"][:] = 0.3125
    t["voiced"] = np.array([True, False, True, True])
    t["ampl"] = np.array([1, nan, 3, 2.])        # mean 2; sorted 1 2 3: median 2; sd sqrt((1 + 0 + 1) / 2) = 1
    t["dom"] = np.array([nan, 7.5, nan, nan])    # one value: mean = median = 7.5, sd NA
    t["pitch"] = np.array([4, 1, 3, 2.])         # even: sorted 1 2 3 4, median (2 + 3) / 2; mean 2.5; sd sqrt(5 / 3)
    t["HNR"] = np.array([inf, 1, 2, 3.])         # mean Inf, sd NaN; sorted 1 2 3 Inf: median 2.5
    t["harmonics"] = np.array([inf, -inf, 2, 3.])  # Inf - Inf: mean NaN, sd NaN; sorted -Inf 2 3 Inf: median 2.5
    t["entropy"] = np.array([-0.0, 0.0, nan, nan])  # the two zeros are one number: median 0
    r = AN.summarize_table_numpy(t)
    assert tuple(r) == NAMES
    assert r["duration"] == 0.3125 and r["voiced"] == 0.75
    assert (r["ampl_mean"], r["ampl_median"], r["ampl_sd"]) == (2.0, 2.0, 1.0)
    assert (r["dom_mean"], r["dom_median"]) == (7.5, 7.5) and math.isnan(r["dom_sd"])
    assert (r["pitch_mean"], r["pitch_median"]) == (2.5, 2.5) and abs(r["pitch_sd"] - math.sqrt(5 / 3)) < 1e-15
    assert r["HNR_mean"] == inf and math.isnan(r["HNR_sd"]) and r["HNR_median"] == 2.5
    assert math.isnan(r["harmonics_mean"]) and math.isnan(r["harmonics_sd"]) and r["harmonics_median"] == 2.5
    assert r["entropy_median"] == 0 and r["entropy_mean"] == 0 and r["entropy_sd"] == 0
    for v in ("amplVoiced", "meanFreq", "quartile50", "specSlope"):  # all NA
        assert all(math.isnan(r[v + "_" + k]) for k in STATS)
    assert all(math.isnan(v) for v in AN.summarize_table_numpy(_blank(0)).values())  # no frames


def test_analyze_numpy_summary_is_the_summary_of_its_table():
    sr, name, kw = CASES[0]
    ref, _ = _reference(0)
    got = AN.analyze_numpy(_signal(sr, _seed(sr, name)), sr, summary=True, **kw)
    want = AN.summarize_table_numpy(ref)
    assert tuple(got) == NAMES
    assert all(got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])) for k in NAMES)
    assert got["duration"] == ref["duration"][0] and 0 < got["voiced"] < 1 and 225 < got["pitch_median"] < 270


def test_library_names_and_size():
    assert AN.summary_columns_native() == AN.SUMMARY_COLUMNS == NAMES
    assert native.lib().sg_analyze_summary_name(44) is None and native.lib().sg_analyze_summary_name(-1) is None
    hdr = open(native.HEADER_PATH).read()
    assert "#define SG_ANALYZE_SUMMARY_COLS 44\n" in hdr


def test_summary_with_plot_raises_before_the_device(tmp_path):
    x = _signal(16000, 1)
    with pytest.raises(NotImplementedError):
        AN.analyze(x, 16000, summary=True, plot=True)
    with pytest.raises(NotImplementedError):
        AN.analyze_numpy(x, 16000, summary=True, plot=True)
    with pytest.raises(NotImplementedError):
        AN.analyze_folder(str(tmp_path / "absent"), plot=True)  # before the folder is listed
    with pytest.raises(NotImplementedError):
        AN.analyze_folder(str(tmp_path / "absent"), savePath=str(tmp_path))


# ------------------------------------------------------------ generated tables
FRAMES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
DENSITY = ("none", "half", "all-but-one")
LEVELS = np.array([-3.5, -1.0, -0.0, 0.0, 5e-324, 0.25, 2.0, 1000.0])  # long runs of ties; the zeros; a subnormal


def _generate(n, density, seed):
    rng = np.random.default_rng(seed)
    t = _blank(n)
    t["duration"][:] = (400 * n + 801) / 16000
    t["voiced"] = rng.random(n) < 0.6
    for j, v in enumerate(AN.SUMMARY_VARS):
        if j % 3 == 0:
            x = LEVELS[rng.integers(0, len(LEVELS), n)]
        elif j % 3 == 1:
            x = rng.standard_normal(n) * 10.0 ** (j - 5)
        else:
            x = np.round(rng.standard_normal(n) * 2) / 2 - 0.5  # a handful of levels of either sign
        if v == "HNR" and n >= 3:
            x[rng.integers(0, n)] = inf
        if v == "harmonics" and n >= 3:
            x[0], x[n - 1] = inf, -inf
        if v == "quartile50" and n >= 2:
            x[:] = -0.0  # nothing but zeros of either sign
            x[::2] = 0.0
        if density == "half":
            x[rng.random(n) < 0.5] = nan
        elif density == "all-but-one" and n:
            keep = rng.integers(0, n)
            x[np.arange(n) != keep] = nan
        t[v] = x
    return t


@lru_cache(maxsize=None)
def _tables():
    out = []
    for i, n in enumerate(FRAMES):
        for j, d in enumerate(DENSITY):
            t = _generate(n, d, 100 * i + j)
            ref = AN.summarize_table_numpy(t)
            for v in t.values():
                v.setflags(write=False)
            out.append((t, ref))
    return out


def _magnitude(x):
    x = np.asarray(x, float)
    x = np.abs(x[np.isfinite(x)])
    return max(1.0, float(x.max())) if len(x) else 1.0


def _check_row(got, ref, table, extra=None):
    """got against ref = summarize_table_numpy(table) at the summation tolerance (plus, per
    variable, extra[v]); returns the worst error as a share of its bound."""
    assert tuple(got) == NAMES
    if len(table["ampl"]) == 0:
        assert all(math.isnan(got[k]) for k in NAMES)
        return 0.0
    assert got["duration"] == ref["duration"] and got["voiced"] == ref["voiced"]
    worst = 0.0
    for v in AN.SUMMARY_VARS:
        x = np.asarray(table[v], float)
        count = int((~np.isnan(x)).sum())
        bound = 1e-9 * _magnitude(x) + (extra[v] if extra else 0.0)
        for k in STATS:
            g, r = got[v + "_" + k], ref[v + "_" + k]
            if math.isnan(r) or math.isinf(r):
                assert g == r or (math.isnan(g) and math.isnan(r)), (v, k, g, r)
            elif k == "median" and count % 2 == 1 and not extra:
                assert g == r, (v, k, g, r)
            else:
                assert abs(g - r) <= bound, (v, k, g, r, bound)
                worst = max(worst, abs(g - r) / bound)
    return worst


def test_generated_tables_cover_the_edges():
    tabs = _tables()
    assert len(tabs) == 45
    refs = [r for _, r in tabs]
    assert any(r["HNR_mean"] == inf and math.isnan(r["HNR_sd"]) and math.isfinite(r["HNR_median"]) for r in refs)
    assert any(math.isnan(r["harmonics_mean"]) and math.isfinite(r["harmonics_median"]) for r in refs)
    assert any(math.isnan(r["ampl_sd"]) and r["ampl_mean"] == r["ampl_median"] for r in refs)  # one value
    t, r = tabs[3 * FRAMES.index(4097)]
    assert r["quartile50_median"] == 0 and len(np.unique(t["ampl"])) <= len(LEVELS)
    assert any(np.any(t["ampl"] == 5e-324) for t, _ in tabs)


def _case_text(t):
    n = len(t["ampl"])
    m = np.full((n, 25), nan)
    for i, k in enumerate(AN.COLUMNS):
        m[:, i] = t[k]
    for i, k in enumerate(AN.TRACK_COLUMNS):
        m[:, 21 + i] = t[k]
    length = 400 * n + 801
    return " ".join([str(n), "1", str(length), "16000"] + [float(v).hex() for v in m.ravel()])


def _build_pins(tmp_path, sanitize):
    exe = str(tmp_path / ("summary_pins_san" if sanitize else "summary_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "summary_pins.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_summary_header_on_the_host_equals_restatement(tmp_path):
    """sg_summary.h (what the lanes of sg_anl_summary run) built for the host as a stand-alone
    program, plainly and under AddressSanitizer and UBSan, on the generated tables. The header
    has one path (no small-n fast path), so there is one run per build."""
    tabs = _tables()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for t, _ in tabs:
            f.write(_case_text(t) + "\n")
    exes = [_build_pins(tmp_path, False)]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }", text=True, capture_output=True)
    if probe.returncode == 0:  # the compiler has the sanitizers' runtimes
        exes.append(_build_pins(tmp_path, True))
    for exe in exes:
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(tabs)
        worst = 0.0
        for line, (t, ref) in zip(lines, tabs):
            got = dict(zip(NAMES, (float.fromhex(x) for x in line.split())))
            worst = max(worst, _check_row(got, ref, t))
        print(os.path.basename(exe), "cases", len(tabs), "worst error / bound %.2e" % worst)


# ------------------------------------------------------------ GPU
def _same_bits(a, b):
    ka, kb = list(a), list(b)
    va, vb = np.array([a[k] for k in ka]), np.array([b[k] for k in kb])
    return ka == kb and va.tobytes() == vb.tobytes()


@pytest.mark.gpu
def test_summarize_table_gpu_equals_restatement():
    """The kernel alone (256 lanes), against the restatement of the very table it saw."""
    worst = 0.0
    for t, ref in _tables():
        worst = max(worst, _check_row(AN.summarize_table(t), ref, t))
        assert _same_bits(AN.summarize_table(t, samplingRate=16000), AN.summarize_table(t))
    print("summarize_table: worst error / bound %.2e" % worst)


@pytest.mark.gpu
@pytest.mark.parametrize("sr", [16000, 22050, 44100, 48000])
def test_summary_kernel_on_real_tables_gpu(sr):
    x = _signal(sr, 1)
    t = AN.analyze(x, sr)
    got = AN.analyze(x, sr, summary=True)
    assert _same_bits(got, AN.summarize_table(t))
    assert got["duration"] == t["duration"][0] == len(x) / sr
    w = _check_row(got, AN.summarize_table_numpy(t), t)
    print(sr, "frames", len(t["ampl"]), "voiced", got["voiced"], "worst error / bound %.2e" % w)
    assert 0 < got["voiced"] < 1 and math.isfinite(got["pitch_sd"])


def _cell_tolerances(ref):
    """Twice the per-cell tolerance of tests/test_analyze.py's _compare for each summarised
    column of the table ref (mean and median are 1-Lipschitz in the sup norm, sd at most
    sqrt(n / (n - 1)) <= sqrt(2)). _compare holds dom and the quartiles exactly, pitch to
    1e-9 relative, HNR and harmonics to 4.35 d / (x (1 - x)) dB (d = 1e-13, 1e-12), and the
    columns analyze() does not rewrite bit-equal to pitch_candidates(), whose own bound against
    the restatement is tests/test_pitch_candidates.py's TOL (exact where it has none)."""
    tol = dict.fromkeys(AN.SUMMARY_VARS, 0.0)
    ok = ~np.isnan(ref["pitch"])
    tol["pitch"] = 1e-9 * float(np.max(ref["pitch"][ok]))
    for k, d in (("HNR", 1e-13), ("harmonics", 1e-12)):
        ok = np.isfinite(ref[k])
        x = _ratio(ref[k][ok])
        tol[k] = float(np.max(4.35 * d / (x * (1 - x)))) if ok.any() else 0.0
    for k in ("ampl", "entropy", "specSlope"):
        ok = np.isfinite(ref[k])
        tol[k] = PC_TOL.get(k, 0.0) * (float(np.max(np.abs(ref[k][ok]))) if k in PC_RELATIVE else 1.0)
    tol["amplVoiced"] = tol["ampl"]
    return {k: 2 * v for k, v in tol.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_summary_gpu_equals_numpy(i):
    """End to end: analyze(x, summary=True) against analyze_numpy(x, summary=True) (which is
    summarize_table_numpy of the cached reference table: the CPU test above)."""
    sr, name, kw = CASES[i]
    ref, _ = _reference(i)
    want = AN.summarize_table_numpy(ref)
    got = AN.analyze(_signal(sr, _seed(sr, name)), sr, summary=True, **kw)
    assert [math.isnan(got[k]) for k in NAMES] == [math.isnan(want[k]) for k in NAMES]
    w = _check_row(got, want, ref, _cell_tolerances(ref))
    print(CASES[i][:2], "worst error / bound %.2e" % w)


@pytest.mark.gpu
def test_analyze_batch_summary_gpu():
    import torch
    sr = 16000
    a, b = _signal(sr, 1), _signal(sr, 3, 0.41)
    parts = [a, b[:800], b, a, _signal(sr, 4, 0.33)]  # [1] is not longer than the window; `a` at two positions
    lens = [len(v) for v in parts] + [-1]              # and a failed call
    offs = list(np.concatenate([[0], np.cumsum(lens[:5])[:-1]]) + 3) + [0]
    host = np.zeros(int(offs[4] + lens[4]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    data = torch.from_numpy(host).cuda()
    r = AN.analyze_batch(data, offs, lens, sr, summary=True)
    assert r["out"].is_cuda and r["out"].dtype == torch.float64 and tuple(r["out"].shape) == (6, 44)
    assert r["columns"] == NAMES and r["frames"][1] == 0 and r["frames"][5] == 0 and min(r["frames"][i] for i in (0, 2, 3, 4)) > 0
    rows = r["out"].cpu().numpy()
    assert np.isnan(rows[1]).all() and np.isnan(rows[5]).all()
    singles = {}
    for i in (0, 2, 3, 4):
        one = AN.analyze(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr, summary=True)
        singles[i] = np.array([one[k] for k in NAMES])
        assert rows[i].tobytes() == singles[i].tobytes(), i
    assert rows[0].tobytes() == rows[3].tobytes()  # the same sound at two positions
    alone = AN.analyze_batch(data, offs[3:4], lens[3:4], sr, summary=True)["out"].cpu().numpy()
    assert alone.shape == (1, 44) and alone[0].tobytes() == rows[0].tobytes()
    plain = AN.analyze_batch(data, offs, lens, sr)  # the tables are those of the plain batch, byte for byte
    assert plain["frames"] == r["frames"] and plain["cols"] == r["cols"] and list(plain["offsets"]) == list(r["offsets"])
    assert r["tables"].cpu().numpy().tobytes() == plain["out"].cpu().numpy().tobytes()
    lst = AN.analyze_batch(data, offs, lens, sr, summary=True, to_host=True)
    assert len(lst) == 6 and all(tuple(d) == NAMES for d in lst)
    assert np.array([[d[k] for k in NAMES] for d in lst]).tobytes() == rows.tobytes()
    empty = AN.analyze_batch(data, [0, 0], [300, -1], sr, summary=True)  # nothing is analysed: the rows are still written
    assert empty["frames"] == [0, 0] and np.isnan(empty["out"].cpu().numpy()).all() and tuple(empty["out"].shape) == (2, 44)


def _write_wav(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.round(x / np.max(np.abs(x)) * 20000).astype("<i2").tobytes())


@pytest.mark.gpu
def test_analyze_folder_gpu(tmp_path):
    _write_wav(tmp_path / "b.wav", _signal(16000, 1), 16000)
    _write_wav(tmp_path / "a.wav", _signal(44100, 1, 0.3), 44100)
    _write_wav(tmp_path / "c.wav", _signal(16000, 3, 0.41), 16000)
    (tmp_path / "notes.txt").write_text("not a sound")
    (tmp_path / "d.wav.bak").write_text("not a sound either")
    rows = AN.analyze_folder(str(tmp_path))
    assert [r["sound"] for r in rows] == ["a.wav", "b.wav", "c.wav"]
    for r in rows:
        assert tuple(r) == ("sound",) + NAMES
        one = AN.analyze(str(tmp_path / r["sound"]), summary=True)
        assert _same_bits({k: r[k] for k in NAMES}, one), r["sound"]
        assert 0 < r["voiced"] < 1
    assert rows[0]["duration"] != rows[1]["duration"]
    tabs = AN.analyze_folder(str(tmp_path), summary=False, verbose=False)
    assert list(tabs) == [str(tmp_path / n) for n in ("a.wav", "b.wav", "c.wav")]
    for p, t in tabs.items():
        one = AN.analyze(p)
        assert t.keys() == one.keys() and all(np.array_equal(t[k], one[k], equal_nan=True) for k in one), p
