"""analyze()'s per-frame stage (R/analyze.R:233-575, R/utilities_analyze.R:22-324):
the numpy restatement pinned by hand, sg_analyze_frames_size against it, and the
GPU (sg_analyze.hip) against it.

No R is installed: soundgen_beta_amd/analyze.py restates the reference statement
by statement with line citations, the CPU tests below pin its parts on cases
worked by hand, and the GPU tests compare the device with it.

Bars. The gates, the NaN pattern and every frequency-valued column (table
look-ups) must match exactly; test_inputs_are_well_conditioned shows that every
discrete decision behind them holds in the restatement with a relative margin
>= 1e-6. The continuous columns are compared absolutely (ampl, entropy, HNR, the
certainties: all in [0, 1]) or relatively (specSlope). The project's bar for an
fp64 path is 1e-9 (tests/test_matchpars.py); the bars held here are 10x the
maxima measured on an MI355X over every case (MEASURED below), all under 1e-9.
"""
import math
import os
import warnings
from functools import lru_cache

import numpy as np
import pytest

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import spectrogram as SP

# Measured on an MI355X, the maximum over every GPU case below
MEASURED = {"ampl": 1.2e-16, "entropy": 8.9e-16, "HNR": 1.4e-14, "domCert": 7.5e-15, "autocorCert": 1.4e-14,
            "specSlope": 4.9e-15}
TOL = {k: 10 * v for k, v in MEASURED.items()}
assert max(TOL.values()) < 1e-9
EXACT = ("cond_silence", "cond_entropy", "dom", "domCand", "peakFreq", "peakFreqCut", "meanFreq", "quartile25",
         "quartile50", "quartile75", "autocorCand", "time", "duration")
MARGIN = 1e-6


# ------------------------------------------------------------ CPU: parts by hand
def test_is_central_local_max_and_rolling_window():
    assert AN.is_central_local_max([1, 1, 3, 2, 1], 2.5)  # the reference's own example
    assert not AN.is_central_local_max([1, 1, 3, 2, 1], 3)  # `>`, not `>=`
    assert not AN.is_central_local_max([0, 3, 3, 1, 0], 1)  # a tie: the FIRST maximum is not the middle
    assert AN.is_central_local_max([0, 1, 3, 3, 0], 1)  # a tie after the middle does not matter
    x = [1, 1, 3, 2, 1, 5, 1]
    assert AN.roll_central_max(x, 3, 2.5) == [3, 6]  # 1-based zoo::index; 7 - 3 + 1 = 5 windows
    assert AN.roll_central_max(x, 7, 2.5) == []  # one window, its maximum (5) is not the middle
    assert AN.roll_central_max(x, 5, 2.5) == [3]  # centres 3, 4, 5: [1,1,3,2,1] only
    assert AN.roll_central_max(x, 9, 0) == []  # wider than the series: no window
    assert AN.roll_central_max([0.2, 0.9], 1, 0.5) == [2]  # width 1: the threshold alone


def test_label_round_trip_decides_row_low():
    # 20 kHz, 180 ms: wl = 3600, 1800 bins of 5.5555... Hz. Bin 9 is 0.05000000000000001 kHz as a
    # double, but as.numeric(rownames(s)) reads "0.05": not > 0.05, so rowLow is the next bin
    from soundgen_beta_amd.morph import _r_seq_len
    raw = _r_seq_len(0.0, 20000 / 2 - 20000 / 3600, 1800)[9] / 1000
    assert raw > 0.05 and AN.rt15(raw) == 0.05
    lab = AN.freq_labels(20000, 3600, 1800)
    assert lab[9] == 0.05 and int(np.nonzero(lab > 0.05)[0][0]) == 10
    d = AN.frame_decisions(8000, AN.repair(20000, windowLength=180))
    assert d["rowLow"] == 11 and d["wl"] == 3600
    assert AN.rt15(1 / 3) == 0.333333333333333 and AN.rt15(22050.0) == 22050.0


def test_amplitude_window():
    # length 31, wl 10, 4 frames: seq(1, 21, length.out = 4) = 1, 7.67, 14.33, 21 -> floor -> 1, 7, 14, 21
    assert list(AN.ampl_starts(31, 10, 4)) == [0, 6, 13, 20]
    s = np.arange(31, dtype=float)
    a = AN.frame_ampl(s, 10, 4)
    assert a[1] == math.sqrt(np.mean(np.arange(6, 17.0) ** 2))  # wl + 1 = 11 samples: 6 .. 16
    assert a[3] == math.sqrt(np.mean(np.arange(20, 31.0) ** 2))  # the last window ends on the last sample
    assert list(AN.ampl_starts(12, 10, 1)) == [0]


def test_silence_rule_drops_the_quietest_frame():
    # every frame is louder than silence = 0.04, yet min(ampl) raises the threshold to itself
    sr = 16000
    t = np.arange(4000) / sr
    x = np.sin(2 * np.pi * 300 * t) * (0.5 + 0.5 * t / t[-1])
    r = AN.analyze_frames_numpy(x, sr)
    assert r["ampl"].min() > 0.04
    q = int(np.argmin(r["ampl"]))
    assert r["cond_silence"][q] == 0 and r["cond_silence"].sum() == len(r["ampl"]) - 1
    assert math.isnan(r["peakFreq"][q]) and not math.isnan(r["entropy"][q])


def test_descriptives_by_hand():
    freq = np.array([0.0, 100, 200, 300, 400, 500])
    frame = np.array([1.0, 2, 8, 4, 3, 2])  # sum 20; cumsum 1 3 11 15 18 20
    d = AN.spectral_descriptives(frame, freq, 1, 4)  # the cut band: bins 1 .. 4 (100 .. 400 Hz)
    assert d["peakFreq"] == 200 and d["meanFreq"] == 200  # cumsum > 10 first at bin 2
    assert d["peakFreqCut"] == 300  # which.max(frame) = 3 indexes the CUT table (100, 200, 300, 400)
    # the cut band 2 8 4 3: sum 17, cumsum 2 10 14 17; >= 4.25 at 200, >= 8.5 at 200, >= 12.75 at 300
    assert (d["quartile25"], d["quartile50"], d["quartile75"]) == (200, 200, 300)
    assert math.isnan(AN.spectral_descriptives(frame[::-1].copy(), freq, 1, 2)["peakFreqCut"])  # arg-max 3 > 2 rows
    assert AN.spectral_descriptives(np.array([1.0, 1, 1, 1, 1, 1]), freq, 0, 6)["meanFreq"] == 300  # `>`: 4 > 3
    assert AN.spectral_descriptives(np.array([1.0, 1, 1, 1]), freq[:4], 0, 4)["quartile50"] == 100  # `>=`: 2 >= 2


def test_spec_slope_is_polyfit():
    rng = np.random.default_rng(0)
    f = np.linspace(80, 6000, 297)
    a = rng.uniform(0, 3, 297) - 2e-4 * f
    assert AN.spec_slope(f, a) == pytest.approx(np.polyfit(f, a, 1)[0], rel=1e-10)
    assert AN.spec_slope(np.array([1.0, 2, 3]), np.array([2.0, 4, 6])) == 2


def test_lag_labels_and_range():
    lf = AN.lag_labels(16000, 800)
    assert lf[0] == 16000 and lf[1] == 8000 and lf[2] == AN.rt15(16000 / 3) == 5333.33333333333
    d = AN.frame_decisions(9600, AN.repair(16000))
    # 75 < 16000 / j < 3500: j = 5 .. 213; row j holds lag j - 1 (the reference's off-by-one)
    assert (d["lag_first"], d["lag_last"]) == (4, 212)
    d = AN.frame_decisions(30000, AN.repair(44100))
    assert d["lag_last"] - d["lag_first"] + 1 == 575 and d["wl"] == 2204 and d["autocorSmooth"] == 7
    assert AN.frame_decisions(9600, AN.repair(16000))["autocorSmooth"] == 3  # 2 ceiling(7 * 16000 / 44100 / 2) - 1
    assert AN.frame_decisions(9600, AN.repair(16000))["domSmooth_bins"] == 11  # 2 ceiling(220 / 20 / 2) - 1


def test_autocor_filter():
    f = AN.autocor_filter(64, "gaussian")
    assert len(f) == 64 and f[0] == 1 and np.all(np.diff(f) < 0) and f[-1] > 0
    # squared twice: the square root is the 2 wl-point window's normalised circular autocorrelation
    w = SP.ft_window(128, "gaussian")
    ac = np.array([np.dot(w, np.roll(w, -k)) for k in range(64)])
    assert np.allclose(np.sqrt(f), ac / ac[0], rtol=0, atol=1e-12)


def test_get_pitch_autocor_by_hand():
    #              0    1    2     3    4    5     6    7    8
    amp = np.array([.1, .8, .2, .805, .3, .75, .2, .9, .1])
    freq = np.array([900.0, 800, 700, 600, 500, 400, 300, 200, 100])
    # peaks (width 3, > .7): rows 1, 3, 5, 7. max .9; the first above .8775 is row 7: bestFreq 200, all kept
    H, c, a = AN.get_pitch_autocor(amp, freq, 0.7, 3, 3)
    assert H == 0.9 and c == [200, 600, 800] and a == [.9, .805, .8]
    amp2 = amp.copy()
    amp2[1] = 0.89  # > .975 * .9: the FIRST such peak is row 1, bestFreq 800; only freq > 444.4 survive
    H, c, a = AN.get_pitch_autocor(amp2, freq, 0.7, 3, 8)
    assert c == [800, 600] and a == [.89, .805]
    amp3 = amp.copy()
    amp3[3] = 0.8  # a tie between rows 1 and 3: order() keeps the earlier first
    assert AN.get_pitch_autocor(amp3, freq, 0.7, 3, 3)[1] == [200, 800, 600]
    assert AN.get_pitch_autocor(amp, freq, 0.95, 3, 1) == (0.9, [], [])  # HNR without an accepted peak
    assert AN.get_pitch_autocor(np.array([.2, 1.01, .3]), freq[:3], 0.7, 3, 1) == (0.9999, [800], [1.01])
    assert AN.get_pitch_autocor(np.array([.2, 1.0, .3]), freq[:3], 0.7, 3, 1)[0] == 0.9999  # `>=`


def test_dom_by_hand():
    freq = np.arange(8) * 100.0
    x = np.array([.05, .5, .05, .02, 1, .3, .2, .1])
    assert AN.get_dom(x, freq, 3, 0.1, 1) == (100, .5)
    assert AN.get_dom(x, freq, 3, 0.1, 2) == (400, 1)  # `idx > pitchFloor_idx`: bin index 2 is not above 2
    assert AN.get_dom(x, freq, 3, 0.6, 1) == (400, 1)
    assert AN.get_dom(x, freq, 9, 0.1, 1) == (math.nan, math.nan) or math.isnan(AN.get_dom(x, freq, 9, 0.1, 1)[0])
    assert AN.dom_certainty(0.5) == 1 / (1 + math.exp(0.5)) and AN.dom_certainty(1 / 3) == 0.5


def test_repairs_warn_and_default():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s = AN.repair(16000, 0.5, silence=2, entropyThres=-1, windowLength=600, overlap=120, wn="kaiser", zp=-5,
                      cutFreq=0, pitchFloor=9000, pitchCeiling=9000, nCands=0, domThres=3, autocorThres=-2)
    assert len(w) == 12
    assert (s["silence"], s["entropyThres"], s["windowLength"], s["step"], s["wn"], s["zp"]) == \
        (0.04, 0.6, 50, 25, "gaussian", 0)
    assert (s["cutFreq"], s["pitchFloor"], s["pitchCeiling"], s["nCands"], s["domThres"], s["autocorThres"]) == \
        (8000, 1, 8000, 1, 0.1, 0.7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert AN.repair(16000, 0.5, step=900)["step"] == 25  # beyond the sound: windowLength / 2
        assert AN.repair(16000, 0.5, nCands=2.6)["nCands"] == 3
    assert len(w) == 1


# ------------------------------------------------------------ sg_analyze_frames_size
SIZE_KEYS = ("wl", "bins", "frames", "cols", "lag_first", "lag_last", "rowLow", "rowHigh", "cut0", "ncut",
             "pitchFloor_idx", "domSmooth_bins", "autocorSmooth")


@pytest.mark.parametrize("sr", [16000, 22050, 44100, 48000, 20000])
def test_sg_analyze_frames_size_equals_restatement(sr):
    """sg_analyze_frames_size (host only) makes frame_decisions' decisions, and the
    amplitude windows start where the restatement's do."""
    n = 0
    wlens = (50, 25, 20, 40, 12) + ((180,) if sr == 20000 else ())
    for wlen in wlens:
        for kw in (dict(), dict(pitchFloor=50, domSmooth=100), dict(pitchFloor=150.5, pitchCeiling=2000, cutFreq=4000,
                                                                 domSmooth=415, nCands=3),
                   dict(step=7.3, autocorSmooth=5, pitchFloor=100)):
            s = AN.repair(sr, None, windowLength=wlen, **kw)
            wl = AN.frame_decisions(0, s)["wl"]
            by = s["step"] / 1000 * sr
            lens = {0, wl - 1, wl, wl + 1, wl + 2, 3 * wl + 17}
            for k in (1, 2, 7):
                for dl in (-1, 0, 1, 2):
                    lens.add(wl + int(math.floor(k * by)) + dl)
            for length in sorted(lens):
                want = AN.frame_decisions(length, s)
                got = AN.frame_decisions_native(length, s)
                assert {k: got[k] for k in SIZE_KEYS} == {k: want[k] for k in SIZE_KEYS}, (wlen, kw, length)
                assert want["frames"] == (0 if length <= wl else len(SP.frame_starts(length, sr, wl, s["step"])))
                assert np.array_equal(AN.ampl_starts_native(length, s, want["frames"]),
                                      AN.ampl_starts(length, wl, want["frames"]))
                n += 1
    assert n > 200
    if sr == 20000:
        assert AN.frame_decisions_native(8000, AN.repair(20000, windowLength=180))["rowLow"] == 11


def test_refusals():
    from soundgen_beta_amd import native
    x = np.sin(np.arange(4000) * 0.1)
    for f, dec in ((AN.analyze_frames_numpy, AN.frame_decisions), (None, AN.frame_decisions_native)):
        with pytest.raises(ValueError, match=r"acf\(\) then returns 801 values"):
            dec(4000, AN.repair(16000, zp=1024))
        dec(4000, AN.repair(16000, zp=800))  # zp up to the window pads nothing
        with pytest.raises(ValueError, match="no frequency label above 6 kHz"):
            dec(4000, AN.repair(8000))
        with pytest.raises(ValueError, match="whole odd number"):
            dec(4000, AN.repair(16000, autocorSmooth=4))
        with pytest.raises(ValueError, match="wider than the 1 lags"):
            dec(4000, AN.repair(16000, pitchFloor=3200, pitchCeiling=4100, cutFreq=7000, autocorSmooth=3))
        with pytest.raises(ValueError, match="no lag between"):
            dec(4000, AN.repair(16000, pitchFloor=3300, pitchCeiling=3900, cutFreq=7000))
        with pytest.raises(native.SoundgenError, match="at most 8") as e:
            dec(4000, AN.repair(16000, nCands=9))
        assert e.value.code == -4
        if f:
            with pytest.raises(ValueError, match="not longer than the window"):
                f(x[:800], 16000)
            with pytest.raises(NotImplementedError, match="'cep' and 'spec'"):
                f(x, 16000, pitchMethods=("autocor", "spec"))
            with pytest.raises(NotImplementedError):
                f(x, 16000, pitchMethods="cep")
            with pytest.raises(ValueError):
                f(x, 16000, pitchMethods=())
    with pytest.raises(native.SoundgenError) as e:
        AN.frame_decisions_native(4000, AN.repair(16000, windowLength=4.625))  # 37 bins: sg_spectrogram_size's limit
    assert e.value.code == -4


# ------------------------------------------------------------ the GPU cases' inputs
def _signal(sr, seed, dur=0.6):
    """A gliding eight-harmonic tone (220 -> 280 Hz) over 2 % noise, with a
    near-silent onset, a gap, and a noise-only tail."""
    rng = np.random.default_rng(seed)
    n = int(dur * sr)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(220 + 100 * t) / sr
    tone = sum(np.sin(h * ph) / h for h in range(1, 9))
    env = ((t > 0.11) & (t < 0.27)) | ((t > 0.37) & (t < 0.46))
    level = np.where(t < 0.1, 0.002, np.where(t > 0.48, 0.3, 0.02))
    return tone * env + level * rng.standard_normal(n)


WINDOW_CASES = [(16000, "wn_" + wn, dict(wn=wn)) for wn in SP.WINDOWS if wn != "gaussian"]
CASES = [
    (16000, "wl20", dict(windowLength=20)),  # wl 320, 160 bins, fewer lags than threads
    (16000, "defaults", dict()),             # wl 800, 400 bins
    (22050, "defaults", dict()),             # 551 bins: odd, the radix-29 path
    (44100, "defaults", dict()),             # 1102 bins, wl 2204: the largest default frame
    (16000, "autocor", dict(pitchMethods=("autocor",))),
    (16000, "dom", dict(pitchMethods=("dom",))),
    (16000, "ncands3", dict(nCands=3, autocorThres=0.5)),
    (22050, "ranges", dict(pitchFloor=100, pitchCeiling=1200, cutFreq=4000, domSmooth=100, autocorSmooth=5,
                           entropyThres=0.5, silence=0.03, domThres=0.2)),
    (16000, "step", dict(step=7.3)),
] + WINDOW_CASES
SEEDS = {}  # (sr, name) -> seed, where the default seed 1 does not keep the margins
IDS = ["%d-%s" % (c[0], c[1]) for c in CASES]


def _seed(sr, name):
    return SEEDS.get((sr, name), 1)


@lru_cache(maxsize=None)
def _reference(i):
    sr, name, kw = CASES[i]
    probe = {}
    ref = AN.analyze_frames_numpy(_signal(sr, _seed(sr, name)), sr, _probe=probe, **kw)
    for v in ref.values():
        v.setflags(write=False)
    return ref, probe


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b))


def _window_margins(x, width, thres, lo=0):
    """The smallest relative margin of the decisions isCentral.localMax makes over
    the centred windows of x: x[c] against the threshold, and against the rest of its window."""
    h = width // 2
    m = math.inf
    for c in range(max(h, lo), len(x) - h):
        m = min(m, _rel(x[c], thres))
        rest = np.delete(x[c - h:c + h + 1], h)
        if len(rest) and x[c] > thres:
            m = min(m, _rel(x[c], rest.max()))
    return m


def _margins(ref, p):
    """The smallest relative margin of every discrete decision of a restatement run."""
    d, s, S, freq = p["d"], p["s"], p["S"], p["freq"]
    out = {}
    out["silence"] = min(_rel(a, p["sil"]) for a in ref["ampl"] if not (a == p["sil"] == ref["ampl"].min()))
    cs = np.nonzero(ref["cond_silence"])[0]
    out["entropy"] = min(_rel(ref["entropy"][f], s["entropyThres"]) for f in cs)
    am, cr = math.inf, math.inf
    for f in cs:
        fr = S[:, f]
        o = np.sort(fr)
        am = min(am, _rel(o[-1], o[-2]))
        cum = np.cumsum(fr)
        cr = min(cr, min(_rel(c, cum[-1] / 2) for c in cum))
        cc = np.cumsum(fr[d["cut0"]:d["cut0"] + d["ncut"]])
        for q in (0.25, 0.5, 0.75):
            cr = min(cr, min(_rel(c, q * cc[-1]) for c in cc))
    out["argmax"], out["crossing"] = am, cr
    out["dom"] = min([_window_margins(x, d["domSmooth_bins"], s["domThres"], d["pitchFloor_idx"])
                      for x in p["normed"].values()] if "dom" in s["pitchMethods"] else [math.inf])
    pk, rule, order, hnr = math.inf, math.inf, math.inf, math.inf
    for a in p["acf"].values():
        pk = min(pk, _window_margins(a, d["autocorSmooth"], s["autocorThres"]))
        hnr = min(hnr, abs(a.max() - 1))
        idx = [i - 1 for i in AN.roll_central_max(a, d["autocorSmooth"], s["autocorThres"])]
        if idx:
            pa = a[idx]
            rule = min(rule, min(_rel(v, 0.975 * pa.max()) for v in pa))
            if len(pa) > 1:
                o = np.sort(pa)
                order = min(order, min(_rel(o[i], o[i + 1]) for i in range(len(o) - 1)))
    out["peaks"], out["rule975"], out["order"], out["hnr1"] = pk, rule, order, hnr
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_inputs_are_well_conditioned(i):
    """Every discrete decision the GPU tests compare exactly holds in the restatement
    alone with a relative margin >= 1e-6, for every frame of every case: the gates,
    the arg-max against the runner-up, every cumulative-sum crossing, every
    peak-or-not window decision and threshold comparison, the 0.975 rule, the
    candidate order, HNR against 1."""
    ref, p = _reference(i)
    m = _margins(ref, p)
    print(CASES[i][:2], {k: "%.2e" % v for k, v in m.items()})
    assert min(m.values()) >= MARGIN, m


def test_inputs_have_frames_of_every_class():
    for i in (1, 3):  # 16 kHz and 44.1 kHz defaults
        ref, _ = _reference(i)
        sil, ent = ref["cond_silence"] == 1, ref["cond_entropy"] == 1
        has_cand = ~np.isnan(ref["autocorCand"][:, 0])
        assert (~sil).sum() >= 3                  # below silence
        assert (sil & ~ent).sum() >= 2            # above silence but too noisy
        assert (ent & has_cand).sum() >= 3        # tracked with a candidate
        assert (ent & ~has_cand).sum() >= 1       # tracked, HNR measured, no accepted peak
        assert np.all(~np.isnan(ref["HNR"][ent])) and np.all(np.isnan(ref["HNR"][~ent]))
        assert np.all(~np.isnan(ref["quartile50"][sil])) and np.all(np.isnan(ref["quartile50"][~sil]))
        assert (~np.isnan(ref["dom"])).sum() >= 3


# ------------------------------------------------------------ GPU
def _compare(got, ref, worst=None):
    """Exact columns exactly (NaN pattern included), continuous ones at TOL; returns the errors."""
    assert got.keys() == ref.keys()
    err = {}
    for k in ref:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, k
        assert np.array_equal(np.isnan(g), np.isnan(r)), k
        ok = ~np.isnan(r)
        if k in EXACT:
            assert np.array_equal(g[ok], r[ok]), k
        elif k == "specSlope":
            err[k] = float(np.max(np.abs(g[ok] - r[ok]) / np.abs(r[ok]))) if ok.any() else 0.0
        else:
            err[k] = float(np.max(np.abs(g[ok] - r[ok]))) if ok.any() else 0.0
    print("analyze_frames errors:", {k: "%.2e" % v for k, v in err.items()})
    for k, v in err.items():
        assert v <= TOL[k], (k, v)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_analyze_frames_gpu_equals_numpy(i):
    sr, name, kw = CASES[i]
    ref, _ = _reference(i)
    _compare(AN.analyze_frames(_signal(sr, _seed(sr, name)), sr, **kw), ref)


@pytest.mark.gpu
def test_scale_branch_and_silent_stretch_gpu():
    sr = 16000
    x = _signal(sr, 1) + 7.0  # all positive: scale() first
    assert x.min() > 0
    ref = AN.analyze_frames_numpy(x, sr)
    assert ref["cond_entropy"].sum() >= 3
    _compare(AN.analyze_frames(x, sr), ref)
    y = _signal(sr, 1)
    y[2000:4400] = 0.0  # three whole frames of zeros: entropy NA for an all-zero band; they still get ampl
    ref = AN.analyze_frames_numpy(y, sr)
    z = np.nonzero(np.isnan(ref["entropy"]))[0]
    assert len(z) >= 2 and np.all(ref["cond_silence"][z] == 0) and not np.isnan(ref["ampl"][z]).any()
    _compare(AN.analyze_frames(y, sr), ref)


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
def test_analyze_frames_batch_equals_single():
    """analyze_frames_batch over 24 synthesized calls of mixed length in HBM (one
    launch sequence) equals analyze_frames() per call on the same samples bit for
    bit, on EVERY non-empty call. One call is refused by the planner (length -1),
    one is cut shorter than the window and one to the window exactly: 0 frames."""
    import torch
    from soundgen_beta_amd import batch
    sr = 16000
    calls = _batch_calls(sr, 24, 7)
    calls[4] = {"kind": "harmonics", "pitch": np.full(1, 150.0), "params": dict(samplingRate=sr)}  # refused
    data, offs, lens = batch.synthesize_packed(calls, 0)
    assert lens[4] == -1 and (np.delete(lens, 4) > 2000).all() and len(set(lens.tolist())) > 10
    lens = lens.copy()
    lens[9] = 500   # shorter than the 800-point window
    lens[13] = 800  # the window exactly: the amplitude window would leave the sound
    lens[17] = 801  # one frame
    kw = dict(nCands=2)
    r = AN.analyze_frames_batch(data, offs, lens, sr, **kw)
    out = r["out"]
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float64
    assert r["cols"] == 19 and len(r["columns"]) == 19 and r["columns"][:3] == ("ampl", "entropy", "HNR")
    h = out.cpu().numpy()
    host = data.cpu().numpy()
    compared = tracked = 0
    for i in range(len(calls)):
        f = r["frames"][i]
        if i in (4, 9, 13):
            assert f == 0
            continue
        assert f == len(SP.frame_starts(int(lens[i]), sr, 800, 25)) and (i != 17 or f == 1)
        got = h[r["offsets"][i]:r["offsets"][i] + f * 19].reshape(f, 19)
        y = host[offs[i]:offs[i] + lens[i]].astype(np.float64)
        one = AN.analyze_frames(y, sr, **kw)
        want = np.column_stack([one[k] for k in AN.COLUMNS] + [one["autocorCand"], one["autocorCert"]])
        assert np.array_equal(got, want, equal_nan=True), i
        tracked += int(one["cond_entropy"].sum())
        compared += 1
    assert compared == 21 and tracked > 50
    lst = AN.analyze_frames_batch(data, offs, lens, sr, to_host=True, **kw)
    assert len(lst[4]["ampl"]) == 0 and lst[13]["autocorCand"].shape == (0, 2)
    assert np.array_equal(lst[0]["HNR"], h[:r["frames"][0] * 19].reshape(-1, 19)[:, 2], equal_nan=True)
    assert np.array_equal(lst[2]["time"], AN.frame_times(int(lens[2]), sr, 25, r["frames"][2])[0])


@pytest.mark.gpu
def test_analyze_frames_file_path(tmp_path):
    from soundgen_beta_amd import api
    sr = 16000
    s = _signal(sr, 1)
    pcm = np.round(20000 * s / np.max(np.abs(s))).astype(np.int16)
    path = os.path.join(str(tmp_path), "s.wav")
    api.write_wav(path, pcm, sr)
    got = AN.analyze_frames(path)
    one = AN.analyze_frames(pcm.astype(np.float64), sr)
    assert all(np.array_equal(got[k], one[k], equal_nan=True) for k in got)
    ref = AN.analyze_frames_numpy(path)
    for k in ("cond_silence", "cond_entropy", "time"):
        assert np.array_equal(got[k], ref[k])
    e_hnr, e_ampl = np.nanmax(np.abs(got["HNR"] - ref["HNR"])), np.max(np.abs(got["ampl"] - ref["ampl"]))
    print("analyze_frames(path): HNR %.2e ampl %.2e" % (e_hnr, e_ampl))
    assert e_hnr <= TOL["HNR"] and e_ampl <= TOL["ampl"]


@pytest.mark.gpu
def test_analyze_frames_errors_gpu():
    import torch
    from soundgen_beta_amd import native
    x = _signal(16000, 1)[:4000]
    with pytest.raises(ValueError, match=r"acf\(\)"):
        AN.analyze_frames(x, 16000, zp=1024)
    with pytest.raises(ValueError, match="6 kHz"):
        AN.analyze_frames(x, 8000)
    with pytest.raises(ValueError, match="not longer than the window"):
        AN.analyze_frames(x[:800], 16000, windowLength=50, step=25)
    with pytest.raises(NotImplementedError):
        AN.analyze_frames(x, 16000, pitchMethods=("autocor", "cep", "spec", "dom"))
    with pytest.raises(ValueError, match="odd"):
        AN.analyze_frames(x, 16000, autocorSmooth=6)
    with pytest.raises(native.SoundgenError) as e:
        AN.analyze_frames(x, 16000, nCands=9)
    assert e.value.code == -4
    with pytest.raises(native.SoundgenError) as e:
        AN.analyze_frames(x, 16000, windowLength=4.625)
    assert e.value.code == -4
    d = torch.zeros(4000, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="6 kHz"):
        AN.analyze_frames_batch(d, [0], [4000], 8000)
    r = AN.analyze_frames_batch(d, [0, 0], [300, 800], 16000)  # nothing longer than the window: nothing launched
    assert r["frames"] == [0, 0]
    assert len(AN.analyze_frames(x, 16000)["ampl"]) == 8  # seq(1, 3200, 400)
