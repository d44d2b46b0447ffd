"""pitch_candidates(): analyze()'s per-frame stage with the cepstral and the spectral
(BaNa) pitch tracker (getPitchCep, R/utilities_analyze.R:337-407; getPitchSpec,
:424-558): the numpy restatement pinned by hand, sg_pitch_candidates_size against
it, sg_bana.h compiled for the host against it, and the GPU (sg_anl_cep, sg_anl_bana
in sg_analyze.hip) against it.

No R is installed: soundgen_beta_amd/analyze.py restates the reference statement by
statement with line citations, the CPU tests pin its parts on cases worked by hand,
and the GPU tests compare the device with it.

Bars. The gates, the NaN pattern and every table look-up column (cepCand included:
its labels come from a host table) must match exactly;
test_pitch_inputs_are_well_conditioned shows that every discrete decision behind them
holds in the restatement with a relative margin >= 1e-6. cepCert, specCand (a quotient
and a mean of labels) and specCert are continuous and compared absolutely (the
certainties, in [0, 1]) or relatively (specCand). The project's bar for an fp64 path
is 1e-9 (tests/test_matchpars.py); the bars held here are 10x the maxima measured on
an MI355X over every case (MEASURED below), all under 1e-9. The columns shared with
analyze_frames keep the bars of tests/test_analyze_frames.py.
"""
import math
import os
import shutil
import subprocess
import warnings
from functools import lru_cache

import numpy as np
import pytest

from soundgen_beta_amd import analyze as AN
from soundgen_beta_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")

# Measured on an MI355X, the maximum over every GPU case below (the first six are the
# columns shared with analyze_frames). specCand measured 0: the device and the
# restatement make the same correctly rounded divisions and means of the same labels;
# a measured 0 is held at one unit in the last place of an fp64 (2.3e-16).
MEASURED = {"ampl": 1.2e-16, "entropy": 1.5e-15, "HNR": 4.6e-15, "domCert": 1.8e-15, "autocorCert": 4.6e-15,
            "specSlope": 4.9e-15, "cepCert": 4.5e-16, "specCand": 0.0, "specCert": 1.2e-16}
TOL = {k: max(10 * v, 2.3e-16) for k, v in MEASURED.items()}
assert max(TOL.values()) < 1e-9
EXACT = ("cond_silence", "cond_entropy", "dom", "domCand", "peakFreq", "peakFreqCut", "meanFreq", "quartile25",
         "quartile50", "quartile75", "autocorCand", "cepCand", "time", "duration")
RELATIVE = ("specSlope", "specCand")
MARGIN = 1e-6
ALL4 = ("autocor", "cep", "spec", "dom")


def _discount(cand, pitchFloor):
    """:400-401, written out independently of the module."""
    semitones = math.log2((cand / pitchFloor) / 16.3516) * 12
    return 1 + 5 / (1 + math.exp(2 - 0.25 * semitones))


def _cert(idx, single=0.4):
    return single + (1 / (1 + math.exp(-(idx - 1))) - 0.5) * 2 * (1 - single)


# ------------------------------------------------------------ CPU: getPitchCep by hand
def _cos_frame(B, parts):
    n = np.arange(B)
    return 1 + sum(a * np.cos(2 * np.pi * q * n / B) for q, a in parts)


def test_cep_layout_quirks():
    # cepSmooth = NULL: 2 * ceiling(31 * samplingRate / 44100 / 2) - 1
    assert AN.cep_layout(400, 44100, 75, 3500, None, 0)[2] == 31
    assert AN.cep_layout(400, 16000, 75, 3500, None, 0)[2] == 11
    # cepZp < length(frame): the frame as it is
    L, pad, cw, l, first, lab = AN.cep_layout(64, 6400, 100, 1000, 3, 63)
    assert (L, pad, cw, l) == (64, 0, 3, 32)
    # rows i with 100 < 3200 / i < 1000: i = 4 .. 31 (3200 / 32 = 100 is not above the floor)
    assert first == 3 and len(lab) == 28 and lab[0] == 800 and lab[-1] == 3200 / 31
    # cepZp = length(frame): the padded branch with nothing to pad; cepSmooth * round(1)
    assert AN.cep_layout(64, 6400, 100, 1000, 3, 64)[:3] == (64, 0, 3)
    # cepZp - B odd: rep(0, 48.5) is 48 zeros, L = 160; round(161 / 64 = 2.52) = 3
    L, pad, cw, l, first, lab = AN.cep_layout(64, 6400, 100, 1000, 3, 161)
    assert (L, pad, cw, l) == (160, 48, 9, 80)
    assert lab[0] == 6400 / (first + 1) / 2 * (160 / 64) and lab[0] < 1000 <= 6400 / first / 2 * 2.5
    # R's round() goes half to even: round(160 / 64 = 2.5) = 2, round(224 / 64 = 3.5) = 4
    assert AN.cep_layout(64, 6400, 100, 1000, 3, 160)[2] == 6
    assert AN.cep_layout(64, 6400, 100, 1000, 3, 224)[2] == 12
    assert AN.cep_layout(400, 16000, 75, 3500, None, 401)[:3] == (400, 0, 11)  # an odd difference of 1: no padding
    assert AN.cep_layout(400, 16000, 75, 3500, None, 1024)[:4] == (1024, 312, 33, 512)
    assert len(AN.cep_layout(400, 16000, 75, 3500, None, 1024)[5]) == 268


def test_get_pitch_cep_by_hand():
    # |fft(1 + a cos(2 pi q n / 64))| / max: 1 at bin 0, a / 2 at bin q. Row i (1-based) of the
    # reference's table holds bin i - 1 and is labelled 6400 / i / 2: bins 4 and 10 are rows 5 and
    # 11, 640 Hz and 290.9 Hz.
    fr = _cos_frame(64, [(4, 0.8), (10, 0.6)])
    tr = {}
    cand, cert = AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 3, 0, 3, tr)
    # peaks .4 (640 Hz) and .3 (290.9 Hz); the larger is the first maximum; 290.9 < 640 / 1.8: dropped
    assert cand == [640.0] and cert[0] == pytest.approx(0.4 / _discount(640.0, 100), rel=1e-12)
    assert len(tr["band"]) == 28 and tr["width"] == 3 and len(tr["rule18"]) == 2
    # the other way round the best peak is 290.9 Hz and 640 > 290.9 / 1.8 stays: ordered by decreasing cep
    fr = _cos_frame(64, [(4, 0.6), (10, 0.8)])
    cand, cert = AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 3, 0, 3)
    assert cand == [3200 / 11, 640.0]
    assert cert == pytest.approx([0.4 / _discount(3200 / 11, 100), 0.3 / _discount(640.0, 100)], rel=1e-12)
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 3, 0, 1)[0] == [3200 / 11]  # nCands after the ordering
    # the discount comes after the ordering: at pitchFloor = 20 it turns the certainties round, not the order
    cand, cert = AN.get_pitch_cep(_cos_frame(64, [(4, 0.7), (10, 0.8)]), 6400, 20, 1000, 0.2, 3, 0, 2)
    assert cand == [3200 / 11, 640.0]
    assert cert == pytest.approx([0.4 / _discount(3200 / 11, 20), 0.35 / _discount(640.0, 20)], rel=1e-12)
    assert _discount(640.0, 100) > _discount(3200 / 11, 100) > 1
    # `>` cepThres; no peak: idx[1:0] is one all-NA row, nothing in the table
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.45, 3, 0, 3) == ([], [])
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.35, 3, 0, 3)[0] == [3200 / 11]
    # a window wider than the band finds nothing (zoo: no window), it is not an error
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 29, 0, 3) == ([], [])
    # cepSmooth = 7 around row 11 still sees a peak; around row 5 (the band starts at row 4) there is no full window
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 7, 0, 3)[0] == [3200 / 11]


def test_get_pitch_cep_padded_branch():
    # cepZp = 161 on 64 bins: 48 zeros either side, L = 160, cepSmooth 3 * 3 = 9, labels * 160 / 64.
    # The cosine at bin 4 of 64 moves to bin 10 of 160: row 11. The band 100 < 8000 / i < 3000 starts
    # at row 3, so row 11 has a full 9-row window (with pitchCeiling = 1000 it starts at row 9 and has none).
    fr = _cos_frame(64, [(4, 0.8)])
    tr = {}
    assert AN.get_pitch_cep(fr, 6400, 100, 1000, 0.2, 3, 161, 2) == ([], [])
    cand, cert = AN.get_pitch_cep(fr, 6400, 100, 3000, 0.2, 3, 161, 2, tr)
    assert tr["width"] == 9 and cand == [6400 / 11 / 2 * 2.5]
    z = np.abs(np.fft.fft(np.concatenate([np.zeros(48), fr, np.zeros(48)])))
    assert cert[0] == pytest.approx(z[10] / z.max() / _discount(cand[0], 100), rel=1e-12)  # the maximum: DC included


# ------------------------------------------------------------ CPU: getPitchSpec by hand
B5 = dict(pitchFloor=75, pitchCeiling=3500, specSinglePeakCert=0.4, specThres=0.3, specMerge=1)


def _bana(peaks, nCands=1, **kw):
    return AN.bana_candidates(peaks, nCands=nCands, **dict(B5, **kw))


def test_bana_table_equals_fixture():
    import json
    with open(os.path.join(HERE, "golden", "rda_fixtures.json")) as f:
        t = json.load(f)["R/sysdata.rda"]["BaNaRatios"]
    assert len(AN.BANA_RATIOS) == 9
    assert [r[0] for r in AN.BANA_RATIOS] == t["value_low"]
    assert [r[1] for r in AN.BANA_RATIOS] == t["value_high"]
    assert [r[2] for r in AN.BANA_RATIOS] == t["divide_lower_by"]


def test_bana_single_peak_branch():
    assert _bana([440.0]) == ([440.0], [0.4])
    assert _bana([75.0]) == ([], []) and _bana([3500.0]) == ([], [])  # strictly inside the range
    assert _bana([60.0]) == ([], []) and _bana([]) == ([], [])
    assert _bana([440.0], specThres=0.4) == ([], [])  # `>` specThres empties the table: the 1:0 row is all NA
    assert _bana([440.0], specSinglePeakCert=0.6, specThres=0.5) == ([440.0], [0.6])


def test_bana_harmonic_series_merges_into_one():
    # 400 / 200 = 2 -> 200; 600 / 200 = 3 -> 200; 600 / 400 = 1.5 -> 400 / 2: 200 three times, specAmplIdx 3
    tr = {}
    assert AN.bana_candidates([200.0, 400, 600], nCands=2, _trace=tr, **B5) == ([200.0], [_cert(3)])
    assert tr["idx"] == [3] and len(tr["ratio"]) == 3 * 18 and len(tr["merge"]) == 2
    assert _cert(3) == pytest.approx(0.4 + (1 / (1 + math.exp(-2)) - 0.5) * 1.2, rel=1e-15) and _cert(1) == 0.4
    # only the five lowest peaks count: a sixth at 1200 (= 2 x 600, 3 x 400, 6 x 200) changes nothing
    five = [200.0, 400, 600, 800, 1000]
    assert _bana(five + [1200.0]) == _bana(five)
    # 400/200, 800/400 (2); 600/200 (3); 800/200 (4); 1000/200 (5); 600/400 (1.5); 1000/400 (2.5); 1000/600 (1.67);
    # 800/600 (1.33): 200 eight times (400 / 1 from 800/400 is the ninth candidate); 1000/800 (1.25): 800 / 4 = 200
    c, a = _bana(five, nCands=3)
    assert c == [200.0, 400.0] and a == [_cert(9), _cert(1)]


def test_bana_borders_are_exclusive():
    assert 142.0 / 100 == 1.42  # exactly the border two rows share
    assert _bana([100.0, 142]) == ([], [])  # 1.42 is in neither (1.29, 1.42) nor (1.42, 1.59)
    assert _bana([100.0, 143], pitchFloor=40) == ([50.0], [0.4])  # 1.43: the lower peak is harmonic 2
    assert _bana([100.0, 143]) == ([], [])  # 50 Hz is below the floor
    assert _bana([100.0, 141], pitchFloor=30) == ([100 / 3], [0.4])  # 1.41: harmonic 3
    assert _bana([100.0, 210]) == ([], []) and _bana([100.0, 190]) == ([], [])  # 2.1 and 1.9 themselves
    assert _bana([100.0, 180]) == ([], [])  # 1.8 closes (1.59, 1.8); (1.8, 1.9) is a gap
    assert _bana([150.0, 300], pitchFloor=150) == ([], []) and _bana([150.0, 300], pitchCeiling=150) == ([], [])


def test_bana_merge_uses_the_running_mean():
    # 416 / 200 = 2.08 -> 200; 657 / 416 = 1.579 -> 416 / 2 = 208; 1117 / 657 = 1.7002 -> 657 / 3 = 219;
    # 657 / 200, 1117 / 200, 1117 / 416 match nothing. 200 and 208 merge (0.057 octaves < 1 / 12) into 204;
    # 204 and 219 do not (0.102), although 208 and 219 would (0.074): the comparison uses the running value
    tr = {}
    c, a = AN.bana_candidates([200.0, 416, 657, 1117], nCands=2, _trace=tr, **B5)
    assert c == [204.0, 219.0] and a == [_cert(2), 0.4]
    assert abs(math.log2(208 / 219)) < 1 / 12 < abs(math.log2(204 / 219))
    assert [round(m[0], 3) for m in tr["merge"]] == [0.057, 0.102]
    assert _bana([200.0, 416, 657, 1117], nCands=2, specThres=0.5) == ([204.0], [_cert(2)])
    assert _bana([200.0, 416, 657, 1117], nCands=2, specThres=0.7) == ([], [])  # everything filtered: NaN
    assert _bana([200.0, 416, 657, 1117], nCands=1) == ([204.0], [_cert(2)])
    # a chain: 200, 205, 211 -> 202.5 (idx 2) -> mean(202.5, 211) = 206.75 (idx 3), not the mean of the three
    # (peaks 200, 410 = 2 x 205, 633 = 3 x 211: 410 / 200 = 2.05 -> 200, 633 / 200 = 3.165 -> 200 again, 633 / 410 =
    # 1.544 -> 205): 200, 200, 205 -> 200 (idx 2) -> 202.5 (idx 3)
    assert _bana([200.0, 410, 633]) == ([202.5], [_cert(3)])
    assert _bana([200.0, 410, 633], specMerge=0) == ([200.0], [0.4])  # |log2(1)| < 0 is false: nothing merges
    c, a = _bana([200.0, 410, 633], specMerge=0, nCands=3)
    assert c == [200.0, 200.0, 205.0] and a == [0.4] * 3


def test_bana_ties_keep_ascending_pitch():
    # 600 / 300 = 2 -> 300; 1000 / 600 = 1.667 -> 600 / 3 = 200; 1000 / 300 matches nothing: two candidates of
    # specAmplIdx 1, equal certainty: order() is stable, the lower pitch stays first
    assert _bana([300.0, 600, 1000], nCands=2) == ([200.0, 300.0], [0.4, 0.4])
    assert _bana([300.0, 600, 1000], nCands=1) == ([200.0], [0.4])
    # a merged candidate outranks them wherever it lies
    # 300 three times (2, 3, 1.5), 1500 / 300 = 5 -> 300, 1500 / 600 = 2.5 -> 600 / 2, 1500 / 900 = 1.67 -> 900 / 3
    assert _bana([300.0, 600, 900, 1500], nCands=3) == ([300.0], [_cert(6)])


def test_get_pitch_spec_window_and_threshold():
    # 16 kHz, 30 ms: 240 bins of 33.3 Hz: width = 2 * ceiling((150 / 33.3 + 1) * 20 / 33.3 / 2) - 1 = 3
    assert AN.spec_width(150, 8000 / 240) == 3 and AN.spec_width(150, 20.0) == 9 and AN.spec_width(150, 8000 / 160) == 1
    assert AN.spec_width(60, 11025 / 551) == 3 and AN.spec_width(-100, 20.0) == -5
    freq = 100.0 * np.arange(12)
    fr = np.array([.1, .2, 1, .2, .5, .1, .36, .1, .34, .1, .1, .1])
    tr = {}
    # peaks above specPeak = .35 at 200, 400, 600 Hz (.34 at 800 Hz is not `>` .35)
    assert AN.get_pitch_spec(fr, freq, 8000 / 240, 75, 3500, 150, 0.35, 0.4, 0.3, 1, 2, _trace=tr) == ([200.0], [_cert(3)])
    assert tr["npeaks"] == 3 and tr["width"] == 3
    assert AN.get_pitch_spec(fr, freq, 8000 / 240, 75, 3500, 150, 0.6, 0.4, 0.3, 1, 2) == ([200.0], [0.4])  # one peak
    assert AN.get_pitch_spec(fr, freq, 8000 / 240, 250, 3500, 150, 0.6, 0.4, 0.3, 1, 2) == ([], [])
    # specHNRslope changes nothing (HNR = NULL)
    assert AN.get_pitch_spec(fr, freq, 8000 / 240, 75, 3500, 150, 0.35, 0.4, 0.3, 1, 2, specHNRslope=0.1)[0] == [200.0]


def test_repair_pitch_warns_and_defaults():
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        s = AN.repair_pitch(16000, 0.5, cepThres=2, specThres=-1, specPeak="a", specSinglePeakCert=1.5, specMerge=-1)
    assert len(w) == 5 and "cepThres" in str(w[0].message)
    assert (s["cepThres"], s["specThres"], s["specPeak"], s["specSinglePeakCert"], s["specMerge"]) == (0.3, 0.3, 0.35, 0.4, 1)
    assert s["pitchMethods"] == ("autocor", "spec", "dom") and s["cepSmooth"] is None and s["nCands"] == 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert AN.repair_pitch(16000, 0.5, silence=2, pitchMethods="cep")["silence"] == 0.04  # repair()'s own
    assert len(w) == 1
    with pytest.raises(ValueError):
        AN.repair_pitch(16000, pitchMethods=())
    with pytest.raises(ValueError):
        AN.repair_pitch(16000, pitchMethods=("autocor", "yin"))


# ------------------------------------------------------------ sg_pitch_candidates_size
@pytest.mark.parametrize("sr", [16000, 20000, 22050, 44100, 48000])
def test_sg_pitch_candidates_size_equals_restatement(sr):
    n = 0
    for wlen in (50, 25, 20, 12):
        for kw in (dict(), dict(cepZp=401), dict(cepZp=1024), dict(cepZp=1200, cepSmooth=3, specSmooth=60),
                   dict(cepZp=2 ** 11, nCands=3, pitchFloor=150.5, pitchCeiling=2000, cutFreq=4000),
                   dict(cepSmooth=5, specSmooth=415, pitchFloor=50)):
            s = AN.repair_pitch(sr, None, windowLength=wlen, pitchMethods=("autocor", "spec", "dom"), **kw)
            wl = AN.pitch_decisions(0, s)["wl"]
            for length in (0, wl, wl + 1, 3 * wl + 17):
                want, got = AN.pitch_decisions(length, s), AN.pitch_decisions_native(length, s)
                keys = AN.PITCH_SIZE_KEYS + ("frames", "cols")
                assert {k: got[k] for k in keys} == {k: want[k] for k in keys}, (wlen, kw, length)
                assert np.array_equal(got["cepf"], want["cepf"]) and want["cols"] == 15 + 6 * s["nCands"]
                n += 1
    assert n == 96
    d = AN.pitch_decisions_native(4000, AN.repair_pitch(16000))
    assert (d["cepL"], d["cepSmooth"], d["cepl"], d["ncep"], d["specWidth"]) == (400, 11, 200, 104, 9)


def test_pitch_refusals():
    x = np.sin(np.arange(4000) * 0.1)
    for dec in (AN.pitch_decisions, AN.pitch_decisions_native):
        def go(**kw):
            return dec(4000, AN.repair_pitch(16000, **kw))
        with pytest.raises(ValueError, match="whole odd number.*zoo"):
            go(pitchMethods=ALL4, cepSmooth=4)
        with pytest.raises(ValueError, match="whole odd number"):
            go(pitchMethods=ALL4, cepZp=800)  # 11 * round(800 / 400): 22
        go(pitchMethods=("autocor", "spec", "dom"), cepSmooth=4)  # not asked for: not refused
        with pytest.raises(ValueError, match="no row of the cepstrum"):
            go(pitchMethods=ALL4, pitchFloor=4100, pitchCeiling=6000, cutFreq=7000, autocorSmooth=1)
        for zp, L in ((8191, 8190), (1034, 1034), (1111, 1110)):  # L / 2 = 4095: too long; 11 x 47; 3 x 5 x 37
            with pytest.raises(native.SoundgenError, match=r"%d-point transform is not supported \(L / 2" % L) as e:
                go(pitchMethods=("cep",), cepZp=zp)
            assert e.value.code == -4
        s22 = AN.repair_pitch(22050, pitchMethods=("cep",), cepZp=601)  # 551 bins + 2 x 25 zeros: L = 601, a prime
        with pytest.raises(native.SoundgenError, match=r"601-point transform is not supported \(L ") as e:
            dec(6000, s22)
        assert e.value.code == -4
        assert dec(6000, AN.repair_pitch(22050, pitchMethods=("cep",), cepZp=609))["cepL"] == 609  # 3 x 7 x 29, complex
        go(pitchMethods=("spec",), cepZp=8191)
        assert go(pitchMethods=("cep",), cepZp=551)["cepL"] == 550  # 275 = 5 x 5 x 11: packed
        assert go(pitchMethods=("cep",), cepZp=1225, cepSmooth=1)["cepL"] == 1224  # 612 = 4 x 9 x 17
        with pytest.raises(ValueError, match="width below 1"):
            go(specSmooth=-100)
        go(pitchMethods=("cep",), specSmooth=-100)
        # a window wider than its band is not refused: it finds no peak
        assert go(pitchMethods=ALL4, cepSmooth=999)["cepSmooth"] == 999
        assert go(specSmooth=20000)["specWidth"] == 1001
        # analyze_frames' refusals hold whatever the methods
        with pytest.raises(ValueError, match=r"acf\(\) then returns 801 values"):
            go(pitchMethods=("spec",), zp=1024)
        with pytest.raises(native.SoundgenError, match="at most 8"):
            go(nCands=9)
    with pytest.raises(ValueError, match="not longer than the window"):
        AN.pitch_candidates_numpy(x[:800], 16000)
    # the functions of analyze_frames still refuse the two methods
    with pytest.raises(NotImplementedError):
        AN.analyze_frames_numpy(x, 16000, pitchMethods=("autocor", "spec", "dom"))
    with pytest.raises(ValueError, match="non-empty subset of 'autocor', 'dom'$"):
        AN.frame_decisions_native(4000, dict(AN.repair(16000), pitchMethods=()))


def test_pitch_matrices_by_hand():
    nan = math.nan
    t = dict(ampl=np.zeros(4), domCand=np.array([nan, 300.0, nan, 310.0]), domCert=np.array([nan, 0.5, nan, 0.6]),
             autocorCand=np.array([[nan, nan], [150.0, 301.0], [nan, nan], [nan, nan]]),
             autocorCert=np.array([[nan, nan], [0.9, 0.8], [nan, nan], [nan, nan]]),
             cepCand=np.array([[nan, nan], [nan, nan], [149.0, nan], [nan, nan]]),
             cepCert=np.array([[nan, nan], [nan, nan], [0.3, nan], [nan, nan]]),
             specCand=np.array([[nan, nan], [152.0, nan], [151.0, 75.5], [305.0, nan]]),
             specCert=np.array([[nan, nan], [0.7, nan], [0.68, 0.4], [0.4, nan]]))
    cands, cert, source, names = AN.pitch_matrices(t)
    assert names == ("dom", "autocor", "cep", "spec") and cands.shape == cert.shape == source.shape == (4, 4)
    want = np.array([[nan, 300, 149, 310], [nan, 150, 151, 305], [nan, 301, 75.5, nan], [nan, 152, nan, nan]])
    assert np.array_equal(cands, want, equal_nan=True)
    assert np.array_equal(cert[:, 1], [0.5, 0.9, 0.8, 0.7]) and np.array_equal(cert[:, 2], [0.3, 0.68, 0.4, nan], equal_nan=True)
    assert source.tolist() == [[-1, 0, 2, 0], [-1, 1, 3, 3], [-1, 1, 3, -1], [-1, 3, -1, -1]]
    assert np.array_equal(np.isnan(cert), np.isnan(cands))
    e = {k: v[:1] * nan for k, v in t.items()}
    assert AN.pitch_matrices(e)[0].shape == (1, 1)  # at least one row
    assert AN.pitch_matrices(dict(ampl=np.zeros(0), domCand=np.zeros(0), domCert=np.zeros(0)))[0].shape == (1, 0)


# ------------------------------------------------------------ sg_bana.h on the host
def _hex(v):
    return float(v).hex()


def _bana_line(peaks, pars, nCands):
    c, a = AN.bana_candidates(peaks, nCands=nCands, **pars)
    five = list(peaks)[:5]
    p = (pars["pitchFloor"], pars["pitchCeiling"], pars["specSinglePeakCert"], pars["specThres"], pars["specMerge"], nCands)
    return " ".join([str(len(peaks))] + [_hex(v) for v in five] + [_hex(v) for v in p] + [str(len(c))] +
                    [_hex(v) for v in c + a])


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bana_header_on_the_host_equals_restatement(tmp_path):
    """sg_bana.h (what one thread of sg_anl_bana runs) built for the host as a
    stand-alone program under AddressSanitizer and UBSan, on the hand-worked cases
    and 4,000 random peak sets, against the restatement's results."""
    lines = []
    hand = ([440.0], [75.0], [60.0], [], [200.0, 400, 600], [200.0, 400, 600, 800, 1000], [200.0, 400, 600, 800, 1000, 1200],
            [100.0, 142], [100.0, 143], [100.0, 141], [100.0, 180], [200.0, 416, 657, 1117], [200.0, 410, 633],
            [300.0, 600, 1000], [300.0, 600, 900, 1500])
    for pk in hand:
        for nC in (1, 2, 3, 8):
            for kw in (dict(), dict(specThres=0.5), dict(specThres=0.7), dict(specMerge=0), dict(pitchFloor=30)):
                lines.append(_bana_line(pk, dict(B5, **kw), nC))
    rng = np.random.default_rng(5)
    for _ in range(4000):
        n = int(rng.integers(0, 9))
        if rng.uniform() < 0.5:  # near-harmonic sets, so that ratios match and candidates merge
            f0 = float(np.exp(rng.uniform(np.log(60), np.log(900))))
            h = np.sort(rng.choice(np.arange(1, 12), size=min(n, 11), replace=False))
            pk = f0 * h * (1 + rng.uniform(-0.02, 0.02, len(h)))
        else:
            pk = np.sort(np.exp(rng.uniform(np.log(40), np.log(6000), n)))
        pars = dict(pitchFloor=float(rng.choice([50, 75, 150.5])), pitchCeiling=float(rng.choice([1200, 3500])),
                    specSinglePeakCert=float(rng.uniform(0.2, 0.8)), specThres=float(rng.uniform(0, 0.9)),
                    specMerge=float(rng.choice([0, 0.5, 1, 2.5])))
        lines.append(_bana_line(np.sort(pk).tolist(), pars, int(rng.integers(1, 9))))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    exe = str(tmp_path / "bana_pins")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "bana_pins.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    tot, bad = (int(v) for v in r.stdout.split()[1::2])
    assert tot == len(lines) == 4300 and bad == 0


# ------------------------------------------------------------ the GPU cases' inputs
def _signal(sr, seed, dur=0.6):
    """tests/test_analyze_frames.py's input: a gliding eight-harmonic tone (220 -> 280 Hz)
    over 2 % noise, with a near-silent onset, a gap, and a noise-only tail."""
    rng = np.random.default_rng(seed)
    n = int(dur * sr)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(220 + 100 * t) / sr
    tone = sum(np.sin(h * ph) / h for h in range(1, 9))
    env = ((t > 0.11) & (t < 0.27)) | ((t > 0.37) & (t < 0.46))
    level = np.where(t < 0.1, 0.002, np.where(t > 0.48, 0.3, 0.02))
    return tone * env + level * rng.standard_normal(n)


# spec is NOT run with 20, 21, 23, 25, 37 or 40 ms windows at 16 kHz: their coarse bins put a harmonic
# ratio exactly on a table border (1400 / 500 = 2.8), a property of the input, not of the code
CASES = [
    (16000, "defaults", dict(pitchMethods=ALL4)),  # B = L = 400: packed, M = 200
    (22050, "defaults", dict(pitchMethods=ALL4)),  # L = 551, odd: the complex 19 x 29 transform
    (44100, "defaults", dict(pitchMethods=ALL4)),  # L = 1102: packed, M = 551; cepSmooth 31
    (16000, "wl30", dict(pitchMethods=ALL4, windowLength=30)),  # B = 240, spec width 3: the smallest for spec
    (16000, "wl20cep", dict(pitchMethods=("cep",), windowLength=20)),  # B = 160: the smallest for cep
    (16000, "cepZp1024", dict(pitchMethods=ALL4, cepZp=1024)),  # L = 1024, cepSmooth 33, band 268
    (16000, "cepZp401", dict(pitchMethods=ALL4, cepZp=401)),  # an odd difference: no padding, L = 400
    (16000, "ncands3", dict(pitchMethods=ALL4, nCands=3, cepThres=0.1, specPeak=0.2)),
    (16000, "specPeak.8", dict(pitchMethods=ALL4, specPeak=0.8)),  # one peak per frame
    (22050, "mix", dict(pitchMethods=ALL4, nCands=2, cepThres=0.15, cepSmooth=5, specPeak=0.15, specSmooth=60,
                        specMerge=0.5)),
    (16000, "cep", dict(pitchMethods=("cep",))),
    (16000, "spec", dict(pitchMethods=("spec",))),
    (16000, "reference-default", dict()),  # analyze()'s own default: autocor, spec, dom
    # cepstrum lengths the planner accepts whose radices (7, 11, 13, 17) and LDS sizes no case above launches
    (22050, "cepZp609", dict(pitchMethods=("cep",), cepZp=609)),  # L = 609, odd: complex 3 x 7 x 29
    (22050, "cepZp551", dict(pitchMethods=("cep",), cepZp=551)),  # cepZp = B: the padded branch with no zeros, L = 551
    (16000, "cepZp551", dict(pitchMethods=("cep",), cepZp=551)),  # L = 550: packed, M = 275 = 5 x 5 x 11
    (16000, "cepZp1225", dict(pitchMethods=("cep",), cepZp=1225, cepSmooth=1)),  # L = 1224, M = 612 = 4 x 3 x 3 x 17
    (16000, "wl38.5", dict(pitchMethods=("cep",), windowLength=38.5)),  # B = 308 = 4 x 7 x 11 in the frames, cepstrum M = 154
    (16000, "wl35.75", dict(pitchMethods=("cep",), windowLength=35.75)),  # B = 286, cepstrum M = 143 = 11 x 13
    (32000, "cepZp4096", dict(pitchMethods=("cep",), cepZp=4096)),  # L = 4096, M = 2048: 82 KB of LDS
    (22050, "cepZp1875", dict(pitchMethods=("cep",), cepZp=1875)),  # L = 1875, odd: complex 3 x 5^4, 68 KB
]
SEEDS = {(44100, "defaults"): 2}  # seed 1 leaves a margin of 4.5e-7 there
IDS = ["%d-%s" % (c[0], c[1]) for c in CASES]


def _seed(sr, name):
    return SEEDS.get((sr, name), 1)


@lru_cache(maxsize=None)
def _reference(i):
    sr, name, kw = CASES[i]
    probe = {}
    ref = AN.pitch_candidates_numpy(_signal(sr, _seed(sr, name)), sr, _probe=probe, **kw)
    for v in ref.values():
        v.setflags(write=False)
    return ref, probe


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b)) if a != b else 0.0


def _window_margins(x, width, thres):
    """The smallest relative margin of the decisions isCentral.localMax makes over the
    centred windows of x: x[c] against the threshold, and against the rest of its window."""
    h = width // 2
    m = math.inf
    for c in range(h, len(x) - h):
        m = min(m, _rel(x[c], thres))
        rest = np.delete(x[c - h:c + h + 1], h)
        if len(rest) and x[c] > thres:
            m = min(m, _rel(x[c], rest.max()))
    return m


def _pairs(pairs):
    return min([_rel(a, b) for a, b in pairs] + [math.inf])


def _margins(p):
    """The smallest relative margin of every discrete decision of the two trackers in a restatement run."""
    s = p["s"]
    out = dict(cep_peaks=math.inf, cep_order=math.inf, cep_rule18=math.inf, spec_peaks=math.inf, spec_ratio=math.inf,
               spec_range=math.inf, spec_merge=math.inf, spec_thres=math.inf)
    for tr in p["cep"].values():
        out["cep_peaks"] = min(out["cep_peaks"], _window_margins(tr["band"], tr["width"], s["cepThres"]))
        out["cep_order"] = min(out["cep_order"], _pairs(tr["order"]))  # the first maximum and the ranking
        out["cep_rule18"] = min(out["cep_rule18"], _pairs(tr["rule18"]))
    for f, tr in p["spec"].items():
        out["spec_peaks"] = min(out["spec_peaks"], _window_margins(p["normed"][f], tr["width"], s["specPeak"]))
        for k in ("ratio", "range", "merge", "thres"):
            out["spec_" + k] = min(out["spec_" + k], _pairs(tr[k]))
    return out


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pitch_inputs_are_well_conditioned(i):
    """Every discrete decision of the two trackers holds in the restatement alone with
    a relative margin >= 1e-6 on every tracked frame of every GPU case: the peak-or-not
    window and threshold decisions, the cepstrum's first maximum, ranking and 1.8 rule,
    each ratio against every border of BaNaRatios, each candidate against the pitch
    range, each merge comparison against specMerge / 12, each certainty against
    specThres. (The decisions of the shared columns are those of
    tests/test_analyze_frames.py, on the same signal.)"""
    ref, p = _reference(i)
    m = _margins(p)
    print(CASES[i][:2], {k: "%.2e" % v for k, v in m.items()})
    assert min(m.values()) >= MARGIN, m
    assert len(p["cep"]) + len(p["spec"]) >= 3


def test_pitch_inputs_have_frames_of_every_class():
    by = {IDS[i]: _reference(i) for i in range(len(CASES))}
    ref, p = by["16000-defaults"]
    ent = ref["cond_entropy"] == 1
    has_cep = ~np.isnan(ref["cepCand"][:, 0])
    assert (ent & has_cep).sum() >= 3 and (ent & ~has_cep).sum() >= 1  # tracked with and without a cep candidate
    assert not has_cep[~ent].any() and np.all(np.isnan(ref["specCand"][~ent]))
    multi = [tr for tr in p["spec"].values() if tr["npeaks"] >= 2]
    assert len(multi) >= 3 and sum(1 for tr in multi if max(tr.get("idx", [1])) >= 2) >= 2  # candidates merged
    ref, p = by["16000-specPeak.8"]
    one = [f for f, tr in p["spec"].items() if tr["npeaks"] == 1]
    assert len(one) >= 3 and sum(1 for f in one if not math.isnan(ref["specCand"][f, 0])) >= 3  # the single-peak branch
    assert all(ref["specCert"][f, 0] == 0.4 for f in one if not math.isnan(ref["specCand"][f, 0]))
    for k in ("16000-ncands3", "22050-mix"):
        ref, p = by[k]
        assert (~np.isnan(ref["specCand"][:, 1])).sum() >= 3  # two kept spec candidates
        assert max(tr["npeaks"] for tr in p["spec"].values()) >= 4
    assert (~np.isnan(by["22050-mix"][0]["cepCand"][:, 1])).sum() >= 3  # two kept cep candidates
    ref, _ = by["16000-cep"]
    assert np.all(np.isnan(ref["specCand"])) and np.all(np.isnan(ref["HNR"])) and np.all(np.isnan(ref["dom"]))
    ref, _ = by["16000-reference-default"]
    assert np.all(np.isnan(ref["cepCand"])) and (~np.isnan(ref["specCand"])).any() and (~np.isnan(ref["HNR"])).any()


CEP_LENGTHS = {"22050-cepZp609": 609, "22050-cepZp551": 551, "16000-cepZp551": 550, "16000-cepZp1225": 1224,
               "16000-wl38.5": 308, "16000-wl35.75": 286, "32000-cepZp4096": 4096, "22050-cepZp1875": 1875}


def test_cep_cases_reach_their_transforms():
    """The cases added for the cepstrum's transform make the library decide the length their
    comments name, and have frames to compare: >= 12 tracked, >= 10 with a cepstral candidate."""
    for i, (sr, name, kw) in enumerate(CASES):
        if IDS[i] not in CEP_LENGTHS:
            continue
        d = AN.pitch_decisions_native(int(0.6 * sr), AN.repair_pitch(sr, **kw))
        assert d["cepL"] == CEP_LENGTHS[IDS[i]], IDS[i]
        ref, p = _reference(i)
        assert len(p["cep"]) >= 12 and (~np.isnan(ref["cepCand"][:, 0])).sum() >= 10, IDS[i]


def test_pitch_candidates_numpy_equals_analyze_frames_numpy_on_shared_keys():
    x = _signal(16000, 1)
    for kw in (dict(), dict(pitchMethods=("autocor",), nCands=2), dict(pitchMethods=("dom",), windowLength=30)):
        a = AN.analyze_frames_numpy(x, 16000, **kw)
        b = AN.pitch_candidates_numpy(x, 16000, **dict(dict(pitchMethods=("autocor", "dom")), **kw))
        assert set(b) == set(a) | set(AN.PITCH_KEYS)
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        assert all(np.all(np.isnan(b[k])) and b[k].shape == a["autocorCand"].shape for k in AN.PITCH_KEYS)
    c = AN.pitch_candidates_numpy(x, 16000, pitchMethods=ALL4)  # the new methods leave the shared keys alone
    a = AN.analyze_frames_numpy(x, 16000)
    assert all(np.array_equal(a[k], c[k], equal_nan=True) for k in a)


# ------------------------------------------------------------ GPU
def _compare(got, ref):
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
        elif k in RELATIVE:
            err[k] = float(np.max(np.abs(g[ok] - r[ok]) / np.abs(r[ok]))) if ok.any() else 0.0
        else:
            err[k] = float(np.max(np.abs(g[ok] - r[ok]))) if ok.any() else 0.0
    print("pitch_candidates errors:", {k: "%.2e" % v for k, v in err.items()})
    for k, v in err.items():
        assert v <= TOL[k], (k, v)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_pitch_candidates_gpu_equals_numpy(i):
    sr, name, kw = CASES[i]
    ref, _ = _reference(i)
    _compare(AN.pitch_candidates(_signal(sr, _seed(sr, name)), sr, **kw), ref)


@pytest.mark.gpu
def test_pitch_candidates_equals_analyze_frames_on_shared_columns_gpu():
    x = _signal(16000, 1)
    for kw in (dict(), dict(pitchMethods=("autocor",), nCands=3, autocorThres=0.5), dict(pitchMethods=("dom",))):
        a = AN.analyze_frames(x, 16000, **kw)
        b = AN.pitch_candidates(x, 16000, **dict(dict(pitchMethods=("autocor", "dom")), **kw))
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
        assert all(np.all(np.isnan(b[k])) for k in AN.PITCH_KEYS)
    a, c = AN.analyze_frames(_signal(44100, 2), 44100), AN.pitch_candidates(_signal(44100, 2), 44100, pitchMethods=ALL4)
    assert all(np.array_equal(a[k], c[k], equal_nan=True) for k in a)


@pytest.mark.gpu
def test_pitch_candidates_batch_equals_single():
    """pitch_candidates_batch over five packed calls (one not longer than the window, the
    others of different lengths) equals pitch_candidates() per call bit for bit."""
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
    r = AN.pitch_candidates_batch(data, offs, lens, sr, **kw)
    assert r["out"].is_cuda and r["out"].dtype == torch.float64 and r["cols"] == 27 == len(r["columns"])
    assert r["columns"][15:] == sum((((k,) * 2) for k in ("autocorCand", "autocorCert", "cepCand", "cepCert", "specCand",
                                                          "specCert")), ())
    assert r["frames"][1] == 0 and r["frames"][4] == 1 and len(set(r["frames"])) == 5
    h = r["out"].cpu().numpy()
    tracked = ncep = nspec = 0
    for i in range(5):
        f = r["frames"][i]
        if f == 0:
            continue
        got = h[r["offsets"][i]:r["offsets"][i] + f * 27].reshape(f, 27)
        one = AN.pitch_candidates(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr, **kw)
        want = np.column_stack([one[k] for k in AN.COLUMNS] + [one["autocorCand"], one["autocorCert"]] +
                               [one[k] for k in AN.PITCH_KEYS])
        assert np.array_equal(got, want, equal_nan=True), i
        tracked += int(one["cond_entropy"].sum())
        ncep += int((~np.isnan(one["cepCand"])).sum())
        nspec += int((~np.isnan(one["specCand"])).sum())
    assert tracked >= 15 and ncep >= 10 and nspec >= 15
    lst = AN.pitch_candidates_batch(data, offs, lens, sr, to_host=True, **kw)
    assert lst[1]["specCand"].shape == (0, 2) and np.array_equal(lst[0]["specCert"], h[:r["frames"][0] * 27].reshape(-1, 27)[:, 25:27],
                                                                 equal_nan=True)


@pytest.mark.gpu
def test_pitch_candidates_errors_gpu():
    import torch
    x = _signal(16000, 1)[:4000]
    with pytest.raises(native.SoundgenError, match="8190-point transform") as e:
        AN.pitch_candidates(x, 16000, pitchMethods=ALL4, cepZp=8191)  # refused by the setup: nothing is launched
    assert e.value.code == -4
    d = torch.zeros(4000, dtype=torch.float32, device="cuda")
    with pytest.raises(native.SoundgenError) as e:
        AN.pitch_candidates_batch(d, [0], [4000], 16000, pitchMethods=("cep",), cepZp=8191)
    assert e.value.code == -4
    with pytest.raises(ValueError, match="whole odd number"):
        AN.pitch_candidates(x, 16000, pitchMethods=ALL4, cepSmooth=6)
    with pytest.raises(ValueError, match="not longer than the window"):
        AN.pitch_candidates(x[:800], 16000)
    r = AN.pitch_candidates_batch(d, [0, 0], [300, 800], 16000)  # nothing longer than the window: nothing launched
    assert r["frames"] == [0, 0] and r["cols"] == 21
    t = AN.pitch_candidates(x, 16000, pitchMethods=ALL4, cepSmooth=999, specSmooth=20000)  # windows wider than their bands
    assert len(t["ampl"]) == 8 and np.all(np.isnan(t["cepCand"])) and np.all(np.isnan(t["specCand"]))
    assert (~np.isnan(t["autocorCand"])).any()
