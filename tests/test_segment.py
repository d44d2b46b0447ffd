"""segment(): the numpy restatement (soundgen_beta_amd/segment.py) pinned by hand on the
reference's quirks, the planner (sg_segment_size / sg_segment_windows) against it, the
host/device header sg_segment.h as a stand-alone program, and the GPU path against the
restatement.

Tolerances of the GPU comparisons. Discrete outputs (row counts, `syllable`, the NaN
pattern, nSyl, nBursts) are compared exactly: every decision the restatement takes on
the GPU cases has a relative margin >= MARGIN (test_gpu_inputs_are_well_conditioned). The
envelope is compared relative to its maximum, times and lengths in ms absolutely, both
with BOUND. BOUND is the next power of ten above 8 x the largest deviation measured on an
MI355X over the cases below (DESIGN.md section 5 has the figures per case); 8 x covers
the spread between inputs outside the test set. Its ceiling is 1e-10: two 2^22-point fp64
transforms are 44 radix-2-equivalent stages at 1.1e-16 each, with four decades of
headroom for the means over a window's points.
"""
import math
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from soundgen_beta_amd import native
from soundgen_beta_amd import segment as SG

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "soundgen_beta_amd", "csrc")
MARGIN = 1e-6
BOUND = 1e-14
SR = 16000
nan = math.nan


# ------------------------------------------------------------------ hand pins (CPU)
def test_normalization_by_hand():
    # min > 0: scale() (centre, sd with n - 1), then / max(|max|, |min|)
    got = SG.normalize([1.0, 2.0, 3.0, 4.0])
    sd = math.sqrt(5 / 3)
    assert np.allclose(got, (np.array([-1.5, -.5, .5, 1.5]) / sd) / (1.5 / sd), rtol=1e-15)
    assert np.allclose(got, [-1, -1 / 3, 1 / 3, 1], rtol=1e-15)
    # min <= 0: no scale(); the larger magnitude is the minimum's
    assert np.array_equal(SG.normalize([-2.0, 1.0, 0.5]), [-1.0, 0.5, 0.25])
    assert np.array_equal(SG.normalize([0.0, 1.0, 4.0]), [0.0, 0.25, 1.0])  # min == 0 is not > 0


def test_window_points_by_hand():
    assert SG.window_points(48000, 16000, 40) == 640.0
    assert SG.window_points(48000, 16000, 40.01) == 641.0  # ceiling
    assert SG.window_points(1000, 16000, 40) == 500.0      # length / 2
    assert SG.window_points(1001, 16000, 40) == 500.5      # ... which may end in .5
    assert SG.window_points(1280, 16000, 40) == 640.0      # not larger than length / 2: kept


def test_hilbert_padding_and_multiplier_by_hand():
    assert SG.hilbert_layout(10) == (16, 3, 2, 10)   # nzp = 6: 3 + 3 zeros, starts one early
    assert SG.hilbert_layout(11) == (16, 2, 1, 11)   # nzp = 5: floor 2 on the left, ceiling 3 on the right
    assert SG.hilbert_layout(16) == (16, 0, 0, 16)   # a power of two: untouched
    assert SG.hilbert_layout(15) == (16, 0, 0, 14)   # diffn == 1: index 0 dropped, n1 - 1 values
    assert SG.hilbert_layout(17) == (32, 7, 6, 17)
    assert np.array_equal(SG.hilbert_multiplier(8), [1, 2, 2, 2, 1, 0, 0, 0])
    assert np.array_equal(SG.hilbert_multiplier(4), [1, 2, 1, 0])
    assert np.array_equal(SG.hilbert_multiplier(2), [2, 2])  # h[2:1] <- 2 overwrites both


@pytest.mark.parametrize("n1", [10, 11, 13, 15, 16, 17, 31])
def test_hilbert_envelope_numpy_equals_scipy(n1):
    """scipy.signal.hilbert on the padded signal, un-padded by the reference's rule: the
    first value lies in the padding and the last sample is dropped (diffn > 1); n1 = 2^p - 1
    gives n1 - 1 values that line up with the sound, the last sample missing."""
    from scipy.signal import hilbert
    x = np.random.default_rng(n1).standard_normal(n1)
    N = 1 << (n1 - 1).bit_length()
    left = (N - n1) // 2
    a = np.abs(hilbert(np.concatenate([np.zeros(left), x, np.zeros(N - n1 - left)])))
    got = SG.hilbert_envelope_numpy(x)
    if N == n1:
        want = a
    elif N - n1 == 1:
        want = a[:n1 - 1]
        assert len(got) == n1 - 1
    else:
        want = a[left - 1:left - 1 + n1]  # R's 1-based floor(diffn / 2) is the sample before the sound
        assert len(got) == n1
    assert np.allclose(got, want, rtol=0, atol=1e-14)
    if N - n1 > 1:  # the shift against the analytic signal of the padded sound, sample by sample
        assert abs(got[1] - a[left]) < 1e-14 and abs(got[-1] - a[left + n1 - 2]) < 1e-14


def test_r_seq_by_by_hand():
    assert np.array_equal(SG.r_seq_by(1.0, 26.0, 1.0), np.arange(1.0, 27.0))
    assert np.array_equal(SG.r_seq_by(1.0, 25.0, 2.5), 1 + 2.5 * np.arange(10))
    s = SG.r_seq_by(1.0, 1.0 + 3 * 0.1, 0.1)  # (to - from) / by = 3.0000000000000004 or 2.99...: the 1e-10 decides
    assert len(s) == 4 and s[-1] <= 1.0 + 3 * 0.1
    assert len(SG.r_seq_by(1.0, 1.29, 0.1)) == 3
    assert np.array_equal(SG.r_seq_by(1.0, 5.5, 5.5), [1.0])


def test_msmooth_by_hand():
    env = np.arange(1.0, 31.0)
    # whole wl: wl + 1 points per mean, not wl
    first, cnt, jump = SG.smoothing_windows(30, 30, 4.0, 75)
    assert np.array_equal(first, np.arange(26)) and set(cnt) == {5} and np.array_equal(jump, cnt)
    assert np.array_equal(SG.env_msmooth(env, 30, 4.0, 75), np.arange(3.0, 29.0))
    # a fractional by: x = 3.5 gives 3.5:8.5 = 3.5 ... 8.5, indices truncated to 3 ... 8
    first, cnt, _ = SG.smoothing_windows(30, 30, 5.0, 50)
    assert np.array_equal(first + 1, [1, 3, 6, 8, 11, 13, 16, 18, 21, 23]) and set(cnt) == {6}
    assert np.array_equal(SG.env_msmooth(env, 30, 5.0, 50)[:3], [3.5, 5.5, 8.5])
    # a fractional wl (length / 2 of an odd length): 1:6.5 is 1 ... 6
    first, cnt, _ = SG.smoothing_windows(11, 11, 5.5, 0)
    assert np.array_equal(first, [0]) and np.array_equal(cnt, [6])
    assert SG.env_msmooth(np.arange(1.0, 12.0), 11, 5.5, 0)[0] == 3.5
    # n1 = 2^p - 1: the envelope has n1 - 1 values and every window still ends inside it
    for n1 in (3, 7, 15, 31, 4095):
        for ov in (0, 50, 80, 99):
            first, cnt, jump = SG.smoothing_windows(n1, n1 - 1, SG.window_points(n1, 16000, 40), ov)
            assert (first + cnt + (jump < cnt)).max() <= n1 - 1
    with pytest.raises(ValueError):
        SG.smoothing_windows(2, 2, 1.0, 80)  # env() stops on a window of one point


def test_timestep_and_threshold():
    x = _signal(4097)
    tr = {}
    SG.segment_numpy(x, SR, _trace=tr)
    m = len(tr["envelope"])
    assert tr["timestep"] == 1000 / SR * (4097 / m)
    assert tr["threshold"] == SG.r_mean(tr["envelope"]) * 0.9


def test_find_syllables_by_hand():
    v = np.array([0, 0, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1, 0], dtype=float)
    s = SG.find_syllables(v, 10.0, 0.5, 20, None, False)  # count > ceiling(20 / 10) = 2
    assert np.array_equal(s["syllable"], [1, 2])
    assert np.array_equal(s["start"], [20, 80]) and np.array_equal(s["end"], [50, 120])
    assert np.array_equal(s["sylLen"], [30, 40])
    assert s["pauseLen"][0] == 30 and np.isnan(s["pauseLen"][1])  # the last pauseLen is NA
    m = SG.find_syllables(v, 10.0, 0.5, 20, 40, True)  # the gap of 30 < 40: merged
    assert np.array_equal(m["start"], [20]) and np.array_equal(m["end"], [120]) and np.array_equal(m["sylLen"], [100])
    assert np.isnan(m["pauseLen"]).all() and np.array_equal(m["syllable"], [1])
    k = SG.find_syllables(v, 10.0, 0.5, 20, 30, True)  # 30 < 30 is false: kept apart
    assert np.array_equal(k["start"], [20, 80])
    t = SG.find_syllables(v, 10.0, 0.5, 30, None, False)  # strict: a run of 3 is not > ceiling(3)
    assert np.array_equal(t["start"], [80]) and np.array_equal(t["end"], [120])
    # the envelope begins above the threshold: the first KEPT syllable starts at 0, although it is the run at 30 ms
    b = SG.find_syllables(np.array([1, 0, 0, 1, 1, 1, 0.0]), 10.0, 0.5, 20, None, False)
    assert np.array_equal(b["start"], [0]) and np.array_equal(b["end"], [30])
    # idx == 1: sum(count[c(1, 0)]) = count[1], overridden by the zero
    f = SG.find_syllables(np.array([1, 1, 1, 0.0]), 10.0, 0.5, 20, None, False)
    assert np.array_equal(f["start"], [0]) and np.array_equal(f["end"], [30])
    # value == threshold is not above it
    assert SG.find_syllables(np.array([.5, .5, .5, .5]), 10.0, 0.5, 20, None, False)["syllable"][0] == 0
    none = SG.find_syllables(np.zeros(6), 10.0, 0.5, 20, 40, True)
    assert sorted(none) == ["dur", "end", "start", "syllable"] and none["syllable"][0] == 0
    assert all(np.isnan(none[c][0]) for c in ("start", "end", "dur"))


def test_merge_chain_by_hand():
    s, e = SG.merge_syllables([0, 50, 100, 300, 330], [40, 90, 140, 320, 400], 20)
    assert np.array_equal(s, [0, 300]) and np.array_equal(e, [140, 400])  # the last merge reads row i + 1 past the end
    s, e = SG.merge_syllables([0.0], [10.0], 20)
    assert np.array_equal(s, [0]) and np.array_equal(e, [10])


def test_find_bursts_by_hand():
    v = np.array([1, 5, 1, 1, 5, 5, 1, 1, 4, 1], dtype=float)
    b = SG.find_bursts(v, 10.0, 20, 0.075, 3)  # n = 2
    assert np.array_equal(b["time"], [20, 50, 60, 90])  # i * timestep, 1-based i; both points of the plateau
    assert np.array_equal(b["ampl"], [5, 5, 5, 4])
    assert np.array_equal(b["interburstInt"][:3], [30, 10, 30]) and np.isnan(b["interburstInt"][3])
    assert np.array_equal(SG.find_bursts(v, 10.0, 29.9, 0.075, 3)["time"], [20, 50, 60, 90])  # floor
    # the right rule is i < nrow - n - 1: at i = 7 of 10 the window i:(i + n) would fit, but local_min_right is 0
    r = np.array([1, 1, 1, 1, 1, 1, 6, 5, 4, 4], dtype=float)
    assert np.array_equal(SG.find_bursts(r, 10.0, 20, 0.075, 3, troughLeft=False, troughRight=True)["time"], [70])
    r6 = np.array([1, 1, 1, 1, 1, 6, 5, 4, 4, 3], dtype=float)  # i = 6 < 7: min(6, 5, 4) = 4, 6 / 4 < 3
    assert len(SG.find_bursts(r6, 10.0, 20, 0.075, 3, troughLeft=False, troughRight=True)["time"]) == 0
    # the left rule is i > n: at i = n the ratio is Inf, at i = n + 1 it is 6 / 4
    assert np.array_equal(SG.find_bursts(np.array([4, 6, 1, 1, 1, 1, 1, 1, 1, 1.0]), 10.0, 20, 0.075, 3)["time"], [20])
    assert len(SG.find_bursts(np.array([4, 4, 6, 1, 1, 1, 1, 1, 1, 1.0]), 10.0, 20, 0.075, 3)["time"]) == 0
    # cond2 is strict, against the global maximum
    assert np.array_equal(SG.find_bursts(np.array([0, 1, 0, 0, 0, 10, 0, 0, 0, 0.0]), 10.0, 10, 0.1, 3)["time"], [60])
    e = SG.find_bursts(np.array([1, 1, 1.0]), 10.0, 0, 2.0, 3)
    assert sorted(e) == ["ampl", "time"] and len(e["time"]) == 0  # no interburstInt column
    with pytest.raises(ValueError, match="negative"):
        SG.find_bursts(v, 10.0, -1, 0.075, 3)
    with pytest.raises(ValueError, match="weird"):
        SG.find_bursts(v, 10.0, "a", 0.075, 3)


def test_summary_by_hand():
    syl = {"syllable": np.array([1., 2.]), "start": np.array([20., 80.]), "end": np.array([50., 120.]),
           "sylLen": np.array([30., 40.]), "pauseLen": np.array([30., nan])}
    bur = {"time": np.array([20., 50, 60, 90]), "ampl": np.array([5., 5, 5, 4]),
           "interburstInt": np.array([30., 10, 30, nan])}
    s = SG.segment_summary(syl, bur)
    assert list(s) == list(SG.SUMMARY_COLUMNS) and len(s) == 11
    assert s["nSyl"] == 2 and s["sylLen_mean"] == 35 and s["sylLen_median"] == 35
    assert abs(s["sylLen_sd"] - math.sqrt(50)) < 1e-14
    assert s["pauseLen_mean"] == 30 and s["pauseLen_median"] == 30 and np.isnan(s["pauseLen_sd"])  # sd without na.rm
    assert s["nBursts"] == 4 and abs(s["interburst_mean"] - 70 / 3) < 1e-14 and s["interburst_median"] == 30
    assert abs(s["interburst_sd"] - math.sqrt(((30 - 70 / 3) ** 2 * 2 + (10 - 70 / 3) ** 2) / 2)) < 1e-13
    one = SG.segment_summary({k: v[:1] for k, v in syl.items()} | {"pauseLen": np.array([nan])},
                             {k: v[:1] for k, v in bur.items()} | {"interburstInt": np.array([nan])})
    assert one["nSyl"] == 1 and one["sylLen_mean"] == 30 and np.isnan(one["sylLen_sd"])
    assert np.isnan(one["pauseLen_mean"]) and np.isnan(one["pauseLen_median"])  # NaN becomes NA
    assert one["nBursts"] == 1 and all(np.isnan(one[k]) for k in ("interburst_mean", "interburst_median", "interburst_sd"))
    none = SG.segment_summary({"syllable": np.array([0.]), "start": np.array([nan]), "end": np.array([nan]),
                               "dur": np.array([nan])}, {"time": np.zeros(0), "ampl": np.zeros(0)})
    assert none["nSyl"] == 1 and none["nBursts"] == 0  # nrow(syllables) is 1 without a syllable
    assert all(np.isnan(v) for k, v in none.items() if k not in ("nSyl", "nBursts"))


def test_interburst_default_and_fallback():
    x = _signal(8192)
    tr = {}
    r = SG.segment_numpy(x, SR, interburstMult=1.5, _trace=tr)
    assert tr["interburst"] == SG.r_median(r["syllables"]["sylLen"]) * 1.5
    tr = {}
    r = SG.segment_numpy(x, SR, shortestSyl=400, _trace=tr)
    assert r["syllables"]["syllable"][0] == 0 and tr["interburst"] == 400  # no syllable: shortestSyl


def test_refusals_on_the_host():
    x = _signal(4096)
    with pytest.raises(NotImplementedError):
        SG.segment_numpy(x, SR, plot=True)
    with pytest.raises(NotImplementedError):
        SG.segment(x, SR, plot=True)
    with pytest.raises(NotImplementedError):
        SG.segment_numpy(x, SR, savePath="/tmp/")
    with pytest.raises(NotImplementedError):
        SG.segment_numpy("sound.wav")
    for f in (SG.segment_numpy, SG.segment):
        with pytest.raises(ValueError, match="negative"):
            f(x, SR, interburst=-1)
        with pytest.raises(ValueError, match="weird"):
            f(x, SR, interburst="5")
        with pytest.raises(ValueError, match="samplingRate"):
            f(x)
        with pytest.raises(ValueError):
            f(x[:1], SR)
    with pytest.raises(ValueError):
        SG.segment_numpy(x[:2], SR)  # a window of one point: env() stops
    P = SG._params(SR)
    with pytest.raises(ValueError):
        SG.segment_size_native(2, P)
    with pytest.raises(native.SoundgenError, match="2\\^22") as e:
        SG.segment_size_native((1 << 22) + 1, P)
    assert e.value.code == -4
    assert SG.segment_size_native(1 << 22, P)["log2n"] == 22
    with pytest.raises(native.SoundgenError) as e:
        SG.segment_size_native((1 << 22) + 1, SG._params(1.0, mode=1))
    assert e.value.code == -4


# ------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("sr", [16000, 22050, 44100, 48000])
def test_planner_equals_restatement(sr):
    """sg_segment_size and the planner's windows (first index, points) and time step equal
    the restatement's exactly, fractional `by` and fractional windowLength_points included."""
    seen_frac_by = seen_frac_wl = seen_jump = False
    for n in (3, 7, 100, 1001, 1500, 2047, 2048, 4095, 4097, 10001, 48000, 65537):
        for wlen, ov in ((40, 80), (40, 75), (25, 33), (31.3, 99), (40, 0), (10, 50), (40, 150), (40, -5)):
            P = SG._params(sr, wlen, min(max(ov, 0), 99))
            wl = SG.window_points(n, sr, wlen)
            N, left, shift, n_env = SG.hilbert_layout(n)
            ov_c = min(max(ov, 0), 99)
            first, cnt, jump = SG.smoothing_windows(n, n_env, wl, ov_c)
            d = SG.segment_size_native(n, P)
            assert d["log2n"] == N.bit_length() - 1 and d["n_env"] == len(first) and d["points"] == cnt[0]
            assert d["cells"] == 19 + len(first) + 5 * ((len(first) + 1) // 2) + 4 * len(first)
            f2, c2, j2, ts = SG.segment_windows_native(n, P, len(first))
            assert np.array_equal(f2, first) and np.array_equal(c2, cnt) and np.array_equal(j2, jump)
            seen_jump |= bool((jump < cnt).any())
            assert ts == 1000 / sr * (n / len(first))
            seen_frac_by |= (wl - ov_c * wl / 100) % 1 != 0
            seen_frac_wl |= wl % 1 != 0
            e = SG.segment_size_native(n, SG._params(1.0, mode=1))
            assert e["n_env"] == n_env == e["cells"]
    assert seen_frac_by and seen_frac_wl
    if sr == 22050:  # by = 176.4: 1 + 5 * by is 882.9999999999999, and 882.99... + j rounds to a whole number from j = 141 on
        assert seen_jump


# ------------------------------------------------------- sg_segment.h as a host program
def _envelopes():
    """Generated envelopes with their settings: none, one and many syllables, merges,
    plateaus (quantized values tie), bursts at both boundaries. Only cases whose decisions
    the restatement takes with a margin >= MARGIN (the header adds in another order)."""
    rng = np.random.default_rng(7)
    out = []
    while len(out) < 300:
        m = int(rng.integers(1, 120))
        kind = int(rng.integers(0, 5))
        if kind == 0:
            v = rng.random(m)
        elif kind == 1:  # plateaus
            v = np.round(rng.random(m) * 4) / 4 + 0.25
        elif kind == 2:  # blocks: syllables with short and long pauses
            v = np.repeat(rng.random(m // 4 + 1) > 0.5, 4)[:m] * 1.0 + 0.01 * rng.random(m)
        elif kind == 3:  # peaks at both ends
            v = 0.1 + 0.05 * rng.random(m)
            v[0] = v[-1] = 1.0
            v[m // 2] = 2.0
        else:  # nothing above the threshold for long
            v = 1.0 + 0.3 * np.cos(np.arange(m) * math.pi)
        s = dict(timestep=float(rng.choice([7.3, 10.0, 12.5])), shortestSyl=float(rng.choice([0, 20, 40])),
                 shortestPause=rng.choice([nan, 15.0, 40.0]).item(), sylThres=float(rng.choice([0.9, 0.5])),
                 interburst=rng.choice([nan, 0.0, 25.0, 2000.0]).item(), interburstMult=float(rng.choice([1, 0.5])),
                 burstThres=0.075, peakToTrough=float(rng.choice([3, 1.05])), troughLeft=bool(rng.integers(0, 2)),
                 troughRight=bool(rng.integers(0, 2)))
        tr = {}
        ref = _tail_numpy(v, s, tr)
        margins = [tr[k] for k in ("threshold", "merge", "cond2", "cond3") if k in tr]
        if not margins or min(margins) >= MARGIN:
            out.append((v, s, ref))
    return out


def _tail_numpy(v, s, tr=None):
    thr = SG.r_mean(v) * s["sylThres"]
    merge = not math.isnan(s["shortestPause"])
    syl = SG.find_syllables(v, s["timestep"], thr, s["shortestSyl"], s["shortestPause"], merge, tr)
    ib = s["interburst"]
    if math.isnan(ib):
        ib = SG.r_median(syl["sylLen"]) * s["interburstMult"] if "sylLen" in syl else s["shortestSyl"]
    bur = SG.find_bursts(v, s["timestep"], ib, s["burstThres"], s["peakToTrough"], s["troughLeft"], s["troughRight"], tr)
    return dict(syl=syl, bur=bur, summary=SG.segment_summary(syl, bur), threshold=thr, interburst=ib)


def _hx(v):
    return "nan" if v != v else float(v).hex()


def _build_pins(tmp_path, sanitize):
    exe = str(tmp_path / ("segment_pins_san" if sanitize else "segment_pins"))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, os.path.join(HERE, "cpp", "segment_pins.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True, timeout=300)
    return exe


def _same(a, b, tol=0.0):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        bool(np.all(np.abs(a - b)[~np.isnan(a)] <= tol * np.maximum(1.0, np.abs(b[~np.isnan(a)]))))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_segment_header_on_the_host_equals_restatement(tmp_path):
    """sg_segment.h (what the lanes of sg_seg_tail run) built for the host as a stand-alone
    program, plain and with -fsanitize=address,undefined, on 300 generated envelopes: counts,
    `syllable` and the NaN pattern exactly; the times and lengths bit for bit (the same fp64
    operations); threshold, means and sds to 1e-13 (R's long double against fp64)."""
    cases = _envelopes()
    kinds = [(c[2]["syl"]["syllable"][0] == 0, len(c[2]["syl"]["syllable"]), len(c[2]["bur"]["time"])) for c in cases]
    assert sum(k[0] for k in kinds) >= 10 and sum((not k[0]) and k[1] == 1 for k in kinds) >= 10
    assert sum(k[1] >= 3 for k in kinds) >= 10 and sum(k[2] >= 3 for k in kinds) >= 10
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for v, s, _ in cases:
            head = [len(v), s["timestep"], math.ceil(s["shortestSyl"] / s["timestep"]), s["sylThres"], s["shortestSyl"],
                    s["shortestPause"], s["interburst"], s["interburstMult"], s["burstThres"], s["peakToTrough"],
                    int(s["troughLeft"]), int(s["troughRight"])]
            f.write(" ".join(_hx(h) for h in head) + " " + " ".join(_hx(x) for x in v) + "\n")
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
        for line, (v, s, ref) in zip(lines, cases):
            h = np.array([float.fromhex(x) if x != "nan" and x != "-nan" else nan for x in line.split()])
            m, rows, found, nb = (int(h[k]) for k in range(4))
            syl, bur = ref["syl"], ref["bur"]
            assert m == len(v) and rows == len(syl["syllable"]) and found == int("sylLen" in syl) and nb == len(bur["time"])
            assert _same(h[5], ref["threshold"], 1e-13) and h[6] == ref["interburst"]
            st = h[19:19 + 5 * rows].reshape(rows, 5)
            bt = h[19 + 5 * rows:].reshape(nb, 3)
            cols = SG.SYLLABLE_COLUMNS if found else ("syllable", "start", "end", "dur")
            for i, k in enumerate(cols):
                assert _same(st[:, i], syl[k]), k
            assert _same(bt[:, 0], bur["time"]) and _same(bt[:, 1], bur["ampl"])
            if nb:
                assert _same(bt[:, 2], bur["interburstInt"])
            assert _same(h[8:19], [ref["summary"][k] for k in SG.SUMMARY_COLUMNS], 1e-13)


# -------------------------------------------------------------------- the GPU cases
def _signal(n, seed=0, gain=1.0):
    """Bursts of a decaying 440 Hz tone, four a second with three amplitudes in turn, on
    low noise, at 16 kHz."""
    rng = np.random.default_rng(seed)
    period = SR // 4
    d = np.arange(period) / SR
    tone = np.exp(-d / 0.04) * np.sin(2 * np.pi * 440 * d)
    k = n // period + 2
    x = np.concatenate([np.zeros(SR // 20), (gain * (0.6 + 0.1 * (np.arange(k) % 3))[:, None] * tone[None, :]).ravel()])
    return x[:n] + 0.01 * rng.standard_normal(n)


BIG = (1 << 22) - 3
CASES = {
    "one-pass 2048": (2048, {}),
    "one-pass 1500": (1500, {}),
    "two-pass 4096": (4096, {}),
    "padded 4097": (4097, {}),
    "minimal padding 4095": (4095, {}),
    "non-square 8192": (8192, {}),
    "typical 48000": (48000, {}),
    "positive": (6000, {}),
    "no syllable": (8192, {"shortestSyl": 400}),
    "shortestPause None": (4097, {"shortestPause": None}),
    "troughRight": (4097, {"troughRight": True}),
    "interburst given": (4097, {"interburst": 100}),
    "skipped value": (4097, {"windowLength": 55.125}),  # 882 points, by = 176.4: the window at 1 + 5 by skips a value
    "largest p": (BIG, {}),
}


def _case_sound(name):
    n, _ = CASES[name]
    x = _signal(n, seed=len(name))
    return x + 2.0 if name == "positive" else x


@lru_cache(maxsize=None)
def _case(name):
    kw = CASES[name][1]
    tr = {}
    x = _case_sound(name)
    ref = SG.segment_numpy(x, SR, _trace=tr, **kw)
    return x, kw, ref, tr


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_inputs_are_well_conditioned(name):
    """Every decision of the restatement on a GPU case (value > threshold, count >
    ceiling(shortestSyl / timestep), the merge comparison, cond2, cond3) has a relative
    margin >= MARGIN, so a deviation within BOUND cannot flip one. cond1 compares a value
    with a maximum over values that include it and needs no margin."""
    x, kw, ref, tr = _case(name)
    margins = {k: tr[k] for k in ("threshold", "count", "merge", "cond2", "cond3") if k in tr}
    assert "threshold" in margins and "cond2" in margins
    assert min(margins.values()) >= MARGIN, margins
    if name == "positive":
        assert x.min() > 0
    if name == "skipped value":
        first, cnt, jump = SG.smoothing_windows(4097, 4097, 882.0, 80)
        assert (jump < cnt).any()
    if name == "no syllable":
        assert ref["syllables"]["syllable"][0] == 0 and "dur" in ref["syllables"]
    elif name != "largest p":
        assert ref["syllables"]["syllable"][0] == 1 and len(ref["bursts"]["time"]) >= 1
    if name == "typical 48000":
        assert len(ref["syllables"]["syllable"]) >= 10 and len(ref["bursts"]["time"]) >= 10


def _deviation(got, ref, dg, tr):
    """Exact comparison of the discrete outputs; the largest deviation of the continuous ones."""
    assert len(dg["envelope"]) == len(tr["envelope"]) and dg["timestep"] == tr["timestep"]
    dev = float(np.max(np.abs(dg["envelope"] - tr["envelope"])) / np.max(tr["envelope"]))
    dev = max(dev, abs(dg["threshold"] - tr["threshold"]) / np.max(tr["envelope"]))
    for part in ("syllables", "bursts"):
        assert sorted(got[part]) == sorted(ref[part]), part
        for k, want in ref[part].items():
            have = got[part][k]
            assert have.shape == want.shape and np.array_equal(np.isnan(have), np.isnan(want)), (part, k)
            ok = ~np.isnan(want)
            if k == "syllable":
                assert np.array_equal(have, want)
            elif ok.any():
                scale = np.max(tr["envelope"]) if k == "ampl" else 1.0
                dev = max(dev, float(np.max(np.abs(have[ok] - want[ok])) / scale))
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("name", [k for k in CASES if k != "largest p"])
def test_segment_gpu_equals_numpy(name):
    x, kw, ref, tr = _case(name)
    dg = {}
    got = SG.segment(x, SR, _detail_out=dg, **kw)
    dev = _deviation(got, ref, dg, tr)
    if name == "minimal padding 4095":  # n1 - 1 raw values: every window ended inside them
        assert len(SG.hilbert_envelope(x)) == 4094
    s_got = SG.segment(x, SR, summary=True, **kw)
    s_ref = SG.segment_summary(ref["syllables"], ref["bursts"])
    assert list(s_got) == list(SG.SUMMARY_COLUMNS)
    assert s_got["nSyl"] == s_ref["nSyl"] and s_got["nBursts"] == s_ref["nBursts"]
    for k in SG.SUMMARY_COLUMNS:
        assert math.isnan(s_got[k]) == math.isnan(s_ref[k]), k
        if not math.isnan(s_ref[k]):
            dev = max(dev, abs(s_got[k] - s_ref[k]))
    print("segment deviation %s: %.3e" % (name, dev))
    assert dev <= BOUND


@pytest.mark.gpu
def test_segment_gpu_largest_p():
    """2^22 - 3 samples, the largest transform: the envelope and the counts."""
    x, kw, ref, tr = _case("largest p")
    dg = {}
    got = SG.segment(x, SR, _detail_out=dg)
    assert len(dg["envelope"]) == len(tr["envelope"])
    dev = float(np.max(np.abs(dg["envelope"] - tr["envelope"])) / np.max(tr["envelope"]))
    print("segment deviation largest p: %.3e" % dev)
    assert dev <= BOUND
    assert len(got["syllables"]["syllable"]) == len(ref["syllables"]["syllable"])
    assert len(got["bursts"]["time"]) == len(ref["bursts"]["time"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1 << 22, (1 << 21) + 1, 4095, 1500, 2])
def test_hilbert_envelope_gpu_equals_numpy(n):
    """The transform alone: 2^22 points without padding; 2^21 + 1, the most padding there
    is; n1 = 2^p - 1 (n1 - 1 values); one workgroup; two samples."""
    x = _signal(n, seed=3)
    want = SG.hilbert_envelope_numpy(x)
    got = SG.hilbert_envelope(x)
    assert got.shape == want.shape
    dev = float(np.max(np.abs(got - want)) / np.max(want))
    print("hilbert deviation %d: %.3e" % (n, dev))
    assert dev <= BOUND


def _batch():
    import torch
    names = [k for k in CASES if k != "largest p"]
    parts = [_case_sound(k).astype(np.float32) for k in names] + [np.zeros(0, dtype=np.float32),
                                                                   np.array([0.5, -0.25], dtype=np.float32)]
    lens = np.array([len(v) for v in parts], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) + 3
    host = np.zeros(int(offs[-1] + lens[-1]) + 5, dtype=np.float32)
    for o, v in zip(offs, parts):
        host[o:o + len(v)] = v
    return parts, offs, lens, torch.from_numpy(host).cuda()


def _equal_results(a, b):
    for part in ("syllables", "bursts"):
        assert sorted(a[part]) == sorted(b[part])
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k], equal_nan=True), (part, k)


@pytest.mark.gpu
def test_segment_batch_equals_single_and_any_chunking():
    """segment_batch over every length of the cases (and an empty and a two-sample sound)
    equals segment() per call bit for bit, and the same batch under a workspace cap that
    forces several chunks equals the uncapped run bit for bit."""
    import torch
    parts, offs, lens, data = _batch()
    da = []
    res = SG.segment_batch(data, offs, lens, SR, _detail_out=da)
    assert res[-1] is None and res[-2] is None
    for i, v in enumerate(parts[:-2]):
        d1 = {}
        one = SG.segment(v.astype(np.float64), SR, _detail_out=d1)
        _equal_results(res[i], one)
        assert np.array_equal(da[i]["envelope"], d1["envelope"]) and da[i]["threshold"] == d1["threshold"]
        assert da[i]["interburst"] == d1["interburst"]
    dev = SG.segment_batch(data, offs, lens, SR, to_host=False)
    assert dev["out"].is_cuda and dev["out"].dtype == torch.float64
    h = dev["out"].cpu().numpy()
    for i in (len(parts) - 2, len(parts) - 1):  # the sounds the reference stops on: counts of 0, a NaN summary
        c = h[dev["offsets"][i]:dev["offsets"][i] + 19]
        assert not c[:8].any() and c[8] == 0 and c[15] == 0 and np.isnan(c[9:15]).all() and np.isnan(c[16:19]).all()
    db = []
    capped = SG.segment_batch(data, offs, lens, SR, workspace_cap=140000, _detail_out=db)  # 8750 cells: 4 chunks and more
    sums = SG.segment_batch(data, offs, lens, SR, summary=True)
    sums_capped = SG.segment_batch(data, offs, lens, SR, summary=True, workspace_cap=70000)
    for i in range(len(parts) - 2):
        _equal_results(res[i], capped[i])
        assert np.array_equal(da[i]["envelope"], db[i]["envelope"])
        assert all(np.array_equal(sums[i][k], sums_capped[i][k], equal_nan=True) for k in SG.SUMMARY_COLUMNS)


@pytest.mark.gpu
def test_segment_refusals_gpu():
    """More than 2^22 transform points by the declared length: refused before any launch."""
    import ctypes as C
    import torch
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    SG.segment(_signal(4097), SR)
    ms = (C.c_double * 6)()
    L.sg_debug_segment_kernel_ms(ms)
    before = list(ms)
    assert all(v > 0 for v in before)
    d = torch.full((5000,), 0.25, dtype=torch.float32, device="cuda")
    with pytest.raises(native.SoundgenError, match="2\\^22") as e:
        SG.segment_batch(d, [0, 0], [4000, (1 << 22) + 1], SR)
    assert e.value.code == -4
    P = SG._params(SR)  # the library's own check, behind the wrapper's call of sg_segment_size
    offs, lens, nc, p_offs, p_lens = native.batch_layout([0, 0], [4000, (1 << 22) + 1])
    ooff, p_ooff = native.out_offsets([SG.segment_size_native(4000, P)["cells"], 19])
    out = torch.full((int(ooff[-1]),), -1.0, dtype=torch.float64, device="cuda")
    rc = L.sg_segment_batch(ctx.ptr, C.c_void_p(d.data_ptr()), p_offs, p_lens, nc, C.byref(P), C.c_void_p(out.data_ptr()),
                            p_ooff)
    assert rc == -4 and b"2^22" in L.sg_last_error(ctx.ptr)
    assert bool((out == -1.0).all())
    L.sg_debug_segment_kernel_ms(ms)
    assert list(ms) == before  # the stage clocks of the run before are untouched: nothing was launched
    L.sg_set_profiling(ctx.ptr, 0)
    with pytest.raises(native.SoundgenError) as e:
        SG.hilbert_envelope(np.zeros((1 << 22) + 1))
    assert e.value.code == -4
