#!/usr/bin/env python3
"""Times analyze()'s formant tracks (soundgen_beta_amd/formants.py; sg_fmt_lags and sg_fmt_roots in
sg_formants.hip, sg_formants.h) on the batch workload of tools/analyze_bench.py: --calls C5 preset
calls already in HBM. After --warmup runs, --steps runs with profiling on record, in the same run,

- the 8 stages of analyze_batch() without formants (sg_debug_track_kernel_ms; to set beside
  profiles/analyze_bench_with_summary.json: the spread of the runs in both files is the noise to
  judge by),
- the two formant kernels behind those tables (sg_debug_formants_kernel_ms), their share of
  analyze()'s device time, the frames analysed, the frames that hit the iteration cap and the
  mean Aberth iterations per analysed frame,

then the wall time of analyze_batch() with and without formants=True (which beside the two kernels
reruns the normalisation statistics, synchronises twice more and allocates the lag scratch), then
the wall time of formants_batch(to_host=True) on the first --sample sounds against
formants_numpy() on the same sounds, with the condition numbers of the Toeplitz systems of the
first 8 sounds' analysed frames. Prints one JSON line.

    python tools/formants_bench.py --out profiles/formants_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("spectrogram", "amplitude", "descriptives_dom", "autocor_peaks", "cepstrum_peaks", "spec_peaks_bana", "path",
          "harmonics")


def mmm(v):
    return [round(float(f(v)), 5) for f in (min, np.median, max)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--nFormants", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "formants_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN, batch, formants as FM, native

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    res = {"tool": "formants_bench", "calls": a.calls, "samplingRate": sr, "order": FM.formant_order(sr),
           "nFormants": a.nFormants, "samples": int(lens[lens > 0].sum()), "steps": a.steps, "warmup": a.warmup}

    L.sg_set_profiling(ctx.ptr, 1)
    st, fm, cnt = (C.c_double * 8)(), (C.c_double * 2)(), (C.c_int64 * 3)()
    prof = []
    for k in range(a.warmup + a.steps):
        r = AN.analyze_batch(data, offs, lens, sr, formants=True, nFormants=a.nFormants)
        L.sg_debug_track_kernel_ms(st)
        L.sg_debug_formants_kernel_ms(fm, cnt)
        if k >= a.warmup:
            prof.append({"stage_ms": dict(zip(STAGES, (round(v, 4) for v in st))), "lags_ms": round(fm[0], 4),
                         "roots_ms": round(fm[1], 4), "capped": int(cnt[0]), "analysed": int(cnt[1]),
                         "iterations": int(cnt[2])})
    L.sg_set_profiling(ctx.ptr, 0)
    res["frames"] = int(sum(r["frames"]))
    dev = [sum(p["stage_ms"].values()) for p in prof]
    fmt = [p["lags_ms"] + p["roots_ms"] for p in prof]
    res["device"] = {"runs": prof, "analyze_device_ms_min_med_max": mmm(dev),
                     "lags_ms_min_med_max": mmm([p["lags_ms"] for p in prof]),
                     "roots_ms_min_med_max": mmm([p["roots_ms"] for p in prof]),
                     "stage_ms_min_med_max": {k: mmm([p["stage_ms"][k] for p in prof]) for k in STAGES}}
    res["formants_over_analyze_device_time"] = round(float(np.median(fmt) / np.median(dev)), 5)
    res["frames_analysed"] = prof[-1]["analysed"]
    res["frames_capped"] = prof[-1]["capped"]
    res["mean_aberth_iterations"] = round(prof[-1]["iterations"] / max(prof[-1]["analysed"], 1), 3)
    res["roots_us_per_analysed_frame"] = round(1000 * float(np.median([p["roots_ms"] for p in prof])) / max(prof[-1]["analysed"], 1), 4)

    # wall time of the whole call with and without the formants: beside the two kernels, formants=True runs the four
    # normalisation-statistics launches again, synchronises the stream twice more and allocates the lag scratch
    wall = []
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        AN.analyze_batch(data, offs, lens, sr)
        t1 = time.perf_counter()
        AN.analyze_batch(data, offs, lens, sr, formants=True, nFormants=a.nFormants)
        t2 = time.perf_counter()
        if k >= a.warmup:
            wall.append((t1 - t0, t2 - t1))
    res["wall_s"] = {"analyze_batch_min_med_max": mmm([w[0] for w in wall]),
                     "analyze_batch_formants_min_med_max": mmm([w[1] for w in wall]),
                     "lag_scratch_bytes": res["frames"] * 65 * 8}

    # wall time against the host restatement on a sample
    n = min(a.sample, a.calls)
    sub = [i for i in range(a.calls) if lens[i] > 0][:n]
    so, sl = [int(offs[i]) for i in sub], [int(lens[i]) for i in sub]
    FM.formants_batch(data, so, sl, sr, nFormants=a.nFormants, to_host=True)
    t0 = time.perf_counter()
    got = FM.formants_batch(data, so, sl, sr, nFormants=a.nFormants, to_host=True)
    t1 = time.perf_counter()
    host = data.cpu().numpy().astype(np.float64)
    worst = 0.0
    same = True
    conds, counts = [], []
    order = FM.formant_order(sr)
    idx = np.abs(np.arange(order)[:, None] - np.arange(order)[None, :])
    t2 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for j, (o, m) in enumerate(zip(so, sl)):
            probe = {}
            ref = FM.formants_numpy(host[o:o + m], sr, nFormants=a.nFormants, _probe=probe)
            if j < 8:  # how well conditioned these frames are: the Toeplitz systems, and whether fp64 and long double
                for f in probe["analysed"]:  # keep the same number of roots
                    fr = probe["frames"][:, f]
                    conds.append(float(np.linalg.cond(FM.lpc_lags(fr, sr, order)[idx])))
                    counts.append(len(FM.find_formants_numpy(fr, sr)) == len(FM.find_formants_numpy(fr, sr, dtype=np.longdouble)))
            for k, v in ref.items():
                same = same and bool(np.array_equal(np.isnan(v), np.isnan(got[j][k])))
                ok = ~np.isnan(v) & ~np.isnan(got[j][k])
                if ok.any():
                    worst = max(worst, float(np.abs(v[ok] - got[j][k][ok]).max()))
    t3 = time.perf_counter()
    res["sample"] = {"sounds": len(sub), "gpu_wall_s": round(t1 - t0, 5), "numpy_wall_s": round(t3 - t2, 5),
                     "numpy_over_gpu": round((t3 - t2) / (t1 - t0), 1), "same_nan_pattern": same,
                     "max_abs_difference_hz": worst, "toeplitz_cond_frames": len(conds),
                     "toeplitz_cond_min_med_max": [float("%.3g" % v) for v in (min(conds), np.median(conds), max(conds))],
                     "fp64_and_long_double_keep_equal_counts": round(float(np.mean(counts)), 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
