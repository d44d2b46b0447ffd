#!/usr/bin/env python3
"""Times analyze(summary = TRUE) (soundgen_beta_amd/analyze.py; sg_anl_summary in
sg_analyze.hip, sg_summary.h) on the batch workload of tools/analyze_bench.py: --calls C5
preset calls already in HBM. After --warmup runs, --steps runs each of the two routes to
the same 44 numbers per sound:

- (a) the route without the kernel: analyze_batch(), the tables copied to the host, and a
  vectorised numpy reduction per sound (nanmean / nanmedian / nanstd(ddof = 1) over the 14
  columns at once; not the long-double restatement, which is a yardstick for values and
  not for speed);
- (b) analyze_batch(summary=True), the n_calls x 44 matrix copied to the host.

With profiling on, every run of (b) records the 8 stages of analyze
(sg_debug_track_kernel_ms, to set beside profiles/analyze_bench.json: the spread of the
runs in both files is the noise to judge by) and the summary kernel
(sg_debug_summary_kernel_ms), and the tool reports the kernel's share of analyze's device
time. Prints one JSON line.

    python tools/analyze_summary_bench.py --out profiles/analyze_summary_bench.json
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


def numpy_rows(h, offsets, frames, cols, var_cols, lens, sr):
    """Route (a)'s reduction: n_calls x 44 from the host copy of the tables."""
    out = np.full((len(frames), 44), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # all-NaN columns, fewer than two values
        for i, f in enumerate(frames):
            if f == 0:
                continue
            t = h[offsets[i]:offsets[i] + f * cols].reshape(f, cols)
            x = t[:, var_cols]
            out[i, 0] = lens[i] / sr
            out[i, 1] = t[:, cols - 2].mean()
            out[i, 2::3] = np.nanmean(x, axis=0)
            out[i, 3::3] = np.nanmedian(x, axis=0)
            out[i, 4::3] = np.nanstd(x, axis=0, ddof=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "analyze_summary_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN, batch, native

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    res = {"tool": "analyze_summary_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup}
    r0 = AN.analyze_batch(data, offs, lens, sr)
    cols, c0 = r0["cols"], r0["cols"] - 4
    names = AN.COLUMNS
    var_cols = [{"pitch": c0, "amplVoiced": c0 + 1, "harmonics": c0 + 3}.get(v, names.index(v) if v in names else -1)
                for v in AN.SUMMARY_VARS]
    res.update(frames=int(sum(r0["frames"])), cols=cols,
               table_bytes_to_host=int(sum(r0["frames"])) * cols * 8, summary_bytes_to_host=a.calls * 44 * 8)
    del r0

    def route_a():
        t0 = time.perf_counter()
        r = AN.analyze_batch(data, offs, lens, sr)
        t1 = time.perf_counter()
        h = r["out"].cpu().numpy()
        t2 = time.perf_counter()
        rows = numpy_rows(h, r["offsets"], r["frames"], cols, var_cols, lens, sr)
        t3 = time.perf_counter()
        return rows, {"analyze_batch_s": round(t1 - t0, 5), "tables_to_host_s": round(t2 - t1, 5),
                      "numpy_reduction_s": round(t3 - t2, 5), "wall_s": round(t3 - t0, 5)}

    def route_b():
        t0 = time.perf_counter()
        r = AN.analyze_batch(data, offs, lens, sr, summary=True)
        t1 = time.perf_counter()
        rows = r["out"].cpu().numpy()
        t2 = time.perf_counter()
        return rows, {"analyze_batch_summary_s": round(t1 - t0, 5), "rows_to_host_s": round(t2 - t1, 5),
                      "wall_s": round(t2 - t0, 5)}

    for _ in range(a.warmup):
        ra, _ = route_a()
        rb, _ = route_b()
    runs_a = [route_a()[1] for _ in range(a.steps)]
    runs_b = [route_b()[1] for _ in range(a.steps)]
    res["route_a_host_numpy"] = {"runs": runs_a, "wall_s_min_med_max": mmm([r["wall_s"] for r in runs_a])}
    res["route_b_device_summary"] = {"runs": runs_b, "wall_s_min_med_max": mmm([r["wall_s"] for r in runs_b])}
    res["route_a_wall_over_route_b_wall"] = round(res["route_a_host_numpy"]["wall_s_min_med_max"][1] /
                                                  res["route_b_device_summary"]["wall_s_min_med_max"][1], 2)
    # the two routes agree (numpy's arithmetic is not R's: a loose check that they are the same numbers)
    ok = np.isfinite(ra) & np.isfinite(rb)
    res["routes_max_rel_difference"] = float(np.max(np.abs(ra[ok] - rb[ok]) / np.maximum(1.0, np.abs(rb[ok]))))
    res["routes_same_nan_pattern"] = bool(np.array_equal(np.isnan(ra), np.isnan(rb)))

    # device time: the eight stages of analyze and the summary kernel, per run
    L.sg_set_profiling(ctx.ptr, 1)
    for _ in range(a.warmup):
        AN.analyze_batch(data, offs, lens, sr, summary=True)
    st, sm = (C.c_double * 8)(), (C.c_double * 1)()
    prof = []
    for _ in range(a.steps):
        AN.analyze_batch(data, offs, lens, sr, summary=True)
        L.sg_debug_track_kernel_ms(st)
        L.sg_debug_summary_kernel_ms(sm)
        prof.append({"stage_ms": dict(zip(STAGES, (round(v, 4) for v in st))), "summary_ms": round(sm[0], 4)})
    L.sg_set_profiling(ctx.ptr, 0)
    dev = [sum(p["stage_ms"].values()) for p in prof]
    res["device"] = {"runs": prof, "analyze_device_ms_min_med_max": mmm(dev),
                     "summary_ms_min_med_max": mmm([p["summary_ms"] for p in prof]),
                     "stage_ms_min_med_max": {k: mmm([p["stage_ms"][k] for p in prof]) for k in STAGES}}
    res["summary_share_of_analyze_device_time"] = round(float(np.median([p["summary_ms"] for p in prof]) / np.median(dev)), 5)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
