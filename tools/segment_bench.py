#!/usr/bin/env python3
"""Times segment (soundgen_beta_amd/segment.py; sg_segment.hip) on two workloads and prints
one JSON line: --calls C5 preset calls already in HBM (the batch optimizePars would
evaluate per step of its search; results left in HBM), and one --seconds long recording at
44.1 kHz (a 2^22-point transform at 60 s). For each workload, after --warmup runs, --steps
runs with every run's wall time and stage times (sg_debug_segment_kernel_ms: statistics,
forward columns, rows, inverse columns, smoothing, tail), so the run-to-run spread is on
record, next to the time of the numpy restatement (segment.segment_numpy) on the same
sounds as context: --host-calls bounds how many of the batch's sounds it is timed on (its
per-sound cost is then scaled to the batch).

    python tools/segment_bench.py --out profiles/segment_bench.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("statistics", "columns_forward", "rows", "columns_inverse", "smoothing", "tail")


def timed(fn, hook, warmup, steps):
    """Per-run wall seconds and stage milliseconds, and their (min, median, max)."""
    for _ in range(warmup):
        fn()
    out = (C.c_double * len(STAGES))()
    runs = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        hook(out)
        runs.append({"wall_s": round(wall, 5), "stage_ms": dict(zip(STAGES, (round(v, 4) for v in out)))})
    dev = sorted(sum(r["stage_ms"].values()) for r in runs)
    summary = {k: [round(f([r["stage_ms"][k] for r in runs]), 4) for f in (min, np.median, max)] for k in STAGES}
    wall = sorted(r["wall_s"] for r in runs)
    return {"runs": runs, "device_ms_min_med_max": [round(dev[0], 3), round(float(np.median(dev)), 3), round(dev[-1], 3)],
            "wall_s_min_med_max": [wall[0], round(float(np.median(wall)), 5), wall[-1]], "stage_ms_min_med_max": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=260)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-calls", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "segment_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, native
    from soundgen_beta_amd import segment as SG

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    res = {"tool": "segment_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup}
    host = data.cpu().numpy()
    sounds = [host[offs[i]:offs[i] + lens[i]].astype(np.float64) for i in range(a.calls) if lens[i] >= 3]

    last = {}
    res["batch"] = timed(lambda: last.update(r=SG.segment_batch(data, offs, lens, sr, to_host=False)),
                         L.sg_debug_segment_kernel_ms, a.warmup, a.steps)
    P = SG._params(sr)
    res["batch"]["log2n"] = sorted({SG.segment_size_native(len(s), P)["log2n"] for s in sounds})
    summ = SG.segment_batch(data, offs, lens, sr, summary=True)
    res["batch"].update(syllables=int(sum(s["nSyl"] for s in summ if s)), bursts=int(sum(s["nBursts"] for s in summ if s)))
    nh = max(1, min(a.host_calls, len(sounds)))
    t0 = time.perf_counter()
    for s in sounds[:nh]:
        SG.segment_numpy(s, sr)
    res["batch"]["numpy_s"] = round((time.perf_counter() - t0) * len(sounds) / nh, 4)
    res["batch"]["numpy_scaled_by"] = round(len(sounds) / nh, 3)
    del last
    torch.cuda.empty_cache()

    n_long = int(a.seconds * sr)
    pool = [s for s in sounds if len(s) >= 4410][:16]
    reps = 1 + n_long // max(1, sum(len(s) for s in pool))
    rec = np.concatenate(pool * reps)[:n_long]
    got = {}
    res["recording"] = timed(lambda: got.update(r=SG.segment(rec, sr, summary=True)), L.sg_debug_segment_kernel_ms, a.warmup,
                             a.steps)
    t0 = time.perf_counter()
    ref = SG.segment_numpy(rec, sr, summary=True)
    res["recording"].update(seconds=round(len(rec) / sr, 2), log2n=SG.segment_size_native(len(rec), P)["log2n"],
                            syllables=int(got["r"]["nSyl"]), bursts=int(got["r"]["nBursts"]),
                            numpy_s=round(time.perf_counter() - t0, 4),
                            counts_equal_numpy=bool(ref["nSyl"] == got["r"]["nSyl"] and ref["nBursts"] == got["r"]["nBursts"]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
