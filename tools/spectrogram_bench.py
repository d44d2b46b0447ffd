#!/usr/bin/env python3
"""Times spectrogram() on the GPU (soundgen_beta_amd/spectrogram.py, sg_spectrogram.hip)
and prints one JSON line:

- spectrogram_batch over --calls C5 preset calls (bench.py's c5_calls) already in
  HBM, matrices left in HBM, with the default settings and with every pass of the
  chain on: wall time of the whole launch sequence (host decisions, uploads,
  kernels) and the device time of each stage (sg_debug_spectrogram_kernel_ms);
- sg_spectrogram on one --seconds long recording (the batch's sounds one after
  another), defaults;
- spectrogram_numpy on --numpy-calls of the calls: the host baseline, and the
  largest difference of the GPU matrices from it on those calls (the check is
  against the restatement, never against the code under test).

    python tools/spectrogram_bench.py --out profiles/spectrogram_bench.json
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

STAGES = ("stats", "frames", "derivative", "median_bins", "median_frames", "quantile_range", "log", "entropy",
          "entropy_quantile", "noise_spectrum", "subtract", "power_scale")
ALL_ON = dict(method="spectralDerivative", smoothTime=3, smoothFreq=3, qTime=0.5, noiseReduction=1.1)


def timed(fn, warmup, steps, L):
    for _ in range(warmup):
        fn()
    wall, ms = [], []
    out = (C.c_double * len(STAGES))()
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        L.sg_debug_spectrogram_kernel_ms(out)
        ms.append(list(out))
    k = int(np.argsort(wall)[len(wall) // 2])
    return wall[k], dict(zip(STAGES, (round(v, 4) for v in ms[k])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--numpy-calls", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "spectrogram_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, native, spectrogram as SP

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    host = data.cpu().numpy()
    idx = [i for i in range(a.calls) if lens[i] >= 2204 + 2 * 662][:a.numpy_calls]
    res = {"tool": "spectrogram_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "failed_calls": int((lens < 0).sum())}
    for name, kw in (("defaults", {}), ("all_passes", ALL_ON)):
        last = {}
        wall, ms = timed(lambda: last.update(r=SP.spectrogram_batch(data, offs, lens, sr, **kw)), a.warmup, a.steps, L)
        out, ooff, shapes = last["r"]
        cells = int(sum(b * f for b, f in shapes))
        t0 = time.perf_counter()
        refs = [SP.spectrogram_numpy(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr, **kw) for i in idx]
        tn = time.perf_counter() - t0
        err = 0.0
        for i, ref in zip(idx, refs):
            b, f = shapes[i]
            got = out[int(ooff[i]):int(ooff[i]) + b * f].cpu().numpy().reshape(f, b).T
            err = max(err, float(np.max(np.abs(got - ref))))
        res[name] = {"wall_s": round(wall, 4), "calls_per_s": round(a.calls / wall, 1),
                     "device_ms": round(sum(ms.values()), 3), "stage_ms": ms, "largest_stage": max(ms, key=ms.get),
                     "frames": int(sum(f for _, f in shapes)), "cells": cells, "output_GB": round(cells * 8 / 1e9, 3),
                     "numpy": {"calls": len(idx), "wall_s": round(tn, 4), "calls_per_s": round(len(idx) / tn, 2)},
                     "max_abs_diff_vs_numpy": err}
        res[name]["speedup_vs_numpy"] = round(res[name]["calls_per_s"] / res[name]["numpy"]["calls_per_s"], 1)
        del out, last
        torch.cuda.empty_cache()
    # one long recording through sg_spectrogram
    n_long = int(a.seconds * sr)
    reps = 1 + n_long // max(1, int(sum(lens[i] for i in idx)))
    rec = np.concatenate([host[offs[i]:offs[i] + lens[i]] for i in idx] * reps)[:n_long].astype(np.float64)
    got = {}
    wall, ms = timed(lambda: got.update(z=SP.spectrogram(rec, sr)), a.warmup, a.steps, L)
    t0 = time.perf_counter()
    ref = SP.spectrogram_numpy(rec, sr)
    tn = time.perf_counter() - t0
    res["recording"] = {"seconds": round(len(rec) / sr, 2), "frames": int(ref.shape[1]), "wall_s": round(wall, 4),
                        "device_ms": round(sum(ms.values()), 3), "stage_ms": ms, "largest_stage": max(ms, key=ms.get),
                        "numpy_wall_s": round(tn, 4), "max_abs_diff_vs_numpy": float(np.max(np.abs(got["z"] - ref)))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
