#!/usr/bin/env python3
"""Times analyze()'s per-frame stage on the GPU (soundgen_beta_amd/analyze.py,
sg_analyze.hip) and prints one JSON line:

- analyze_frames_batch over --calls C5 preset calls (bench.py's c5_calls) already in
  HBM, tables left in HBM: wall time of the whole launch sequence (host decisions,
  the filter table, uploads, kernels) and the device time of each stage
  (sg_debug_analyze_kernel_ms);
- analyze_frames on one --seconds long recording (the batch's sounds one after another);
- analyze_frames_numpy on --numpy-calls of the calls: the host baseline, and whether
  the GPU tables agree with it on those calls (the gates exactly; the largest
  difference of HNR).

    python tools/analyze_frames_bench.py --out profiles/analyze_frames_bench.json
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

STAGES = ("spectrogram", "amplitude", "descriptives_dom", "autocor_peaks")


def timed(fn, warmup, steps, L):
    for _ in range(warmup):
        fn()
    wall, ms = [], []
    out = (C.c_double * len(STAGES))()
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        L.sg_debug_analyze_kernel_ms(out)
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
    assert torch.cuda.is_available(), "analyze_frames_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN, batch, native

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    host = data.cpu().numpy()
    idx = [i for i in range(a.calls) if lens[i] >= 2 * 2204][:a.numpy_calls]
    res = {"tool": "analyze_frames_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "failed_calls": int((lens < 0).sum())}
    last = {}
    wall, ms = timed(lambda: last.update(r=AN.analyze_frames_batch(data, offs, lens, sr)), a.warmup, a.steps, L)
    r = last["r"]
    h = r["out"].cpu().numpy()
    t0 = time.perf_counter()
    refs = [AN.analyze_frames_numpy(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr) for i in idx]
    tn = time.perf_counter() - t0
    err, gates = 0.0, True
    for i, ref in zip(idx, refs):
        f, c = r["frames"][i], r["cols"]
        got = h[int(r["offsets"][i]):int(r["offsets"][i]) + f * c].reshape(f, c)
        gates = gates and np.array_equal(got[:, 13], ref["cond_silence"]) and np.array_equal(got[:, 14], ref["cond_entropy"])
        d = np.abs(got[:, 2] - ref["HNR"])
        if np.isfinite(d).any():
            err = max(err, float(np.nanmax(d)))
    frames = int(sum(r["frames"]))
    tracked = int(np.nansum(h[:frames * r["cols"]].reshape(-1, r["cols"])[:, 14]))
    res["batch"] = {"wall_s": round(wall, 4), "calls_per_s": round(a.calls / wall, 1),
                    "device_ms": round(sum(ms.values()), 3), "stage_ms": ms, "largest_stage": max(ms, key=ms.get),
                    "frames": frames, "tracked_frames": tracked,
                    "numpy": {"calls": len(idx), "wall_s": round(tn, 4), "calls_per_s": round(len(idx) / tn, 2)},
                    "gates_equal_numpy": bool(gates), "max_abs_diff_HNR_vs_numpy": err}
    res["batch"]["speedup_vs_numpy"] = round(res["batch"]["calls_per_s"] / res["batch"]["numpy"]["calls_per_s"], 1)
    del r, last
    torch.cuda.empty_cache()
    # one long recording through sg_analyze_frames
    n_long = int(a.seconds * sr)
    reps = 1 + n_long // max(1, int(sum(lens[i] for i in idx)))
    rec = np.concatenate([host[offs[i]:offs[i] + lens[i]] for i in idx] * reps)[:n_long].astype(np.float64)
    got = {}
    wall, ms = timed(lambda: got.update(t=AN.analyze_frames(rec, sr)), a.warmup, a.steps, L)
    res["recording"] = {"seconds": round(len(rec) / sr, 2), "frames": int(len(got["t"]["ampl"])),
                        "tracked_frames": int(got["t"]["cond_entropy"].sum()), "wall_s": round(wall, 4),
                        "device_ms": round(sum(ms.values()), 3), "stage_ms": ms, "largest_stage": max(ms, key=ms.get)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
