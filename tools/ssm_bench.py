#!/usr/bin/env python3
"""Times ssm() on the GPU (soundgen_beta_amd/ssm.py, sg_ssm.hip) and prints one JSON line:

- ssm_batch over --calls C5 preset calls (bench.py's c5_calls) already in HBM, with
  the default mfcc settings and with input = 'audiogram': wall time of the whole
  launch sequence (host decisions, uploads, kernels, novelty copied back) and the
  device time of each stage (sg_debug_ssm_kernel_ms);
- sg_ssm on one --seconds long recording (the batch's sounds one after another);
- the Gram kernel's fp64 rate: issued = 2048 flop per v_mfma_f64_16x16x4_f64 (tile
  padding included), useful = 2 L n^2 per sound (what the reference's double loop
  computes), and issued / device time over --fp64-peak-tflops (the vendor's fp64
  matrix figure for the MI355X);
- ssm_numpy on --numpy-calls of the calls, the host baseline, and the ratio.

    python tools/ssm_bench.py --out profiles/ssm_bench.json
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

STAGES = ("stats", "frames", "feat", "winstat", "gram", "novelty", "out")


def gram_flops(S, lens, sr, D_of, kw):
    """(issued, useful) flops of sg_ssm_gram over the sounds of `lens`."""
    issued = useful = 0
    for n_samp in lens:
        nf, n, win, _ = S.ssm_size(int(n_samp), sr, **kw)
        if n == 0:
            continue
        L = D_of * win
        nt = (n + 15) // 16
        issued += nt * (nt + 1) // 2 * ((L + 3) // 4) * 2048
        useful += 2 * L * n * n
    return issued, useful


def timed(fn, warmup, steps, L, ctx):
    for _ in range(warmup):
        fn()
    wall, ms = [], []
    out = (C.c_double * 7)()
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        L.sg_debug_ssm_kernel_ms(out)
        ms.append(list(out))
    k = int(np.argsort(wall)[len(wall) // 2])
    return wall[k], dict(zip(STAGES, (round(v, 4) for v in ms[k])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--numpy-calls", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fp64-peak-tflops", type=float, default=78.6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "ssm_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, native, ssm as S

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    res = {"tool": "ssm_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "failed_calls": int((lens < 0).sum())}
    for name, kw, D in (("mfcc", {}, 12), ("audiogram", {"input": "audiogram"}, 200)):
        last = {}
        wall, ms = timed(lambda: last.update(nov=S.ssm_batch(data, offs, lens, sr, **kw)), a.warmup, a.steps, L, ctx)
        issued, useful = gram_flops(S, lens, sr, D, {})
        dev = sum(ms.values())
        g = ms["gram"] * 1e-3
        top = max(ms, key=ms.get)
        res[name] = {"wall_s": round(wall, 4), "calls_per_s": round(a.calls / wall, 1), "device_ms": round(dev, 3),
                     "stage_ms": ms, "largest_stage": top, "novelty_points": int(sum(len(v) for v in last["nov"])),
                     "gram_flop_issued": issued, "gram_flop_useful": useful,
                     "gram_tflops_issued": round(issued / g / 1e12, 4) if g > 0 else None,
                     "gram_tflops_useful": round(useful / g / 1e12, 4) if g > 0 else None,
                     "gram_share_of_fp64_matrix_peak": round(issued / g / 1e12 / a.fp64_peak_tflops, 5) if g > 0
                     else None}
    # the host baseline on the first --numpy-calls calls that synthesized
    host = data.cpu().numpy()
    idx = [i for i in range(a.calls) if lens[i] > 1][:a.numpy_calls]
    t0 = time.perf_counter()
    for i in idx:
        S.ssm_numpy(host[offs[i]:offs[i] + lens[i]].astype(np.float64), sr, returnSSM=False)
    tn = time.perf_counter() - t0
    res["numpy"] = {"calls": len(idx), "wall_s": round(tn, 4), "calls_per_s": round(len(idx) / tn, 2)}
    res["mfcc"]["speedup_vs_numpy"] = round(res["mfcc"]["calls_per_s"] / res["numpy"]["calls_per_s"], 1)
    # one long recording through sg_ssm
    n_long = int(a.seconds * sr)
    reps = 1 + n_long // max(1, int(sum(lens[i] for i in idx)))
    rec = np.concatenate([host[offs[i]:offs[i] + lens[i]] for i in idx] * reps)
    rec = rec[:n_long].astype(np.float64)
    out = {}
    wall, ms = timed(lambda: out.update(S.ssm(rec, sr)), a.warmup, a.steps, L, ctx)
    nf, n, win, K = S.ssm_size(len(rec), sr)
    issued, useful = gram_flops(S, [len(rec)], sr, 12, {})
    g = ms["gram"] * 1e-3
    res["recording"] = {"seconds": round(len(rec) / sr, 2), "n_frames": nf, "n": n, "wall_s": round(wall, 4),
                        "device_ms": round(sum(ms.values()), 3), "stage_ms": ms, "largest_stage": max(ms, key=ms.get),
                        "gram_tflops_issued": round(issued / g / 1e12, 4) if g > 0 else None,
                        "gram_share_of_fp64_matrix_peak": round(issued / g / 1e12 / a.fp64_peak_tflops, 5) if g > 0
                        else None}
    res["fp64_matrix_peak_tflops_assumed"] = a.fp64_peak_tflops
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
