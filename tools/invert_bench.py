#!/usr/bin/env python3
"""Times invert_spectrogram() on the GPU (soundgen_beta_amd/invert.py, sg_invert.hip) and
prints one JSON line:

- invert_spectrogram_batch over the magnitude matrices that spectrogram_batch (output =
  'original', default settings) leaves in HBM for --calls C5 preset calls (bench.py's
  c5_calls), --iters iterations from zero phases: wall time of the whole call (host tables,
  uploads, kernels of every chunk), and the device time of each stage
  (sg_debug_invert_kernel_ms) in total and per iteration. `inverse` and `overlap-add` run
  iters + 1 times (the output is one more A+), the others iters times;
- beside it the device time of spectrogram_device's frame stage (sg_spg_frames, one forward
  pass over the same frames) in the same run: an iteration is about one forward and one
  inverse pass;
- the share of an iteration that the overlap-add into a materialised x takes: what gathering
  the overlap-add inside the forward frames could save at most;
- invert_spectrogram_numpy (the fp64 restatement, a direct DFT) on --numpy-calls of the calls
  for --numpy-iters iterations: wall time, per iteration, and the largest relative difference
  of the GPU's e_k from its own on those calls and iterations.

    python tools/invert_bench.py --out profiles/invert_bench.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--numpy-calls", type=int, default=64)
    ap.add_argument("--numpy-iters", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workspace-cap", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "invert_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, invert as IV, native, spectrogram as SP

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    lens = np.where(lens > 0, lens, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    mag, moff, shapes = SP.spectrogram_batch(data, offs, lens, sr, output="original")
    spg = (C.c_double * 12)()
    frame_ms = []
    for _ in range(a.warmup + a.steps):
        SP.spectrogram_batch(data, offs, lens, sr, output="original")
        L.sg_debug_spectrogram_kernel_ms(spg)
        frame_ms.append(spg[1])
    frames = int(sum(f for _, f in shapes))
    need = [IV.invert_size(int(n), sr)["workspace_bytes"] for n in lens]
    res = {"tool": "invert_bench", "calls": a.calls, "iters": a.iters, "samplingRate": sr, "samples": int(lens.sum()),
           "frames": frames, "rows": shapes[0][0], "workspace_GB": round(sum(need) / 1e9, 3),
           "workspace_cap": a.workspace_cap, "spectrogram_frame_stage_ms": round(float(np.median(frame_ms[a.warmup:])), 4)}
    wall, ms = [], []
    last = None
    for k in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = IV.invert_spectrogram_batch(mag, moff, shapes, sr, lengths=lens, nIter=a.iters, workspace_cap=a.workspace_cap)
        wall.append(time.perf_counter() - t0)
        ms.append(IV.kernel_ms())
    k = a.warmup + int(np.argsort(wall[a.warmup:])[a.steps // 2])
    st = ms[k]
    runs = {"forward": a.iters, "error fold": a.iters, "inverse": a.iters + 1, "overlap-add": a.iters + 1}
    per = {s: st[s] / n for s, n in runs.items()}
    res["wall_s"] = round(wall[k], 4)
    res["calls_per_s"] = round(a.calls / wall[k], 1)
    res["stage_ms"] = {s: round(v, 4) for s, v in st.items()}
    res["device_ms"] = round(sum(st.values()), 3)
    res["per_iteration_ms"] = {s: round(v, 4) for s, v in per.items()}
    res["iteration_ms"] = round(sum(per.values()), 4)
    res["iteration_over_spectrogram_frame_stage"] = round(sum(per.values()) / res["spectrogram_frame_stage_ms"], 3)
    res["overlap_add_share_of_iteration"] = round(per["overlap-add"] / sum(per.values()), 4)
    err = last[2]
    ok = np.isfinite(err[:, 0])
    res["e_first_median"] = float(np.median(err[ok, 0]))
    res["e_last_median"] = float(np.median(err[ok, -1]))
    res["non_increasing_calls"] = int(np.sum(np.all(np.diff(err[ok], axis=1) <= 0, axis=1)))
    res["calls_with_frames"] = int(ok.sum())
    # the restatement on a sample of the calls
    idx = [i for i in range(a.calls) if shapes[i][1] > 0][:a.numpy_calls]
    hm = mag.cpu().numpy()
    t0 = time.perf_counter()
    worst = 0.0
    for i in idx:
        r, f = shapes[i]
        S = hm[moff[i]:moff[i] + r * f].reshape(f, r).T
        _, e = IV.invert_spectrogram_numpy(S, sr, length=int(lens[i]), nIter=a.numpy_iters)
        worst = max(worst, float(np.max(np.abs(err[i, :a.numpy_iters] - e) / e)))
    tn = time.perf_counter() - t0
    res["numpy"] = {"calls": len(idx), "iters": a.numpy_iters, "wall_s": round(tn, 3),
                    "wall_s_per_iteration": round(tn / max(a.numpy_iters, 1), 3), "max_rel_diff_of_e": worst}
    L.sg_set_profiling(ctx.ptr, 0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
