#!/usr/bin/env python3
"""Times time_stretch() and shift_pitch() on the GPU (soundgen_beta_amd/stretch.py,
sg_stretch.hip) and prints one JSON line. Two workloads, default spectrogram() settings:

- `batch`: the sounds of --calls C5 preset calls (bench.py's c5_calls) as synthesize_packed
  leaves them in HBM: thousands of short sounds, parallelism to spare in (sound, bin);
- `long`: one recording of --seconds s at 44.1 kHz (a tone on noise, seeded): frames are the
  long dimension and only M + 1 lanes walk them.

For each, per stage device time (sg_debug_stretch_kernel_ms) of time_stretch(factor = 1.37) and
of shift_pitch(1.25) = time_stretch(1.25) then the resampler n : n_s. Beside them, in the same
run, the device time of stft_batch + istft_batch on the same sounds
(sg_debug_invert_kernel_ms): the kernels this feature adds to. Every figure is the median of --steps runs after --warmup, with the smallest
and the largest beside it: [median, min, max] milliseconds. Wall time of the whole call too.

    python tools/stretch_bench.py --out profiles/stretch_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(float(x) for x in v)
    return [round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=60)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "stretch_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, invert as IV, native, stretch as ST

    sr = 44100
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)

    def timed(fn, stages):
        """[median, min, max] of every stage and of the wall time over the steps."""
        rows, wall = [], []
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            rows.append(stages())
        rows, wall = rows[a.warmup:], wall[a.warmup:]
        out = {s: spread([r[s] for r in rows]) for s in rows[0]}
        out["device_total"] = spread([sum(r.values()) for r in rows])
        out["wall"] = spread(wall)
        return out

    def workload(data, offs, lens):
        res = {"sounds": len(lens), "samples": int(np.sum(lens))}
        z = [ST.stretch_size(int(n), sr, out_length=ST._out_length(int(n), 1.37)) for n in lens]
        res["frames_in"] = int(sum(s["frames_in"] for s in z))
        res["frames_out_1.37"] = int(sum(s["frames_out"] for s in z))
        res["workspace_GB_1.37"] = round(sum(s["workspace_bytes"] for s in z) / 1e9, 3)
        # the floor: the parent's kernels on the same sounds
        spec = {}

        def fwd():
            spec["v"] = IV.stft_batch(data, offs, lens, sr)
        res["stft_batch"] = timed(fwd, IV.kernel_ms)
        sp, soff, shapes = spec["v"]
        res["istft_batch"] = timed(lambda: IV.istft_batch(sp, soff, shapes, sr, lengths=lens), IV.kernel_ms)
        del sp, spec
        mid = {}
        res["time_stretch_1.37"] = timed(lambda: ST.time_stretch_batch(data, offs, lens, sr, factor=1.37), ST.kernel_ms)

        def st125():
            mid["v"] = ST.time_stretch_batch(data, offs, lens, sr, factor=1.25)
        res["shift_pitch_1.25_stretch"] = timed(st125, ST.kernel_ms)
        m, moff, mlen = mid["v"]
        ok = (np.asarray(lens) > 0) & (mlen > 0)
        res["shift_pitch_1.25_resample"] = timed(
            lambda: ST.resample_batch(m, moff, np.where(ok, mlen, 0), up=np.where(ok, lens, 1), down=np.where(ok, mlen, 1)),
            ST.kernel_ms)
        return res

    out = {"tool": "stretch_bench", "samplingRate": sr, "steps": a.steps, "warmup": a.warmup, "unit": "ms [median, min, max]"}
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    lens = np.where(lens > 0, lens, 0)
    out["batch"] = workload(data, offs, lens)
    del data
    n = int(a.seconds * sr)
    rng = np.random.default_rng(1)
    x = np.sin(2 * np.pi * 1234.5 * np.arange(n) / sr + 0.3) + 0.2 * rng.standard_normal(n)
    out["long"] = workload(torch.from_numpy(x).cuda(), np.zeros(1, dtype=np.int64), np.asarray([n], dtype=np.int64))
    L.sg_set_profiling(ctx.ptr, 0)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
