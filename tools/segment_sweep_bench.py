#!/usr/bin/env python3
"""Times a parameter sweep of segment() (soundgen_beta_amd/optimize.py segment_sweep;
sg_segment_sweep in sg_segment.hip) against the loop it replaces, on the --calls C5 preset
calls of tools/segment_bench.py already in HBM, and prints one JSON line. For 1, 16 and 64
parameter rows, once with all rows in one envelope group and once spread over 4 groups
(windowLength 40, 30, 25, 20 ms):
  * sweep: segment_sweep(to_host=False) followed by sweep_fitness, with the envelope staged
    in LDS by the tail and, alternating with it in the same process, read in place
    (sg_set_sweep_staging); per run the wall time and the device time per stage
    (sg_debug_sweep_kernel_ms);
  * loop: one segment_batch(summary=True, to_host=True) per row, the wall time of all rows.
After --warmup runs of each, --steps runs of each in turn, every run on record.
--loop-only times the loop alone: with SG_HIP_LIB set to a library built from the parent
commit (which has segment_batch and not the sweep) that is the parent's figure, and
--parent FILE merges such a run's JSON into this one's and adds the ratios.

    python tools/segment_sweep_bench.py --out profiles/segment_sweep_bench.json
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
WINDOWS = (40, 30, 25, 20)


def grid(rows, groups):
    """rows parameter rows over `groups` envelope groups; the tail's parameters vary by row."""
    r = np.arange(rows)
    return dict(windowLength=[WINDOWS[i % groups] for i in r], shortestSyl=[30 + 5 * (i % 5) for i in r],
                sylThres=[0.7 + 0.05 * (i % 7) for i in r], burstThres=[0.05 + 0.01 * (i % 4) for i in r],
                peakToTrough=[2 + 0.25 * (i % 6) for i in r])


def mmm(v):
    v = sorted(v)
    return [round(v[0], 5), round(float(np.median(v)), 5), round(v[-1], 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=260)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "segment_sweep_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, native
    from soundgen_beta_amd import segment as SG

    sr = 44100
    data, offs, lens = batch.synthesize_packed(bench.c5_calls(a.calls), 0)
    L = native.lib()
    ctx = native.default_context(0)
    res = {"tool": "segment_sweep_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup, "library": os.path.relpath(native.LIB_PATH, ROOT), "workloads": []}
    key = np.arange(a.calls, dtype=np.float64) % 7
    ms = (C.c_double * len(STAGES))()

    def loop(g):
        for i in range(len(g["windowLength"])):
            SG.segment_batch(data, offs, lens, sr, summary=True, **{k: v[i] for k, v in g.items()})

    for groups in (1, 4):
        for rows in a.rows:
            g = grid(rows, groups)
            w = {"rows": rows, "groups": min(groups, rows)}
            arms = {"loop": lambda: loop(g)}
            if not a.loop_only:
                from soundgen_beta_amd import optimize as OP

                def sweep(staging):  # the stage clock's events are part of the sweep's wall time, not of the loop's
                    L.sg_set_sweep_staging(staging)
                    L.sg_set_profiling(ctx.ptr, 1)
                    m = OP.segment_sweep(data, offs, lens, sr, g, to_host=False)
                    L.sg_set_profiling(ctx.ptr, 0)
                    L.sg_debug_sweep_kernel_ms(ms)
                    stage = list(ms)
                    OP.sweep_fitness(m, "nBursts", key)
                    return stage
                arms.update(sweep_lds=lambda: sweep(1), sweep_global=lambda: sweep(0))
            for f in arms.values():
                for _ in range(a.warmup):
                    f()
            runs = {k: [] for k in arms}
            for _ in range(a.steps):
                for k, f in arms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    stage = f()
                    wall = time.perf_counter() - t0
                    runs[k].append({"wall_s": round(wall, 6)} if stage is None else
                                   {"wall_s": round(wall, 6), "stage_ms": dict(zip(STAGES, (round(v, 4) for v in stage)))})
            for k, v in runs.items():
                w[k] = {"runs": v, "wall_s_min_med_max": mmm([r["wall_s"] for r in v])}
                if "stage_ms" in v[0]:
                    w[k]["stage_ms_median"] = {s: round(float(np.median([r["stage_ms"][s] for r in v])), 4) for s in STAGES}
                    w[k]["device_ms_min_med_max"] = mmm([sum(r["stage_ms"].values()) for r in v])
            if not a.loop_only:
                L.sg_set_sweep_staging(1)
                w["loop_over_sweep_wall"] = round(w["loop"]["wall_s_min_med_max"][1] / w["sweep_lds"]["wall_s_min_med_max"][1], 2)
            res["workloads"].append(w)
    if a.parent:
        with open(a.parent) as f:
            parent = json.loads(f.readline())
        for w, p in zip(res["workloads"], parent["workloads"]):
            assert (w["rows"], w["groups"]) == (p["rows"], p["groups"])
            w["parent_loop"] = p["loop"]
            w["parent_loop_over_sweep_wall"] = round(p["loop"]["wall_s_min_med_max"][1] /
                                                     w["sweep_lds"]["wall_s_min_med_max"][1], 2)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
