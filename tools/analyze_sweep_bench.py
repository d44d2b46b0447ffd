#!/usr/bin/env python3
"""Times a parameter sweep of analyze(summary = TRUE) (soundgen_beta_amd/analyze.py analyze_sweep;
sg_analyze_sweep in sg_analyze.hip) against the loop it replaces in optimize_pars(), on the --calls
C5 preset calls of tools/segment_sweep_bench.py already in HBM, and prints one JSON line. Row sets:
  * one          1 row (nothing to share);
  * tail16       16 rows that differ in the tail's parameters only (one candidate group);
  * grid         the reference's example (R/optimize.R:95-108) as a 4 x 4 grid of (specThres,
                 specSmooth) with the default pitchMethods: one store, 16 candidate groups;
  * grid_spec    the same grid with pitchMethods = 'spec' alone (no autocorrelation at all);
  * frames4      16 rows in 4 frame groups (windowLength 50, 40, 25, 20 ms).
Arms, each followed by sweep_fitness on the device:
  * loop         one analyze_batch(summary=True) per row (what optimize_pars() ran before);
  * sweep        analyze_sweep with the autocorrelation store on (the default);
  * sweep_off    the store off (sg_set_analyze_sweep_store(0)).
After --warmup runs of each arm, --steps runs of each in turn with profiling off, every run on record;
then --steps profiled runs of each sweep arm record the device time of the ten stages
(sg_debug_analyze_sweep_kernel_ms), so that the stage clock's events stay out of the wall times.
--loop-only times the loop alone: with SG_HIP_LIB set to a library built from the parent commit
that is the parent's figure, and --parent FILE merges such a run's JSON into this one's, adds the
ratios and checks the conditions (every set of 16 rows: the sweep's median wall below the parent
loop's minimum; one row: at most the parent loop's maximum).

    python tools/analyze_sweep_bench.py --out profiles/analyze_sweep_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"sweep": 1, "sweep_off": 0}


def row_sets():
    thres, smooth = (0.1, 0.2, 0.3, 0.4), (50, 100, 150, 200)
    grid = [dict(specThres=a, specSmooth=b) for a in thres for b in smooth]
    tail = [dict(certWeight=0.1 + 0.05 * i, shortestSyl=20 + 10 * (i % 4), shortestPause=40 + 10 * (i % 3), smooth=1 + (i % 2),
                 interpolWin=2 + i % 3, priorSD=4 + i % 5) for i in range(16)]
    frames = [dict(windowLength=(50, 40, 25, 20)[i % 4], certWeight=0.3 + 0.1 * (i // 4)) for i in range(16)]
    return {"one": [dict()], "tail16": tail, "grid": grid, "grid_spec": [dict(r, pitchMethods=("spec",)) for r in grid],
            "frames4": frames}


def mmm(v):
    v = sorted(v)
    return [round(v[0], 5), round(float(np.median(v)), 5), round(v[-1], 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=260)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sets", nargs="+", default=list(row_sets()))
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "analyze_sweep_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN
    from soundgen_beta_amd import batch, native
    from soundgen_beta_amd import optimize as OP

    sr = 44100
    data, offs, lens = batch.synthesize_packed(bench.c5_calls(a.calls), 0)
    L = native.lib()
    ctx = native.default_context(0)
    res = {"tool": "analyze_sweep_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup, "library": os.path.relpath(native.LIB_PATH, ROOT), "workloads": []}
    key = np.arange(a.calls, dtype=np.float64) % 7
    sets = row_sets()

    for name in a.sets:
        rows = sets[name]
        w = {"set": name, "rows": len(rows)}

        def loop():
            m = torch.stack([AN.analyze_batch(data, offs, lens, sr, summary=True, **kw)["out"] for kw in rows])
            OP.sweep_fitness(m, "pitch_median", key)

        def sweep(mode, profiled=False):
            L.sg_set_analyze_sweep_store(mode)
            L.sg_set_profiling(ctx.ptr, int(profiled))
            m = AN.analyze_sweep(data, offs, lens, sr, rows)
            L.sg_set_profiling(ctx.ptr, 0)
            OP.sweep_fitness(m, "pitch_median", key)
            return AN.sweep_kernel_ms() if profiled else None
        arms = {"loop": loop}
        if not a.loop_only:
            w["groups"] = [int(max(g) + 1) if len(g) else 0 for g in AN.sweep_plan(sr, rows)]
            arms.update({k: (lambda m=m: sweep(m)) for k, m in MODES.items()})
        for f in arms.values():
            for _ in range(a.warmup):
                f()
        runs = {k: [] for k in arms}
        for _ in range(a.steps):
            for k, f in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                runs[k].append({"wall_s": round(time.perf_counter() - t0, 6)})
        if not a.loop_only:  # the device stages in runs of their own: the stage clock's events stay out of the wall times
            for k, m in MODES.items():
                for r in runs[k]:
                    r["stage_ms"] = {s: round(v, 4) for s, v in sweep(m, True).items()}
        for k, v in runs.items():
            w[k] = {"runs": v, "wall_s_min_med_max": mmm([r["wall_s"] for r in v])}
            if "stage_ms" in v[0]:
                w[k]["stage_ms_median"] = {s: round(float(np.median([r["stage_ms"][s] for r in v])), 4) for s in AN.SWEEP_STAGES}
                w[k]["device_ms_min_med_max"] = mmm([sum(r["stage_ms"].values()) for r in v])
        if not a.loop_only:
            L.sg_set_analyze_sweep_store(1)
            w["loop_over_sweep_wall"] = round(w["loop"]["wall_s_min_med_max"][1] / w["sweep"]["wall_s_min_med_max"][1], 2)
        res["workloads"].append(w)
    if a.parent:
        with open(a.parent) as f:
            parent = json.loads(f.readline())
        res["parent_library"] = parent["library"]
        res["conditions"] = {}
        for w, p in zip(res["workloads"], parent["workloads"]):
            assert (w["set"], w["rows"]) == (p["set"], p["rows"])
            w["parent_loop"] = p["loop"]
            lo, _, hi = p["loop"]["wall_s_min_med_max"]
            med = w["sweep"]["wall_s_min_med_max"][1]
            w["parent_loop_over_sweep_wall"] = round(p["loop"]["wall_s_min_med_max"][1] / med, 2)
            res["conditions"][w["set"]] = bool(med < lo) if w["rows"] == 16 else bool(med <= hi)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
