#!/usr/bin/env python3
"""Times analyze (soundgen_beta_amd/analyze.py; sg_anl_path and sg_anl_harm in
sg_analyze.hip) on the two workloads of tools/pitch_candidates_bench.py and prints one
JSON line: --calls C5 preset calls already in HBM (tables left in HBM), and one --seconds
long recording at 44.1 kHz. For each workload, after --warmup runs, --steps runs each of

- pitch_candidates        (sg_debug_pitch_kernel_ms: 6 stages),
- analyze                 (sg_debug_track_kernel_ms: the same 6 stages, which must cost the
  same -- the spread of the runs is the noise to judge that by -- then the path stage and
  the harmonics),
- pitch_candidates with the tables copied to the host plus the numpy tail
  (analyze.pitch_path_numpy per sound): the only route to a pitch contour without the two
  new stages; --host-calls bounds how many of the batch's sounds the host tail is timed on
  (its per-sound cost is then scaled to the batch),

with every run's stage times, so the run-to-run spread is on record. --pathfinding (default
'fast') is passed to analyze and to the numpy tail: 'exact' times sg_anl_path_exact.

    python tools/analyze_bench.py --out profiles/analyze_bench.json
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

STAGES = ("spectrogram", "amplitude", "descriptives_dom", "autocor_peaks", "cepstrum_peaks", "spec_peaks_bana", "path",
          "harmonics")


def timed(fn, hook, n, warmup, steps):
    """Per-run wall seconds and stage milliseconds, and their (min, median, max)."""
    for _ in range(warmup):
        fn()
    out = (C.c_double * n)()
    runs = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        hook(out)
        runs.append({"wall_s": round(wall, 5), "stage_ms": dict(zip(STAGES[:n], (round(v, 4) for v in out)))})
    dev = sorted(sum(r["stage_ms"].values()) for r in runs)
    summary = {k: [round(f([r["stage_ms"][k] for r in runs]), 4) for f in (min, np.median, max)] for k in STAGES[:n]}
    wall = sorted(r["wall_s"] for r in runs)
    return {"runs": runs, "device_ms_min_med_max": [round(dev[0], 3), round(float(np.median(dev)), 3), round(dev[-1], 3)],
            "wall_s_min_med_max": [wall[0], round(float(np.median(wall)), 5), wall[-1]], "stage_ms_min_med_max": summary}


def host_tail(tables, sr, step, pathfinding):
    """The numpy tail per sound: seconds."""
    from soundgen_beta_amd import analyze as AN
    t0 = time.perf_counter()
    for t in tables:
        if len(t["ampl"]):
            AN.pitch_path_numpy(t, step, sr, pathfinding=pathfinding)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-calls", type=int, default=256)
    ap.add_argument("--pathfinding", default="fast")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "analyze_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN, batch, native

    sr, step = 44100, 25.0
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    res = {"tool": "analyze_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup, "pathfinding": a.pathfinding,
           "library": os.path.relpath(native.LIB_PATH, ROOT)}

    def run_all(pitch_fn, analyze_fn, tables_fn, scale):
        out = {"pitch_candidates": timed(pitch_fn, L.sg_debug_pitch_kernel_ms, 6, a.warmup, a.steps),
               "analyze": timed(analyze_fn, L.sg_debug_track_kernel_ms, 8, a.warmup, a.steps)}
        st = out["analyze"]["stage_ms_min_med_max"]
        dev = out["analyze"]["device_ms_min_med_max"][1]
        out["path_and_harmonics_share_of_device_time"] = round((st["path"][1] + st["harmonics"][1]) / dev, 4)
        host = []
        for _ in range(a.steps):  # the host route: the tables to the host, then the numpy tail
            t0 = time.perf_counter()
            tables = tables_fn()
            fetch = time.perf_counter() - t0
            host.append({"candidates_to_host_s": round(fetch, 5), "numpy_tail_s": round(host_tail(tables, sr, step, a.pathfinding) * scale, 5)})
        out["host_route"] = {"runs": host, "tail_scaled_by": scale}
        tail = float(np.median([h["numpy_tail_s"] for h in host]))
        out["numpy_tail_s_over_path_and_harmonics_s"] = round(tail / ((st["path"][1] + st["harmonics"][1]) / 1e3), 1)
        return out

    last = {}
    nh = max(1, min(a.host_calls, a.calls))
    res["batch"] = run_all(lambda: last.update(p=AN.pitch_candidates_batch(data, offs, lens, sr)),
                           lambda: last.update(r=AN.analyze_batch(data, offs, lens, sr, pathfinding=a.pathfinding)),
                           lambda: AN.pitch_candidates_batch(data, offs, lens, sr, to_host=True)[:nh], a.calls / nh)
    r = last["r"]
    h = r["out"].cpu().numpy()[:sum(r["frames"]) * r["cols"]].reshape(-1, r["cols"])
    res["batch"].update(frames=int(sum(r["frames"])), tracked_frames=int(np.nansum(h[:, 14])),
                        voiced_frames=int(h[:, r["cols"] - 2].sum()))
    del r, last, h
    torch.cuda.empty_cache()
    host = data.cpu().numpy()
    idx = [i for i in range(a.calls) if lens[i] >= 2 * 2204][:16]
    n_long = int(a.seconds * sr)
    reps = 1 + n_long // max(1, int(sum(lens[i] for i in idx)))
    rec = np.concatenate([host[offs[i]:offs[i] + lens[i]] for i in idx] * reps)[:n_long].astype(np.float64)
    got = {}
    res["recording"] = run_all(lambda: got.update(p=AN.pitch_candidates(rec, sr)), lambda: got.update(t=AN.analyze(rec, sr, pathfinding=a.pathfinding)),
                               lambda: [AN.pitch_candidates(rec, sr)], 1.0)
    res["recording"].update(seconds=round(len(rec) / sr, 2), frames=int(len(got["t"]["ampl"])),
                            tracked_frames=int(got["t"]["cond_entropy"].sum()), voiced_frames=int(got["t"]["voiced"].sum()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
