#!/usr/bin/env python3
"""Times pitch_candidates (soundgen_beta_amd/analyze.py; sg_anl_cep and sg_anl_bana in
sg_analyze.hip) on the two workloads of tools/analyze_frames_bench.py and prints one
JSON line: --calls C5 preset calls already in HBM (tables left in HBM), and one
--seconds long recording at 44.1 kHz. For each workload, after --warmup runs, --steps
runs each of

- analyze_frames                       (sg_debug_analyze_kernel_ms: 4 stages),
- pitch_candidates, ('autocor', 'dom') (sg_debug_pitch_kernel_ms: the same 4 stages
  must cost the same; the spread of the runs is the noise to judge that by),
- pitch_candidates, analyze()'s default ('autocor', 'spec', 'dom'),
- pitch_candidates, all four methods,

with every run's stage times, so the run-to-run spread is on record.

    python tools/pitch_candidates_bench.py --out profiles/pitch_candidates_bench.json
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

STAGES = ("spectrogram", "amplitude", "descriptives_dom", "autocor_peaks", "cepstrum_peaks", "spec_peaks_bana")
ALL4 = ("autocor", "cep", "spec", "dom")


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
    return {"runs": runs, "device_ms_min_med_max": [round(dev[0], 3), round(float(np.median(dev)), 3), round(dev[-1], 3)],
            "stage_ms_min_med_max": summary}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "pitch_candidates_bench needs a GPU"
    import bench
    from soundgen_beta_amd import analyze as AN, batch, native

    sr = 44100
    calls = bench.c5_calls(a.calls)
    data, offs, lens = batch.synthesize_packed(calls, 0)
    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    res = {"tool": "pitch_candidates_bench", "calls": a.calls, "samplingRate": sr, "samples": int(lens[lens > 0].sum()),
           "steps": a.steps, "warmup": a.warmup}
    variants = (("analyze_frames", None, 4), ("pitch_autocor_dom", ("autocor", "dom"), 6),
                ("pitch_default", ("autocor", "spec", "dom"), 6), ("pitch_all4", ALL4, 6))

    def run_all(single, batch_fn):
        out = {}
        for name, methods, n in variants:
            if methods is None:
                fn, hook = (lambda: single(None)), L.sg_debug_analyze_kernel_ms
            else:
                fn, hook = (lambda m=methods: batch_fn(m)), L.sg_debug_pitch_kernel_ms
            out[name] = timed(fn, hook, n, a.warmup, a.steps)
        return out

    last = {}
    res["batch"] = run_all(lambda _: last.update(r=AN.analyze_frames_batch(data, offs, lens, sr)),
                           lambda m: last.update(r=AN.pitch_candidates_batch(data, offs, lens, sr, pitchMethods=m)))
    r = last["r"]
    h = r["out"].cpu().numpy()[:sum(r["frames"]) * r["cols"]].reshape(-1, r["cols"])
    res["batch"]["frames"] = int(sum(r["frames"]))
    res["batch"]["tracked_frames"] = int(np.nansum(h[:, 14]))
    res["batch"]["frames_with_cep_candidate"] = int((~np.isnan(h[:, 17])).sum())
    res["batch"]["frames_with_spec_candidate"] = int((~np.isnan(h[:, 19])).sum())
    del r, last, h
    torch.cuda.empty_cache()
    host = data.cpu().numpy()
    idx = [i for i in range(a.calls) if lens[i] >= 2 * 2204][:16]
    n_long = int(a.seconds * sr)
    reps = 1 + n_long // max(1, int(sum(lens[i] for i in idx)))
    rec = np.concatenate([host[offs[i]:offs[i] + lens[i]] for i in idx] * reps)[:n_long].astype(np.float64)
    got = {}
    res["recording"] = run_all(lambda _: got.update(t=AN.analyze_frames(rec, sr)),
                               lambda m: got.update(t=AN.pitch_candidates(rec, sr, pitchMethods=m)))
    res["recording"].update(seconds=round(len(rec) / sr, 2), frames=int(len(got["t"]["ampl"])),
                            tracked_frames=int(got["t"]["cond_entropy"].sum()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
