#!/usr/bin/env python3
"""Times findformants on whole sounds (soundgen_beta_amd/formants.py: find_formants_sounds_batch; sg_fmt_sound_* in
sg_formants.hip) and matchPars' starting point (matchpars.py: match_pars_init_batch) on the batch workload of
tools/formants_bench.py: --calls C5 preset calls already in HBM. After --warmup runs, --steps runs with profiling on
record the four stage times of sg_debug_formants_whole_kernel_ms and the capped / analysed / iteration counts, and
from the chunk-lag stage its achieved fp64 rate: 2 N (order + 1) floating-point operations per sound of N samples,
against the vector fp64 peak (half the 157.3 TFLOP/s fp32 vector peak). Then, profiling off, the wall time of
find_formants_sounds_batch on all sounds, and of match_pars_init_batch on the first --sample analysable sounds beside
as many single match_pars_init calls (alternating). Prints one JSON line.

    python tools/formants_whole_bench.py --out profiles/formants_whole_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 157.3e12 / 2
STAGES = ("mean", "chunk_lags", "fold", "roots")


def mmm(v):
    return [round(float(f(v)), 5) for f in (min, np.median, max)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=260)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "formants_whole_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, formants as FM, matchpars as MP, native

    sr = 44100
    data, offs, lens = batch.synthesize_packed(bench.c5_calls(a.calls), 0)
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    order, chunk, _ = FM.formants_whole_size(sr, 1)
    ok = lens > order
    samples = int(lens[ok].sum())
    chunks = int(sum(FM.formants_whole_size(sr, int(n))[2] for n in lens[ok]))
    flops = 2.0 * samples * (order + 1)
    res = {"tool": "formants_whole_bench", "calls": a.calls, "samplingRate": sr, "order": order, "chunk": chunk,
           "sounds_analysed": int(ok.sum()), "samples": samples, "chunks": chunks, "chunk_lag_flops": flops,
           "fp64_vector_peak_flops": FP64_VECTOR_PEAK, "steps": a.steps, "warmup": a.warmup}

    L = native.lib()
    ctx = native.default_context(0)
    L.sg_set_profiling(ctx.ptr, 1)
    prof = []
    for k in range(a.warmup + a.steps):
        FM.find_formants_sounds_batch(data, offs, lens, sr)
        ms, (capped, analysed, iters) = FM.formants_whole_profile()
        if k >= a.warmup:
            prof.append(dict({s: round(ms[s], 4) for s in STAGES}, capped=capped, analysed=analysed, iterations=iters))
    L.sg_set_profiling(ctx.ptr, 0)
    res["device"] = {"runs": prof, "stage_ms_min_med_max": {s: mmm([p[s] for p in prof]) for s in STAGES}}
    lag_ms = float(np.median([p["chunk_lags"] for p in prof]))
    res["chunk_lags_tflops"] = round(flops / (lag_ms * 1e-3) / 1e12, 3)
    res["chunk_lags_share_of_fp64_vector_peak"] = round(flops / (lag_ms * 1e-3) / FP64_VECTOR_PEAK, 4)
    res["capped"], res["analysed"] = prof[-1]["capped"], prof[-1]["analysed"]
    res["mean_aberth_iterations"] = round(prof[-1]["iterations"] / max(prof[-1]["analysed"], 1), 3)

    wall = []
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        FM.find_formants_sounds_batch(data, offs, lens, sr)  # returns when the stream has finished
        if k >= a.warmup:
            wall.append(time.perf_counter() - t0)
    res["find_formants_sounds_batch_wall_s_min_med_max"] = mmm(wall)
    print(json.dumps(res), file=sys.stderr)  # the kernels' part, should the rest fail

    # matchPars' starting point: one batch beside single calls on the same (float32-rounded) sounds, alternating
    sub = [i for i in range(a.calls) if lens[i] > sr // 10][:a.sample]
    so, sl = offs[sub], lens[sub]
    host = [data[int(o):int(o + n)].cpu().numpy().astype(np.float64) for o, n in zip(so, sl)]
    tb, ts = [], []
    for k in range(1 + 2):
        t0 = time.perf_counter()
        got = MP.match_pars_init_batch(data, so, sl, sr)
        t1 = time.perf_counter()
        single = []
        for x in host:
            try:
                single.append(MP.match_pars_init(x, sr))
            except ValueError:
                single.append(None)
        t2 = time.perf_counter()
        if k >= 1:
            tb.append(t1 - t0)
            ts.append(t2 - t1)
    res["match_pars_init"] = {"sounds": len(sub), "batch_wall_s_min_med_max": mmm(tb), "single_calls_wall_s_min_med_max": mmm(ts),
                              "single_over_batch": round(float(np.median(ts) / np.median(tb)), 2),
                              "entries_none": sum(g is None for g in got),
                              "entries_equal_single": sum(g == s for g, s in zip(got, single))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
