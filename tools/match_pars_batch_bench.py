#!/usr/bin/env python3
"""Times the hill climb of many targets at once (soundgen_beta_amd/matchpars.py match_pars_batch)
and the pairwise similarity matrix of a folder of sounds (compare_sounds_matrix; sg_mel_pair and
sg_mel_pair_reduce in sg_mel.hip) against the loops they replace, and prints one JSON line.
Arms, --targets synthesized targets at 16 kHz, pars sylLen and pitchAnchors, maxIter 10, pop 1,
target k on its own R stream RRng(k + 1):
  * loop          one match_pars() per target;
  * batch         one match_pars_batch() (its results are checked against the loop's once).
Arms, the --calls C5 preset calls of bench.py already in HBM (44.1 kHz):
  * matrix_loop   per sound get_mel_spec_gpu() of it and one compare_sounds_batch() against all;
  * matrix        compare_sounds_matrix() on the packed batch.
After --warmup runs of each arm, --steps runs of each in turn with profiling off, every run on
record; then --steps profiled runs of the pair call of `matrix` and of one generation's worth of
pairs (--targets pairs) record the device time of the two kernels (sg_debug_mel_pair_kernel_ms).
--loop-only times the loop arms alone, which use only what the parent commit has: run from a
checkout of the parent commit that is the parent's figure, and --parent FILE merges such a run's
JSON into this one's, adds the ratios and checks the condition (batch and matrix: the median wall
at most the parent loop's maximum).

    python tools/match_pars_batch_bench.py --out profiles/match_pars_batch_bench.json
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

PARS = ["sylLen", "pitchAnchors"]


def target_calls(n, sr, seed=11):
    rng = np.random.default_rng(seed)
    calls = []
    for _ in range(n):
        f0 = float(np.exp(rng.uniform(np.log(90), np.log(400))))
        calls.append({"kind": "soundgen", "args": {
            "sylLen": float(rng.uniform(150, 600)), "samplingRate": sr, "temperature": 0, "addSilence": 0,
            "pitchAnchors": {"time": [0, 1], "value": [f0, f0 * float(rng.uniform(0.7, 1.5))]},
            "formants": str(rng.choice(list("aoieu")))}})
    return calls


def mmm(v):
    v = sorted(v)
    return [round(v[0], 5), round(float(np.median(v)), 5), round(v[-1], 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--calls", type=int, default=260)
    ap.add_argument("--maxIter", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "match_pars_batch_bench needs a GPU"
    import bench
    from soundgen_beta_amd import batch, native
    from soundgen_beta_amd import matchpars as MP
    from soundgen_beta_amd.rrng import RRng

    sr = 16000
    targets = [np.asarray(y, dtype=np.float64) for y in batch.synthesize(target_calls(a.targets, sr), 0)]
    sr2 = 44100
    data, offs, lens = batch.synthesize_packed(bench.c5_calls(a.calls), 0)
    assert (lens > 0).all()
    host = data.cpu().numpy()
    sounds = [host[o:o + n].astype(np.float64) for o, n in zip(offs, lens)]
    L = native.lib()
    ctx = native.default_context(0)
    res = {"tool": "match_pars_batch_bench", "targets": a.targets, "maxIter": a.maxIter, "pop": 1, "calls": a.calls,
           "matrix_samples": int(lens[lens > 0].sum()), "steps": a.steps, "warmup": a.warmup,
           "tree": os.path.relpath(ROOT, os.getcwd())}
    last = {}

    def loop():
        last["loop"] = [MP.match_pars(t, sr, PARS, maxIter=a.maxIter, rng=RRng(k + 1)) for k, t in enumerate(targets)]

    def batched():
        last["batch"] = MP.match_pars_batch(targets, sr, PARS, maxIter=a.maxIter,
                                            rngs=[RRng(k + 1) for k in range(len(targets))])

    def matrix_loop():
        rows = []
        for y in sounds:
            _, summ = MP.compare_sounds_batch(MP.get_mel_spec_gpu(y, sr2), data, offs, lens, sr2)
            rows.append(summ)
        last["matrix_loop"] = np.array(rows)

    def matrix():
        last["matrix"] = MP.compare_sounds_matrix((data, offs, lens, sr2))[0]

    arms = {"loop": loop, "matrix_loop": matrix_loop}
    if not a.loop_only:
        arms = {"loop": loop, "batch": batched, "matrix_loop": matrix_loop, "matrix": matrix}
    for f in arms.values():
        for _ in range(a.warmup):
            f()
    runs = {k: [] for k in arms}
    for _ in range(a.steps):
        for k, f in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            runs[k].append(round(time.perf_counter() - t0, 6))
    for k, v in runs.items():
        res[k] = {"wall_s": v, "wall_s_min_med_max": mmm(v)}
    res["evaluated"] = int(sum(r["evaluated"] for r in last["loop"]))
    if not a.loop_only:
        same = all(b is not None and b["evaluated"] == r["evaluated"] and b["pars"] == r["pars"] and
                   [h["sim"] for h in b["history"]] == [h["sim"] for h in r["history"]]
                   for b, r in zip(last["batch"], last["loop"]))
        res["batch_equals_loop"] = bool(same)
        res["matrix_equals_loop"] = bool(np.array_equal(last["matrix"], last["matrix_loop"], equal_nan=True))
        res["loop_over_batch_wall"] = round(res["loop"]["wall_s_min_med_max"][1] / res["batch"]["wall_s_min_med_max"][1], 2)
        res["matrix_loop_over_matrix_wall"] = round(res["matrix_loop"]["wall_s_min_med_max"][1] /
                                                    res["matrix"]["wall_s_min_med_max"][1], 2)
        # the two kernels' device time, in runs of their own: the stage clock's events stay out of the walls
        prof = {"matrix": [], "generation": []}
        with MP.MelSet(data, offs, lens, sr2) as S:
            iu, ju = np.triu_indices(S.n)
            tri = np.stack([iu, ju], axis=1)
            gen = np.stack([np.arange(a.targets) % S.n, (np.arange(a.targets) * 7 + 3) % S.n], axis=1)
            res["matrix_pairs"], res["matrix_columns_max"] = int(len(tri)), int(S.ncols.max())
            for name, pairs in (("matrix", tri), ("generation", gen)):
                for _ in range(a.steps):
                    L.sg_set_profiling(ctx.ptr, 1)
                    MP.compare_sounds_pairs(S, S, pairs)
                    L.sg_set_profiling(ctx.ptr, 0)
                    out = np.zeros(2)
                    L.sg_debug_mel_pair_kernel_ms(out.ctypes.data_as(C.POINTER(C.c_double)))
                    prof[name].append([round(float(out[0]), 4), round(float(out[1]), 4)])
        res["kernel_ms"] = {k: {"runs_pair_reduce": v,
                                "sg_mel_pair_min_med_max": mmm([r[0] for r in v]),
                                "sg_mel_pair_reduce_min_med_max": mmm([r[1] for r in v])} for k, v in prof.items()}
    if a.parent:
        with open(a.parent) as f:
            parent = json.loads(f.readline())
        assert (parent["targets"], parent["maxIter"], parent["calls"]) == (a.targets, a.maxIter, a.calls)
        res["conditions"] = {}
        for new, old in (("batch", "loop"), ("matrix", "matrix_loop")):
            res["parent_" + old] = parent[old]
            med = res[new]["wall_s_min_med_max"][1]
            res["parent_%s_over_%s_wall" % (old, new)] = round(parent[old]["wall_s_min_med_max"][1] / med, 2)
            res["conditions"][new] = bool(med <= parent[old]["wall_s_min_med_max"][2])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
