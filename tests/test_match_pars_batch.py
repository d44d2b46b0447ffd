"""match_pars_batch() (soundgen_beta_amd/matchpars.py): the hill climb of many targets at once.
On the CPU the per-target stepper both drivers share, under a stub scorer; on the GPU the
equality of each target's result with match_pars() of that target alone."""
import math

import numpy as np
import pytest

from soundgen_beta_amd import matchpars as MP
from soundgen_beta_amd import rrng

PARS = ["sylLen", "pitchAnchors"]
SEEDS = (3, 4, 5, 6)
# what each stub target "sounds like": the climb moves sylLen and the mean pitch towards it
GOALS = ((420.0, 180.0), (150.0, 260.0), (300.0, 120.0), (520.0, 210.0))
REFUSED = 77.0  # a starting sylLen the stub planner refuses


def _stub_sim(k, p):
    """A deterministic similarity of candidate pars p to stub target k, in (0, 1]."""
    syl, f0 = GOALS[k]
    return 1.0 / (1.0 + abs(p["sylLen"] - syl) / 100 + abs(float(np.mean(p["pitchAnchors"]["value"])) - f0) / 50)


def _start(k, refused=()):
    return {"sylLen": REFUSED if k in refused else 300.0,
            "pitchAnchors": {"time": [0, .5, 1], "value": [150.0, 170.0 + 5 * k, 140.0]}, "samplingRate": 16000}


def _climb(k, pop, maxIter, refused=()):
    return MP._Climb(PARS, _start(k, refused), rrng.RRng(SEEDS[k]), .25, .1, maxIter, .001, pop)


def _single(k, pop, maxIter, refused=()):
    def score(plist):
        return [_stub_sim(k, p) for p in plist], [-1 if p["sylLen"] == REFUSED else 100 for p in plist]
    return MP._climb_single(_climb(k, pop, maxIter, refused), score)


def _batched(pop, maxIter, refused=()):
    last = {}
    gen = [0]

    def score(items):
        gen[0] += 1
        ks = [k for k, _ in items]
        assert ks == sorted(ks)  # a target's mutants stay together, in target order
        for k in set(ks):
            assert ks.count(k) == (1 if gen[0] == 1 else pop)
            last[k] = gen[0]
        return [_stub_sim(k, p) for k, p in items], [-1 if p["sylLen"] == REFUSED else 100 for _, p in items]
    return MP._climb_batch([_climb(k, pop, maxIter, refused) for k in range(4)], score), last


@pytest.mark.parametrize("pop", [1, 3])
def test_stepper_batched_equals_single(pop):
    """Four targets with their own R streams under a stub scorer: the batched driver gives each
    target exactly the history, pars, sims and `evaluated` of the single driver with that seed,
    and the targets leave the active set in different generations."""
    maxIter = 7
    res, last = _batched(pop, maxIter)
    for k in range(4):
        want = _single(k, pop, maxIter)
        got = res[k]
        assert got["evaluated"] == want["evaluated"]
        assert len(got["history"]) == len(want["history"])
        for a, b in zip(got["history"], want["history"]):
            assert a["pars"] == b["pars"] and a["sim"] == b["sim"]
        assert got["pars"] == want["pars"]
        # the counter's rule: a generation costs pop candidates, the start one
        assert (got["evaluated"] - 1) % pop == 0
    assert len(set(last.values())) > 1, last  # the targets finished in different generations
    assert any(len(r["history"]) > 1 for r in res)  # and the climb did climb


def test_stepper_refused_start_gives_none():
    """A target whose starting call the (stub) planner refuses gets None; the single driver raises
    for it; the other targets' results are what they are without it."""
    res, _ = _batched(1, 5, refused=(2,))
    ref, _ = _batched(1, 5)
    assert res[2] is None and ref[2] is not None
    with pytest.raises(ValueError, match="Invalid initial pars"):
        _single(2, 1, 5, refused=(2,))
    for k in (0, 1, 3):
        assert res[k]["evaluated"] == ref[k]["evaluated"] and res[k]["pars"] == ref[k]["pars"]
        assert [h["sim"] for h in res[k]["history"]] == [h["sim"] for h in ref[k]["history"]]


def _targets(sr):
    from soundgen_beta_amd import api
    spec = ((220, [150, 220], "a"), (310, [240, 180], "i"), (390, [120, 160], "o"))
    # float32-representable samples: the analysis of match_pars_init_batch() reads float32
    return [np.float32(api.soundgen(sylLen=s, pitchAnchors={"time": [0, 1], "value": v}, formants=f, temperature=0,
                                    samplingRate=sr, addSilence=0)).astype(np.float64) for s, v, f in spec]


@pytest.mark.gpu
@pytest.mark.parametrize("temp0,pop", [(True, 3), (False, 1)])
def test_match_pars_batch_equals_match_pars(temp0, pop):
    """Three targets climbed at once equal three match_pars() runs with the same seeds: history
    length, pars (deep), `evaluated`, and the similarities bit for bit. Without temperature 0
    soundgen() itself draws from each target's stream inside the shared plan."""
    sr = 16000
    targets = _targets(sr)
    assert all(0.2 * sr <= len(t) <= 0.4 * sr for t in targets)
    init = {"sylLen": 300, "pitchAnchors": {"time": [0, 1], "value": [130, 190]}, "addSilence": 0}
    if temp0:
        init["temperature"] = 0
    seeds = (3, 4, 5)
    got = MP.match_pars_batch(targets, sr, PARS, init=init, maxIter=4, pop=pop,
                              rngs=[rrng.RRng(s) for s in seeds])
    assert len(got) == 3
    for k, s in enumerate(seeds):
        want = MP.match_pars(targets[k], sr, PARS, init=init, maxIter=4, pop=pop, rng=rrng.RRng(s))
        assert got[k]["evaluated"] == want["evaluated"]
        assert len(got[k]["history"]) == len(want["history"])
        for a, b in zip(got[k]["history"], want["history"]):
            assert a["pars"] == b["pars"]
            assert a["sim"] == b["sim"] and math.isfinite(a["sim"]), (k, a["sim"], b["sim"])
        assert got[k]["pars"] == want["pars"]


@pytest.mark.gpu
def test_match_pars_batch_analyze_target():
    """analyzeTarget=True, maxIter=1 and no pars ("match pars based on acoustic analysis alone"):
    each target's pars equal match_pars(..., analyzeTarget=True) of that target alone."""
    sr = 16000
    targets = _targets(sr)
    got = MP.match_pars_batch(targets, sr, [], maxIter=1, analyzeTarget=True)
    for k, t in enumerate(targets):
        want = MP.match_pars(t, sr, [], maxIter=1, analyzeTarget=True)
        assert got[k] is not None and got[k]["pars"] == want["pars"], k
        assert got[k]["evaluated"] == want["evaluated"] == 1
        assert got[k]["history"][0]["sim"] == want["history"][0]["sim"]
