"""Regenerate tests/golden/*.npz — restatement-derived golden vectors.

R is absent from the build container, so these vectors come
from the C oracle (oracle/sg_oracle.c, itself checked against the NumPy twin in
tests/test_oracle.py); they pin the HIP path and guard the oracle against
regressions. tools/r_golden.R writes the same cases from real R where R exists.

    python tests/golden/make_golden.py

compare_sounds_one_target.npz is of another kind: values the GPU library itself returned at an
earlier commit (see compare_sounds_one_target below); rerunning its recorder today records
today's library, so the committed file is not to be regenerated.

    python tests/golden/make_golden.py compare_sounds_one_target [FILE]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import oracle as O  # noqa: E402

rng = np.random.default_rng(20261015)
NORMALS = rng.standard_normal(4000)

CASES = {
    # R/source.R:167-172: pitch = getSmoothContour(200 -> 300, len = 3500), samplingRate = 16000
    "roxygen_harmonics": (np.linspace(0, 1, 3500) * 100 + 200, dict(samplingRate=16000), None),
    "tone_150_16k": (np.full(1750, 150.0), dict(samplingRate=16000, rolloff=-12, rolloffOct=-12, pitchFloor=50), None),
    "subharm_16k": (np.full(3500, 320.0), dict(samplingRate=16000, nonlinBalance=100, subFreq=110, subDep=90,
                                              jitterDep=1, shimmerDep=10), NORMALS),
}


def main():
    out = {}
    for name, (pitch, params, normals) in CASES.items():
        y = O.generate_harmonics(pitch, normals=normals, **params)
        out[name + "__pitch"] = pitch
        out[name + "__y"] = y
        out[name + "__params"] = np.array(repr(params))
        if normals is not None:
            out[name + "__normals"] = normals
    np.savez_compressed(os.path.join(HERE, "harmonics_golden.npz"), **out)
    print("wrote", len(CASES), "cases")


def compare_sounds_one_target(path=None):
    """compare_sounds_batch() over the world of tests/test_compare_pairs.py (needs the GPU):
    windowLength 10, 13, 40 x penalizeLengthDif x the three targets x the seven candidate slots,
    out[wl, penalize, target, slot, method] and summary[wl, penalize, target, slot]. Recorded at
    the commit before sg_compare_sounds_batch and sg_compare_sounds_pairs came to share their
    kernels (there the one-target entry had its own kernel and reduced on the host), so the
    test that reads it holds the shared path to what both entries returned then."""
    sys.path.insert(0, os.path.dirname(HERE))
    import test_compare_pairs as W
    from soundgen_beta_amd import matchpars as MP
    from soundgen_beta_amd.native import SoundgenError

    world = W._World()
    out = np.full((len(W.WLS), 2, 3, 7, 4), -7.0)
    summ = np.full((len(W.WLS), 2, 3, 7), -7.0)
    raised = np.zeros((len(W.WLS), 2, 3), dtype=bool)  # the entry refused this target
    for a, wl in enumerate(W.WLS):
        for b, penalize in enumerate((False, True)):
            for t in range(3):
                try:
                    per, s = MP.compare_sounds_batch(world.spec("t", t, wl), world.cdata, world.coffs, world.clens,
                                                     W.SR, windowLength=wl, penalizeLengthDif=penalize)
                except SoundgenError:
                    raised[a, b, t] = True
                    continue
                out[a, b, t] = np.stack([per[m] for m in W.M], axis=1)
                summ[a, b, t] = s
    path = path or os.path.join(HERE, "compare_sounds_one_target.npz")
    np.savez_compressed(path, wls=np.array(W.WLS), out=out, summary=summ, raised=raised)
    print("wrote", path, out.size + summ.size, "doubles")


if __name__ == "__main__":
    if sys.argv[1:2] == ["compare_sounds_one_target"]:
        compare_sounds_one_target(*sys.argv[2:3])
    else:
        main()
