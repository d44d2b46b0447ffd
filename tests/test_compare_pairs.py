"""Mel spectra resident in HBM (matchpars.MelSet, sg_mel_set_*) and compareSounds() over a list
of (target, candidate) pairs of them (compare_sounds_pairs, compare_sounds_matrix: sg_mel_pair,
sg_mel_pair_reduce), against the one-target entry sg_compare_sounds_batch bit for bit, both
entries against the values recorded before they came to share those kernels, and against the
numpy restatement at its own bars."""
import math
import os

import numpy as np
import pytest

from soundgen_beta_amd import _abi
from soundgen_beta_amd import matchpars as MP
from soundgen_beta_amd.native import SoundgenError

pytestmark = pytest.mark.gpu

SR = 16000
WLS = (10, 13, 40)  # nb = 50, 65, 200: fewer bands than lanes, one band past a wave, the default
FAILED = 3          # the candidate slot with lengths = -1
M = ("cor", "cosine", "pixel", "dtw")


def _calls(n, seed):
    rng = np.random.default_rng(seed)
    calls = []
    for _ in range(n):
        f0 = float(np.exp(rng.uniform(np.log(90), np.log(500))))
        calls.append({"kind": "soundgen", "args": {
            "sylLen": float(rng.uniform(150, 500)), "samplingRate": SR, "temperature": 0, "addSilence": 0,
            "pitchAnchors": {"time": [0, 1], "value": [f0, f0 * float(rng.uniform(0.7, 1.5))]},
            "formants": str(rng.choice(list("aoieu"))), "rolloff": float(rng.uniform(-18, -6)),
            "noiseAnchors": {"time": [0, 300], "value": [float(rng.uniform(-40, -10))] * 2}},
            "uniforms": rng.uniform(size=200000)})
    return calls


class _World:
    """The sounds every test reads: computed once, never written."""

    def __init__(self):
        import torch
        from soundgen_beta_amd import api, batch
        data, offs, lens = batch.synthesize_packed(_calls(6, 5), 0)
        assert (lens > 0).all()
        # seven candidate slots: the six sounds and, at FAILED, a slot the planner "refused"
        self.cdata = data
        self.coffs = np.insert(offs, FAILED, 0)
        self.clens = np.insert(lens, FAILED, -1)
        host = data.cpu().numpy()
        self.cands = [None if n < 0 else host[o:o + n].astype(np.float64)
                      for o, n in zip(self.coffs, self.clens)]
        kw = dict(samplingRate=SR, temperature=0, addSilence=0, formants="ae")
        self.targets = [
            np.asarray(api.soundgen(sylLen=100, pitchAnchors={"time": [0, 1], "value": [150, 220]}, **kw), np.float64),
            np.asarray(api.soundgen(sylLen=700, pitchAnchors={"time": [0, 1], "value": [260, 140]}, **kw), np.float64),
            np.zeros(4000)]
        self.tlens = np.array([len(t) for t in self.targets], dtype=np.int64)
        self.toffs = np.concatenate([[0], np.cumsum(self.tlens)[:-1]]).astype(np.int64)
        self.tdata = torch.from_numpy(np.concatenate(self.targets)).to("cuda:0")
        self._sets, self._spec = {}, {}

    def sets(self, wl):
        """(float64 set of the targets, float32 set of the candidate slots) at windowLength wl."""
        if wl not in self._sets:
            self._sets[wl] = (MP.MelSet(self.tdata, self.toffs, self.tlens, SR, windowLength=wl),
                              MP.MelSet(self.cdata, self.coffs, self.clens, SR, windowLength=wl))
        return self._sets[wl]

    def spec(self, kind, i, wl):
        """get_mel_spec_gpu() of target / candidate i (the candidate's float32 samples widened)."""
        key = (kind, i, wl)
        if key not in self._spec:
            y = self.targets[i] if kind == "t" else self.cands[i]
            self._spec[key] = MP.get_mel_spec_gpu(y, SR, windowLength=wl)
        return self._spec[key]


@pytest.fixture(scope="module")
def world():
    w = _World()
    yield w
    for a, b in w._sets.values():
        a.close()
        b.close()


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("wl", WLS)
def test_mel_set_spec_equals_single_sound(world, wl):
    """MelSet.spec(i) is get_mel_spec_gpu() of sound i bit for bit (a float64 set; a float32 set:
    of the float32 samples widened), with its shape, and within 1e-9 of the numpy get_mel_spec."""
    tset, cset = world.sets(wl)
    nb = int(100 * wl / 20)
    assert (tset.n, tset.nb, cset.n, cset.nb) == (3, nb, 7, nb)
    for kind, S, sounds in (("t", tset, world.targets), ("c", cset, world.cands)):
        for i, y in enumerate(sounds):
            got = S.spec(i)
            assert got.shape == (nb, S.ncols[i])
            if y is None:
                assert S.ncols[i] == 0
                continue
            ref = world.spec(kind, i, wl)
            assert got.shape == ref.shape and np.array_equal(got, ref), (kind, i)
            want = MP.get_mel_spec(y, SR, windowLength=wl)
            assert got.shape == want.shape, (kind, i)
            if want.size:
                np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    assert tset.ncols[2] == 0 and tset.ncols[0] > 0  # the silent target keeps no column


@pytest.mark.parametrize("wl", WLS)
@pytest.mark.parametrize("penalize", [True, False])
def test_pairs_equal_one_target_entry(world, wl, penalize):
    """Every (target, candidate slot) pair, one of them twice: bit-equal to
    compare_sounds_batch(get_mel_spec_gpu(target), ...) per method and in the summary, NaN for the
    failed slot, within 1e-6 of the numpy compare_sounds; and pairs inside one set (a self pair)."""
    tset, cset = world.sets(wl)
    pairs = [(t, c) for t in range(3) for c in range(7)] + [(1, 4)]
    per, summ = MP.compare_sounds_pairs(tset, cset, pairs, penalizeLengthDif=penalize)
    assert _same(summ[-1], summ[pairs.index((1, 4))]) and all(_same(per[m][-1], per[m][pairs.index((1, 4))]) for m in M)
    shorter = longer = False
    for t in range(3):
        tspec = world.spec("t", t, wl)
        try:
            rper, rsumm = MP.compare_sounds_batch(tspec, world.cdata, world.coffs, world.clens, SR, windowLength=wl,
                                                  penalizeLengthDif=penalize)
        except SoundgenError:  # the one-target entry refuses an nb x 0 target: NaN throughout
            assert tspec.shape[1] == 0
            rper, rsumm = {m: np.full(7, np.nan) for m in M}, np.full(7, np.nan)
        tnp = MP.get_mel_spec(world.targets[t], SR, windowLength=wl)
        for c in range(7):
            k = pairs.index((t, c))
            for m in M:
                assert _same(per[m][k], rper[m][c]), (t, c, m, per[m][k], rper[m][c])
            assert _same(summ[k], rsumm[c]), (t, c, summ[k], rsumm[c])
            if c == FAILED:
                assert all(math.isnan(per[m][k]) for m in M) and math.isnan(summ[k])
                continue
            want = MP.compare_sounds(None, tnp, world.cands[c], SR, windowLength=wl, summary=False,
                                     penalizeLengthDif=penalize)
            for m in M:
                assert (math.isnan(want[m]) and math.isnan(per[m][k])) or abs(per[m][k] - want[m]) <= 1e-6, \
                    (t, c, m, per[m][k], want[m])
            vals = [v for v in want.values() if not math.isnan(v)]
            if vals:
                assert abs(summ[k] - np.mean(vals)) <= 1e-6
            else:
                assert math.isnan(summ[k])
            if tset.ncols[t] > 0:
                shorter |= tset.ncols[t] < cset.ncols[c]
                longer |= tset.ncols[t] > cset.ncols[c]
    assert shorter and longer  # matchColumns' padding on the target's side and on the candidate's
    # pairs inside one set: a self pair, and one pair twice
    inner = [(0, 0), (1, 2), (5, 1), (1, 2)]
    per, summ = MP.compare_sounds_pairs(cset, cset, inner, penalizeLengthDif=penalize)
    for k, (t, c) in enumerate(inner):
        rper, rsumm = MP.compare_sounds_batch(world.spec("c", t, wl), world.cdata, world.coffs, world.clens, SR,
                                              windowLength=wl, penalizeLengthDif=penalize)
        assert all(_same(per[m][k], rper[m][c]) for m in M) and _same(summ[k], rsumm[c]), (t, c)


def test_both_entries_reproduce_the_recorded_one_target_values(world):
    """sg_compare_sounds_batch and sg_compare_sounds_pairs share their kernels, so the bit-for-bit
    assertions between them above compare one path with itself. This one anchors both to
    tests/golden/compare_sounds_one_target.npz: what compare_sounds_batch() returned for this
    world (every windowLength, both penalizeLengthDif, 3 targets x 7 slots, the silent target and
    the failed slot among them) at the commit before the fold, when the one-target entry had a
    kernel of its own and reduced on the host (make_golden.py compare_sounds_one_target; two
    recordings in separate processes gave identical files). Every value, bit for bit."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                              "compare_sounds_one_target.npz")) as z:
        gout, gsumm, raised, wls = z["out"], z["summary"], z["raised"], z["wls"]
    assert tuple(wls) == WLS and gout.shape == (3, 2, 3, 7, 4) and gsumm.shape == (3, 2, 3, 7)
    assert not raised.any()  # the entry refused no target then, the nb x 0 one included
    pairs = [(t, c) for t in range(3) for c in range(7)]
    for a, wl in enumerate(WLS):
        tset, cset = world.sets(wl)
        for b, penalize in enumerate((False, True)):
            for t in range(3):
                per, summ = MP.compare_sounds_batch(world.spec("t", t, wl), world.cdata, world.coffs, world.clens, SR,
                                                    windowLength=wl, penalizeLengthDif=penalize)
                got = np.stack([per[m] for m in M], axis=1)
                assert _same(got, gout[a, b, t]), (wl, penalize, t, got, gout[a, b, t])
                assert _same(summ, gsumm[a, b, t]), (wl, penalize, t, summ, gsumm[a, b, t])
            per, summ = MP.compare_sounds_pairs(tset, cset, pairs, penalizeLengthDif=penalize)
            got = np.stack([per[m] for m in M], axis=1).reshape(3, 7, 4)
            assert _same(got, gout[a, b]), (wl, penalize)
            assert _same(summ.reshape(3, 7), gsumm[a, b]), (wl, penalize)
    # what the fixture holds: numbers for every live pair of a voiced target, the silent target's
    # 0 / ncol = 0 (penalizeLengthDif) or NaN, and NaN for the failed slot
    live = [c for c in range(7) if c != FAILED]
    assert np.isfinite(gout[:, :, :2][:, :, :, live]).all() and np.isfinite(gsumm[:, :, :2][:, :, :, live]).all()
    assert (gout[:, 1, 2][:, live] == 0).all() and (gsumm[:, 1, 2][:, live] == 0).all()
    assert np.isnan(gout[:, 0, 2]).all() and np.isnan(gsumm[:, 0, 2]).all()
    assert np.isnan(gout[:, :, :, FAILED]).all() and np.isnan(gsumm[:, :, :, FAILED]).all()


def test_mel_spec_of_a_sound_within_one_window(world):
    """get_mel_spec_gpu() (mel_spec_device) and MelSet.spec() copy a spectrum out through one
    helper: the two voiced targets at windowLength 13 agree bit for bit, and a sound of exactly
    one window (208 samples) and a shorter one (150), one frame each, are within 1e-9 of the
    numpy get_mel_spec through either."""
    import torch
    wl = 13
    tset, _ = world.sets(wl)
    for i in (0, 1):
        assert np.array_equal(tset.spec(i), world.spec("t", i, wl)), i
    winpts = 208  # round(0.013 * 16000)
    shorts = [world.targets[1][2000:2000 + winpts], world.targets[1][2000:2150]]
    lens = np.array([len(y) for y in shorts], dtype=np.int64)
    offs = np.array([0, winpts], dtype=np.int64)
    with MP.MelSet(torch.from_numpy(np.concatenate(shorts)).to("cuda:0"), offs, lens, SR, windowLength=wl) as S:
        for i, y in enumerate(shorts):
            want = MP.get_mel_spec(y, SR, windowLength=wl)
            got = MP.get_mel_spec_gpu(y, SR, windowLength=wl)
            assert want.shape == (65, 1) and got.shape == want.shape, (i, got.shape, want.shape)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
            assert np.array_equal(S.spec(i), got), i


def test_pair_is_independent_of_the_call(world):
    """A pair's five numbers are the same bits alone, in another order, and with the candidate set
    built from a superset of sounds laid out differently."""
    import torch
    tset, cset = world.sets(40)
    pairs = [(t, c) for t in range(3) for c in range(7)]
    per, summ = MP.compare_sounds_pairs(tset, cset, pairs)
    rev = pairs[::-1]
    rper, rsumm = MP.compare_sounds_pairs(tset, cset, rev)
    assert _same(rsumm[::-1], summ) and all(_same(rper[m][::-1], per[m]) for m in M)
    k = pairs.index((1, 4))
    aper, asumm = MP.compare_sounds_pairs(tset, cset, [(1, 4)])
    assert _same(asumm[0], summ[k]) and all(_same(aper[m][0], per[m][k]) for m in M)
    # a superset: two other sounds in front, the candidate slots behind them in reverse order
    extra = torch.from_numpy(np.concatenate([np.float32(world.targets[1]), np.float32(world.targets[0])])).to("cuda:0")
    e = extra.numel()
    data = torch.cat([extra, world.cdata])
    offs = np.concatenate([[0, len(world.targets[1])], (world.coffs + e)[::-1]])
    lens = np.concatenate([[len(world.targets[1]), len(world.targets[0])], world.clens[::-1]])
    with MP.MelSet(data, offs, lens, SR) as big:
        assert big.n == 9
        bper, bsumm = MP.compare_sounds_pairs(tset, big, [(t, 2 + 6 - c) for t, c in pairs])
    assert _same(bsumm, summ) and all(_same(bper[m], per[m]) for m in M)


def test_mirror_and_matrix(world):
    """Five sounds of differing lengths in one set: pair (i, j) and pair (j, i) are bit-equal,
    compare_sounds_matrix() (one triangle, mirrored) equals the full n x n pair call, and a
    non-silent sound's similarity to itself is exactly 1 by every method."""
    import torch
    sounds = [world.targets[0], world.targets[1], world.targets[2], world.cands[0], world.cands[1]]
    lens = np.array([len(s) for s in sounds], dtype=np.int64)
    assert len(set(lens)) == 5
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    data = torch.from_numpy(np.concatenate(sounds)).to("cuda:0")
    n = 5
    full = [(i, j) for i in range(n) for j in range(n)]
    with MP.MelSet(data, offs, lens, SR) as S:
        per, summ = MP.compare_sounds_pairs(S, S, full)
        msumm, mper = MP.compare_sounds_matrix(S)
    F = summ.reshape(n, n)
    assert _same(F, F.T)
    assert _same(msumm, F)
    for m in M:
        P = per[m].reshape(n, n)
        assert _same(P, P.T), m
        assert _same(mper[m], P), m
        assert all(P[i, i] == 1.0 for i in (0, 1, 3, 4)), (m, np.diag(P))
    assert all(F[i, i] == 1.0 for i in (0, 1, 3, 4))
    assert np.isfinite(F[np.ix_((0, 1, 3, 4), (0, 1, 3, 4))]).all()
    # the tuple form builds (and frees) its own set
    tsumm, _ = MP.compare_sounds_matrix((data, offs, lens, SR))
    assert _same(tsumm, F)


def test_refusals(world):
    """Sets of different windowLength, an index of -1 and an index of n: SG_E_ARG with `out`
    untouched; no pairs: empty arrays."""
    tset, cset = world.sets(40)
    other, _ = world.sets(13)
    for T, Cs, pairs in ((other, cset, [(0, 0)]), (tset, cset, [(0, 0), (-1, 0)]), (tset, cset, [(0, 7)]),
                         (tset, cset, [(3, 0)])):
        out = np.full((len(pairs), 4), -7.0)
        with pytest.raises(SoundgenError) as e:
            MP.compare_sounds_pairs(T, Cs, pairs, out=out)
        assert e.value.code == _abi.SG_E_ARG
        assert (out == -7.0).all()
    per, summ = MP.compare_sounds_pairs(tset, cset, [])
    assert summ.shape == (0,) and all(per[m].shape == (0,) for m in M)
