"""CPU: bench.py --dump-outputs. dump_outputs() writes a seeded sample of an output buffer:
float32/float64 .npy files, the same for the same arguments, read only from the calls'
own samples (never from the padding between them), under the size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _buffer(n_calls, max_len, dtype):
    rng = np.random.default_rng(7)
    lens = rng.integers(1, max_len, n_calls)
    lens[::7] = 0  # calls that were not synthesized
    pad = (lens + 63) // 64 * 64
    offs = np.cumsum(pad) - pad
    buf = np.full(int(offs[-1] + pad[-1]) + 64, np.nan, dtype)  # NaN wherever no call's sample lies
    for o, n in zip(offs, lens):
        buf[o:o + n] = (np.arange(n) + o) % 1021
    return buf, offs, lens


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_a_fixed_sample_of_the_calls_samples(tmp_path):
    buf, offs, lens = _buffer(3000, 50000, np.float32)  # 75 M samples: more than the waveform budget
    ids = np.arange(3000) + 5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), lambda pos: buf[pos], 4, offs, lens, ids)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["lengths", "point_index", "points", "waveform_calls", "waveforms"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["lengths"], lens)
    w, k = a["waveforms"], 0
    assert w.dtype == np.float32 and bench.DUMP_WAVE_BYTES // 4 - 50000 < len(w) <= bench.DUMP_WAVE_BYTES // 4
    for i, n in a["waveform_calls"].astype(np.int64):
        assert n == lens[i - 5] > 0
        assert np.array_equal(w[k:k + n], buf[offs[i - 5]:offs[i - 5] + n])
        k += n
    assert k == len(w)
    cat = np.concatenate([buf[o:o + n] for o, n in zip(offs, lens)])
    assert len(a["points"]) == bench.DUMP_POINTS
    assert np.array_equal(cat[a["point_index"].astype(np.int64)], a["points"])


def test_dump_of_a_small_float64_output_is_whole(tmp_path):
    buf, offs, lens = _buffer(20, 300, np.float64)
    bench.dump_outputs(str(tmp_path), lambda pos: buf[pos], 8, offs, lens, np.arange(20), ".rank1")
    a = _load(tmp_path)
    assert sorted(a) == [k + ".rank1" for k in ("lengths", "point_index", "points", "waveform_calls", "waveforms")]
    assert a["waveforms.rank1"].dtype == np.float64
    assert np.array_equal(a["waveforms.rank1"], np.concatenate([buf[o:o + n] for o, n in zip(offs, lens)]))
    assert np.array_equal(a["waveform_calls.rank1"][:, 0], np.nonzero(lens)[0])
