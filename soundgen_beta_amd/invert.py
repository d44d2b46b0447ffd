"""stft(), istft() and invert_spectrogram(): sound from a spectrogram.

spectrogram() leaves magnitude matrices; these three keep the phases, go back, and find a
sound for magnitudes that have none (Griffin & Lim 1984). No reference counterpart: the
operator pair is stated here once and restated twice, in numpy below and on the device
(csrc/sg_invert.h, csrc/sg_invert.hip). Everything is bound by spectrogram()'s arguments
and decisions (window length in points, zero padding, frame starts, window) and fp64.

    N = wl + 2 pad, M = N / 2, s_i = frame_starts(...)[i], w = ft_window(wl, wn)

  A    frame i is w[t] x[s_i + t], zero-padded as getFrameBank pads it; bins 0 .. M of its
       N-point DFT, unscaled as stats::fft gives them. That is M + 1 bins: the Nyquist bin is
       kept. spectrogram()'s matrix is the modulus of the first M.
  A+   the least-squares inverse: a frame's M + 1 bins extended Hermitian, the real part of
       the inverse DFT / N, the pad dropped, then
           x^[t] = sum_i w[t - s_i] y_i[t - s_i] / sum_i w[t - s_i]^2
       over the frames that cover t, added in frame order. A sample whose denominator is 0
       -- none covers it (a step longer than the window, the tail behind the last frame), or
       only zeros of the window do ('hanning''s ends) -- is 0, the minimum-norm choice. There
       is no other floor.
  invert_spectrogram: X_0 = S exp(i phi_0); nIter times x = A+ X, Z = A x, X = S Z / |Z| on the
       constrained bins (X = S where |Z| = 0); the result is A+ X. S has M rows
       (spectrogram()'s shape; the Nyquist bin is then unconstrained, starts at 0 and is
       carried through) or M + 1. Both are alternating projections between the range of A
       and the set of spectra with the prescribed magnitudes, so the error
           e_k = sqrt(sum (|A x_k| - S)^2 / sum S^2)   over the constrained bins
       cannot increase in exact arithmetic.

A matrix is rows x frames like spectrogram()'s; on the device it is kept frame after frame.
stft() normalises its input as getFrameBank does (spectrogram()'s own statistics), so
abs(stft(x))[:M] is spectrogram(x, output = 'original'); the iteration applies A without it:
the normalisation belongs to spectrogram()'s input, not to A. What comes back from istft()
and invert_spectrogram() is therefore in the domain of getFrameBank's normalised sound; the
original scale is not in a spectrogram. Any non-negative matrix is accepted as magnitudes
('processed' is not undone); a negative or NaN cell is refused.

The *_numpy restatements take dtype (np.float64 or np.longdouble): the same statements in
either precision, a direct DFT so that no library transform hides a format.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import native
from . import spectrogram as SP

_DEFAULTS = dict(windowLength=50, step=None, overlap=70, wn="gaussian", zp=0, smoothFreq=0, smoothTime=0, qTime=0,
                 percentNoise=10, noiseReduction=0, contrast=.2, brightness=0, method="spectrum", output="processed")


def _args(kw):
    bad = sorted(set(kw) - set(_DEFAULTS))
    if bad:
        raise TypeError("unexpected argument(s) %s: the arguments are spectrogram()'s" % ", ".join(bad))
    a = dict(_DEFAULTS)
    a.update(kw)
    return a


# ------------------------------------------------------------------ the restatement
def _geometry(samplingRate, a):
    step = SP._step(a["windowLength"], a["step"], a["overlap"])
    wl = int(math.floor(a["windowLength"] / 1000 * samplingRate / 2) * 2)
    zpExtra = int(math.floor((a["zp"] - wl) / 2) * 2)
    pad = zpExtra // 2 if zpExtra > 0 else 0
    return wl, pad, wl + 2 * pad, step


def _starts(length, samplingRate, wl, step):
    if length <= 1 or length < wl:
        return np.zeros(0, dtype=np.int64)
    return SP.frame_starts(length, samplingRate, wl, step)


def min_length(frames, samplingRate, **kw):
    """The shortest sound that spectrogram() cuts into `frames` frames."""
    wl, _, _, step = _geometry(samplingRate, _args(kw))
    if frames <= 0:
        return 0
    n = max(wl, 2, int(math.floor(1 + (frames - 1) * (step / 1000 * samplingRate))) + wl - 1)
    while len(_starts(n, samplingRate, wl, step)) < frames:
        n += 1
    return n


@functools.lru_cache(maxsize=4)
def _dft_rows(N, rows, dtype):
    """W[k, n] = exp(-2 pi i k n / N), k < rows, n < N, in dtype; the index reduced in
    integers, the quadrant points exact."""
    dtype = np.dtype(dtype).type
    cd = np.result_type(dtype, np.complex64)
    ang = (8 * np.arctan(dtype(1))) * np.arange(N).astype(dtype) / dtype(N)
    w = (np.cos(ang) - 1j * np.sin(ang)).astype(cd)
    for q, v in enumerate((1, -1j, -1, 1j)):
        if (q * N) % 4 == 0:
            w[q * N // 4] = v
    W = w[(np.arange(rows, dtype=np.int64)[:, None] * np.arange(N, dtype=np.int64)[None, :]) % N]
    W.setflags(write=False)
    return W


def _normalize(s, dtype):
    """getFrameBank's normalisation (SP.normalize_sound) in dtype."""
    s = np.asarray(s, dtype=dtype)
    if s.min() > 0:
        c = s - s.sum() / dtype(len(s))
        s = c / np.sqrt(np.sum(c * c) / dtype(len(s) - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / max(abs(s.max()), abs(s.min()))


def _analysis(x, starts, w, pad, N, rows, dtype):
    """A: frames x rows."""
    wl = len(w)
    bank = np.zeros((len(starts), N), dtype=dtype)
    for i, s in enumerate(starts):
        bank[i, pad:pad + wl] = w * x[s:s + wl]
    return bank @ _dft_rows(N, rows, dtype).T


def _synthesis(X, starts, w, pad, N, length, dtype):
    """A+: X is frames x rows, rows = N / 2 or N / 2 + 1."""
    M, wl = N // 2, len(w)
    c = np.full(X.shape[1], 2, dtype=dtype)
    c[0] = 1
    if X.shape[1] == M + 1:
        c[M] = 1
    # Re(X_0) + (-1)^n Re(X_M) + 2 sum_{0 < k < M} Re(X_k exp(+2 pi i k n / N)): the Hermitian extension's inverse
    y = ((X * c) @ np.conj(_dft_rows(N, X.shape[1], dtype))).real / dtype(N)
    num = np.zeros(length, dtype=dtype)
    den = np.zeros(length, dtype=dtype)
    for i, s in enumerate(starts):
        num[s:s + wl] += w * y[i, pad:pad + wl]
        den[s:s + wl] += w * w
    out = np.zeros(length, dtype=dtype)
    ok = den != 0
    out[ok] = num[ok] / den[ok]
    return out


def _setup(length, samplingRate, a, dtype):
    if a["wn"] not in SP.WINDOWS:
        raise ValueError("wn must be one of %s" % (SP.WINDOWS,))
    wl, pad, N, step = _geometry(samplingRate, a)
    return wl, pad, N, _starts(length, samplingRate, wl, step), SP.ft_window(wl, a["wn"]).astype(dtype)


def stft_numpy(x, samplingRate, nyquist=True, dtype=np.float64, **kw):
    """A of the sound x, normalised as getFrameBank does: (M + 1 or M) x frames, complex."""
    dtype = np.dtype(dtype).type
    a = _args(kw)
    x = np.asarray(x, dtype=np.float64).ravel()
    wl, pad, N, starts, w = _setup(len(x), samplingRate, a, dtype)
    if len(x) < wl:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    return _analysis(_normalize(x, dtype), starts, w, pad, N, N // 2 + (1 if nyquist else 0), dtype).T


def _rows_of(X, N):
    if X.ndim != 2 or X.shape[0] not in (N // 2, N // 2 + 1):
        raise ValueError("a spectrum of %d-point frames has %d or %d rows, not %s" % (N, N // 2, N // 2 + 1, X.shape[:1]))
    return X.shape[0]


def istft_numpy(X, samplingRate, length=None, dtype=np.float64, **kw):
    """A+ of the spectrum X (M or M + 1 rows x frames): `length` samples (default: the
    shortest sound with that many frames)."""
    dtype = np.dtype(dtype).type
    a = _args(kw)
    X = np.asarray(X)
    if length is None:
        length = min_length(X.shape[1], samplingRate, **kw)
    wl, pad, N, starts, w = _setup(length, samplingRate, a, dtype)
    _rows_of(X, N)
    if len(starts) != X.shape[1]:
        raise ValueError("a sound of %d samples has %d frames, the spectrum %d" % (length, len(starts), X.shape[1]))
    return _synthesis(X.T.astype(np.result_type(dtype, np.complex64)), starts, w, pad, N, length, dtype)


def invert_spectrogram_numpy(S, samplingRate, length=None, nIter=32, phase0=None, dtype=np.float64, details=False, **kw):
    """The iteration of the module docstring on the magnitudes S (M or M + 1 rows x
    frames): (sound, e_1 .. e_nIter). details=True adds the smallest constrained |Z| met,
    relative to the largest of its iteration (the conditioning of the projection)."""
    dtype = np.dtype(dtype).type
    cd = np.result_type(dtype, np.complex64)
    a = _args(kw)
    S = np.asarray(S, dtype=np.float64)
    if not np.all(S >= 0):
        raise ValueError("a magnitude is negative or NaN")
    if length is None:
        length = min_length(S.shape[1], samplingRate, **kw)
    wl, pad, N, starts, w = _setup(length, samplingRate, a, dtype)
    rows, M = _rows_of(S, N), N // 2
    if len(starts) != S.shape[1]:
        raise ValueError("a sound of %d samples has %d frames, the matrix %d" % (length, len(starts), S.shape[1]))
    St = S.T.astype(dtype)
    X = np.zeros((len(starts), M + 1), dtype=cd)
    if phase0 is None:
        X[:, :rows] = St
    else:
        ph = np.asarray(phase0, dtype=np.float64).T.astype(dtype)
        X[:, :rows] = St * np.cos(ph) + 1j * (St * np.sin(ph))
    e, worst = np.zeros(nIter, dtype=dtype), math.inf
    for k in range(nIter):
        x = _synthesis(X, starts, w, pad, N, length, dtype)
        Z = _analysis(x, starts, w, pad, N, M + 1, dtype)
        az = np.abs(Z[:, :rows])
        with np.errstate(invalid="ignore", divide="ignore"):
            e[k] = np.sqrt(np.sum((az - St) ** 2) / np.sum(St ** 2))
            if az.size:
                worst = min(worst, float(az.min() / az.max()))
            X = Z.copy()
            X[:, :rows] = np.where(az > 0, (St * Z[:, :rows]) / np.where(az > 0, az, 1), St)
    x = _synthesis(X, starts, w, pad, N, length, dtype)
    return (x, e, worst) if details else (x, e)


# ------------------------------------------------------------------ on the GPU (sg_invert.hip)
def _params(samplingRate, a):
    SP._settings(a["wn"], a["smoothFreq"], a["smoothTime"], a["method"], a["output"], False, False)
    return SP._params(samplingRate, a["windowLength"], a["step"], a["overlap"], a["wn"], a["zp"], a["smoothFreq"],
                      a["smoothTime"], a["qTime"], a["percentNoise"], a["noiseReduction"], a["contrast"], a["brightness"],
                      a["method"], a["output"])


def invert_size(length, samplingRate, rows=0, **kw):
    """sg_invert_size (host only): dict(wl, N, bins, frames, samples, workspace_bytes) for a sound
    of `length` samples; rows: 0, or a row count to validate. Raises SoundgenError with
    spectrogram()'s code and text for a frame length the device transform lacks."""
    return _size(native.lib(), _params(samplingRate, _args(kw)), length, rows)


def _size(L, P, length, rows=0):
    o = [C.c_int32() for _ in range(4)] + [C.c_int64(), C.c_int64()]
    rc = L.sg_invert_size(int(length), C.byref(P), int(rows), *[C.byref(v) for v in o])
    native.host_check(rc, L.sg_invert_size_error)
    return dict(zip(("wl", "N", "bins", "frames", "samples", "workspace_bytes"), (v.value for v in o)))


def _same_rows(shapes):
    rows = {int(r) for r, _ in shapes}
    if len(rows) > 1:
        raise ValueError("the matrices of a batch have one row count, not %s" % sorted(rows))
    return rows.pop() if rows else 0


def stft_batch(data, offsets, lengths, samplingRate, nyquist=True, to_host=False, device=0, **kw):
    """A of a batch of sounds already in HBM (`data`: a float32 or float64 CUDA tensor, call i
    at offsets[i], lengths[i] samples), each normalised as getFrameBank does
    (sg_spg_stft_batch). The spectra stay in HBM: (out, out_offsets, shapes) with `out` a
    complex128 CUDA tensor, call i's spectrum at out_offsets[i] as shapes[i] = (rows, frames),
    frame after frame. to_host=True returns the list of rows x frames arrays instead."""
    import torch
    L = native.lib()
    P = _params(samplingRate, _args(kw))
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    if data.dtype not in (torch.float32, torch.float64):
        raise TypeError("stft_batch: data must be float32 or float64")
    shapes = []
    for i in range(nc):
        z = _size(L, P, int(lens[i]))
        shapes.append((z["bins"] + (1 if nyquist else 0), z["frames"]))
    ooff, p_ooff = native.out_offsets([r * f for r, f in shapes])
    ctx = native.default_context(device)
    out = torch.empty(max(int(ooff[-1]), 1), dtype=torch.complex128, device=data.device)
    torch.cuda.synchronize(data.device)
    rows = shapes[0][0] if shapes else _size(L, P, 0)["bins"] + (1 if nyquist else 0)
    native.check(L.sg_spg_stft_batch(ctx.ptr, C.c_void_p(data.data_ptr()), int(data.dtype == torch.float64), p_offs, p_lens,
                                     nc, C.byref(P), rows, C.c_void_p(out.data_ptr()), p_ooff), ctx.ptr)
    if not to_host:
        return out, ooff[:-1].copy(), shapes
    h = out.cpu().numpy()
    return [h[ooff[i]:ooff[i + 1]].reshape(shapes[i][1], shapes[i][0]).T.copy() for i in range(nc)]


def _lengths(L, P, shapes, lengths, samplingRate, kw, offsets, cells):
    if lengths is None:
        lengths = [min_length(f, samplingRate, **kw) for _, f in shapes]
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
    if len(lens) != len(shapes):
        raise ValueError("one length per matrix")
    rows = _same_rows(shapes)
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if len(offs) != len(shapes):
        raise ValueError("one offset per matrix")
    for i, (_, f) in enumerate(shapes):
        z = _size(L, P, int(lens[i]), rows)
        if z["frames"] != f:
            raise ValueError("call %d: a sound of %d samples has %d frames, the matrix %d" % (i, lens[i], z["frames"], f))
        if offs[i] < 0 or offs[i] + rows * f > cells:
            raise ValueError("call %d: its matrix leaves the buffer" % i)
    return lens, rows, offs


def istft_batch(spec, spec_offsets, shapes, samplingRate, lengths=None, to_host=False, device=0, **kw):
    """A+ of a batch of spectra in HBM as stft_batch leaves them (sg_spg_istft_batch):
    (out, out_offsets) with `out` an fp64 CUDA tensor, call i's lengths[i] samples at
    out_offsets[i] (lengths=None: the shortest sounds with those frame counts)."""
    import torch
    L = native.lib()
    P = _params(samplingRate, _args(kw))
    if spec.dtype != torch.complex128:
        raise TypeError("istft_batch: spec must be complex128")
    lens, rows, soff = _lengths(L, P, shapes, lengths, samplingRate, kw, spec_offsets, spec.numel())
    nc = len(shapes)
    i64p = C.POINTER(C.c_int64)
    ooff, p_ooff = native.out_offsets(lens)
    ctx = native.default_context(device)
    out = native.device_out(spec, ooff[-1])
    if nc:
        native.check(L.sg_spg_istft_batch(ctx.ptr, C.c_void_p(spec.data_ptr()), soff.ctypes.data_as(i64p),
                                          lens.ctypes.data_as(i64p), nc, C.byref(P), rows, C.c_void_p(out.data_ptr()),
                                          p_ooff), ctx.ptr)
    if not to_host:
        return out, ooff[:-1].copy()
    h = out.cpu().numpy()
    return [h[ooff[i]:ooff[i + 1]].copy() for i in range(nc)]


def r_phases(rng, shapes):
    """runif(frames * rows, -pi, pi) per matrix from the project's R stream (rrng.RRng), drawn
    in column order (frame after frame): one flat array in the batch's layout."""
    n = int(sum(r * f for r, f in shapes))
    u = np.asarray(rng.random(n), dtype=np.float64) if n else np.zeros(0)
    return -math.pi + (math.pi - -math.pi) * u  # runif: a + (b - a) u


def invert_spectrogram_batch(mag, mag_offsets, shapes, samplingRate, lengths=None, nIter=32, phase0=None, rng=None,
                             workspace_cap=0, to_host=False, device=0, **kw):
    """invert_spectrogram of a batch of magnitude matrices in HBM, as spectrogram_batch
    leaves them: its (out, out_offsets, shapes) are this function's first three arguments
    (sg_invert_spectrogram_batch). phase0: an fp64 CUDA tensor of initial phases in mag's
    layout (same offsets), or None for zero; rng (rrng.RRng) draws them instead
    (r_phases). Returns (out, out_offsets, errors): `out` an fp64 CUDA tensor with call i's
    lengths[i] samples at out_offsets[i], errors an nc x nIter array of e_k. workspace_cap: bytes
    a chunk of the batch may take (0: 1 GiB)."""
    import torch
    L = native.lib()
    P = _params(samplingRate, _args(kw))
    if mag.dtype != torch.float64:
        raise TypeError("invert_spectrogram_batch: mag must be float64")
    if nIter < 0:
        raise ValueError("nIter must be >= 0")
    lens, rows, moff = _lengths(L, P, shapes, lengths, samplingRate, kw, mag_offsets, mag.numel())
    nc = len(shapes)
    i64p = C.POINTER(C.c_int64)
    if phase0 is not None and rng is not None:
        raise ValueError("phase0 or rng, not both")
    if rng is not None:
        flat = np.zeros(int(mag.numel()))
        ph = r_phases(rng, shapes)
        k = 0
        for i, (r, f) in enumerate(shapes):
            flat[moff[i]:moff[i] + r * f] = ph[k:k + r * f]
            k += r * f
        phase0 = torch.from_numpy(flat).to(mag.device)
    if phase0 is not None and (phase0.dtype != torch.float64 or phase0.numel() < mag.numel()):
        raise TypeError("invert_spectrogram_batch: phase0 must be float64 in mag's layout")
    ooff, p_ooff = native.out_offsets(lens)
    ctx = native.default_context(device)
    out = native.device_out(mag, ooff[-1])
    err = np.full((nc, nIter), math.nan)
    if nc:
        native.check(L.sg_invert_spectrogram_batch(
            ctx.ptr, C.c_void_p(mag.data_ptr()), moff.ctypes.data_as(i64p),
            C.c_void_p(phase0.data_ptr()) if phase0 is not None else None, lens.ctypes.data_as(i64p), nc, C.byref(P), rows,
            int(nIter), int(workspace_cap), C.c_void_p(out.data_ptr()), p_ooff,
            err.ctypes.data_as(C.POINTER(C.c_double)) if nIter else None), ctx.ptr)
    if not to_host:
        return out, ooff[:-1].copy(), err
    h = out.cpu().numpy()
    return [h[ooff[i]:ooff[i + 1]].copy() for i in range(nc)], err


# ------------------------------------------------------------------ one sound from the host
def _device(device):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("stft / istft / invert_spectrogram run on the GPU; none is available")
    return torch.device("cuda", device)


def stft(x, samplingRate=None, nyquist=True, device=0, **kw):
    """A of one sound (a numeric vector with samplingRate, or the path of a mono 16-bit PCM
    file), normalised as getFrameBank does, on the GPU: (M + 1 or M) x frames, complex."""
    import torch
    s, sr = SP._input(x, samplingRate)
    P = _params(sr, _args(kw))  # the refusals, before any launch
    if len(s) < _size(native.lib(), P, len(s))["wl"]:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    d = torch.from_numpy(np.array(s, dtype=np.float64)).to(_device(device))
    return stft_batch(d, [0], [len(s)], sr, nyquist=nyquist, to_host=True, device=device, **kw)[0]


def istft(X, samplingRate, length=None, device=0, **kw):
    """A+ of one spectrum (M or M + 1 rows x frames) on the GPU: `length` samples (default:
    the shortest sound with that many frames), in the domain of the normalised sound."""
    import torch
    X = np.asarray(X, dtype=np.complex128)
    if X.ndim != 2:
        raise ValueError("istft: X is rows x frames")
    shapes = [X.shape]
    lens, _, _ = _lengths(native.lib(), _params(samplingRate, _args(kw)), shapes, None if length is None else [length],
                          samplingRate, kw, [0], X.size)
    d = torch.from_numpy(np.array(X.T).ravel()).to(_device(device))
    return istft_batch(d, [0], shapes, samplingRate, lengths=lens, to_host=True, device=device, **kw)[0]


def invert_spectrogram(S, samplingRate, length=None, nIter=32, phase0=None, rng=None, return_error=False, device=0, **kw):
    """A sound whose spectrogram(output = 'original') approaches S (M or M + 1 rows x frames,
    non-negative), by nIter alternating projections from the phases phase0 (an array shaped
    like S, or None for zero) or from rng's runif(frames * rows, -pi, pi). return_error=True:
    (sound, e_1 .. e_nIter)."""
    import torch
    S = np.asarray(S, dtype=np.float64)
    if S.ndim != 2:
        raise ValueError("invert_spectrogram: S is rows x frames")
    shapes = [S.shape]
    lens, _, _ = _lengths(native.lib(), _params(samplingRate, _args(kw)), shapes, None if length is None else [length],
                          samplingRate, kw, [0], S.size)
    dev = _device(device)
    d = torch.from_numpy(np.array(S.T).ravel()).to(dev)
    if phase0 is not None:
        phase0 = np.asarray(phase0, dtype=np.float64)
        if phase0.shape != S.shape:
            raise ValueError("phase0 is shaped like S")
        phase0 = torch.from_numpy(np.array(phase0.T).ravel()).to(dev)
    out, err = invert_spectrogram_batch(d, [0], shapes, samplingRate, lengths=lens, nIter=nIter, phase0=phase0, rng=rng,
                                        to_host=True, device=device, **kw)
    return (out[0], err[0]) if return_error else out[0]


STAGES = ("statistics", "forward", "start", "inverse", "overlap-add", "error fold")


def kernel_ms():
    """sg_debug_invert_kernel_ms: the device milliseconds per stage (STAGES) of the last
    stft / istft / invert_spectrogram run on a context with profiling on, summed over its
    iterations and chunks; `forward` includes the projection inside the iteration."""
    ms = (C.c_double * len(STAGES))()
    native.check(native.lib().sg_debug_invert_kernel_ms(ms))
    return dict(zip(STAGES, ms))
