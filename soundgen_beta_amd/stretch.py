"""time_stretch(), shift_pitch() and resample(): a phase vocoder and a band-limited resampler.

A sound's duration without its pitch, its pitch without its duration, and the resampler the
second needs. No reference counterpart: the operators are stated here once and restated
twice, in numpy below and on the device (csrc/sg_stretch.h, csrc/sg_stretch.hip). The
vocoder sits between the operator pair (A, A+) of invert.py and is bound by spectrogram()'s
arguments and decisions like it; everything is fp64.

    N = wl + 2 pad, M = N / 2, s_i = the frame starts of the sound (n samples, F_in frames),
    t_j = the frame starts of a sound of n_out samples (F_out frames), g_j = t_j - t_j-1

  Time stretch. Given n_out and a position q_j in [0, F_in - 1] for every output frame:
       X = A x, M + 1 rows, WITHOUT getFrameBank's normalisation (the iteration's A of
       invert.py): the result is on the input's scale. For output frame j
           i = min(floor(q_j), F_in - 1), a = q_j - i, i1 = min(i + 1, F_in - 1), h = s_i1 - s_i,
           m_j[k] = (1 - a) |X_i[k]| + a |X_i1[k]|,
           d = (arg X_i1[k] - arg X_i[k]) - 2 pi ((k h) mod N) / N, wrapped: d -= 2 pi rint(d / 2 pi),
           (d / h)_j = d / h: the deviation of the instantaneous frequency at q_j from the
           bin's own 2 pi k / N; 0 where h = 0 (the last frame, equal starts).
       The phase starts at psi_0[k] = arg X_i(0)[k] and for j >= 1
           psi_j[k] = (psi_j-1[k] + 2 pi ((k g_j) mod N) / N) + g_j (d / h)_j-1, wrapped alike after
           every step; the index products are reduced in integers.
       X'_j[k] = m_j[k] (cos psi_j[k] + i sin psi_j[k]) and y = A+ X', n_out samples.
       With q_j = j and n_out = n this is X' = X up to rounding, so y = x wherever a frame covers
       a sample. time_stretch(factor) takes n_out = floor(n factor + 0.5) and q_j = min(j / factor,
       F_in - 1); positions= and length= replace them, and positions need not be monotone (a
       reversal, a freeze).
  Resample. up and down reduced by their gcd, D = max(up, down), Z = 16, n_out = ceil(n up / down):
           y[r] = sum_m x[m] (up / D) sinc(num / D) (1 + cos(pi num / (Z D))) / 2,   num = r down - m up
       (an exact integer) over 0 <= m < n with |num| < Z D, in ascending m. sinc(0) = 1; otherwise
       sinc(num / D) = sin(pi num / D) / (pi num / D) with the sine taken on num reduced mod 2 D to
       sign * sin(pi rem / D), 0 <= rem <= D / 2: exactly 0 at the non-zero multiples of D, so up = down
       returns x bit for bit. A Hann-windowed sinc of 16 zero crossings on either side with its
       cutoff at the lower Nyquist rate. Refused: D / min(up, down) above 64 (more than 2,048 taps a
       sample), up or down at 2^31 or above, n_out at 2^31 or above.
  Pitch shift. time_stretch by `multiplier` to n_s = floor(n multiplier + 0.5) samples, then
       resample by n : n_s: exactly n samples, every frequency multiplied by `multiplier`.
       Formants move with the pitch: keeping them in place is out of scope, as are transient
       handling and phase locking.

The *_numpy restatements take dtype (np.float64 or np.longdouble) as invert.py's do.
"""
import ctypes as C
import math

import numpy as np

from . import invert as IV
from . import native
from . import spectrogram as SP

Z = 16
MAX_RATIO = 64
LIMIT = 1 << 31


# ------------------------------------------------------------------ the integer side
def _ratio(up, down):
    if int(up) != up or int(down) != down or up < 1 or down < 1:
        raise ValueError("up and down are positive whole numbers")
    up, down = int(up), int(down)
    if up >= LIMIT or down >= LIMIT:
        raise ValueError("up or down is 2^31 or more")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if max(up, down) > MAX_RATIO * min(up, down):
        raise ValueError("a ratio of %d : %d is beyond 1 : %d (more than 2,048 taps a sample)" % (up, down, MAX_RATIO))
    return up, down, max(up, down)


def _n_out(n, up, down):
    n_out = -((-n * up) // down)
    if n_out >= LIMIT:
        raise ValueError("the output has 2^31 samples or more")
    return n_out


def _rates(samplingRate, newRate, up, down):
    if (up is None) != (down is None) or (up is None) == (newRate is None):
        raise ValueError("resample: give newRate (with samplingRate), or up and down")
    if up is None:
        if samplingRate is None or int(samplingRate) != samplingRate or int(newRate) != newRate:
            raise ValueError("resample: samplingRate and newRate are whole numbers; give up= and down= otherwise")
        up, down = int(newRate), int(samplingRate)
    return _ratio(up, down)


def _out_length(n, factor):
    if not (factor > 0 and math.isfinite(factor)):
        raise ValueError("factor must be a positive number")
    return int(math.floor(n * factor + 0.5))


def _positions(positions, factor, f_in, f_out):
    """The fp64 positions of an output's f_out frames, checked."""
    if positions is None:
        if factor is None:
            raise ValueError("time_stretch: give factor or positions")
        q = np.minimum(np.arange(f_out, dtype=np.float64) / float(factor), float(f_in - 1))
    else:
        q = np.ascontiguousarray(np.asarray(positions, dtype=np.float64).ravel())
    if len(q) != f_out:
        raise ValueError("the output has %d frames, not %d positions" % (f_out, len(q)))
    if not np.all((q >= 0) & (q <= f_in - 1)):  # a NaN fails both
        raise ValueError("a position is not in [0, %d]" % (f_in - 1))
    return q


# ------------------------------------------------------------------ the restatement
def _vocoder(X, s_in, t_out, q, N, dtype):
    """X' (F_out x (M + 1)) from X (F_in x (M + 1), complex in dtype) by the module docstring."""
    cd = np.result_type(dtype, np.complex64)
    f_in, M1 = X.shape
    tw = 8 * np.arctan(dtype(1))
    k = np.arange(M1, dtype=np.int64)
    mag, arg = np.abs(X), np.arctan2(X.imag, X.real)
    out = np.zeros((len(t_out), M1), dtype=cd)
    psi = dh_prev = None
    for j in range(len(t_out)):
        qj = float(q[j])
        i = min(int(math.floor(qj)), f_in - 1)
        a = dtype(qj - i)  # exact in fp64
        i1 = min(i + 1, f_in - 1)
        h = int(s_in[i1] - s_in[i])
        m = (1 - a) * mag[i] + a * mag[i1]
        if h > 0:
            d = (arg[i1] - arg[i]) - (tw * ((k * (h % N)) % N).astype(dtype)) / dtype(N)
            d = d - tw * np.rint(d / tw)
            dh = d / dtype(h)
        else:
            dh = np.zeros(M1, dtype=dtype)
        if j == 0:
            psi = arg[i].copy()
        else:
            g = int(t_out[j] - t_out[j - 1])
            v = (psi + (tw * ((k * (g % N)) % N).astype(dtype)) / dtype(N)) + dtype(g) * dh_prev
            psi = v - tw * np.rint(v / tw)
        dh_prev = dh
        out[j] = m * np.cos(psi) + 1j * (m * np.sin(psi))
    return out


def time_stretch_numpy(x, samplingRate, factor=None, positions=None, length=None, dtype=np.float64, return_spectrum=False,
                       **kw):
    """The time stretch of the module docstring: n_out samples, or (samples, X' as (M + 1) x F_out)."""
    dtype = np.dtype(dtype).type
    a = IV._args(kw)
    x = np.asarray(x, dtype=np.float64).ravel()
    n = len(x)
    wl, pad, N, s_in, w = IV._setup(n, samplingRate, a, dtype)
    if n < wl or len(s_in) == 0:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    n_out = _out_length(n, factor) if length is None else int(length)
    t_out = IV._starts(n_out, samplingRate, wl, IV._geometry(samplingRate, a)[3])
    if len(t_out) == 0:
        raise ValueError("an output of %d samples is shorter than the window (%d)" % (n_out, wl))
    q = _positions(positions, factor, len(s_in), len(t_out))
    X = IV._analysis(x.astype(dtype), s_in, w, pad, N, N // 2 + 1, dtype)
    Y = _vocoder(X, s_in, t_out, q, N, dtype)
    y = IV._synthesis(Y, t_out, w, pad, N, n_out, dtype)
    return (y, Y.T) if return_spectrum else y


def _weights(num, up, D, dtype):
    pi = 4 * np.arctan(dtype(1))
    v = num % (2 * D)  # [0, 2 D)
    sign = np.where(v >= D, -1, 1)
    rem = np.where(v >= D, v - D, v)
    rem = np.where(2 * rem > D, D - rem, rem)
    s = sign.astype(dtype) * np.sin(pi * rem.astype(dtype) / dtype(D))
    nd = num.astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = s / (pi * nd / dtype(D))
    hann = dtype(0.5) * (1 + np.cos(pi * nd / dtype(Z * D)))
    gain = dtype(up) / dtype(D)
    return np.where(num == 0, gain, gain * sinc * hann)


def resample_numpy(x, samplingRate=None, newRate=None, up=None, down=None, dtype=np.float64):
    """The resampler of the module docstring: ceil(n up / down) samples in dtype."""
    dtype = np.dtype(dtype).type
    up, down, D = _rates(samplingRate, newRate, up, down)
    xs = np.asarray(x).ravel().astype(dtype)
    n = len(xs)
    n_out = _n_out(n, up, down)
    acc = np.zeros(n_out, dtype=dtype)
    if n_out == 0:
        return acc
    c = np.arange(n_out, dtype=np.int64) * down
    W = Z * D
    lo = np.maximum((c - W) // up + 1, 0)
    hi = np.minimum(-((-(c + W)) // up) - 1, n - 1)
    for t in range(int((hi - lo).max()) + 1):  # ascending m for every output sample
        m = lo + t
        ok = m <= hi
        mm = np.where(ok, m, 0)
        term = xs[mm] * _weights(c - mm * up, up, D, dtype)
        acc[ok] = acc[ok] + term[ok]
    return acc


def shift_pitch_numpy(x, samplingRate, multiplier, dtype=np.float64, **kw):
    """time_stretch_numpy by `multiplier`, then resample_numpy by n : n_s: n samples."""
    n = len(np.asarray(x).ravel())
    s = time_stretch_numpy(x, samplingRate, factor=multiplier, dtype=dtype, **kw)
    return resample_numpy(s, up=n, down=len(s), dtype=dtype)


# ------------------------------------------------------------------ on the GPU (sg_stretch.hip)
def _err(L, rc):
    native.host_check(rc, L.sg_stretch_size_error)


def stretch_size(length, samplingRate=None, out_length=None, up=None, down=None, **kw):
    """sg_stretch_size (host only). With samplingRate and out_length (and spectrogram()'s
    arguments): dict(frames_in, frames_out, workspace_bytes) of a time stretch from `length` to
    `out_length` samples. With up and down: dict(n_out, taps) of the resampler. Raises
    SoundgenError with the library's code and text."""
    L = native.lib()
    if up is not None or down is not None:
        n_out, taps = C.c_int64(), C.c_int64()
        _err(L, L.sg_stretch_size(int(length), None, 0, int(up), int(down), None, None, None, C.byref(n_out), C.byref(taps)))
        return dict(n_out=n_out.value, taps=taps.value)
    return _vocoder_size(L, IV._params(samplingRate, IV._args(kw)), length, out_length)


def _vocoder_size(L, P, length, out_length):
    fi, fo, ws = C.c_int32(), C.c_int32(), C.c_int64()
    _err(L, L.sg_stretch_size(int(length), C.byref(P), int(out_length), 0, 0, C.byref(fi), C.byref(fo), C.byref(ws), None, None))
    return dict(frames_in=fi.value, frames_out=fo.value, workspace_bytes=ws.value)


def _per_call(v, nc, what):
    if v is None or np.isscalar(v):
        return [v] * nc
    if len(v) != nc:
        raise ValueError("one %s per call" % what)
    return list(v)


def _packed(data):
    import torch
    if data.dtype not in (torch.float32, torch.float64):
        raise TypeError("data must be float32 or float64")
    return int(data.dtype == torch.float64)


def _split(out, ooff, nc):
    h = out.cpu().numpy()
    return [h[ooff[i]:ooff[i + 1]].copy() for i in range(nc)]


def time_stretch_batch(data, offsets, lengths, samplingRate, factor=None, positions=None, out_lengths=None, workspace_cap=0,
                       return_spectrum=False, to_host=False, device=0, **kw):
    """The time stretch of a batch of sounds already in HBM (`data`: a float32 or float64 CUDA
    tensor, call i at offsets[i], lengths[i] samples; sg_time_stretch_batch). factor: one number
    or one per call; positions: None or one array (or None) per call; out_lengths: None or one
    length (or None) per call. The results stay in HBM: (out, out_offsets, out_lengths) with `out`
    an fp64 CUDA tensor; to_host=True returns the list of sounds instead. A sound shorter than
    the window has no frames, as in stft_batch: its result is silence. return_spectrum=True adds
    (spec, spec_offsets, shapes): X' as stft_batch lays spectra out. workspace_cap: bytes a chunk
    of the batch may take (0: 1 GiB)."""
    import torch
    L = native.lib()
    P = IV._params(samplingRate, IV._args(kw))
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    is64 = _packed(data)
    fac, pos, olen = _per_call(factor, nc, "factor"), _per_call(positions, nc, "array of positions"), _per_call(out_lengths, nc, "length")
    wl = IV._size(L, P, 0)["wl"]
    bins = IV._size(L, P, 0)["bins"]
    outl, qs, shapes = [], [], []
    for i in range(nc):
        n = max(int(lens[i]), 0)
        if olen[i] is None and fac[i] is None:
            raise ValueError("time_stretch: give factor or out_lengths")
        n_out = _out_length(n, fac[i]) if olen[i] is None else int(olen[i])
        z = _vocoder_size(L, P, n, n_out)
        if z["frames_in"] == 0:
            q = np.zeros(0)
        elif z["frames_out"] == 0:
            raise ValueError("call %d: an output of %d samples is shorter than the window (%d)" % (i, n_out, wl))
        else:
            q = _positions(pos[i], fac[i], z["frames_in"], z["frames_out"])
        outl.append(n_out)
        qs.append(q)
        shapes.append((bins + 1, len(q)))
    outl = np.ascontiguousarray(np.asarray(outl, dtype=np.int64))
    flat = np.ascontiguousarray(np.concatenate(qs + [np.zeros(1)]))
    poff, p_poff = native.out_offsets([len(q) for q in qs])
    pcnt = np.ascontiguousarray(np.asarray([len(q) for q in qs], dtype=np.int64))
    ooff, p_ooff = native.out_offsets(outl)
    soff, p_soff = native.out_offsets([r * f for r, f in shapes])
    i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    ctx = native.default_context(device)
    out = native.device_out(data, ooff[-1])
    spec = torch.empty(max(int(soff[-1]), 1), dtype=torch.complex128, device=data.device) if return_spectrum else None
    torch.cuda.synchronize(data.device)
    if nc:
        native.check(L.sg_time_stretch_batch(
            ctx.ptr, C.c_void_p(data.data_ptr()), is64, p_offs, p_lens, nc, C.byref(P), outl.ctypes.data_as(i64p),
            flat.ctypes.data_as(dp), p_poff, pcnt.ctypes.data_as(i64p), C.c_void_p(out.data_ptr()), p_ooff, int(workspace_cap),
            C.c_void_p(spec.data_ptr()) if return_spectrum else None, p_soff if return_spectrum else None), ctx.ptr)
    res = _split(out, ooff, nc) if to_host else (out, ooff[:-1].copy(), outl)
    if not return_spectrum:
        return res
    if to_host:
        h = spec.cpu().numpy()
        return res, [h[soff[i]:soff[i + 1]].reshape(shapes[i][1], shapes[i][0]).T.copy() for i in range(nc)]
    return res, (spec, soff[:-1].copy(), shapes)


def resample_batch(data, offsets, lengths, samplingRate=None, newRate=None, up=None, down=None, to_host=False, device=0):
    """The resampler on a batch of sounds already in HBM (sg_resample_batch). samplingRate and
    newRate (whole numbers), or up and down: one number or one per call. (out, out_offsets,
    out_lengths) in HBM, or the list of sounds with to_host=True."""
    L = native.lib()
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    is64 = _packed(data)
    ups, downs, outl = [], [], []
    for i, (a, b, c, d) in enumerate(zip(*[_per_call(v, nc, "ratio") for v in (samplingRate, newRate, up, down)])):
        u, dn, _ = _rates(a, b, c, d)
        ups.append(u)
        downs.append(dn)
        outl.append(_n_out(max(int(lens[i]), 0), u, dn))
    ups, downs, outl = (np.ascontiguousarray(np.asarray(v, dtype=np.int64)) for v in (ups, downs, outl))
    ooff, p_ooff = native.out_offsets(outl)
    i64p = C.POINTER(C.c_int64)
    ctx = native.default_context(device)
    out = native.device_out(data, ooff[-1])
    if nc:
        native.check(L.sg_resample_batch(ctx.ptr, C.c_void_p(data.data_ptr()), is64, p_offs, p_lens, nc, ups.ctypes.data_as(i64p),
                                         downs.ctypes.data_as(i64p), C.c_void_p(out.data_ptr()), p_ooff), ctx.ptr)
    return _split(out, ooff, nc) if to_host else (out, ooff[:-1].copy(), outl)


def shift_pitch_batch(data, offsets, lengths, samplingRate, multiplier, workspace_cap=0, to_host=False, device=0, **kw):
    """shift_pitch of a batch of sounds already in HBM: time_stretch_batch by `multiplier` (one
    number or one per call), then resample_batch by n : n_s on the stretched sounds, which stay
    in HBM in between. (out, out_offsets, out_lengths) with out_lengths = lengths; a sound
    shorter than the window comes back as silence."""
    lens = np.asarray(lengths, dtype=np.int64)
    mid, moff, mlen = time_stretch_batch(data, offsets, lengths, samplingRate, factor=multiplier, workspace_cap=workspace_cap,
                                         device=device, **kw)
    ok = (lens > 0) & (mlen > 0)
    return resample_batch(mid, moff, np.where(ok, mlen, 0), up=np.where(ok, lens, 1), down=np.where(ok, mlen, 1),
                          to_host=to_host, device=device)


# ------------------------------------------------------------------ one sound from the host
def _one(x, samplingRate, device):
    import torch
    s, sr = SP._input(x, samplingRate)
    return s, sr, lambda v: torch.from_numpy(np.array(v, dtype=np.float64)).to(IV._device(device))


def time_stretch(x, samplingRate=None, factor=None, positions=None, length=None, return_spectrum=False, device=0, **kw):
    """One sound (a numeric vector with samplingRate, or the path of a mono 16-bit PCM file)
    `factor` times as long at the same pitch, on the GPU and on the input's scale. positions
    (one per output frame, in input frames) and length (samples) replace factor's.
    return_spectrum=True: (sound, X' as (M + 1) x frames)."""
    s, sr, put = _one(x, samplingRate, device)
    P = IV._params(sr, IV._args(kw))  # the refusals, before any launch
    if len(s) < IV._size(native.lib(), P, len(s))["wl"]:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    r = time_stretch_batch(put(s), [0], [len(s)], sr, factor=factor, positions=None if positions is None else [positions],
                           out_lengths=None if length is None else [length], return_spectrum=return_spectrum, to_host=True,
                           device=device, **kw)
    return (r[0][0], r[1][0]) if return_spectrum else r[0]


def resample(x, samplingRate=None, newRate=None, up=None, down=None, device=0):
    """One sound at newRate instead of samplingRate (whole numbers), or by up : down, on the GPU:
    ceil(n up / down) samples through a Hann-windowed sinc of 16 zero crossings."""
    import torch
    _rates(samplingRate, newRate, up, down)
    s = np.asarray(x, dtype=np.float64).ravel()
    d = torch.from_numpy(np.array(s)).to(IV._device(device))
    return resample_batch(d, [0], [len(s)], samplingRate=samplingRate, newRate=newRate, up=up, down=down, to_host=True,
                          device=device)[0]


def shift_pitch(x, samplingRate=None, multiplier=1.0, device=0, **kw):
    """One sound with every frequency multiplied by `multiplier` and its length kept, on the
    GPU. Formants move with the pitch."""
    s, sr, put = _one(x, samplingRate, device)
    P = IV._params(sr, IV._args(kw))
    if len(s) < IV._size(native.lib(), P, len(s))["wl"]:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    return shift_pitch_batch(put(s), [0], [len(s)], sr, multiplier, to_host=True, device=device, **kw)[0]


STAGES = ("resample", "forward", "vocoder", "inverse", "overlap-add")


def kernel_ms():
    """sg_debug_stretch_kernel_ms: the device milliseconds per stage (STAGES) of the last
    time_stretch or resample run on a context with profiling on, summed over its chunks."""
    ms = (C.c_double * len(STAGES))()
    native.check(native.lib().sg_debug_stretch_kernel_ms(ms))
    return dict(zip(STAGES, ms))
