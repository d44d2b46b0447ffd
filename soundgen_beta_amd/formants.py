"""analyze()'s formant tracks (R/analyze.R:486-502): per frame that passed cond_silence,
phonTools::findformants(frame, samplingRate, verify = FALSE) with its defaults, and the first
nFormants of what it keeps as f1_freq, f1_width, f2_freq, ... (NaN for NA).

phonTools is not in the reference tree. findformants is restated from phonTools 0.2-2.1 as
documented; PARITY IS UNPINNED against R, as for dtw::dtw (sg_dtw_symmetric2) and R's nmmin.
The steps, with the constants that soundgen_beta_amd/csrc/sg_formants.h holds for the device:

    order       round(fs / 1000) + 3 (R's half-even round)
    frame       y[0] = x[0], y[i] = x[i] - exp(-2 pi 50 / fs) x[i - 1]; y - mean(y); times the
                Hann window 0.5 (1 - cos(2 pi i / (n - 1)))
    lags        r[k] = sum_i y[i] y[i + k], k = 0..order, unnormalised
    predictor   T a = -r[1..order], T the Toeplitz matrix of r[0..order - 1]. phonTools calls
                solve() (LU); here Levinson-Durbin (tests/test_formants.py measures both against
                a long-double solution). r[0] <= 0, a non-finite value or a prediction error <= 0
                give an NA row, as the reference's try() does
    roots       polyroot(rev(coeffs)): all roots of z^p + a1 z^(p - 1) + ... + ap, here by the
                Aberth-Ehrlich iteration from p points on a circle of radius 0.9, stopped when
                every root has settled: its correction satisfies |w| <= 4 eps |z|, or has reached
                the rounding noise of P / P' and stopped shrinking (aberth_roots); given up (NA
                row) after 64 steps
    formants    formant = round(atan2(Im z, Re z) fs / (2 pi), 2), bandwidth = -(fs / pi)
                log|z|, ordered by formant (order(): ties by root index), kept where
                bandwidth < 600 & formant > 200 & formant < fs / 2
Stated difference: R's round(x, 2) multiplies in long double; the device computes
nearbyint(100 x) / 100 in fp64. The two differ only where 100 x lies within an ulp of a half.

- find_formants_numpy: the restatement for one frame, in fp64 or (the tests' reference)
  long double; formants_numpy: analyze()'s per-frame table with analyze_frames_numpy()'s
  host decisions (window, frame starts, gate).
- formants / formants_batch / find_formants_frames: the same on the GPU (sg_formants.hip:
  sg_fmt_lags, one workgroup per frame; sg_fmt_roots, one wave per frame, one root per lane).
  The order is limited to 64 (samplingRate < 61.5 kHz): SoundgenError(SG_E_UNSUPPORTED) above.
- find_formants_sound / find_formants_sounds_batch: findformants on a whole sound of any
  length (matchPars()' initial formants, R/matchPars.R:130): the sound does not fit a frame's
  LDS, so sg_fmt_sound_* cut it into chunks of 4096 samples whose sums are folded in chunk
  order, then sg_fmt_roots. At most 8 kept rows are returned.
Out of scope: formants in the device summary kernel (analyze(summary=True,
formants=True) reduces the formant table on the host), the R binding, smoothVars on formants.
"""
import ctypes as C
import math

import numpy as np

from . import native

MAX_FORMANTS = 8
MAX_ORDER = 64
PREEMPH_HZ = 50.0
MAX_BW = 600.0
MIN_FORMANT = 200.0
RADIUS = 0.9
MAX_ITER = 64


def formant_columns(nFormants):
    """f1_freq, f1_width, f2_freq, ... (R/analyze.R:563)."""
    return tuple("f%d_%s" % (i + 1, k) for i in range(nFormants) for k in ("freq", "width"))


def formant_order(fs):
    """round(fs / 1000) + 3, R's round (half to even, as Python's)."""
    return int(round(fs / 1000)) + 3


def _check_n(nFormants):
    if not isinstance(nFormants, (int, np.integer)) or isinstance(nFormants, bool) or not 1 <= nFormants <= MAX_FORMANTS:
        raise ValueError("formants: nFormants must be a whole number in 1..%d" % MAX_FORMANTS)
    return int(nFormants)


def _check_order(fs):
    order = formant_order(fs)
    if order > MAX_ORDER:
        raise native.SoundgenError(-4, "formants: the order round(samplingRate / 1000) + 3 = %d exceeds %d (one root "
                                   "per lane of a wave): samplingRate must stay below 61.5 kHz" % (order, MAX_ORDER))
    return order


# ---------------------------------------------------------------- the restatement
def _two_pi(dtype):
    return 8 * np.arctan(dtype(1))


def lpc_lags(frame, fs, order, dtype=np.float64):
    """Steps 2-5: the lags r[0..order] of the pre-emphasised, demeaned, Hann-windowed frame."""
    x = np.asarray(frame, dtype=dtype)
    n = len(x)
    coeff = -np.exp(-_two_pi(dtype) * dtype(PREEMPH_HZ) / dtype(fs))
    y = x.copy()
    y[1:] = x[1:] + coeff * x[:-1]
    y = y - y.sum() / n
    y = y * (dtype(0.5) * (1 - np.cos(_two_pi(dtype) * np.arange(n, dtype=dtype) / dtype(n - 1))))
    return np.array([np.dot(y[:n - k], y[k:]) for k in range(order + 1)], dtype=dtype)


def levinson(r, dtype=np.float64):
    """Levinson-Durbin for T a = -r[1..p]: a1..ap, or None where the frame gets an NA row."""
    r = np.asarray(r, dtype=dtype)
    p = len(r) - 1
    E = r[0]
    if not (E > 0 and np.isfinite(E)):
        return None
    a = np.zeros(p, dtype=dtype)
    for m in range(1, p + 1):
        acc = r[m] + np.dot(a[:m - 1], r[m - 1:0:-1][:m - 1])
        k = -acc / E
        a[:m - 1] = a[:m - 1] + k * a[:m - 1][::-1]
        a[m - 1] = k
        E = E * (1 - k * k)
        if not (E > 0 and np.isfinite(E)):
            return None
    return a


def toeplitz_solve(r):
    """phonTools' route: solve(T, -r[1..p]) by LU, in fp64."""
    r = np.asarray(r, dtype=np.float64)
    p = len(r) - 1
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    return np.linalg.solve(r[idx], -r[1:])


def aberth_roots(a, dtype=np.float64, max_iter=MAX_ITER):
    """All roots of z^p + a[0] z^(p - 1) + ... + a[p - 1] by the Aberth-Ehrlich iteration,
    every root corrected from the previous iterate of all the others: (roots, iterations), roots
    None when max_iter steps do not settle every root. A root settles, for good, when its
    correction satisfies |w| <= 4 eps |z|, or when the corrections have reached the rounding
    noise of P / P' and stopped shrinking: |w| <= sqrt(eps) |z| and |w| >= half the previous |w|
    (sg_formants.h: fmt_aberth_step)."""
    a = np.asarray(a, dtype=dtype)
    p = len(a)
    cd = np.result_type(dtype, np.complex64)
    eps = np.finfo(dtype).eps
    tol2 = (4 * eps) ** 2
    prev = np.full(p, np.inf, dtype=dtype)
    settled = np.zeros(p, dtype=bool)
    ang = _two_pi(dtype) * (np.arange(p, dtype=dtype) + dtype(0.25)) / dtype(p)
    z = (dtype(RADIUS) * (np.cos(ang) + 1j * np.sin(ang))).astype(cd)
    off = ~np.eye(p, dtype=bool)
    with np.errstate(all="ignore"):
        for it in range(1, max_iter + 1):
            P = np.ones(p, dtype=cd)
            D = np.zeros(p, dtype=cd)
            for i in range(p):
                D = D * z + P
                P = P * z + a[i]
            N = P / D
            diff = z[:, None] - z[None, :]
            inv = np.zeros((p, p), dtype=cd)
            inv[off] = 1 / diff[off]
            w = N / (1 - N * inv.sum(axis=1))
            z = z - w
            w2, z2 = w.real ** 2 + w.imag ** 2, z.real ** 2 + z.imag ** 2
            settled |= (w2 <= tol2 * z2) | ((w2 <= eps * z2) & (w2 >= 0.25 * prev))
            prev = w2
            if np.all(settled):
                return z, it
    return None, max_iter


def roots_to_formants(z, fs):
    """Step 8's conversion: (unrounded frequency, formant = round(f, 2) as fp64, bandwidth)."""
    dtype = z.real.dtype.type
    freq = np.arctan2(z.imag, z.real) * (dtype(fs) / _two_pi(dtype))
    formant = np.rint(100 * freq).astype(np.float64) / 100.0
    bw = -(dtype(fs) / (_two_pi(dtype) / 2)) * (dtype(0.5) * np.log(z.real ** 2 + z.imag ** 2))
    return freq, formant, bw


def select_formants(formant, bw, fs):
    """Step 8's order and filter: the indices of the kept roots, in order(formant) (stable)."""
    o = np.argsort(formant, kind="stable")
    return np.array([i for i in o if bw[i] < MAX_BW and formant[i] > MIN_FORMANT and formant[i] < fs / 2], dtype=int)


def formants_from_coeffs(a, fs, dtype=np.float64, raw=False, max_iter=MAX_ITER):
    """The root stage, the conversion and the selection for the predictor a1..ap: the kept
    (formant, bandwidth) rows as an fp64 array of shape (k, 2), k == 0 where the iteration gives
    up. raw=True: a dict with `kept` (that array), `failed`, `iterations`, `roots`, and per root
    `freq` (unrounded, Hz), `formant`, `bandwidth` and `keep` (the indices kept, in order)."""
    z, it = aberth_roots(a, dtype, max_iter)
    if z is None:
        kept = np.zeros((0, 2))
        return dict(kept=kept, failed=True, iterations=it) if raw else kept
    freq, formant, bw = roots_to_formants(z, fs)
    keep = select_formants(formant, bw, fs)
    kept = np.stack([formant[keep], bw[keep].astype(np.float64)], axis=1) if len(keep) else np.zeros((0, 2))
    if raw:
        return dict(kept=kept, failed=False, iterations=it, roots=z, freq=freq, formant=formant, bandwidth=bw, keep=keep)
    return kept


def find_formants_numpy(frame, fs, dtype=np.float64, raw=False, max_iter=None):
    """phonTools::findformants(frame, fs, verify = FALSE) restated (see the module docstring):
    the full kept list as an fp64 array of (formant, bandwidth) rows; no row where the frame
    gets NA. dtype=np.longdouble is the tests' reference: every step in long double, the
    iteration run to long-double convergence (up to 4 * 64 steps unless max_iter says
    otherwise). raw=True: formants_from_coeffs()'s dict plus `r` and `a`."""
    order = formant_order(fs)
    if len(frame) <= order:
        raise ValueError("find_formants: a frame must have more than order = %d samples" % order)
    if max_iter is None:
        max_iter = MAX_ITER if dtype is np.float64 else 4 * MAX_ITER
    with np.errstate(all="ignore"):
        r = lpc_lags(frame, fs, order, dtype)
        a = levinson(r, dtype)
    if a is None:
        kept = np.zeros((0, 2))
        return dict(kept=kept, failed=True, iterations=0, r=r, a=None) if raw else kept
    out = formants_from_coeffs(a, fs, dtype, raw, max_iter)
    if raw:
        out.update(r=r, a=a)
    return out


def _rows(found, nFormants):
    row = np.full(2 * nFormants, math.nan)
    k = min(len(found), nFormants)
    row[:2 * k] = found[:k].ravel()
    return row


def _dict(m, nFormants):
    return {k: m[:, i].copy() for i, k in enumerate(formant_columns(nFormants))}


def formants_numpy(x, samplingRate=None, nFormants=3, dtype=np.float64, _probe=None, **kw):
    """analyze()'s formant columns restated on the host (R/analyze.R:486-502): a dict f1_freq,
    f1_width, ... of per-frame arrays; a frame that fails cond_silence, and a row past the kept
    count, is NaN. kw: analyze_frames_numpy()'s arguments, whose host decisions (window, frame
    starts, gate) are reused. _probe (a dict) receives `frames` (wl x frames, getFrameBank's) and
    `analysed` (the frame indices that pass the gate)."""
    from .analyze import analyze_frames_numpy
    from .spectrogram import _input, get_frame_bank
    nFormants = _check_n(nFormants)
    sound, sr = _input(x, samplingRate)
    _check_order(sr)
    kw.pop("pitchMethods", None)  # the gate does not depend on them
    probe = {}
    t = analyze_frames_numpy(sound, sr, _probe=probe, **kw)
    s, d = probe["s"], probe["d"]
    with np.errstate(invalid="ignore", divide="ignore"):
        bank = get_frame_bank(sound, sr, d["wl"], s["wn"], s["step"], 0)
    gate = np.nonzero(t["cond_silence"] == 1)[0]
    m = np.full((bank.shape[1], 2 * nFormants), math.nan)
    for f in gate:                                                            # :487
        m[f] = _rows(find_formants_numpy(bank[:, f], sr, dtype), nFormants)   # :489-500
    if _probe is not None:
        _probe.update(frames=bank, analysed=gate)
    return _dict(m, nFormants)


# ------------------------------------------------------- on the GPU (sg_formants.hip)
def _gate_settings(samplingRate, duration, kw):
    """repair()'s dict for the gate: the pitch methods do not enter it."""
    from .analyze import PITCH_METHODS, repair
    kw = dict(kw)
    kw.pop("pitchMethods", None)
    return repair(samplingRate, duration, pitchMethods=PITCH_METHODS, **kw)


def formants_size(s, nFormants):
    """sg_formants_size (host only): (order, cols) for repair()'s dict s."""
    from .analyze import _host_check, _params
    L = native.lib()
    P = _params(s)
    order, cols = C.c_int32(), C.c_int32()
    rc = L.sg_formants_size(C.byref(P), int(nFormants), C.byref(order), C.byref(cols))
    _host_check(rc)
    return order.value, cols.value


def _formants_sound(sound, s, nFormants, device):
    """sg_formants_sound for repair()'s dict s: the frames x 2 nFormants table."""
    from .analyze import _check, _params, _too_short, frame_decisions_native
    from .analyze import PITCH_METHODS
    s = dict(s, pitchMethods=PITCH_METHODS)
    formants_size(s, nFormants)
    d = frame_decisions_native(len(sound), s)
    if len(sound) <= d["wl"]:
        raise _too_short(len(sound), d["wl"])
    ctx = native.default_context(device)
    sound = np.ascontiguousarray(sound, dtype=np.float64)
    out = np.zeros(d["frames"] * 2 * nFormants)
    dp = C.POINTER(C.c_double)
    P = _params(s)
    _check(native.lib().sg_formants_sound(ctx.ptr, sound.ctypes.data_as(dp), len(sound), C.byref(P), nFormants,
                                          out.ctypes.data_as(dp)), ctx.ptr)
    return out.reshape(d["frames"], 2 * nFormants)


def formants(x, samplingRate=None, nFormants=3, device=0, **kw):
    """analyze()'s formant columns on the GPU (sg_formants_sound, fp64): a dict f1_freq,
    f1_width, ... of per-frame arrays, NaN for NA. x: a numeric vector with samplingRate, or the
    path of a mono 16-bit PCM file; kw: analyze_frames()' arguments (silence, windowLength, step,
    overlap, wn, ...), which decide the window, the frames and the gate."""
    from .spectrogram import _input
    nFormants = _check_n(nFormants)
    sound, sr = _input(x, samplingRate)
    s = _gate_settings(sr, len(sound) / sr, kw)
    return _dict(_formants_sound(sound, s, nFormants, device), nFormants)


def formants_behind(data, offs, lens, s, nFormants, tables, table_offsets, table_cols, frames, device=0):
    """sg_formants_batch behind finished tables in HBM (analyze_frames_batch's, pitch_candidates_
    batch's or analyze_batch's `out`, `offsets`, `cols` and `frames`): (an fp64 CUDA tensor, the
    int64 offsets of each call's frames x 2 nFormants table in it, one more than the calls)."""
    from .analyze import PITCH_METHODS, _check, _params
    nFormants = _check_n(nFormants)
    s = dict(s, pitchMethods=PITCH_METHODS)
    formants_size(s, nFormants)
    L = native.lib()
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    toff = np.ascontiguousarray(table_offsets, dtype=np.int64)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    nc = len(offs)
    foff, p_foff = native.out_offsets([int(f) * 2 * nFormants for f in fr])
    out = native.device_out(data, foff[-1])
    ctx = native.default_context(device)
    P = _params(s)
    _check(L.sg_formants_batch(ctx.ptr, C.c_void_p(data.data_ptr()), offs.ctypes.data_as(i64p), lens.ctypes.data_as(i64p),
                               nc, C.byref(P), nFormants, C.c_void_p(tables.data_ptr()), toff.ctypes.data_as(i64p),
                               int(table_cols), fr.ctypes.data_as(i32p), C.c_void_p(out.data_ptr()), p_foff), ctx.ptr)
    return out, foff


def _host_tables(out, foff, frames, nFormants):
    h = out.cpu().numpy()
    return [h[foff[i]:foff[i + 1]].reshape(int(frames[i]), 2 * nFormants).copy() for i in range(len(frames))]


def formants_batch(data, offsets, lengths, samplingRate, nFormants=3, to_host=False, device=0, **kw):
    """formants(call i, samplingRate, ...) for a batch of sounds already in HBM (`data`: a
    float32 CUDA tensor laid out as for analyze_frames_batch): analyze_frames_batch() for the
    gate, then sg_formants_batch behind its tables, which stay in HBM. Returns a dict with `out`
    (an fp64 CUDA tensor), `offsets` (call i's table starts at out[offsets[i]]), `frames`, `cols`
    (2 nFormants) and `columns`; a call's table equals formants()' bit for bit, wherever it
    stands in the batch. A call without frames (not longer than the window, or of length < 0)
    writes nothing. to_host=True returns the list of per-call dicts formants() returns."""
    from .analyze import analyze_frames_batch
    nFormants = _check_n(nFormants)
    s = _gate_settings(samplingRate, None, kw)
    formants_size(s, nFormants)
    kw = dict(kw)
    kw.pop("pitchMethods", None)
    g = analyze_frames_batch(data, offsets, lengths, samplingRate, device=device, **kw)
    out, foff = formants_behind(data, offsets, lengths, s, nFormants, g["out"], g["offsets"], g["cols"], g["frames"], device)
    if not to_host:
        return dict(out=out, offsets=foff[:-1].copy(), frames=g["frames"], cols=2 * nFormants,
                    columns=formant_columns(nFormants))
    return [_dict(m, nFormants) for m in _host_tables(out, foff, g["frames"], nFormants)]


def find_formants_frames(frames, fs, nFormants=3, device=0):
    """sg_formants_frames: the two kernels alone on caller-given frames (an array of shape
    (nframes, n): no gate, no normalisation, no analysis window); an fp64 array of shape
    (nframes, 2 nFormants), NaN for NA."""
    from .analyze import _check
    nFormants = _check_n(nFormants)
    _check_order(fs)
    fr = np.ascontiguousarray(frames, dtype=np.float64)
    if fr.ndim != 2:
        raise ValueError("find_formants_frames: frames must have shape (nframes, n)")
    ctx = native.default_context(device)
    out = np.zeros((fr.shape[0], 2 * nFormants))
    dp = C.POINTER(C.c_double)
    _check(native.lib().sg_formants_frames(ctx.ptr, fr.ctypes.data_as(dp), fr.shape[1], fr.shape[0], float(fs), nFormants,
                                           out.ctypes.data_as(dp)), ctx.ptr)
    return out


# ------------------------------------------- a whole sound (matchPars; sg_fmt_sound_*)
def formants_whole_size(fs, length):
    """sg_formants_whole_size (host only, no GPU call): (order, chunk, nchunks) for a sound of
    `length` samples at fs. SoundgenError(SG_E_UNSUPPORTED) for an order above 64 or more than
    2^31 - 1 chunks."""
    L = native.lib()
    order, chunk, nchunks = C.c_int32(), C.c_int32(), C.c_int64()
    native.check(L.sg_formants_whole_size(float(fs), int(length), C.byref(order), C.byref(chunk), C.byref(nchunks)))
    return order.value, chunk.value, nchunks.value


def _kept_rows(row):
    m = np.asarray(row, dtype=np.float64).reshape(MAX_FORMANTS, 2)
    return m[~np.isnan(m[:, 0])].copy()


def find_formants_sound(x, fs, device=0):
    """phonTools::findformants(x, fs, verify = FALSE) on a whole sound of any length on the GPU
    (sg_formants_whole, fp64: the chunked kernels sg_fmt_sound_* of sg_formants.hip, then
    sg_fmt_roots): the kept (formant, bandwidth) rows in ascending order of formant, an array of
    shape (n_kept, 2). At most 8 rows are returned (a stated limit; matchPars reads 3).
    find_formants_numpy(x, fs) is the host restatement. ValueError for a sound not longer than
    the order; SoundgenError(SG_E_UNSUPPORTED) for an order above 64."""
    from .analyze import _check
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    order = formants_whole_size(fs, len(x))[0]  # the refusals that need no device
    if len(x) <= order:
        raise ValueError("find_formants_sound: the sound must have more than order = %d samples" % order)
    ctx = native.default_context(device)
    out = np.zeros(2 * MAX_FORMANTS)
    dp = C.POINTER(C.c_double)
    _check(native.lib().sg_formants_whole(ctx.ptr, x.ctypes.data_as(dp), len(x), float(fs), out.ctypes.data_as(dp)), ctx.ptr)
    return _kept_rows(out)


def find_formants_sounds_batch(data, offsets, lengths, fs, to_host=False, device=0):
    """find_formants_sound(call i, fs) for a batch of sounds already in HBM (`data`: a float32 CUDA
    tensor, call i at offsets[i], lengths[i] samples -- the layout of batch.synthesize_packed)
    in one launch sequence (sg_formants_whole_batch): an fp64 CUDA tensor of shape (n_calls, 16),
    a call's row (formant, bandwidth) pairs with NaN behind the kept ones; all NaN for a call not
    longer than the order (a failed call of length < 0 too). A call's row is the same bit for
    bit alone, in any batch and at any position of it. to_host=True returns the list of per-call
    (n_kept, 2) arrays find_formants_sound() returns."""
    from .analyze import _check
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    formants_whole_size(fs, int(lens.max()) if nc else 0)  # the refusals that need no device
    ctx = native.default_context(device)
    out = native.device_out(data, nc * 2 * MAX_FORMANTS)
    _check(native.lib().sg_formants_whole_batch(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, float(fs),
                                                C.c_void_p(out.data_ptr())), ctx.ptr)
    out = out[:nc * 2 * MAX_FORMANTS].reshape(nc, 2 * MAX_FORMANTS)
    if not to_host:
        return out
    return [_kept_rows(r) for r in out.cpu().numpy()]


def formants_whole_profile():
    """sg_debug_formants_whole_kernel_ms: (the device milliseconds of the mean, the chunk lags,
    their fold and the roots in the last profiled run, (capped, analysed, iterations) of the last
    run)."""
    ms = (C.c_double * 4)()
    n = (C.c_int64 * 3)()
    native.lib().sg_debug_formants_whole_kernel_ms(ms, n)
    return dict(zip(("mean", "chunk_lags", "fold", "roots"), (float(v) for v in ms))), (int(n[0]), int(n[1]), int(n[2]))


def formants_counts():
    """sg_debug_formants_kernel_ms' counters of the last run: (frames that hit the iteration
    cap, frames analysed, the Aberth iterations those took)."""
    ms = (C.c_double * 2)()
    n = (C.c_int64 * 3)()
    native.lib().sg_debug_formants_kernel_ms(ms, n)
    return int(n[0]), int(n[1]), int(n[2])


def formant_summary(table, nFormants):
    """The 6 nFormants summary cells of a formant table (a dict of per-frame arrays) as
    analyze(summary = TRUE) forms them (R/analyze.R:791-796): <column>_mean, _median, _sd over
    the non-NA frames, in R's arithmetic (segment.py's r_mean, r_median, r_sd)."""
    from .segment import r_mean, r_median, r_sd
    out = {}
    for k in formant_columns(nFormants):
        v = np.asarray(table[k], float)
        v = v[~np.isnan(v)]
        out[k + "_mean"], out[k + "_median"], out[k + "_sd"] = r_mean(v), r_median(v), r_sd(v)
    return out
