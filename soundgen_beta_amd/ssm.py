"""ssm(): self-similarity matrix and novelty contour of a sound (R/SSM.R:63-360).

- ssm_numpy: the host restatement the GPU is compared against, restated from
  the sources:
    ssm()                   R/SSM.R:63-210 (input handling :100-110, the integer
                            decisions :111-128, melfcc call :131-139, the input
                            rows :140-148)
    selfsim()               R/SSM.R:224-265
    getCheckerboardKernel() R/SSM.R:281-324
    getNovelty()            R/SSM.R:337-360
    zeroOne()               R/utilities_math.R:58-61
    melfcc(spec_out = TRUE) tuneR_1.3.2.tar.gz::tuneR/R/melfcc.R:31-87 (pre-emphasis
                            :32-35, powspec :41, audspec :44, spec2cep :66, lifter :70)
    spec2cep(type = "t2")   tuneR/R/spec2cep.R:13-24, :50 (dctm23 / dctm2, dctm %*% log(spec))
    lifter(lift = 0.6)      tuneR/R/lifter.R:21-29 (c(1, (1:(ncep-1))^lift))
    normalize(unit = "32")  tuneR/R/normalize.R:19-43 as ssm() uses it on a numeric
                            vector: centre, then divide by max|x| (skipped when
                            all.equal(m, 0)); the final scaling to the 32-bit integer
                            range is a common factor of every frame that neither
                            similarity sees, and is not restated
  powspec, fft2melmx and the pre-emphasis are those of matchpars.py.
- Quirks kept: kernelSize is counted in windowLength frames, not in steps
  (R/SSM.R:117-119); the dmvnorm branch of the checkerboard kernel (size >= 50)
  takes kernelSD as a variance (R/SSM.R:298); a file path skips normalize, so its
  samples keep their offset and scale (the scale moves cepstrum 1 alone) and its
  result differs from the numeric-vector call on the same samples; zeroOne of the
  whole matrix has no na.rm, so one NaN cell makes the matrix NaN and the
  novelty all 0; winIdx may repeat a window.
- ssm / ssm_batch: the same on the GPU (sg_ssm.hip: fp64 frames, features, a
  batched Gram matrix on the matrix pipe, novelty), one sound from the host or
  a packed batch already in HBM (batch.synthesize_packed's layout).
"""
import ctypes as C
import math
import os
import struct
import wave as _wave

import numpy as np

from . import native
from .matchpars import fft2melmx, powspec
from .morph import _r_seq_len

_INPUTS = ("mfcc", "audiogram", "spectrum")
_SIMILS = ("cosine", "cor")


def _rround(x):
    return int(np.round(x))  # R's round(): half to even


def zero_one(x):
    """zeroOne(), R/utilities_math.R:58-61 (min / max without na.rm)."""
    x = np.asarray(x, float)
    if np.isnan(x).any():
        return np.full(x.shape, np.nan)
    x = x - x.min()
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / x.max()


# ---------------------------------------------------------------- melfcc
def dctm2(nbands, ncep):
    """spec2cep's dctm2: the orthogonal DCT-II, first row / sqrt(2); ncep x nbands."""
    i = np.arange(ncep, dtype=float)[:, None]
    odd = np.arange(1, 2 * nbands, 2, dtype=float)[None, :]
    d = np.cos(i * odd / (2 * nbands) * np.pi) * math.sqrt(2 / nbands)
    d[0] = d[0] / math.sqrt(2)
    return d


def lifter_weights(ncep, lift=0.6):
    """lifter(): c(1, (1:(ncep-1))^lift)."""
    if ncep < 2:
        raise ValueError("lifter: ncep must be >= 2 (R's 1:(ncep-1) runs backwards below that)")
    return np.concatenate([[1.0], np.arange(1, ncep, dtype=float) ** lift])


def cepstra(aspectrum, numcep):
    """lifter(spec2cep(aspectrum, ncep = numcep, type = 't2')$cep): numcep x frames."""
    with np.errstate(divide="ignore", invalid="ignore"):
        cep = dctm2(aspectrum.shape[0], numcep) @ np.log(aspectrum)
    return lifter_weights(numcep)[:, None] * cep


def melfcc(x, sr, wintime, hoptime, maxfreq, nbands, numcep):
    """tuneR::melfcc(spec_out = TRUE, frames_in_rows = FALSE): cepstra (numcep x nf),
    aspectrum (nbands x nf), pspectrum (nfft / 2 x nf)."""
    x = np.asarray(x, float)
    pre = x.copy()
    pre[1:] = x[1:] - 0.97 * x[:-1]
    P = powspec(pre, sr, wintime, hoptime)
    nfreqs = P.shape[0]
    nbands = int(nbands)
    wts = fft2melmx((nfreqs - 1) * 2, sr, nbands, 1.0, 0.0, maxfreq)[:, :nfreqs]
    A = wts @ P
    return {"cepstra": cepstra(A, numcep) if numcep else None, "aspectrum": A, "pspectrum": P}


# ---------------------------------------------------------------- integer decisions
def win_idx(ncol, win):
    """selfsim()'s window decisions for ncol frames: (win after the clamp to
    floor(ncol / 2) and the odd-making rule, 1-based winIdx)."""
    if win > ncol // 2:
        win = ncol // 2
    if win % 2 == 0:
        win = max(int(math.ceil(win / 2)) * 2 - 1, 1)
    numWins = int(math.ceil(ncol / win))
    idx = [_rround(v) for v in _r_seq_len(1.0, float(ncol - win), numWins)]
    return win, idx


def ssm_size(length, samplingRate, windowLength=40, overlap=75, step=None, ssmWin=40, kernelLen=200):
    """(n_frames, n, win, kernelSize) of ssm() for a sound of `length` samples
    (R/SSM.R:111-119, powspec's frame count, selfsim's windows); n_frames = n = 0
    for length <= 1 (R's length(x) > 1 test), win then the unclamped value."""
    sr = samplingRate
    if step is None:
        step = windowLength * (1 - overlap / 100)
    win = max(1, _rround(ssmWin / step / 2) * 2 - 1)
    frame_points = sr * windowLength / 1000
    kernelSize = _rround(kernelLen * sr / 1000 / frame_points / 2) * 2
    if length <= 1:
        return 0, 0, win, kernelSize
    winpts = _rround(windowLength / 1000 * sr)
    steppts = _rround(step / 1000 * sr)
    nf = int((length - winpts - 1) / steppts + 1e-10) + 1 if length > winpts else 1
    win, idx = win_idx(nf, win)
    return nf, len(idx), win, kernelSize


# ---------------------------------------------------------------- selfsim / novelty
def selfsim_raw(m, norm=False, simil="cosine", win=1):
    """selfsim() (R/SSM.R:224-262) before its final zeroOne: m is features x frames."""
    m = np.asarray(m, float)
    if m.ndim == 1:
        m = m[None, :]
    ncol = m.shape[1]
    win, idx = win_idx(ncol, int(win))
    if norm:
        m = np.stack([zero_one(m[:, j]) for j in range(ncol)], axis=1)
    V = np.stack([m[:, a - 1:a - 1 + win].T.ravel() for a in idx])  # frame after frame
    if simil == "cor":
        V = V - V.mean(axis=1, keepdims=True)
    elif simil != "cosine":
        raise ValueError("simil must be 'cosine' or 'cor'")
    G = V @ V.T
    nn = np.einsum("ij,ij->i", V, V)
    with np.errstate(invalid="ignore", divide="ignore"):
        return G / np.sqrt(nn[:, None] * nn[None, :])


def selfsim(m, norm=False, simil="cosine", win=1):
    """selfsim(), R/SSM.R:224-265."""
    return zero_one(selfsim_raw(m, norm, simil, win))


def get_checkerboard_kernel(size, kernel_mean=0.0, kernelSD=0.5):
    """getCheckerboardKernel(), R/SSM.R:281-324."""
    size = int(size)
    if size < 2:
        raise ValueError("getCheckerboardKernel: size must be >= 2")
    x = np.array(_r_seq_len(-1.0, 1.0, size))
    if size < 50:
        d = np.exp(-0.5 * ((x - kernel_mean) / kernelSD) ** 2) / (kernelSD * math.sqrt(2 * math.pi))
        k = d[:, None] * d[None, :]
    else:  # mvtnorm::dmvnorm(sigma = diag(2) * kernelSD): kernelSD as a variance
        q = (x - kernel_mean) ** 2 / kernelSD
        k = np.exp(-0.5 * (q[:, None] + q[None, :])) / (2 * math.pi * kernelSD)
    lo, hi = size // 2, (size + 1) // 2
    k[:lo, hi:] = -k[:lo, hi:]
    k[hi:, :hi] = -k[hi:, :hi]
    return k / k.max()


def get_novelty(ssm, kernelSize, kernelSD):
    """getNovelty(), R/SSM.R:337-360."""
    ssm = np.asarray(ssm, float)
    K = int(kernelSize)
    kern = get_checkerboard_kernel(K, kernelSD=kernelSD)
    n = ssm.shape[0]
    h = K // 2
    P = np.zeros((n + K, n + K))
    P[h:h + n, h:h + n] = ssm
    kv = kern.ravel() - kern.mean()
    kk = float(kv @ kv)
    out = np.zeros(n)
    for i in range(n):
        p = P[i:i + K, i:i + K].ravel()
        if np.isnan(p).any() or p.max() == p.min():
            continue  # cor() is NA: novelty[is.na(novelty)] = 0
        pv = p - p.mean()
        den = math.sqrt(float(pv @ pv) * kk)
        out[i] = float(pv @ kv) / den if den > 0 else 0.0
    return out


def novelty_patch_sd(ssm, kernelSize):
    """Standard deviation of every zero-padded K x K diagonal patch getNovelty
    correlates (a diagnostic: a near-constant patch makes its correlation round-off)."""
    ssm = np.asarray(ssm, float)
    K, n = int(kernelSize), ssm.shape[0]
    h = K // 2
    P = np.zeros((n + K, n + K))
    P[h:h + n, h:h + n] = ssm
    return np.array([P[i:i + K, i:i + K].std() for i in range(n)])


# ---------------------------------------------------------------- ssm
def read_wave(path):
    """tuneR::readWave of a mono 16-bit PCM file: (integer-valued samples, rate).
    The stdlib wave module reads plain PCM; the WAVE_FORMAT_EXTENSIBLE header that
    tuneR::writeWave (and write_wav) emits is refused by older versions of it,
    so that layout (PCM subformat) is parsed here."""
    try:
        with _wave.open(os.fspath(path), "rb") as w:
            nch, width, sr = w.getnchannels(), w.getsampwidth(), w.getframerate()
            raw = w.readframes(w.getnframes())
    except _wave.Error:
        nch, width, sr, raw = _read_extensible(path)
    if nch != 1 or width != 2:
        raise ValueError("ssm: only mono 16-bit PCM files are supported")
    return np.frombuffer(raw, dtype="<i2").astype(np.float64), sr


def _read_extensible(path):
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"RIFF" or b[8:12] != b"WAVE":
        raise ValueError("ssm: not a RIFF/WAVE file: %s" % (path,))
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(b):
        cid, size = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        body = b[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None or len(fmt) < 16:
        raise ValueError("ssm: no fmt / data chunk: %s" % (path,))
    tag, nch, sr, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]  # the subformat GUID's first two bytes
    if tag != 1:
        raise ValueError("ssm: only PCM files are supported")
    return nch, bits // 8, sr, data


def normalize32(x):
    """tuneR::normalize(unit = '32') up to its final integer scaling: centre, / max|x|."""
    x = np.asarray(x, float)
    x = x - x.mean()
    m = float(np.max(np.abs(x)))
    return x / m if m > 1.5e-8 else x  # !isTRUE(all.equal(m, 0))


def _input(x, samplingRate):
    """(samples, samplingRate, normalize flag) of ssm()'s x (R/SSM.R:100-110)."""
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        s, sr = read_wave(x)
        return s, sr, False
    s = np.asarray(x, dtype=np.float64).ravel()
    if len(s) <= 1:
        raise ValueError("ssm: x must be a file path or a numeric vector longer than 1")
    if samplingRate is None:
        raise ValueError("Please specify samplingRate, eg 44100")
    return s, samplingRate, True


def _settings(sr, windowLength, overlap, step, ssmWin, maxFreq, nBands, MFCC, input, simil, kernelLen, plot):
    if plot:
        raise NotImplementedError("ssm(plot = TRUE): plotting is out of scope")
    if input not in _INPUTS:
        raise ValueError("input must be one of %s" % (_INPUTS,))
    if simil not in _SIMILS:
        raise ValueError("simil must be 'cosine' or 'cor'")
    if step is None:
        step = windowLength * (1 - overlap / 100)
    if nBands is None:
        nBands = 100 * windowLength / 20
    if maxFreq is None:
        maxFreq = math.floor(sr / 2)
    mf = [int(v) for v in MFCC]
    if not mf or min(mf) < 1 or max(mf) > int(nBands) or max(mf) < 2:
        raise ValueError("MFCC indices must lie in 1..nBands, with max(MFCC) >= 2")
    return step, nBands, maxFreq, mf


def ssm_numpy(x, samplingRate=None, windowLength=40, overlap=75, step=None, ssmWin=40, maxFreq=None, nBands=None,
              MFCC=range(2, 14), input="mfcc", norm=False, simil="cosine", returnSSM=True, kernelLen=200,
              kernelSD=.2, plot=False, device=0):
    """ssm() (R/SSM.R:63-210) restated on the host: {'ssm', 'novelty'}. returnSSM =
    'raw' (no counterpart in R; the tests' conditioning checks) adds 'raw', the
    similarity before zeroOne, and 'kernelSize'."""
    s, sr, do_norm = _input(x, samplingRate)
    step, nBands, maxFreq, mf = _settings(sr, windowLength, overlap, step, ssmWin, maxFreq, nBands, MFCC, input,
                                          simil, kernelLen, plot)
    _, _, win, K = ssm_size(0, sr, windowLength, overlap, step, ssmWin, kernelLen)
    if K < 2:
        raise ValueError("ssm: kernelLen is shorter than two windows")
    if do_norm:
        s = normalize32(s)
    mel = melfcc(s, sr, windowLength / 1000, step / 1000, maxFreq, nBands, max(mf) if input == "mfcc" else 0)
    if input == "mfcc":
        target = mel["cepstra"][np.array(mf) - 1]
    elif input == "audiogram":
        target = mel["aspectrum"]
    else:
        target = mel["pspectrum"]
    raw = selfsim_raw(target, norm=norm, simil=simil, win=win)
    S = zero_one(raw)
    nov = get_novelty(S, K, kernelSD)
    if returnSSM == "raw":  # diagnostics: the similarity before zeroOne as well
        return {"ssm": S, "novelty": nov, "raw": raw, "kernelSize": K}
    return {"ssm": S, "novelty": nov} if returnSSM else {"novelty": nov}


# ------------------------------------------------------- on the GPU (sg_ssm.hip)
def _params(sr, windowLength, overlap, step, ssmWin, maxFreq, nBands, mf, input, norm, simil, kernelLen, kernelSD,
            normalize):
    from . import _abi
    nan = math.nan
    arr = (C.c_int32 * len(mf))(*mf)
    P = _abi.sg_ssm_params(float(sr), float(windowLength), float(overlap), nan if step is None else float(step),
                           float(ssmWin), nan if maxFreq is None else float(maxFreq),
                           nan if nBands is None else float(nBands), float(kernelLen), float(kernelSD),
                           C.cast(arr, C.POINTER(C.c_int32)), len(mf), _INPUTS.index(input), int(bool(norm)),
                           _SIMILS.index(simil), int(bool(normalize)))
    P._keep = arr
    return P


def ssm_size_native(length, samplingRate, windowLength=40, overlap=75, step=None, ssmWin=40, kernelLen=200):
    """sg_ssm_size (host only): the library's (n_frames, n, win, kernelSize)."""
    P = _params(samplingRate, windowLength, overlap, step, ssmWin, None, None, [2], "mfcc", False, "cosine",
                kernelLen, .2, True)
    o = [C.c_int32() for _ in range(4)]
    rc = native.lib().sg_ssm_size(int(length), C.byref(P), *[C.byref(v) for v in o])
    if rc < 0:
        raise native.SoundgenError(rc, "sg_ssm_size")
    return tuple(v.value for v in o)


def ssm(x, samplingRate=None, windowLength=40, overlap=75, step=None, ssmWin=40, maxFreq=None, nBands=None,
        MFCC=range(2, 14), input="mfcc", norm=False, simil="cosine", returnSSM=True, kernelLen=200, kernelSD=.2,
        plot=False, device=0):
    """ssm() (R/SSM.R:63-210) computed on the GPU (sg_ssm, fp64): {'ssm', 'novelty'}
    ('novelty' alone for returnSSM = False). x: a numeric vector with samplingRate,
    or the path of a mono 16-bit PCM file (not normalized, as in R)."""
    s, sr, do_norm = _input(x, samplingRate)
    _, _, _, mf = _settings(sr, windowLength, overlap, step, ssmWin, maxFreq, nBands, MFCC, input, simil, kernelLen,
                            plot)
    L = native.lib()
    ctx = native.default_context(device)
    P = _params(sr, windowLength, overlap, step, ssmWin, maxFreq, nBands, mf, input, norm, simil, kernelLen,
                kernelSD, do_norm)
    o = [C.c_int32() for _ in range(4)]
    native.check(L.sg_ssm_size(len(s), C.byref(P), *[C.byref(v) for v in o]), ctx.ptr)
    n = o[1].value
    s = np.ascontiguousarray(s)
    S = np.zeros(n * n) if returnSSM else None
    nov = np.zeros(n)
    dp = C.POINTER(C.c_double)
    native.check(L.sg_ssm(ctx.ptr, s.ctypes.data_as(dp), len(s), C.byref(P),
                          S.ctypes.data_as(dp) if returnSSM else None, nov.ctypes.data_as(dp)), ctx.ptr)
    return {"ssm": S.reshape(n, n).T, "novelty": nov} if returnSSM else {"novelty": nov}


def ssm_batch(data, offsets, lengths, samplingRate, windowLength=40, overlap=75, step=None, ssmWin=40, maxFreq=None,
              nBands=None, MFCC=range(2, 14), input="mfcc", norm=False, simil="cosine", returnSSM=False,
              kernelLen=200, kernelSD=.2, device=0):
    """ssm(x = call i, samplingRate, ...) for a batch of sounds already in HBM
    (`data`: a float32 CUDA tensor, call i at offsets[i], lengths[i] samples --
    the layout of batch.synthesize_packed), in one launch sequence
    (sg_ssm_batch). Returns the list of novelty vectors, and with returnSSM the
    list of matrices as well; a call of length <= 1 (failed or empty: R's
    length(x) > 1 test) gives empty arrays."""
    _, _, _, mf = _settings(samplingRate, windowLength, overlap, step, ssmWin, maxFreq, nBands, MFCC, input, simil,
                            kernelLen, False)
    L = native.lib()
    ctx = native.default_context(device)
    P = _params(samplingRate, windowLength, overlap, step, ssmWin, maxFreq, nBands, mf, input, norm, simil,
                kernelLen, kernelSD, True)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    ns = np.zeros(nc, dtype=np.int64)
    o = [C.c_int32() for _ in range(4)]
    for i in range(nc):
        native.check(L.sg_ssm_size(int(lens[i]), C.byref(P), *[C.byref(v) for v in o]), ctx.ptr)
        ns[i] = o[1].value
    noff, p_noff = native.out_offsets(ns)
    soff, p_soff = native.out_offsets(ns * ns)
    nov = np.zeros(max(int(noff[-1]), 1))
    S = np.zeros(max(int(soff[-1]), 1)) if returnSSM else None
    n_out = np.zeros(max(nc, 1), dtype=np.int32)
    dp = C.POINTER(C.c_double)
    native.check(L.sg_ssm_batch(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                n_out.ctypes.data_as(C.POINTER(C.c_int32)), nov.ctypes.data_as(dp),
                                p_noff, S.ctypes.data_as(dp) if returnSSM else None,
                                p_soff if returnSSM else None), ctx.ptr)
    if not np.array_equal(n_out[:nc], ns):
        raise native.SoundgenError(-1, "sg_ssm_batch: n_out disagrees with sg_ssm_size")
    novs = [nov[noff[i]:noff[i + 1]].copy() for i in range(nc)]
    if not returnSSM:
        return novs
    return novs, [S[soff[i]:soff[i + 1]].reshape(int(ns[i]), int(ns[i])).T.copy() for i in range(nc)]
