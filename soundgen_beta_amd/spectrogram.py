"""spectrogram(): STFT spectrogram and its denoising chain (R/spectrogram.R:94-276).

- spectrogram_numpy: the host restatement the GPU is compared against, restated
  from the sources, statement by statement:
    spectrogram()      R/spectrogram.R:94-276 (step :118, input :120-152, the FFT
                       :169-178, spectralDerivative :180-188, the rolling medians
                       :192-201, qTime :202-206, re-normalisation :209-213, noise
                       reduction :215-229, contrast / brightness :231-241, return :271-275)
    getFrameBank()     R/spectrogram.R:337-369 (normalisation :345-348, starts :350-351,
                       zero padding :355-367)
    ftwindow_modif()   R/spectrogram.R:288-304; gaussian.w :313-319
    seewave windows    seewave_2.0.5.tar.gz::seewave/R/seewave.r: bartlett.w :7293-7301,
                       blackman.w :7308-7314, flattop.w :7417-7424, hamming.w :7431-7437,
                       hanning.w :7444-7450, rectangle.w :7514-7519
    getEntropy()       R/utilities_math.R:143-161, the 'weiner' branch
    zoo::rollmedian    zoo_1.8-0.tar.gz::zoo/R/rollmean.R:193-226 (fill = 0)
    quantile (type 7)  R's stats::quantile.default: index = 1 + (n - 1) p, qs = x[lo],
                       interpolated only where index > lo and x[hi] != x[lo]
    seq(from, to, by)  R's seq.default: from + (0:n) by, n = as.integer((to - from) / by + 1e-10)
- Quirks kept (what the statements do, not what their comments say). z is bins x
  frames and Z = t(abs(z)) is frames x bins, so every apply(Z1, 1, ...) runs over
  one FRAME's spectrum:
    * smoothTime is a rolling median along frequency within a frame (:192-196),
      smoothFreq one along frames within a bin (:197-201);
    * qTime subtracts each frame's quantile over its bins (:202-206);
    * dZ_dt (:182) is the difference along bins, dZ_df (:184) along frames;
    * Z1 - noiseReduction * noise_spectrum (:225) recycles a length-nbins vector
      down the columns of a frames x bins matrix: cell (f, b) gets
      noise_spectrum[(f + b nframes) mod nbins] (0-based), not noise_spectrum[b];
    * rollmedian(fill = 0) writes 0 into the first and last k %/% 2 points and
      stops for k > length; an even k goes through runmed's "changing k" warning
      and a recycled assignment, which is NOT restated: even k > 1 raises ValueError;
    * when 1 + (n - 1) p is an integer the quantile is an element, x - q is exactly
      0 for it, and the nonpositives rule (:209-212) moves it to the floor;
    * frame starts are floor(seq(1, max(1, length - wl), step / 1000 * sr)): a
      fractional `by`, with seq's 1e-10 deciding the count at the boundary;
    * scale() only if min(sound) > 0, then / max|x| -- for a file as well (unlike
      ssm()); an all-zero sound is 0 / 0 and the result is all NaN;
    * zero padding by floor((zp - wl) / 2) * 2 points, only when positive; bins
      1 .. N / 2 are kept (DC in, Nyquist out);
    * ftwindow_modif accepts 'rectangle' (the roxygen text says "rectangular");
      seewave's flattop.w ends its sum at the 4 pi term (the next line of the
      source starts with a minus sign and is a statement of its own);
    * log first, then subtract the minimum log (:211-213); contrast defaults to
      .2, so the power step runs by default.
- spectrogram / spectrogram_batch: the same on the GPU (sg_spectrogram.hip, fp64
  throughout), one sound from the host or a packed batch already in HBM
  (batch.synthesize_packed's layout) whose matrices stay in HBM.

A matrix is returned bins x frames like R's t(Z) / t(Z1); the device keeps it
frame after frame (each frame's bins contiguous), which is R's column-major
memory image of that matrix.
"""
import ctypes as C
import math

import numpy as np

from . import native
from .ssm import read_wave

WINDOWS = ("bartlett", "blackman", "flattop", "hamming", "hanning", "rectangle", "gaussian")
_METHODS = ("spectrum", "spectralDerivative")
_OUTPUTS = ("original", "processed")


# ---------------------------------------------------------------- parts
def ft_window(wl, wn="gaussian"):
    """ftwindow_modif(wl, wn), R/spectrogram.R:288-304."""
    wl = int(wl)
    if wl < 4:
        raise ValueError("ft_window: wl must be >= 4")
    n = wl - 1
    i = np.arange(0, n + 1, dtype=float)
    if wn == "bartlett":
        m = n // 2
        return np.concatenate([(2 * np.arange(0, m, dtype=float)) / n,
                               2 - ((2 * np.arange(m, n + 1, dtype=float)) / n)])
    if wn == "blackman":
        return 0.42 - 0.5 * np.cos(2 * np.pi * i / n) + 0.08 * np.cos(4 * np.pi * i / n)
    if wn == "flattop":  # the source's sum ends here (see the module docstring)
        return 0.2156 - 0.4160 * np.cos(2 * np.pi * i / n) + 0.2781 * np.cos(4 * np.pi * i / n)
    if wn == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * i / n)
    if wn == "hanning":
        return 0.5 - 0.5 * np.cos(2 * np.pi * i / n)
    if wn == "rectangle":
        return np.ones(wl)
    if wn == "gaussian":
        j = np.arange(1, wl + 1, dtype=float)
        return (np.exp(-12 * ((j / wl) - 0.5) ** 2) - math.exp(-12)) / (1 - math.exp(-12))
    raise ValueError("wn must be one of %s" % (WINDOWS,))


def r_quantile(x, p):
    """quantile(x, probs = p), type 7 as R computes it."""
    x = np.sort(np.asarray(x, float))
    n = len(x)
    index = 1 + max(n - 1, 0) * p
    lo, hi = int(math.floor(index)), int(math.ceil(index))
    qs = x[lo - 1]
    if index > lo and x[hi - 1] != qs:
        h = index - lo
        qs = (1 - h) * qs + h * x[hi - 1]
    return qs


def _check_k(k, name):
    if k != int(k):
        raise ValueError("%s must be a whole number" % name)
    k = int(k)
    if k > 1 and k % 2 == 0:
        raise ValueError("%s must be odd: zoo::rollmedian's even-k path (runmed's warning and a recycled "
                         "assignment) is not restated" % name)
    return k


def roll_median(x, k, axis=-1):
    """zoo::rollmedian(x, k, fill = 0) along `axis`; k <= 1: x unchanged (the
    callers' `> 1` tests); even k and k > length raise."""
    x = np.asarray(x, float)
    k = _check_k(k, "k")
    if k <= 1:
        return x.copy()
    n = x.shape[axis]
    if k > n:
        raise ValueError("rollmedian: k = %d is larger than the series (%d)" % (k, n))
    h = k // 2
    xs = np.moveaxis(x, axis, -1)
    out = np.zeros_like(xs)
    win = np.lib.stride_tricks.sliding_window_view(xs, k, axis=-1)
    out[..., h:n - h] = np.median(win, axis=-1)  # odd k: the middle element itself
    return np.moveaxis(out, -1, axis)


def get_entropy(x):
    """getEntropy(x, type = 'weiner'), R/utilities_math.R:143-161; NaN for R's NA."""
    x = np.asarray(x, float)
    if np.sum(x) == 0:
        return math.nan
    x = np.where(x <= 0, 1e-10, x)
    return math.exp(np.mean(np.log(x))) / np.mean(x)


def _step(windowLength, step, overlap):
    return windowLength * (1 - overlap / 100) if step is None else step


def frame_starts(length, samplingRate, wl, step):
    """0-based first sample of every frame: floor(seq(1, max(1, length - wl),
    step / 1000 * samplingRate)) - 1 (R/spectrogram.R:350-351; indexing truncates)."""
    frm, to = 1.0, float(max(1, length - wl))
    by = step / 1000 * samplingRate
    if not by > 0:
        raise ValueError("step must be > 0")
    n = int((to - frm) / by + 1e-10)
    seq = np.minimum(frm + np.arange(0, n + 1, dtype=float) * by, to)
    return np.floor(seq).astype(np.int64) - 1


def spectrogram_size(length, samplingRate, windowLength=50, step=None, overlap=70, zp=0):
    """(wl, N, bins, frames) of spectrogram() for a sound of `length` samples: the
    window in points, the FFT length after zero padding, N / 2 bins, and the frame
    count (0 for length <= 1 or a sound shorter than the window)."""
    step = _step(windowLength, step, overlap)
    wl = int(math.floor(windowLength / 1000 * samplingRate / 2) * 2)
    zpExtra = int(math.floor((zp - wl) / 2) * 2)
    N = wl + max(zpExtra, 0)
    if length <= 1 or length < wl:
        return wl, N, N // 2, 0
    return wl, N, N // 2, len(frame_starts(length, samplingRate, wl, step))


def normalize_sound(sound):
    """getFrameBank's normalisation, R/spectrogram.R:345-348."""
    s = np.asarray(sound, float)
    if s.min() > 0:  # scale(): centre, / sd with n - 1
        c = s - s.mean()
        s = c / math.sqrt(np.sum(c * c) / (len(s) - 1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / max(abs(s.max()), abs(s.min()))


def get_frame_bank(sound, samplingRate, windowLength_points, wn, step, zp):
    """getFrameBank(), R/spectrogram.R:337-369: N x frames."""
    wl = int(windowLength_points)
    sound = np.asarray(sound, float)
    if len(sound) < wl:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    s = normalize_sound(sound)
    starts = frame_starts(len(s), samplingRate, wl, step)
    filt = ft_window(wl, wn)
    zpExtra = int(math.floor((zp - wl) / 2) * 2)
    half = zpExtra // 2 if zpExtra > 0 else 0
    bank = np.zeros((wl + 2 * half, len(starts)))
    for j, a in enumerate(starts):
        bank[half:half + wl, j] = s[a:a + wl] * filt
    return bank


# ------------------------------------------------ the chain, on Z1 = frames x bins
def spectral_derivative(Z):
    """:180-185. dZ_dt differs along bins, dZ_df along frames (see the docstring)."""
    dZ_dt = np.hstack([np.zeros((Z.shape[0], 1)), np.diff(Z, axis=1)])
    dZ_df = np.vstack([np.zeros((1, Z.shape[1])), np.diff(Z, axis=0)])
    return np.sqrt(dZ_dt ** 2 + dZ_df ** 2)


def smooth_time(Z1, k):
    """:192-196: t(apply(Z1, 1, rollmedian)) -- along the bins of each frame."""
    return roll_median(Z1, k, axis=1)


def smooth_freq(Z1, k):
    """:197-201: apply(Z1, 2, rollmedian) -- along the frames of each bin."""
    return roll_median(Z1, k, axis=0)


def subtract_qtime(Z1, q):
    """:202-206: each frame minus the quantile of its own bins."""
    return np.stack([row - r_quantile(row, q) for row in Z1])


def renormalize(Z1):
    """:209-213: log of the positives, the rest at the smallest log, minus the minimum."""
    Z1 = np.array(Z1, float)
    pos = Z1 > 0
    nonpos = Z1 <= 0
    Z1[pos] = np.log(Z1[pos])
    Z1[nonpos] = Z1[pos].min() if pos.any() else math.inf
    return Z1 - Z1.min()  # min() without na.rm: one NaN makes the matrix NaN


def noise_frames(Z1, percentNoise):
    """:217-221: (entropy per frame, its quantile, the selected frames)."""
    entr = np.array([get_entropy(row) for row in Z1])
    ok = entr[~np.isnan(entr)]
    if len(ok) == 0:
        return entr, math.nan, np.zeros(0, dtype=np.int64)
    q = r_quantile(ok, 1 - percentNoise / 100)
    with np.errstate(invalid="ignore"):
        return entr, q, np.nonzero(entr >= q)[0]


def subtract_noise(Z1, noise_spectrum, noiseReduction):
    """:225: the vector recycles down the columns of the frames x bins matrix."""
    nf, nb = Z1.shape
    f, b = np.meshgrid(np.arange(nf), np.arange(nb), indexing="ij")
    return Z1 - (noiseReduction * np.asarray(noise_spectrum, float))[(f + b * nf) % nb]


def denoise(Z, smoothFreq=0, smoothTime=0, qTime=0, percentNoise=10, noiseReduction=0, contrast=.2, brightness=0,
            method="spectrum"):
    """:164-165, :180-241 on Z (frames x bins): Z1, frames x bins."""
    if method not in _METHODS:
        raise ValueError("method must be one of %s" % (_METHODS,))
    contrast_exp = math.exp(3 * contrast)
    brightness_exp = math.exp(3 * brightness)
    Z1 = spectral_derivative(Z) if method == "spectralDerivative" else np.array(Z, float)
    if smoothTime > 1:
        Z1 = smooth_time(Z1, smoothTime)
    if smoothFreq > 1:
        Z1 = smooth_freq(Z1, smoothFreq)
    if qTime > 0:
        Z1 = subtract_qtime(Z1, qTime)
    with np.errstate(invalid="ignore", divide="ignore"):
        Z1 = renormalize(Z1)
        if noiseReduction > 0:
            _, _, idx = noise_frames(Z1, percentNoise)
            if len(idx) > 0:
                Z1 = subtract_noise(Z1, Z1[idx].mean(axis=0), noiseReduction)
            Z1 = np.where(Z1 <= 0, 0.0, Z1)
        if contrast_exp != 1:
            Z1 = Z1 ** contrast_exp
        Z1 = Z1 / Z1.max()
        if brightness_exp != 1:
            Z1 = Z1 / brightness_exp
        if brightness_exp < 1:
            Z1 = np.where(Z1 > 1, 1.0, Z1)
    return Z1


# ---------------------------------------------------------------- spectrogram
def _input(x, samplingRate):
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        return read_wave(x)
    s = np.asarray(x, dtype=np.float64).ravel()
    if len(s) <= 1:
        raise ValueError("spectrogram: x must be a file path or a numeric vector longer than 1")
    if samplingRate is None:
        raise ValueError("Please specify samplingRate, eg 44100")
    return s, samplingRate


def _settings(wn, smoothFreq, smoothTime, method, output, plot, osc):
    if plot or osc:
        raise NotImplementedError("spectrogram(plot = TRUE / osc = TRUE): plotting is out of scope")
    if output not in _OUTPUTS:
        raise NotImplementedError("spectrogram(output = %r): only 'original' and 'processed' return a matrix"
                                  % (output,))
    if wn not in WINDOWS:
        raise ValueError("wn must be one of %s" % (WINDOWS,))
    if method not in _METHODS:
        raise ValueError("method must be one of %s" % (_METHODS,))
    return _check_k(smoothFreq, "smoothFreq"), _check_k(smoothTime, "smoothTime")


def spectrogram_numpy(x, samplingRate=None, windowLength=50, step=None, overlap=70, wn="gaussian", zp=0, smoothFreq=0,
                      smoothTime=0, qTime=0, percentNoise=10, noiseReduction=0, contrast=.2, brightness=0,
                      method="spectrum", output="processed", plot=False, osc=False):
    """spectrogram() (R/spectrogram.R:94-276) restated on the host: bins x frames."""
    s, sr = _input(x, samplingRate)
    _settings(wn, smoothFreq, smoothTime, method, output, plot, osc)
    step = _step(windowLength, step, overlap)
    wl = int(math.floor(windowLength / 1000 * sr / 2) * 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        bank = get_frame_bank(s, sr, wl, wn, step, zp)
        z = np.fft.fft(bank, axis=0)[:bank.shape[0] // 2]
        Z = np.abs(z).T
    if output == "original":
        return Z.T
    return denoise(Z, smoothFreq, smoothTime, qTime, percentNoise, noiseReduction, contrast, brightness, method).T


# ------------------------------------------------------- on the GPU (sg_spectrogram.hip)
def _params(sr, windowLength, step, overlap, wn, zp, smoothFreq, smoothTime, qTime, percentNoise, noiseReduction,
            contrast, brightness, method, output):
    from . import _abi
    return _abi.sg_spectrogram_params(float(sr), float(windowLength), math.nan if step is None else float(step),
                                      float(overlap), float(zp), float(smoothFreq), float(smoothTime), float(qTime),
                                      float(percentNoise), float(noiseReduction), float(contrast), float(brightness),
                                      WINDOWS.index(wn), _METHODS.index(method), _OUTPUTS.index(output), 0)


def _size(L, P, length):
    o = [C.c_int32() for _ in range(4)]
    rc = L.sg_spectrogram_size(int(length), C.byref(P), *[C.byref(v) for v in o])
    native.host_check(rc, L.sg_spectrogram_size_error)
    return tuple(v.value for v in o)


def spectrogram_size_native(length, samplingRate, windowLength=50, step=None, overlap=70, zp=0):
    """sg_spectrogram_size (host only): the library's (wl, N, bins, frames). Raises
    SoundgenError (SG_E_UNSUPPORTED) for an FFT length the device transform lacks."""
    P = _params(samplingRate, windowLength, step, overlap, "gaussian", zp, 0, 0, 0, 10, 0, .2, 0, "spectrum",
                "processed")
    return _size(native.lib(), P, length)


def _check_extent(kF, kT, bins, frames, what=""):
    if kT > 1 and kT > bins:
        raise ValueError("rollmedian: smoothTime = %d is larger than the %d bins of a frame" % (kT, bins))
    if kF > 1 and kF > frames:
        raise ValueError("rollmedian: smoothFreq = %d is larger than the %d frames%s" % (kF, frames, what))


def spectrogram(x, samplingRate=None, windowLength=50, step=None, overlap=70, wn="gaussian", zp=0, smoothFreq=0,
                smoothTime=0, qTime=0, percentNoise=10, noiseReduction=0, contrast=.2, brightness=0,
                method="spectrum", output="processed", plot=False, osc=False, device=0):
    """spectrogram() (R/spectrogram.R:94-276) computed on the GPU (sg_spectrogram,
    fp64): bins x frames. x: a numeric vector with samplingRate, or the path of a
    mono 16-bit PCM file (normalized like a vector, as in R)."""
    s, sr = _input(x, samplingRate)
    kF, kT = _settings(wn, smoothFreq, smoothTime, method, output, plot, osc)
    L = native.lib()
    P = _params(sr, windowLength, step, overlap, wn, zp, smoothFreq, smoothTime, qTime, percentNoise, noiseReduction,
                contrast, brightness, method, output)
    wl, _, bins, frames = _size(L, P, len(s))
    if len(s) < wl:
        raise ValueError("the sound is shorter than the window (R indexes past its end: NA)")
    if output == "processed":
        _check_extent(kF, kT, bins, frames)
    ctx = native.default_context(device)
    s = np.ascontiguousarray(s)
    out = np.zeros(bins * frames)
    dp = C.POINTER(C.c_double)
    native.check(L.sg_spectrogram(ctx.ptr, s.ctypes.data_as(dp), len(s), C.byref(P), out.ctypes.data_as(dp)), ctx.ptr)
    return out.reshape(frames, bins).T


def spectrogram_batch(data, offsets, lengths, samplingRate, windowLength=50, step=None, overlap=70, wn="gaussian",
                      zp=0, smoothFreq=0, smoothTime=0, qTime=0, percentNoise=10, noiseReduction=0, contrast=.2,
                      brightness=0, method="spectrum", output="processed", to_host=False, device=0):
    """spectrogram(x = call i, samplingRate, ...) for a batch of sounds already in
    HBM (`data`: a float32 CUDA tensor, call i at offsets[i], lengths[i] samples --
    the layout of batch.synthesize_packed), in one launch sequence
    (sg_spectrogram_batch). The matrices stay in HBM: returns (out, out_offsets,
    shapes) with `out` an fp64 CUDA tensor, call i's matrix at out_offsets[i] as
    shapes[i] = (bins, frames), stored frame after frame (out[o:o + bins * frames]
    .view(frames, bins).T is bins x frames). to_host=True returns the list of
    bins x frames arrays instead. A call with lengths[i] <= 1 or shorter than the
    window has 0 frames."""
    kF, kT = _settings(wn, smoothFreq, smoothTime, method, output, False, False)
    L = native.lib()
    P = _params(samplingRate, windowLength, step, overlap, wn, zp, smoothFreq, smoothTime, qTime, percentNoise,
                noiseReduction, contrast, brightness, method, output)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    shapes = []
    for i in range(nc):
        _, _, bins, frames = _size(L, P, int(lens[i]))
        if frames and output == "processed":
            _check_extent(kF, kT, bins, frames, " of call %d" % i)
        shapes.append((bins, frames))
    ooff, p_ooff = native.out_offsets([b * f for b, f in shapes])
    ctx = native.default_context(device)
    bo = np.zeros(max(nc, 1), dtype=np.int32)
    fo = np.zeros(max(nc, 1), dtype=np.int32)
    i32p = C.POINTER(C.c_int32)
    out = native.device_out(data, ooff[-1])
    native.check(L.sg_spectrogram_batch(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                        C.c_void_p(out.data_ptr()), p_ooff, bo.ctypes.data_as(i32p),
                                        fo.ctypes.data_as(i32p)), ctx.ptr)
    if [(int(b), int(f)) for b, f in zip(bo[:nc], fo[:nc])] != shapes:
        raise native.SoundgenError(-1, "sg_spectrogram_batch: shapes disagree with sg_spectrogram_size")
    if not to_host:
        return out, ooff[:-1].copy(), shapes
    h = out.cpu().numpy()
    return [h[ooff[i]:ooff[i + 1]].reshape(shapes[i][1], shapes[i][0]).T.copy() for i in range(nc)]
