"""segment(): syllables and vocal bursts from the smoothed Hilbert envelope of a sound
(R/segment.R:79-219, R/utilities_segment.R), restated in numpy statement by statement
(segment_numpy and its pieces: the oracle of the feature) and computed on the GPU
(segment, segment_batch, hilbert_envelope: sg_segment.hip, fp64).

The envelope is seewave::env(envt = "hil", msmooth = c(windowLength_points, overlap))
(seewave_2.0.5.tar.gz::seewave/R/seewave.r:2457-2541) over seewave::hilbert
(:3328-3367): a Hilbert transform of the whole sound zero-padded to a power of two.

Quirks of the reference that change the numbers, all kept (tests/test_segment.py pins
each by hand):
  * scale() (centre, then sqrt(sum(x^2) / (n - 1))) only for min(sound) > 0, then the
    division by max(|max|, |min|) (segment.R:119-123);
  * windowLength_points = ceiling(windowLength * samplingRate / 1000), replaced by
    length / 2 when larger: it may end in .5 (:127-130);
  * hilbert pads floor(nzp / 2) zeros on the left and ceiling(nzp / 2) on the right;
    h is 1 at 1 and n / 2 + 1, 2 at 2 ... n / 2, 0 above (h[2:(n / 2)] with n = 2 is
    h[c(2, 1)]: both become 2); the un-padding ht[floor(diffn / 2):(n1 + floor(diffn /
    2) - 1)] starts one sample early, so the envelope's first value lies in the padding
    and the sound's last sample is dropped; for diffn == 1 the index 0 is dropped
    silently: n1 - 1 values, which then line up with the sound again (the dropped
    index cancels the early start), the last sample still missing; env keeps n = n1;
  * msmooth: step = seq(1, n - wl, wl - ov * wl / 100) with a fractional `by` and seq's
    1e-10; each value is mean(wave[x:(x + wl)]): trunc(|(x + wl) - x| + 1 + FLT_EPSILON)
    points (wl + 1 for a whole wl), from a fractional x, the indices truncated -- and
    where x is a rounding error below a whole number, x + j is too until the sum rounds
    to the whole number: the window then skips one value (_window_indices);
  * timestep = 1000 / samplingRate * (length(sound) / length(envelope));
  * findSyllables: runs of value > threshold kept if count > ceiling(shortestSyl /
    timestep), strictly; start = sum(count[1:(idx - 1)]) * timestep, where 1:0 is
    c(1, 0) (idx == 1 sums count[1]); the first KEPT syllable starts at 0 whenever the
    envelope begins above the threshold, even when that first run itself was too short
    to be kept; mergeSyllables' inner `&` reads row i + 1 past the end as NA (NA & FALSE
    is FALSE: harmless); pauseLen of the last syllable is NA; no syllable: one row
    syllable = 0, NA elsewhere, a `dur` column instead of sylLen / pauseLen;
  * interburst = median(sylLen) * interburstMult, or shortestSyl without a syllable;
  * findBursts: n = floor(interburst / timestep); the left rule is i > n, the right one
    i < nrow - n - 1; local_min = 0 outside (the ratio is Inf); every point of a plateau
    that ties the window's maximum is a burst; time = i * timestep with 1-based i;
    interburstInt of the last burst is NA;
  * summary: nSyl = nrow(syllables) (1 without a syllable); pauseLen_sd = sd(pauseLen)
    has no na.rm and the last pauseLen is NA: it is always NA; NaN becomes NA.
NA and NaN are both NaN here. What the sources cannot settle without an R interpreter
(mean / median / sd of the column a frame lacks: sylLen and pauseLen without a syllable,
interburstInt without a burst) is NaN as well: DESIGN.md section 8 lists the cases.

Sums: R's mean() is a long double sum, divided, plus one refinement pass over x - mean.
r_mean restates that in np.longdouble (numpy adds pairwise where R adds in order: below
the last bit of a double either way). The GPU adds in fp64 in a fixed order
(sg_segment.hip) and is compared with a tolerance.
"""
import ctypes as C
import math

import numpy as np

from . import native

SUMMARY_COLUMNS = ("nSyl", "sylLen_mean", "sylLen_median", "sylLen_sd", "pauseLen_mean", "pauseLen_median",
                   "pauseLen_sd", "nBursts", "interburst_mean", "interburst_median", "interburst_sd")
SYLLABLE_COLUMNS = ("syllable", "start", "end", "sylLen", "pauseLen")
BURST_COLUMNS = ("time", "ampl", "interburstInt")
MAX_LOG2 = 22  # the longest transform of the device path: 2^22 points
FLT_EPSILON = 1.1920928955078125e-07
HEAD = 8  # cells of a sound's device output in front of the summary row (sg_segment.h)
_LD = np.longdouble


# --------------------------------------------------------------------- R's arithmetic
def r_seq_by(frm, to, by):
    """seq.default(from, to, by), by > 0: from + (0:n) * by, n = as.integer((to - from) /
    by + 1e-10), pmin(to) (sg_rmath.h r_seq_by is the same statement for the planner)."""
    d = to - frm
    if d == 0.0 and to == 0.0:
        return np.array([to])
    if abs(d) / max(abs(to), abs(frm)) < 100 * 2.220446049250313e-16:
        return np.array([frm])
    nn = d / by
    if nn < 0:
        return np.zeros(0)
    n = int(nn + 1e-10)
    return np.minimum(frm + np.arange(0, n + 1, dtype=np.float64) * by, to)


def r_mean(v):
    """mean.default of a double vector (summary.c rsum / real_mean): NaN for length 0."""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    if n == 0:
        return math.nan
    ld = v.astype(_LD)
    s = ld.sum() / n
    if np.isfinite(s):
        s = s + (ld - s).sum() / n
    return float(s)


def r_median(v):
    """median.default without NA: the middle of sort(), or the mean of the middle two."""
    v = np.sort(np.asarray(v, dtype=np.float64))
    n = len(v)
    if n == 0:
        return math.nan
    h = (n + 1) // 2
    return float(v[h - 1]) if n % 2 else r_mean(v[h - 1:h + 1])


def r_sd(v):
    """sd(): cov.c's two-pass variance in long double (the mean refined once), n - 1."""
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    if n < 2 or np.isnan(v).any():
        return math.nan
    ld = v.astype(_LD)
    m = ld.sum() / n
    m = m + (ld - m).sum() / n
    return float(np.sqrt(((ld - m) ** 2).sum() / (n - 1)))


# ---------------------------------------------------------------------- the envelope
def normalize(sound):
    """segment.R:119-123."""
    s = np.asarray(sound, dtype=np.float64)
    if s.min() > 0:  # scale(): x - colMeans(x), then / sqrt(sum(x^2) / max(1, n - 1))
        n = len(s)
        s = s - float(s.astype(_LD).sum() / n)
        s = s / math.sqrt(float((s.astype(_LD) ** 2).sum()) / max(1, n - 1))
    return s / max(abs(s.max()), abs(s.min()))


def window_points(n, samplingRate, windowLength):
    """windowLength_points (segment.R:127-130): a double, possibly ending in .5."""
    wl = float(math.ceil(windowLength * samplingRate / 1000))
    return n / 2 if wl > n / 2 else wl


def hilbert_layout(n1):
    """(N, left zeros, shift, n_env) of hilbert()'s padding and un-padding for n1 samples:
    the envelope's value k (0-based) is |ht[shift + k]| of the padded transform."""
    if n1 < 1:
        raise ValueError("hilbert: empty wave")
    N = 1 << (n1 - 1).bit_length()  # 2^ceiling(log2(n)); n itself when log2(n) is whole
    diffn = N - n1
    left = diffn // 2
    if diffn == 0:
        return N, 0, 0, n1
    if left == 0:  # diffn == 1: ht[0:(n1 - 1)], the 0 dropped
        return N, 0, 0, n1 - 1
    return N, left, left - 1, n1


def hilbert_multiplier(n):
    """h of hilbert() (:3349-3356) for an even n."""
    h = np.zeros(n)
    h[[0, n // 2]] = 1
    lo, hi = 2, n // 2  # h[2:(n/2)] <- 2; 2:1 counts down
    idx = np.arange(lo, hi + 1) if hi >= lo else np.arange(lo, hi - 1, -1)
    h[idx - 1] = 2
    return h


def hilbert_envelope_numpy(x):
    """Mod(seewave::hilbert(x)) (:3328-3367), un-padded by the reference's rule."""
    w = np.asarray(x, dtype=np.float64).ravel()
    n1 = len(w)
    N, left, _, _ = hilbert_layout(n1)
    if N != n1:
        w = np.concatenate([np.zeros(left), w, np.zeros(N - n1 - left)])
    ht = np.fft.ifft(np.fft.fft(w) * hilbert_multiplier(N))  # fft(fft(wave) * h, inverse = TRUE) / n
    diffn = N - n1
    if diffn > 0:
        idx = np.arange(diffn // 2, n1 + diffn // 2 - 1 + 1)  # 1-based; a 0 selects nothing
        ht = ht[idx[idx > 0] - 1]
    return np.abs(ht)


def _window_indices(step, c):
    """1-based indices of wave[x:(x + wl)] for every x of `step`, c points each: from:to is
    from + 0, from + 1, ... in fp64 (seq.c seq_colon), and the index truncates. A from just
    below a whole number (1 + i * by rounds) gives from + j just below one too until the sum
    rounds to the whole number itself: from there on the indices are one further, and the
    window skips one value."""
    return (step[:, None] + np.arange(c, dtype=np.float64)[None, :]).astype(np.int64)


def smoothing_windows(n, n_env, wl, overlap):
    """env()'s msmooth windows (:2489-2498) for a wave of n rows whose envelope has n_env
    values: (0-based first index, points, jump) of every window x:(x + wl); point j of a
    window is the envelope's value first + j, and first + j + 1 from j = jump on (jump =
    points: no skipped value)."""
    if wl == 0 or wl == 1:
        raise ValueError("'smooth' window length cannot be equal to %d" % wl)
    step = r_seq_by(1.0, n - wl, wl - (overlap * wl / 100))
    to = step + wl
    cnt = (np.abs(to - step) + 1 + FLT_EPSILON).astype(np.int64)  # length of from:to (seq.c seq_colon)
    first = step.astype(np.int64)  # x[as.integer(...)]: truncation
    jump = cnt.copy()
    for c in np.unique(cnt):
        rows = np.nonzero(cnt == c)[0]
        for a in range(0, len(rows), 4096):
            r = rows[a:a + 4096]
            off = _window_indices(step[r], int(c)) - first[r, None] - np.arange(int(c))[None, :]
            if off.min() < 0 or off.max() > 1 or (np.diff(off, axis=1) < 0).any():
                raise NotImplementedError("a smoothing window that skips more than one value")
            jump[r] = np.where(off.max(axis=1) > 0, off.argmax(axis=1), c)
    if (first + cnt - 1 + (jump < cnt)).max(initial=0) > n_env:
        raise ValueError("a smoothing window leaves the envelope (NA in R)")
    return first - 1, cnt, jump


def env_msmooth(env, n, wl, overlap):
    """wave <- apply(as.matrix(step), 1, function(x) mean(wave[x:(x + msmooth[1])]))."""
    env = np.asarray(env, dtype=np.float64)
    first, cnt, _ = smoothing_windows(n, len(env), wl, overlap)
    step = r_seq_by(1.0, n - wl, wl - (overlap * wl / 100))
    out = np.zeros(len(first))
    ld = env.astype(_LD)
    for c in np.unique(cnt):  # one count in practice
        rows = np.nonzero(cnt == c)[0]
        for a in range(0, len(rows), 1024):
            r = rows[a:a + 1024]
            w = ld[_window_indices(step[r], int(c)) - 1]
            s = w.sum(axis=1) / int(c)
            s = s + (w - s[:, None]).sum(axis=1) / int(c)
            out[r] = s.astype(np.float64)
    return out


def hilbert_envelope_smoothed(sound, samplingRate, windowLength, overlap):
    """segment.R:119-140: (envelope values, timestep in ms)."""
    s = normalize(sound)
    n = len(s)
    wl = window_points(n, samplingRate, windowLength)
    v = env_msmooth(hilbert_envelope_numpy(s), n, wl, overlap)
    return v, 1000 / samplingRate * (n / len(v))


# -------------------------------------------------------------- syllables and bursts
def _rle(a):
    a = np.asarray(a)
    cut = np.nonzero(a[1:] != a[:-1])[0] + 1
    b = np.concatenate([[0], cut, [len(a)]])
    return a[b[:-1]], np.diff(b)


def _margin(trace, key, value, ref):
    if trace is not None and np.isfinite(value) and ref != 0:
        m = abs(value - ref) / abs(ref)
        trace[key] = min(trace.get(key, math.inf), m)


def merge_syllables(start, end, shortestPause, _trace=None):
    """mergeSyllables (utilities_segment.R:80-91) on the start / end columns."""
    start, end = list(start), list(end)
    i = 1
    while i < len(start):
        while True:
            inside = i < len(start)
            # start[i + 1] past the end is NA: NA < shortestPause is NA, NA & FALSE is FALSE
            gap = start[i] - end[i - 1] if inside else math.nan
            if inside:
                _margin(_trace, "merge", gap, shortestPause)
            if not (inside and gap < shortestPause):
                break
            end[i - 1] = end[i]
            del start[i], end[i]
        i += 1
    return np.array(start, dtype=np.float64), np.array(end, dtype=np.float64)


def find_syllables(value, timestep, threshold, shortestSyl, shortestPause, mergeSyl, _trace=None):
    """findSyllables (utilities_segment.R:18-69): a dict of columns."""
    value = np.asarray(value, dtype=np.float64)
    if _trace is not None:
        for v in value:
            _margin(_trace, "threshold", v, threshold)
        q = shortestSyl / timestep
        if q != 0:
            _trace["count"] = min(_trace.get("count", math.inf), abs(q - round(q)) / q if q != round(q) else math.inf)
    val, count = _rle((value > threshold).astype(np.int64))
    keep = np.nonzero((val == 1) & (count > math.ceil(shortestSyl / timestep)))[0]
    nan = math.nan
    if len(keep) == 0:
        return {"syllable": np.array([0.0]), "start": np.array([nan]), "end": np.array([nan]), "dur": np.array([nan])}
    start = np.zeros(len(keep))
    for k, idx0 in enumerate(keep):
        idx = idx0 + 1  # 1-based; 1:(idx - 1) with idx == 1 is c(1, 0): count[1]
        sel = count[:idx - 1] if idx >= 2 else count[:1]
        start[k] = int(sel.sum()) * timestep
    if val[0] == 1:
        start[0] = 0
    end = start + count[keep] * timestep
    if mergeSyl:
        start, end = merge_syllables(start, end, shortestPause, _trace)
    sylLen = end - start
    pauseLen = np.full(len(start), nan)
    pauseLen[:-1] = start[1:] - end[:-1]
    return {"syllable": np.arange(1, len(start) + 1, dtype=np.float64), "start": start, "end": end, "sylLen": sylLen,
            "pauseLen": pauseLen}


def find_bursts(value, timestep, interburst, burstThres, peakToTrough, troughLeft=True, troughRight=False,
                _trace=None):
    """findBursts (utilities_segment.R:104-177): a dict of columns (no interburstInt column
    when there is no burst, as in R)."""
    if isinstance(interburst, bool) or not isinstance(interburst, (int, float, np.integer, np.floating)):
        raise ValueError("interburst is weird: %r" % (interburst,))
    if interburst < 0:
        raise ValueError("interburst is negative")
    v = np.asarray(value, dtype=np.float64)
    N = len(v)
    n = int(math.floor(interburst / timestep))
    vmax = v.max()
    time, ampl = [], []
    for i in range(1, N + 1):
        left, right = i > n, i < N - n - 1
        lml = v[i - n - 1:i].min() if left else 0.0
        lmr = v[i - 1:i + n].min() if right else 0.0
        ll = i - n if left else 1
        lr = i + n if right else N
        cond1 = v[i - 1] == v[ll - 1:lr].max()
        with np.errstate(divide="ignore", invalid="ignore"):
            r2 = v[i - 1] / vmax
            r3l = np.float64(v[i - 1]) / lml
            r3r = np.float64(v[i - 1]) / lmr
        if cond1:  # the margins that matter: a point that is no local maximum is no burst either way
            _margin(_trace, "cond2", r2, burstThres)
            if troughLeft:
                _margin(_trace, "cond3", r3l, peakToTrough)
            if troughRight:
                _margin(_trace, "cond3", r3r, peakToTrough)
        if cond1 and r2 > burstThres and (r3l > peakToTrough if troughLeft else True) and \
                (r3r > peakToTrough if troughRight else True):
            time.append(i * timestep)
            ampl.append(v[i - 1])
    out = {"time": np.array(time, dtype=np.float64), "ampl": np.array(ampl, dtype=np.float64)}
    if time:
        ib = np.full(len(time), math.nan)
        ib[:-1] = np.diff(out["time"])
        out["interburstInt"] = ib
    return out


def segment_summary(syllables, bursts):
    """The eleven columns of segment.R:194-212, NaN for NA."""
    nan = math.nan
    sl, pl, ib = syllables.get("sylLen"), syllables.get("pauseLen"), bursts.get("interburstInt")
    nS, nB = len(syllables["syllable"]), len(bursts["time"])
    pl_ok = None if pl is None else pl[~np.isnan(pl)]
    ib_ok = None if ib is None else ib[~np.isnan(ib)]
    r = {
        "nSyl": nS,
        "sylLen_mean": nan if sl is None else r_mean(sl),
        "sylLen_median": nan if sl is None else r_median(sl),
        "sylLen_sd": nan if sl is None else r_sd(sl),
        "pauseLen_mean": nan if pl is None else r_mean(pl_ok),
        "pauseLen_median": r_median(pl_ok) if nS > 1 and pl is not None else nan,
        "pauseLen_sd": nan if pl is None else r_sd(pl),  # no na.rm: the last pauseLen is NA
        "nBursts": nB,
        "interburst_mean": nan if ib is None else r_mean(ib_ok),
        "interburst_median": r_median(ib_ok) if nB > 0 and ib is not None else nan,
        "interburst_sd": nan if ib is None else r_sd(ib_ok),
    }
    return r


def _repair(x, samplingRate, windowLength, overlap, shortestPause, interburst, plot, savePath):
    if plot or isinstance(savePath, str):
        raise NotImplementedError("segment(plot = TRUE / savePath): plotting is out of scope")
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        raise NotImplementedError("segment(x = a file name): reading files is out of scope; pass the samples")
    s = np.asarray(x, dtype=np.float64).ravel()
    if len(s) <= 1:
        raise ValueError("segment: x must be a numeric vector longer than 1")
    if samplingRate is None:
        raise ValueError("Please specify samplingRate, eg 44100")
    if interburst is not None:
        if isinstance(interburst, bool) or not isinstance(interburst, (int, float, np.integer, np.floating)):
            raise ValueError("interburst is weird: %r" % (interburst,))
        if interburst < 0:
            raise ValueError("interburst is negative")
    overlap = min(max(overlap, 0), 99)
    mergeSyl = not (shortestPause is None or (isinstance(shortestPause, float) and math.isnan(shortestPause)))
    return s, overlap, mergeSyl


def segment_numpy(x, samplingRate=None, windowLength=40, overlap=80, shortestSyl=40, shortestPause=40, sylThres=0.9,
                  interburst=None, interburstMult=1, burstThres=0.075, peakToTrough=3, troughLeft=True,
                  troughRight=False, summary=False, plot=False, savePath=None, _trace=None):
    """segment() (R/segment.R:79-219) restated on the host. _trace: a dict that receives
    the envelope, the scalars and the smallest relative margin of every decision taken
    ('threshold', 'count', 'merge', 'cond2', 'cond3')."""
    s, overlap, mergeSyl = _repair(x, samplingRate, windowLength, overlap, shortestPause, interburst, plot, savePath)
    value, timestep = hilbert_envelope_smoothed(s, samplingRate, windowLength, overlap)
    threshold = r_mean(value) * sylThres
    syl = find_syllables(value, timestep, threshold, shortestSyl, shortestPause, mergeSyl, _trace)
    if interburst is None:
        interburst = r_median(syl["sylLen"]) * interburstMult if "sylLen" in syl else shortestSyl
    bur = find_bursts(value, timestep, interburst, burstThres, peakToTrough, troughLeft, troughRight, _trace)
    if _trace is not None:
        _trace.update(envelope=value, timestep=timestep, threshold=threshold, interburst=interburst)
    if summary:
        return segment_summary(syl, bur)
    return {"syllables": syl, "bursts": bur}


# ------------------------------------------------------- on the GPU (sg_segment.hip)
def _params(samplingRate, windowLength=40, overlap=80, shortestSyl=40, shortestPause=40, sylThres=0.9,
            interburst=None, interburstMult=1, burstThres=0.075, peakToTrough=3, troughLeft=True, troughRight=False,
            mode=0, workspace_cap=0):
    from . import _abi
    nan = math.nan
    return _abi.sg_segment_params(float(samplingRate), float(windowLength), float(overlap), float(shortestSyl),
                                  nan if shortestPause is None else float(shortestPause), float(sylThres),
                                  nan if interburst is None else float(interburst), float(interburstMult),
                                  float(burstThres), float(peakToTrough), int(bool(troughLeft)),
                                  int(bool(troughRight)), int(mode), 0, int(workspace_cap))


def segment_size_native(length, P):
    """sg_segment_size (host only): dict(log2n, n_env, points, cells) for a sound of `length`
    samples; n_env is the smoothed envelope's length (the raw one's for mode 1)."""
    L = native.lib()
    o = [C.c_int32() for _ in range(3)]
    cells = C.c_int64()
    rc = L.sg_segment_size(int(length), C.byref(P), *[C.byref(v) for v in o], C.byref(cells))
    native.host_check(rc, L.sg_segment_size_error, value_error=True)
    return dict(log2n=o[0].value, n_env=o[1].value, points=o[2].value, cells=cells.value)


def segment_windows_native(length, P, n):
    """sg_segment_windows (host only): the planner's smoothing windows, (0-based first
    index, points, jump) as smoothing_windows gives them, and its timestep."""
    L = native.lib()
    first, cnt, jump = (np.zeros(max(n, 1), dtype=np.int64) for _ in range(3))
    ts = C.c_double()
    i64p = C.POINTER(C.c_int64)
    rc = L.sg_segment_windows(int(length), C.byref(P), first.ctypes.data_as(i64p), cnt.ctypes.data_as(i64p),
                              jump.ctypes.data_as(i64p), n, C.byref(ts))
    native.host_check(rc, L.sg_segment_size_error, value_error=True)
    return first[:n], cnt[:n], jump[:n], ts.value


def _unpack(h, summary):
    """A sound's device cells -> segment()'s value."""
    m, rows, found, nb = (int(h[k]) for k in range(4))
    if summary:
        r = dict(zip(SUMMARY_COLUMNS, (float(v) for v in h[HEAD:HEAD + 11])))
        r["nSyl"], r["nBursts"] = int(r["nSyl"]), int(r["nBursts"])
        return r
    s0 = HEAD + 11 + m
    b0 = s0 + 5 * ((m + 1) // 2)
    st = h[s0:s0 + 5 * rows].reshape(rows, 5)
    bt = h[b0:b0 + 3 * nb].reshape(nb, 3)
    if found:
        syl = {k: st[:, i].copy() for i, k in enumerate(SYLLABLE_COLUMNS)}
    else:
        syl = {"syllable": st[:, 0].copy(), "start": st[:, 1].copy(), "end": st[:, 2].copy(), "dur": st[:, 3].copy()}
    bur = {"time": bt[:, 0].copy(), "ampl": bt[:, 1].copy()}
    if nb:
        bur["interburstInt"] = bt[:, 2].copy()
    return {"syllables": syl, "bursts": bur}


def _detail(h):
    m = int(h[0])
    return dict(envelope=h[HEAD + 11:HEAD + 11 + m].copy(), timestep=float(h[4]), threshold=float(h[5]),
                interburst=float(h[6]))


def _check(rc, ctx):
    native.host_check(rc, lambda: native.lib().sg_last_error(ctx), value_error=True)


def segment(x, samplingRate=None, windowLength=40, overlap=80, shortestSyl=40, shortestPause=40, sylThres=0.9,
            interburst=None, interburstMult=1, burstThres=0.075, peakToTrough=3, troughLeft=True, troughRight=False,
            summary=False, plot=False, savePath=None, device=0, _detail_out=None):
    """segment() computed on the GPU (sg_segment, fp64): {'syllables', 'bursts'} with the
    reference's columns, or the eleven named values for summary = True."""
    s, overlap, _ = _repair(x, samplingRate, windowLength, overlap, shortestPause, interburst, plot, savePath)
    P = _params(samplingRate, windowLength, overlap, shortestSyl, shortestPause, sylThres, interburst, interburstMult,
                burstThres, peakToTrough, troughLeft, troughRight)
    d = segment_size_native(len(s), P)
    ctx = native.default_context(device)
    s = np.ascontiguousarray(s)
    out = np.zeros(d["cells"])
    dp = C.POINTER(C.c_double)
    _check(native.lib().sg_segment(ctx.ptr, s.ctypes.data_as(dp), len(s), C.byref(P), out.ctypes.data_as(dp)), ctx.ptr)
    if _detail_out is not None:
        _detail_out.update(_detail(out))
    return _unpack(out, summary)


def hilbert_envelope(x, device=0):
    """Mod(seewave::hilbert(x)), un-padded by the reference's rule, on the GPU."""
    s = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
    P = _params(1.0, mode=1)
    d = segment_size_native(len(s), P)
    ctx = native.default_context(device)
    out = np.zeros(d["cells"])
    dp = C.POINTER(C.c_double)
    _check(native.lib().sg_segment(ctx.ptr, s.ctypes.data_as(dp), len(s), C.byref(P), out.ctypes.data_as(dp)), ctx.ptr)
    return out[:d["n_env"]]


def segment_batch(data, offsets, lengths, samplingRate, windowLength=40, overlap=80, shortestSyl=40, shortestPause=40,
                  sylThres=0.9, interburst=None, interburstMult=1, burstThres=0.075, peakToTrough=3, troughLeft=True,
                  troughRight=False, summary=False, to_host=True, workspace_cap=0, device=0, _detail_out=None):
    """segment(x = call i, samplingRate, ...) for a batch of sounds already in HBM (`data`:
    a float32 CUDA tensor, call i at offsets[i], lengths[i] samples -- the layout of
    batch.synthesize_packed) in one launch sequence (sg_segment_batch). A call the
    reference stops on (fewer than three samples) gives None. to_host = False returns
    dict(out = the fp64 CUDA tensor, offsets, cells): the layout sg_segment_batch
    documents. workspace_cap: bytes of transform workspace per chunk of the batch (0:
    the library's default); the results do not depend on it."""
    if interburst is not None and (isinstance(interburst, bool) or not isinstance(interburst, (int, float)) or
                                   interburst < 0):
        raise ValueError("interburst is weird or negative: %r" % (interburst,))
    overlap = min(max(overlap, 0), 99)
    P = _params(samplingRate, windowLength, overlap, shortestSyl, shortestPause, sylThres, interburst, interburstMult,
                burstThres, peakToTrough, troughLeft, troughRight, 0, workspace_cap)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    cells = [segment_size_native(int(n), P)["cells"] if n >= 3 else HEAD + 11 for n in lens]
    ooff, p_ooff = native.out_offsets(cells)
    ctx = native.default_context(device)
    out = native.device_out(data, ooff[-1])
    _check(native.lib().sg_segment_batch(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                         C.c_void_p(out.data_ptr()), p_ooff), ctx.ptr)
    if not to_host:
        return dict(out=out, offsets=ooff[:-1].copy(), cells=cells)
    h = out.cpu().numpy()
    res = []
    for i in range(nc):
        c = h[ooff[i]:ooff[i + 1]]
        res.append(_unpack(c, summary) if lens[i] >= 3 else None)
        if _detail_out is not None:
            _detail_out.append(_detail(c) if lens[i] >= 3 else None)
    return res
