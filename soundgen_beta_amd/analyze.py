"""analyze()'s per-frame stage (R/analyze.R:233-575, R/utilities_analyze.R:22-324).

The second stage of analyze(): everything it computes on each frame before the
sequential host logic (prior, findVoicedSegments, pathfinder, median smoothing)
takes over.

- analyze_frames_numpy: the host restatement the GPU is compared against, restated
  from the sources, statement by statement:
    analyze()            R/analyze.R: normalisation :233-237, argument repairs :240-341,
                         the autocorrelation filter :402-407, getFrameBank / spectrogram
                         :421-453, amplitude :455-462, entropy :464-473, the
                         autocorrelation bank :475-484, analyzeFrame per frame :529-557,
                         time / duration :566-572
    analyzeFrame()       R/utilities_analyze.R:22-175 (descriptives :45-69, dom :72-96,
                         autocor :98-113, the dom certainty :151-159)
    getDom()             R/utilities_analyze.R:190-233
    getPitchAutocor()    R/utilities_analyze.R:250-324
    isCentral.localMax() R/utilities_math.R:614-617
    zoo::rollapply       width w, align = 'center': one value per full window, n - w + 1 of them
    stats::acf           demeaned, sum(x[t] x[t + k]) / n, divided by lag 0, lag.max =
                         min(lag.max, n - 1)
- analyze_frames / analyze_frames_batch: the same on the GPU (sg_analyze.hip, fp64).

What is returned is the stage's output BEFORE the pathfinder, so:
    * HNR is the raw maximum autocorrelation in (pitchFloor, pitchCeiling); to_dB
      (:702) comes after the pathfinder and is not applied;
    * quartile25 / 50 / 75 are NOT blanked for unvoiced frames (:689 comes after
      the pathfinder).
Differences from the reference's defaults: pitchMethods accepts a non-empty subset
of ('autocor', 'dom'); the reference's default also has 'spec', and 'cep' exists:
both raise NotImplementedError here (they and the pathfinder are the next step).
Formants (phonTools is not in the reference tree), plots, summary and savePath are
out of scope.

Quirks kept (what the statements do):
    * the frequency labels pass through R's character row names (spectrogram.R:176,
      as.numeric(rownames(s))): a 15-significant-digit round trip; rowLow, rowHigh,
      the cut band and pitchFloor_idx are decided on the round-tripped values, and
      every frequency-valued column is 1000 * such a value. The lag labels
      samplingRate / (1:wl) (:484) make the same trip;
    * row j of the autocorrelation bank holds lag j - 1 but is labelled sr / j (:484);
    * the amplitude window starts at floor(seq(1, length - wl, length.out = frames)[f])
      and has wl + 1 samples (a:(a + wl) is inclusive); it is not the frame's window;
    * silence = max(silence, min(ampl)) (:462): the quietest frame is never analysed;
    * peakFreqCut = meanSpec_cut$freq[which.max(frame)]: the full-spectrum arg-max used
      as an index into the cut table (NaN past its end);
    * the autocorrelation filter squares twice (:404-405);
    * normalising in analyze() and again in getFrameBank is idempotent (the second
      pass divides by exactly 1), so it is done once.
Refused, because the reference stops there: zp that pads the frame (acf() returns
wl + 1 values for a wl-row column, :479), no label above 6 kHz (rowLow:rowHigh with
NA), a sound not longer than the window, an empty lag range, a cut band of fewer than
2 bins (lm()). An even autocorSmooth (zoo's even-width alignment is not restated)
and one wider than the lag range are refused too. A frame louder than `silence`
whose entropy is NA makes the reference stop (`if (NA && ...)`); here it is just not tracked.

A table is a dict of per-frame arrays (NaN for R's NA); COLUMNS gives the order of
the device table's columns, autocorCand / autocorCert being nCands wide.
"""
import ctypes as C
import math
import warnings

import numpy as np

from . import native
from .morph import _r_seq_len
from .spectrogram import WINDOWS, _input, frame_starts, ft_window, get_entropy, get_frame_bank, normalize_sound

PITCH_METHODS = ("autocor", "dom")
MAX_CANDS = 8
# the device table's fixed columns; then autocorCand[nCands], autocorCert[nCands]
COLUMNS = ("ampl", "entropy", "HNR", "dom", "peakFreq", "peakFreqCut", "meanFreq", "quartile25", "quartile50",
           "quartile75", "specSlope", "domCand", "domCert", "cond_silence", "cond_entropy")
NFIXED = len(COLUMNS)


# ---------------------------------------------------------------- parts
def rt15(v):
    """as.numeric(as.character(v)): R prints 15 significant digits."""
    return float("%.15g" % v)


def is_central_local_max(x, threshold):
    """isCentral.localMax(), R/utilities_math.R:614-617 (which.max: the FIRST maximum)."""
    x = np.asarray(x, float)
    middle = int(math.ceil(len(x) / 2))
    return bool(int(np.argmax(x)) + 1 == middle and x[middle - 1] > threshold)


def roll_central_max(x, width, threshold):
    """zoo::rollapply(as.zoo(x), width, align = 'center', isCentral.localMax): 1-based
    indices (zoo::index) of the TRUE windows. len(x) - width + 1 windows; none if width > len(x)."""
    x = np.asarray(x, float)
    h = width // 2
    return [c + 1 for c in range(h, len(x) - (width - 1 - h)) if is_central_local_max(x[c - h:c - h + width], threshold)]


def freq_labels(samplingRate, wl, bins):
    """as.numeric(rownames(s)) (R/spectrogram.R:173-176): kHz, after the character round trip."""
    Y = _r_seq_len(0.0, (samplingRate / 2) - (samplingRate / wl), bins)
    return np.array([rt15(y / 1000) for y in Y])


def lag_labels(samplingRate, wl):
    """as.numeric(names(autoCorrelation)) for rownames = samplingRate / (1:wl) (:484)."""
    return np.array([rt15(samplingRate / j) for j in range(1, wl + 1)])


def ampl_starts(length, wl, frames):
    """0-based first sample of each amplitude window: floor(myseq[x]) - 1 (:456-459)."""
    if frames <= 0:
        return np.zeros(0, dtype=np.int64)
    return np.array([int(math.floor(v)) - 1 for v in _r_seq_len(1.0, float(length - wl), frames)], dtype=np.int64)


def frame_ampl(sound, wl, frames):
    """:456-460: RMS of sound[myseq[x]:(myseq[x] + wl)], wl + 1 samples."""
    return np.array([math.sqrt(np.mean(sound[a:a + wl + 1] ** 2)) for a in ampl_starts(len(sound), wl, frames)])


def autocor_filter(wl, wn):
    """:403-407."""
    filt = ft_window(2 * wl, wn)
    powerSpectrum_filter = np.abs(np.fft.fft(filt)) ** 2
    acf_filter = np.abs(np.fft.ifft(powerSpectrum_filter) * len(filt)) ** 2  # fft(inverse = TRUE): unnormalised
    acf_filter = acf_filter[:wl]
    return acf_filter / acf_filter.max()


def r_acf(x, lags):
    """stats::acf(x, plot = FALSE)$acf at the given lags: demeaned, / n, / lag 0,
    clamped to [-1, 1] as R's C code does."""
    x = np.asarray(x, float)
    n = len(x)
    x = x - x.mean()
    c0 = np.dot(x, x) / n
    se = math.sqrt(c0)
    out = np.empty(len(lags))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, k in enumerate(lags):
            a = (np.dot(x[:n - k], x[k:]) / n) / (se * se)
            out[i] = 1.0 if a > 1 else (-1.0 if a < -1 else a)
    return out


def spectral_descriptives(frame, freq, cut0, ncut):
    """analyzeFrame :45-69. freq: 1000 * labels (Hz); the cut band is freq[cut0:cut0 + ncut]."""
    frame = np.asarray(frame, float)
    amplitude = np.sum(frame)                                                 # :47
    am = int(np.argmax(frame))
    peakFreq = freq[am]                                                       # :48
    meanFreq = _first(freq, np.cumsum(frame) > amplitude / 2)                 # :49
    fc, ac = freq[cut0:cut0 + ncut], frame[cut0:cut0 + ncut]                  # :52-53
    peakFreqCut = fc[am] if am < ncut else math.nan                           # :58
    amplitude_cut = np.sum(ac)                                                # :59
    cum_cut = np.cumsum(ac)                                                   # :62
    q = [_first(fc, cum_cut >= p * amplitude_cut) for p in (0.25, 0.5, 0.75)]  # :63-68
    return dict(peakFreq=peakFreq, peakFreqCut=peakFreqCut, meanFreq=meanFreq, quartile25=q[0], quartile50=q[1],
                quartile75=q[2], specSlope=spec_slope(fc, ac))


def _first(values, mask):
    i = np.nonzero(mask)[0]
    return values[i[0]] if len(i) else math.nan  # min(which(<none>)) is Inf: NA


def spec_slope(freq, amp):
    """summary(lm(amp ~ freq))$coef[2, 1] (:69): the least-squares slope."""
    xc = freq - np.mean(freq)
    return float(np.sum(xc * (amp - np.mean(amp))) / np.sum(xc * xc))


def get_dom(frame, freq, domSmooth_bins, domThres, pitchFloor_idx):
    """getDom(), R/utilities_analyze.R:190-233 on frame / max(frame): (dom, pitchAmpl) or (NaN, NaN)."""
    idx = [i for i in roll_central_max(frame, domSmooth_bins, domThres) if i > pitchFloor_idx]  # :209-217
    if not idx:
        return math.nan, math.nan
    return freq[idx[0] - 1], frame[idx[0] - 1]                                # :223-226


def get_pitch_autocor(amp, freq, autocorThres, autocorSmooth, nCands):
    """getPitchAutocor(), R/utilities_analyze.R:250-324 on the rows already cut to
    (pitchFloor, pitchCeiling) (:262-263): (HNR, candidates, certainties)."""
    amp = np.asarray(amp, float)
    HNR = float(np.max(amp))                                                  # :264
    idx = [i - 1 for i in roll_central_max(amp, autocorSmooth, autocorThres)]  # :277-285
    cand, cert = [], []
    if idx:
        pa = amp[idx]
        best = freq[idx[int(np.nonzero(pa > 0.975 * pa.max())[0][0])]]        # :292-293
        keep = [i for i in idx if freq[i] > best / 1.8]                       # :296
        keep.sort(key=lambda i: -amp[i])                                      # :299 order(): stable, earlier first
        keep = keep[:nCands]                                                  # :306-308
        cand, cert = [freq[i] for i in keep], [amp[i] for i in keep]
    if HNR >= 1:                                                              # :318-320
        HNR = 0.9999
    return HNR, cand, cert


def dom_certainty(HNR):
    """:151-153."""
    return 1 / (1 + math.exp(3 * HNR - 1))


# ---------------------------------------------------------------- settings
def _num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def repair(samplingRate, duration=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian", zp=0,
           cutFreq=6000, pitchMethods=PITCH_METHODS, entropyThres=0.6, pitchFloor=75, pitchCeiling=3500, nCands=1,
           domThres=0.1, domSmooth=220, autocorThres=0.7, autocorSmooth=None):
    """The argument repairs of R/analyze.R:240-341 with R's warnings. duration (s):
    None skips the two repairs that need it (a batch has no single duration)."""
    sr = samplingRate
    if isinstance(pitchMethods, str):
        pitchMethods = (pitchMethods,)
    pitchMethods = tuple(pitchMethods)
    for m in pitchMethods:
        if m in ("cep", "spec"):
            raise NotImplementedError("pitchMethods = %r: only 'autocor' and 'dom' are built; 'cep' and 'spec' "
                                      "(in the reference's default) are not" % (m,))
        if m not in PITCH_METHODS:
            raise ValueError("pitchMethods must be a subset of %s" % (PITCH_METHODS,))
    if not pitchMethods:
        raise ValueError("pitchMethods must not be empty")
    if not _num(silence) or silence < 0 or silence > 1:                       # :240-243
        silence = 0.04
        warnings.warn('"silence" must be between 0 and 1; defaulting to 0.04')
    if not _num(entropyThres) or entropyThres < 0 or entropyThres > 1:        # :244-247
        entropyThres = 0.6
        warnings.warn('"entropyThres" must be between 0 and 1; defaulting to 0.6')
    if not _num(windowLength) or windowLength <= 0 or (duration is not None and windowLength > duration * 1000):
        windowLength = 50                                                     # :249-254
        warnings.warn('"windowLength" must be between 0 and sound_duration ms; defaulting to 50 ms')
    if not _num(step):                                                        # :258-270
        if not _num(overlap) or overlap < 0 or overlap > 99:
            # the reference resets overlap and leaves step NULL, then stops at `step <= 0`;
            # the evident intent (step from the reset overlap) is what is restated
            overlap = 50
            warnings.warn('If "step" is not specified, overlap must be between 0 and 99%; overlap reset to 50%')
        step = windowLength * (1 - overlap / 100)
    elif _num(overlap) and overlap != 50:
        warnings.warn('"overlap" is ignored if "step" is not NULL')
    if step <= 0 or (duration is not None and step > duration * 1000):        # :271-275
        step = windowLength / 2
        warnings.warn('"step" must be between 0 and sound_duration ms; defaulting to windowLength / 2')
    if step > windowLength:                                                   # :276-279
        warnings.warn('"step" should normally not be larger than "windowLength" ms: you are skipping parts of the '
                      'sound!')
    if wn not in WINDOWS:                                                     # :280-287
        wn = "gaussian"
        warnings.warn('Implemented "wn": %s. Defaulting to "gaussian"' % ", ".join(sorted(WINDOWS)))
    if not _num(zp):                                                          # :288-293
        zp = 0
    elif zp < 0:
        zp = 0
        warnings.warn('"zp" must be non-negative; defaulting to 0')
    if not _num(cutFreq) or cutFreq <= 0:                                     # :294-298
        cutFreq = sr / 2
        warnings.warn('"cutFreq" must be positive; defaulting to samplingRate / 2')
    if not _num(pitchFloor) or pitchFloor <= 0 or pitchFloor > sr / 2:        # :299-304
        pitchFloor = 1
        warnings.warn('"pitchFloor" must be between 0 and pitchCeiling; defaulting to 1 Hz')
    if not _num(pitchCeiling) or pitchCeiling > sr / 2:                       # :305-309
        pitchCeiling = sr / 2
        warnings.warn('"pitchCeiling" must be between 0 and Nyquist; defaulting to samplingRate / 2')
    if pitchFloor > pitchCeiling:                                             # :310-315
        pitchFloor, pitchCeiling = 1, sr / 2
        warnings.warn('"pitchFloor" cannot be above "pitchCeiling"; defaulting to 1 Hz and samplingRate / 2, '
                      'respectively')
    if not _num(nCands) or nCands < 1:                                        # :328-333
        nCands = 1
        warnings.warn('"nCands" must be a positive integer; defaulting to 1')
    else:
        nCands = int(np.round(nCands))
    if not _num(domThres) or domThres < 0 or domThres > 1:                    # :335-338
        domThres = 0.1
        warnings.warn('"domThres" must be between 0 and 1; defaulting to 0.1')
    if not _num(autocorThres) or autocorThres < 0 or autocorThres > 1:        # :339-342
        autocorThres = 0.7
        warnings.warn('"autocorThres" must be between 0 and 1; defaulting to 0.7')
    if not _num(domSmooth):
        raise ValueError("domSmooth must be a number")
    if autocorSmooth is not None and not _num(autocorSmooth):
        autocorSmooth = None  # !is.numeric(autocorSmooth): the default (utilities_analyze.R:267)
    return dict(samplingRate=sr, silence=silence, windowLength=windowLength, step=step, wn=wn, zp=zp,
                cutFreq=cutFreq, pitchMethods=pitchMethods, entropyThres=entropyThres, pitchFloor=pitchFloor,
                pitchCeiling=pitchCeiling, nCands=nCands, domThres=domThres, domSmooth=domSmooth,
                autocorThres=autocorThres, autocorSmooth=autocorSmooth)


def frame_decisions(length, s):
    """Every integer decision of the stage for a sound of `length` samples and the
    repaired settings s (repair()'s dict): what sg_analyze_frames_size makes bit-equal."""
    sr = s["samplingRate"]
    wl = int(math.floor(s["windowLength"] / 1000 * sr / 2) * 2)               # :255
    if wl < 4:
        raise ValueError("analyze: the window is shorter than 4 points")
    zpExtra = int(math.floor((s["zp"] - wl) / 2) * 2)
    if zpExtra > 0:
        raise ValueError("analyze: zp = %g pads the %d-point frame; acf() then returns %d values for the %d-row "
                         "column of autocorBank (R/analyze.R:479) and the reference stops" % (s["zp"], wl, wl + 1, wl))
    bins = wl // 2
    lab = freq_labels(sr, wl, bins)
    low, high = np.nonzero(lab > 0.05)[0], np.nonzero(lab > 6)[0]             # :466-467
    if len(low) == 0 or len(high) == 0:
        raise ValueError("analyze: no frequency label above 6 kHz (samplingRate / 2 must exceed 6000 Hz): rowHigh "
                         "is NA and rowLow:rowHigh stops in the reference")
    freq = 1000 * lab                                                         # utilities_analyze.R:45
    cut = np.nonzero((freq > s["pitchFloor"]) & (freq < s["cutFreq"]))[0]     # :52-53
    if len(cut) < 2:
        raise ValueError("analyze: fewer than 2 bins between pitchFloor and cutFreq; lm(amp ~ freq) stops in the "
                         "reference")
    pf = np.nonzero(lab > s["pitchFloor"] / 1000)[0]                          # utilities_analyze.R:216
    bin_ = sr / 2 / bins                                                      # :73
    domSmooth_bins = int(2 * math.ceil(s["domSmooth"] / bin_ / 2) - 1)        # :206
    if domSmooth_bins < 1:
        raise ValueError("analyze: domSmooth must be positive")
    a = s["autocorSmooth"]
    if a is None:
        a = 2 * math.ceil(7 * sr / 44100 / 2) - 1                             # :268
    if a != int(a) or a < 1 or int(a) % 2 == 0:
        raise ValueError("analyze: autocorSmooth must be a whole odd number (zoo's even-width alignment is not "
                         "restated)")
    lf = lag_labels(sr, wl)
    rows = np.nonzero((lf > s["pitchFloor"]) & (lf < s["pitchCeiling"]))[0]   # :262-263
    if len(rows) == 0:
        raise ValueError("analyze: no lag between pitchFloor and pitchCeiling (max(numeric(0)) in the reference)")
    if int(a) > len(rows):
        raise ValueError("analyze: autocorSmooth = %d is wider than the %d lags between pitchFloor and pitchCeiling"
                         % (int(a), len(rows)))
    if s["nCands"] > MAX_CANDS:
        raise native.SoundgenError(-4, "analyze: nCands = %d; at most %d candidates are kept" % (s["nCands"], MAX_CANDS))
    if length <= wl:
        frames = 0
    else:
        frames = len(frame_starts(length, sr, wl, s["step"]))
    return dict(wl=wl, bins=bins, frames=frames, cols=NFIXED + 2 * s["nCands"], lag_first=int(rows[0]),
                lag_last=int(rows[-1]), rowLow=int(low[0]) + 1, rowHigh=int(high[0]) + 1, cut0=int(cut[0]),
                ncut=len(cut), pitchFloor_idx=int(pf[0]) + 1, domSmooth_bins=domSmooth_bins, autocorSmooth=int(a))


def frame_times(length, samplingRate, step, frames):
    """:566-572: (time, duration)."""
    duration = length / samplingRate
    if frames <= 0:
        return np.zeros(0), np.zeros(0)
    t = _r_seq_len(step / 2, duration * 1000 - step / 2, frames)
    return np.round(np.array(t, float)), np.full(frames, duration)


def _empty(frames, nCands):
    t = {k: np.full(frames, math.nan) for k in COLUMNS}
    t["autocorCand"] = np.full((frames, nCands), math.nan)
    t["autocorCert"] = np.full((frames, nCands), math.nan)
    return t


def _too_short(length, wl):
    return ValueError("analyze: the sound (%d samples) is not longer than the window (%d): the amplitude window "
                      "sound[a:(a + wl)] leaves it (NA) in the reference" % (length, wl))


# ---------------------------------------------------------------- the restatement
def analyze_frames_numpy(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian",
                         zp=0, cutFreq=6000, pitchMethods=PITCH_METHODS, entropyThres=0.6, pitchFloor=75,
                         pitchCeiling=3500, nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7,
                         autocorSmooth=None, _probe=None):
    """The per-frame stage of analyze() restated on the host (see the module docstring).
    _probe: a dict that receives the intermediate vectors (for the conditioning tests)."""
    sound, sr = _input(x, samplingRate)
    s = repair(sr, len(sound) / sr, silence, windowLength, step, overlap, wn, zp, cutFreq, pitchMethods, entropyThres,
               pitchFloor, pitchCeiling, nCands, domThres, domSmooth, autocorThres, autocorSmooth)
    d = frame_decisions(len(sound), s)
    wl, bins, frames, nC = d["wl"], d["bins"], d["frames"], s["nCands"]
    if len(sound) <= wl:
        raise _too_short(len(sound), wl)
    with np.errstate(invalid="ignore", divide="ignore"):
        sound = normalize_sound(sound)                                        # :233-237 (once: see the docstring)
        acf_filter = autocor_filter(wl, s["wn"])                              # :402-407
        frameBank = get_frame_bank(sound, sr, wl, s["wn"], s["step"], 0)      # :421-429
        S = np.abs(np.fft.fft(frameBank, axis=0)[:bins])                      # :438-453, output = 'original'
        ampl = frame_ampl(sound, wl, frames)                                  # :456-460
        sil = max(s["silence"], ampl.min())                                   # :462
        entropy = np.array([get_entropy(S[d["rowLow"] - 1:d["rowHigh"], f]) for f in range(frames)])  # :466-470
        cond_silence = ampl > sil                                             # :472
        cond_entropy = cond_silence & (entropy < s["entropyThres"])           # :473
    freq = 1000 * freq_labels(sr, wl, bins)
    lagf = lag_labels(sr, wl)[d["lag_first"]:d["lag_last"] + 1]
    lags = list(range(d["lag_first"], d["lag_last"] + 1))
    t = _empty(frames, nC)
    t["ampl"], t["entropy"] = ampl, entropy
    t["cond_silence"], t["cond_entropy"] = cond_silence.astype(float), cond_entropy.astype(float)
    if _probe is not None:
        _probe.update(S=S, freq=freq, lagf=lagf, sil=sil, d=d, s=s, acf={}, normed={})
    for f in np.nonzero(cond_silence)[0]:                                     # :529-557
        frame = S[:, f]
        for k, v in spectral_descriptives(frame, freq, d["cut0"], d["ncut"]).items():
            t[k][f] = v
        if not cond_entropy[f]:                                               # trackPitch
            continue
        normed = frame / frame.max()                                          # utilities_analyze.R:72
        if "dom" in s["pitchMethods"]:                                        # :77-96
            t["dom"][f], t["domCert"][f] = get_dom(normed, freq, d["domSmooth_bins"], s["domThres"],
                                                   d["pitchFloor_idx"])
            t["domCand"][f] = t["dom"][f]
        if "autocor" in s["pitchMethods"]:                                    # :99-113
            a = r_acf(frameBank[:, f], lags) / acf_filter[d["lag_first"]:d["lag_last"] + 1]  # :479-481
            HNR, cand, cert = get_pitch_autocor(a, lagf, s["autocorThres"], d["autocorSmooth"], nC)
            t["HNR"][f] = HNR
            t["autocorCand"][f, :len(cand)] = cand
            t["autocorCert"][f, :len(cert)] = cert
            if not math.isnan(t["dom"][f]) and not math.isnan(HNR):           # :151-159
                t["domCert"][f] = dom_certainty(HNR)
            if _probe is not None:
                _probe["acf"][int(f)] = a
        if _probe is not None:
            _probe["normed"][int(f)] = normed
    t["time"], t["duration"] = frame_times(len(sound), sr, s["step"], frames)
    return t


# ------------------------------------------------------- on the GPU (sg_analyze.hip)
def _params(s):
    from . import _abi
    methods = (1 if "autocor" in s["pitchMethods"] else 0) | (2 if "dom" in s["pitchMethods"] else 0)
    a = s["autocorSmooth"]
    return _abi.sg_analyze_params(float(s["samplingRate"]), float(s["silence"]), float(s["windowLength"]),
                                  float(s["step"]), 50.0, float(s["zp"]), float(s["cutFreq"]),
                                  float(s["entropyThres"]), float(s["pitchFloor"]), float(s["pitchCeiling"]),
                                  float(s["nCands"]), float(s["domThres"]), float(s["domSmooth"]),
                                  float(s["autocorThres"]), math.nan if a is None else float(a),
                                  WINDOWS.index(s["wn"]), methods)


def _raise(rc, msg):
    if rc == -1:
        raise ValueError(msg)
    raise native.SoundgenError(rc, msg)


def frame_decisions_native(length, s):
    """sg_analyze_frames_size (host only): the library's frame_decisions()."""
    L = native.lib()
    P = _params(s)
    o = [C.c_int32() for _ in range(6)]
    extra = (C.c_int32 * 8)()
    rc = L.sg_analyze_frames_size(int(length), C.byref(P), *[C.byref(v) for v in o], extra)
    if rc < 0:
        _raise(rc, L.sg_analyze_frames_size_error().decode())
    keys = ("wl", "bins", "frames", "cols", "lag_first", "lag_last")
    d = {k: v.value for k, v in zip(keys, o)}
    d.update(zip(("rowLow", "rowHigh", "cut0", "ncut", "pitchFloor_idx", "domSmooth_bins", "autocorSmooth"), extra))
    return d


def ampl_starts_native(length, s, frames):
    L = native.lib()
    P = _params(s)
    out = np.zeros(max(frames, 1), dtype=np.int64)
    rc = L.sg_analyze_frames_ampl_starts(int(length), C.byref(P), out.ctypes.data_as(C.POINTER(C.c_int64)), frames)
    if rc < 0:
        _raise(rc, L.sg_analyze_frames_size_error().decode())
    return out[:frames]


def _table(m, nC, length, sr, step):
    """frames x cols device rows -> the dict."""
    t = {k: m[:, i].copy() for i, k in enumerate(COLUMNS)}
    t["autocorCand"] = m[:, NFIXED:NFIXED + nC].copy()
    t["autocorCert"] = m[:, NFIXED + nC:NFIXED + 2 * nC].copy()
    t["time"], t["duration"] = frame_times(length, sr, step, m.shape[0])
    return t


def _check(rc, ctx):
    if rc < 0:
        _raise(rc, native.lib().sg_last_error(ctx).decode())


def analyze_frames(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian", zp=0,
                   cutFreq=6000, pitchMethods=PITCH_METHODS, entropyThres=0.6, pitchFloor=75, pitchCeiling=3500,
                   nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7, autocorSmooth=None, device=0):
    """The per-frame stage of analyze() (R/analyze.R:233-575) on the GPU (sg_analyze_frames,
    fp64): a dict of per-frame arrays, NaN for NA. x: a numeric vector with
    samplingRate, or the path of a mono 16-bit PCM file. HNR is the raw maximum
    autocorrelation (to_dB at :702 comes after the pathfinder) and the quartiles are
    not blanked for unvoiced frames (:689 likewise). pitchMethods: a subset of
    ('autocor', 'dom'); the reference's default also has 'spec' (see the module docstring)."""
    sound, sr = _input(x, samplingRate)
    s = repair(sr, len(sound) / sr, silence, windowLength, step, overlap, wn, zp, cutFreq, pitchMethods, entropyThres,
               pitchFloor, pitchCeiling, nCands, domThres, domSmooth, autocorThres, autocorSmooth)
    d = frame_decisions_native(len(sound), s)
    if len(sound) <= d["wl"]:
        raise _too_short(len(sound), d["wl"])
    ctx = native.default_context(device)
    sound = np.ascontiguousarray(sound)
    out = np.zeros(d["frames"] * d["cols"])
    dp = C.POINTER(C.c_double)
    P = _params(s)
    _check(native.lib().sg_analyze_frames(ctx.ptr, sound.ctypes.data_as(dp), len(sound), C.byref(P),
                                          out.ctypes.data_as(dp)), ctx.ptr)
    return _table(out.reshape(d["frames"], d["cols"]), s["nCands"], len(sound), sr, s["step"])


def analyze_frames_batch(data, offsets, lengths, samplingRate, silence=0.04, windowLength=50, step=None, overlap=50,
                         wn="gaussian", zp=0, cutFreq=6000, pitchMethods=PITCH_METHODS, entropyThres=0.6,
                         pitchFloor=75, pitchCeiling=3500, nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7,
                         autocorSmooth=None, to_host=False, device=0):
    """analyze_frames(call i, samplingRate, ...) for a batch of sounds already in HBM
    (`data`: a float32 CUDA tensor, call i at offsets[i], lengths[i] samples -- the
    layout of batch.synthesize_packed), in one launch sequence (sg_analyze_frames_batch).
    The tables stay in HBM: returns a dict with `out` (an fp64 CUDA tensor), `offsets`
    (call i's table starts at out[offsets[i]]), `frames` (rows per call), `cols` and
    `columns` (the fixed column order, then nCands autocorCand and nCands autocorCert);
    call i's table is out[o:o + frames * cols].view(frames, cols). A call not longer
    than the window has 0 frames and writes nothing. The repairs that need a sound's
    duration (windowLength, step) are not made. to_host=True returns the list of
    per-call dicts analyze_frames returns."""
    import torch
    s = repair(samplingRate, None, silence, windowLength, step, overlap, wn, zp, cutFreq, pitchMethods, entropyThres,
               pitchFloor, pitchCeiling, nCands, domThres, domSmooth, autocorThres, autocorSmooth)
    L = native.lib()
    P = _params(s)
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
    nc = len(offs)
    ds = [frame_decisions_native(int(n), s) for n in lens]
    cols = NFIXED + 2 * s["nCands"]
    frames = [d["frames"] for d in ds]
    ooff = np.concatenate([[0], np.cumsum([f * cols for f in frames])]).astype(np.int64)
    ctx = native.default_context(device)
    out = torch.empty(max(int(ooff[-1]), 1), dtype=torch.float64, device=data.device)
    fo = np.zeros(max(nc, 1), dtype=np.int32)
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    torch.cuda.synchronize(data.device)  # the library runs on its own stream
    _check(L.sg_analyze_frames_batch(ctx.ptr, C.c_void_p(data.data_ptr()), offs.ctypes.data_as(i64p),
                                     lens.ctypes.data_as(i64p), nc, C.byref(P), C.c_void_p(out.data_ptr()),
                                     ooff.ctypes.data_as(i64p), fo.ctypes.data_as(i32p)), ctx.ptr)
    if [int(f) for f in fo[:nc]] != frames:
        raise native.SoundgenError(-1, "sg_analyze_frames_batch: frame counts disagree with sg_analyze_frames_size")
    if not to_host:
        return dict(out=out, offsets=ooff[:-1].copy(), frames=frames, cols=cols,
                    columns=COLUMNS + ("autocorCand",) * s["nCands"] + ("autocorCert",) * s["nCands"])
    h = out.cpu().numpy()
    return [_table(h[ooff[i]:ooff[i + 1]].reshape(frames[i], cols), s["nCands"], int(lens[i]), samplingRate, s["step"])
            for i in range(nc)]
