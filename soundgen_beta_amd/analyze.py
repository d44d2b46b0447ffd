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
Differences from the reference's defaults: analyze_frames*' pitchMethods accepts a
non-empty subset of ('autocor', 'dom'); the reference's default also has 'spec', and
'cep' exists: both raise NotImplementedError there. pitch_candidates* (at the end of
this module) run all four: getPitchCep (R/utilities_analyze.R:337-407) and getPitchSpec
(:424-558) restated likewise and on the GPU (sg_anl_cep, sg_anl_bana), plus
pitch_matrices (the pathfinder's inputs, R/analyze.R:578-591). The pathfinder is not built.
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


def _run(sound, sr, s, decisions, params, table, entry, device):
    """analyze_frames() and pitch_candidates() behind their repairs: `decisions` is the
    stage's *_decisions_native, `params` builds the C struct, `table` the dict, `entry`
    names the C entry point."""
    d = decisions(len(sound), s)
    if len(sound) <= d["wl"]:
        raise _too_short(len(sound), d["wl"])
    ctx = native.default_context(device)
    sound = np.ascontiguousarray(sound)
    out = np.zeros(d["frames"] * d["cols"])
    dp = C.POINTER(C.c_double)
    P = params(s)
    _check(getattr(native.lib(), entry)(ctx.ptr, sound.ctypes.data_as(dp), len(sound), C.byref(P),
                                        out.ctypes.data_as(dp)), ctx.ptr)
    return table(out.reshape(d["frames"], d["cols"]), s["nCands"], len(sound), sr, s["step"])


def _run_batch(data, offsets, lengths, samplingRate, s, frames_of, params, table, cand_keys, entry, to_host, device):
    """The *_batch forms likewise: frames_of(length, P) is the stage's frame count of a
    sound, cand_keys name the nCands-wide column groups behind the fixed columns, and
    the C entry points are entry + "_batch" and (in the text of the cross-check) entry + "_size"."""
    L = native.lib()
    P = params(s)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    nC = s["nCands"]
    frames = [frames_of(int(n), P) for n in lens]
    cols = NFIXED + len(cand_keys) * nC
    ooff, p_ooff = native.out_offsets([f * cols for f in frames])
    ctx = native.default_context(device)
    fo = np.zeros(max(nc, 1), dtype=np.int32)
    out = native.device_out(data, ooff[-1])
    _check(getattr(L, entry + "_batch")(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                        C.c_void_p(out.data_ptr()), p_ooff,
                                        fo.ctypes.data_as(C.POINTER(C.c_int32))), ctx.ptr)
    if [int(f) for f in fo[:nc]] != frames:
        raise native.SoundgenError(-1, "%s_batch: frame counts disagree with %s_size" % (entry, entry))
    if not to_host:
        return dict(out=out, offsets=ooff[:-1].copy(), frames=frames, cols=cols,
                    columns=COLUMNS + sum(((k,) * nC for k in cand_keys), ()))
    h = out.cpu().numpy()
    return [table(h[ooff[i]:ooff[i + 1]].reshape(frames[i], cols), nC, int(lens[i]), samplingRate, s["step"])
            for i in range(nc)]


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
    return _run(sound, sr, s, frame_decisions_native, _params, _table, "sg_analyze_frames", device)


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
    s = repair(samplingRate, None, silence, windowLength, step, overlap, wn, zp, cutFreq, pitchMethods, entropyThres,
               pitchFloor, pitchCeiling, nCands, domThres, domSmooth, autocorThres, autocorSmooth)
    return _run_batch(data, offsets, lengths, samplingRate, s, lambda n, P: frame_decisions_native(n, s)["frames"],
                      _params, _table, ("autocorCand", "autocorCert"), "sg_analyze_frames", to_host, device)


# ------------------------------------------------- pitch_candidates: 'cep' and 'spec'
ALL_PITCH_METHODS = ("autocor", "cep", "spec", "dom")
PITCH_DEFAULT_METHODS = ("autocor", "spec", "dom")  # analyze()'s default (R/analyze.R:191)
PITCH_KEYS = ("cepCand", "cepCert", "specCand", "specCert")
# BaNaRatios (R/sysdata.rda): a ratio of two spectral peaks strictly inside (value_low,
# value_high) says the lower peak is harmonic number divide_lower_by. After Ba, Yang,
# Demirkol & Heinzelman (2012), "BaNa: A hybrid approach for noise resilient pitch
# detection", IEEE Statistical Signal Processing Workshop. Rows in the data frame's order.
BANA_RATIOS = ((1.9, 2.1, 1.0), (2.8, 3.2, 1.0), (1.42, 1.59, 2.0), (3.8, 4.2, 1.0), (1.29, 1.42, 3.0),
               (4.8, 5.2, 1.0), (2.4, 2.6, 2.0), (1.59, 1.8, 3.0), (1.15, 1.29, 4.0))
PITCH_SOURCES = ("dom", "autocor", "cep", "spec")  # pitch_matrices' source codes index this


def hz_to_semitones(h):
    """HzToSemitones(), R/utilities_math.R:16-18."""
    return math.log2(h / 16.3516) * 12


def cep_layout(B, samplingRate, pitchFloor, pitchCeiling, cepSmooth, cepZp):
    """What getPitchCep decides before it sees the frame (R/utilities_analyze.R:346-367)
    for a B-bin frame: (L, pad, effective cepSmooth, l, first row 0-based, labels of the
    rows with pitchFloor < freq < pitchCeiling)."""
    if cepSmooth is None:                                                     # :346-348
        cepSmooth = 2 * math.ceil(31 * samplingRate / 44100 / 2) - 1
    if cepZp < B:                                                             # :350-351
        pad = 0
    else:
        pad = int((cepZp - B) / 2)                                            # :353 rep(0, x) truncates x
        cepSmooth = cepSmooth * round(cepZp / B)                              # :355 R's round: half to even
    L = B + 2 * pad
    l = L // 2                                                                # :361
    lab = [samplingRate / k / 2 * (L / B) for k in range(1, l + 1)]           # :364
    rows = [i for i, f in enumerate(lab) if f > pitchFloor and f < pitchCeiling]  # :367
    first = rows[0] if rows else 0
    return L, pad, cepSmooth, l, first, np.array([lab[i] for i in rows], float)


def get_pitch_cep(frame, samplingRate, pitchFloor, pitchCeiling, cepThres, cepSmooth, cepZp, nCands, _trace=None):
    """getPitchCep(), R/utilities_analyze.R:337-407, on frame / max(frame): (candidates,
    certainties), best first; ([], []) where the reference makes NULL or one all-NA row
    (idx[1:0] for no peak, :386). _trace (a dict) receives the band and the comparisons
    (a, b) behind the discrete decisions."""
    frame = np.asarray(frame, float)
    B = len(frame)
    L, pad, cepSmooth, l, first, freq = cep_layout(B, samplingRate, pitchFloor, pitchCeiling, cepSmooth, cepZp)
    frameZP = np.concatenate([np.zeros(pad), frame, np.zeros(pad)])           # :350-354
    cepstrum = np.abs(np.fft.fft(frameZP))                                    # :359
    cepstrum = cepstrum / cepstrum.max()                                      # :360 over all L values
    cep = cepstrum[first:first + len(freq)]                                   # :362-367 row i holds cepstrum[i]
    idx = [i - 1 for i in roll_central_max(cep, int(cepSmooth), cepThres)]    # :371-377
    if _trace is not None:
        _trace.update(band=cep, width=int(cepSmooth), order=[], rule18=[])
    if not idx:
        return [], []
    absCepPeak = idx[int(np.argmax(cep[idx]))]                                # :379 which.max: the first maximum
    keep = [i for i in idx if freq[i] > freq[absCepPeak] / 1.8]               # :381
    keep.sort(key=lambda i: -cep[i])                                          # :385 order(): stable, earlier first
    if _trace is not None:
        o = sorted(cep[idx])
        _trace["order"] = [(o[i], o[i + 1]) for i in range(len(o) - 1)]
        _trace["rule18"] = [(freq[i], freq[absCepPeak] / 1.8) for i in idx]
    keep = keep[:nCands]                                                      # :386
    cand = [float(freq[i]) for i in keep]
    cert = [float(cep[i] / (1 + 5 / (1 + math.exp(2 - .25 * hz_to_semitones(freq[i] / pitchFloor)))))
            for i in keep]                                                    # :400-401, after the ordering
    return cand, cert


def bana_candidates(peaks, pitchFloor, pitchCeiling, specSinglePeakCert, specThres, specMerge, nCands, _trace=None):
    """getPitchSpec() from its peak table on, R/utilities_analyze.R:461-555. peaks: the
    frequencies (Hz) of ALL the frame's peaks, ascending. (candidates, certainties)."""
    tr = _trace if _trace is not None else {}
    for k in ("ratio", "range", "merge", "thres"):
        tr.setdefault(k, [])
    peaks = [float(v) for v in peaks]
    if len(peaks) == 0:
        return [], []
    if len(peaks) == 1:                                                       # :461-472
        tr["range"] += [(peaks[0], pitchCeiling), (peaks[0], pitchFloor)]
        if not (peaks[0] < pitchCeiling and peaks[0] > pitchFloor):
            return [], []
        pitchCand, pitchAmpl = [peaks[0]], [specSinglePeakCert]
    else:
        peaks = peaks[:5]                                                     # :475
        n = len(peaks)
        pitchCand = []
        for i in range(2, n + 1):                                             # :487-496, kept where A > B
            for j in range(1, n):
                if not i > j:
                    continue
                ratio = peaks[i - 1] / peaks[j - 1]                           # :492
                for low, high, div in BANA_RATIOS:                            # :503-506 both borders exclusive
                    tr["ratio"] += [(ratio, low), (ratio, high)]
                    if ratio > low and ratio < high:
                        pitchCand.append(peaks[j - 1] / div)
        for c in pitchCand:
            tr["range"] += [(c, pitchFloor), (c, pitchCeiling)]
        pitchCand = sorted(c for c in pitchCand if c > pitchFloor and c < pitchCeiling)  # :511-512
        if not pitchCand:
            return [], []
        specAmplIdx = [1] * len(pitchCand)
        c = 0
        while c + 1 < len(pitchCand):                                         # :521-536
            dist = abs(math.log2(pitchCand[c] / pitchCand[c + 1]))
            tr["merge"].append((dist, specMerge / 12))
            if dist < specMerge / 12:
                specAmplIdx[c] += 1
                pitchCand[c] = (pitchCand[c] + pitchCand[c + 1]) / 2          # mean(c(running value, next))
                del pitchCand[c + 1], specAmplIdx[c + 1]
            else:
                c += 1
        pitchAmpl = [specSinglePeakCert + (1 / (1 + math.exp(-(a - 1))) - 0.5) * 2 * (1 - specSinglePeakCert)
                     for a in specAmplIdx]                                    # :537-539
        o = sorted(range(len(pitchCand)), key=lambda i: -pitchAmpl[i])        # :544-547 order(): stable
        pitchCand, pitchAmpl = [pitchCand[i] for i in o], [pitchAmpl[i] for i in o]
        tr["idx"] = [specAmplIdx[i] for i in o]
    tr["thres"] += [(a, specThres) for a in pitchAmpl]
    keep = [i for i in range(len(pitchCand)) if pitchAmpl[i] > specThres][:nCands]  # :550-555
    return [pitchCand[i] for i in keep], [pitchAmpl[i] for i in keep]


def spec_width(specSmooth, bin):
    """getPitchSpec's rolling width (R/utilities_analyze.R:438)."""
    return 2 * math.ceil((specSmooth / bin + 1) * 20 / bin / 2) - 1


def get_pitch_spec(frame, freq, bin, pitchFloor, pitchCeiling, specSmooth, specPeak, specSinglePeakCert, specThres,
                   specMerge, nCands, specHNRslope=None, _trace=None):
    """getPitchSpec(), R/utilities_analyze.R:424-558, on frame / max(frame) with HNR = NULL
    as analyze() passes it (:134: the threshold is specPeak, specHNRslope unused). freq:
    1000 * the round-tripped labels (:458). (candidates, certainties), best first."""
    width = int(spec_width(specSmooth, bin))                                  # :438
    idx = roll_central_max(frame, width, specPeak)                            # :440-457
    if _trace is not None:
        _trace.update(width=width, npeaks=len(idx))
    return bana_candidates([freq[i - 1] for i in idx], pitchFloor, pitchCeiling, specSinglePeakCert, specThres,
                           specMerge, nCands, _trace)


def repair_pitch(samplingRate, duration=None, pitchMethods=PITCH_DEFAULT_METHODS, cepThres=0.3, cepSmooth=None,
                 cepZp=0, specThres=0.3, specPeak=0.35, specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150,
                 specMerge=1, **kw):
    """repair() plus the repairs of R/analyze.R:343-363, with R's warnings; pitchMethods:
    a non-empty subset of ('autocor', 'cep', 'spec', 'dom')."""
    if isinstance(pitchMethods, str):
        pitchMethods = (pitchMethods,)
    pitchMethods = tuple(pitchMethods)
    for m in pitchMethods:
        if m not in ALL_PITCH_METHODS:
            raise ValueError("pitchMethods must be a subset of %s" % (ALL_PITCH_METHODS,))
    if not pitchMethods:
        raise ValueError("pitchMethods must not be empty")
    s = repair(samplingRate, duration, pitchMethods=PITCH_METHODS, **kw)
    s["pitchMethods"] = pitchMethods
    if not _num(cepThres) or cepThres < 0 or cepThres > 1:                    # :343-346
        cepThres = 0.3
        warnings.warn('"cepThres" must be between 0 and 1; defaulting to 0.3')
    if not _num(specThres) or specThres < 0 or specThres > 1:                 # :347-350
        specThres = 0.3
        warnings.warn('"specThres" must be between 0 and 1; defaulting to 0.3')
    if not _num(specPeak) or specPeak < 0 or specPeak > 1:                    # :351-354
        specPeak = 0.35
        warnings.warn('"specPeak" must be between 0 and 1; defaulting to 0.35')
    if not _num(specSinglePeakCert) or specSinglePeakCert < 0 or specSinglePeakCert > 1:  # :355-359
        specSinglePeakCert = 0.4
        warnings.warn('"specSinglePeakCert" must be between 0 and 1; defaulting to 0.4')
    if not _num(specMerge) or specMerge < 0:                                  # :360-363
        specMerge = 1
        warnings.warn('"specMerge" must be non-negative; defaulting to 1 semitone')
    if cepSmooth is not None and not _num(cepSmooth):
        cepSmooth = None  # !is.numeric(cepSmooth): the default (utilities_analyze.R:346)
    if not _num(cepZp) or not _num(specSmooth):
        raise ValueError("cepZp and specSmooth must be numbers")
    if not _num(specHNRslope):
        specHNRslope = 0.8  # unused: analyze() passes HNR = NULL
    s.update(cepThres=cepThres, cepSmooth=cepSmooth, cepZp=cepZp, specThres=specThres, specPeak=specPeak,
             specSinglePeakCert=specSinglePeakCert, specHNRslope=specHNRslope, specSmooth=specSmooth,
             specMerge=specMerge)
    return s


PITCH_SIZE_KEYS = ("wl", "bins", "lag_first", "lag_last", "rowLow", "rowHigh", "cut0", "ncut", "pitchFloor_idx",
                   "domSmooth_bins", "autocorSmooth", "cepL", "cepSmooth", "cepl", "cep0", "ncep", "specWidth")


def _transformable(L):
    M = L if L % 2 else L // 2
    if M < 1 or M > 2048:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31):
        while M % p == 0:
            M //= p
    return M == 1


def pitch_decisions(length, s):
    """frame_decisions() plus every integer decision of the two trackers for the
    repaired settings s (repair_pitch()'s dict): what sg_pitch_candidates_size makes
    bit-equal. cepf: the labels of the cepstral band."""
    d = frame_decisions(length, dict(s, pitchMethods=PITCH_METHODS))
    sr, B = s["samplingRate"], d["bins"]
    L, pad, cw, l, first, cepf = cep_layout(B, sr, s["pitchFloor"], s["pitchCeiling"], s["cepSmooth"], s["cepZp"])
    sw = spec_width(s["specSmooth"], sr / 2 / B)
    whole = cw == int(cw) and 1 <= cw <= 1e9
    d.update(cols=NFIXED + 6 * s["nCands"], cepL=L, cepSmooth=int(cw) if whole else 0, cepl=l, cep0=first, ncep=len(cepf),
             specWidth=min(int(sw), 1000000000) if sw >= 1 else 0, cepf=cepf)
    if "cep" in s["pitchMethods"]:
        if not _transformable(L):
            raise native.SoundgenError(-4, "analyze: the cepstrum's %d-point transform is not supported (%s must be at "
                                       "most 2048 with no prime factor above 31); R's fft() takes any length"
                                       % (L, "L" if L % 2 else "L / 2"))
        if not whole or int(cw) % 2 == 0:
            raise ValueError("analyze: the effective cepSmooth (cepSmooth * round(cepZp / bins) when cepZp pads the "
                             "frame) must be a whole odd number (zoo's even-width alignment is not restated)")
        if len(cepf) == 0:
            raise ValueError("analyze: no row of the cepstrum between pitchFloor and pitchCeiling (rollapply gets an "
                             "empty series in the reference)")
    if "spec" in s["pitchMethods"] and sw < 1:
        raise ValueError("analyze: specSmooth gives getPitchSpec's rolling window a width below 1 (rollapply stops in "
                         "the reference)")
    return d


def _pitch_args(a):
    """The formals of pitch_candidates*() as the keyword arguments of repair_pitch()."""
    return {k: a[k] for k in ("silence", "windowLength", "step", "overlap", "wn", "zp", "cutFreq", "pitchMethods",
                              "entropyThres", "pitchFloor", "pitchCeiling", "nCands", "domThres", "domSmooth",
                              "autocorThres", "autocorSmooth", "cepThres", "cepSmooth", "cepZp", "specThres", "specPeak",
                              "specSinglePeakCert", "specHNRslope", "specSmooth", "specMerge")}


def pitch_candidates_numpy(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian",
                           zp=0, cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6, pitchFloor=75,
                           pitchCeiling=3500, nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7,
                           autocorSmooth=None, cepThres=0.3, cepSmooth=None, cepZp=0, specThres=0.3, specPeak=0.35,
                           specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150, specMerge=1, _probe=None):
    """analyze_frames_numpy() with all four pitch trackers of analyzeFrame()
    (R/utilities_analyze.R:71-144): the host restatement pitch_candidates() is compared
    against. Returns analyze_frames_numpy()'s dict plus cepCand, cepCert, specCand and
    specCert (frames x nCands, NaN for NA and for a method not asked for).
    _probe: receives analyze_frames_numpy()'s intermediates and, per tracked frame,
    the traces of get_pitch_cep / get_pitch_spec (`cep`, `spec`).

    Not built (sequential host logic over these candidates): the prior
    (R/analyze.R:593-612), findVoicedSegments and the pathfinder, and the pitchAutocor /
    pitchCep / pitchSpec columns (:659-667), which hinge on what as.numeric does with
    zero-length list elements and cannot be settled without R."""
    sound, sr = _input(x, samplingRate)
    s = repair_pitch(sr, len(sound) / sr, **_pitch_args(locals()))
    d = pitch_decisions(len(sound), s)
    base = [m for m in s["pitchMethods"] if m in PITCH_METHODS]
    probe = {} if _probe is None else _probe
    kw = {k: s[k] for k in ("silence", "windowLength", "step", "wn", "zp", "cutFreq", "entropyThres", "pitchFloor",
                            "pitchCeiling", "nCands", "domThres", "domSmooth", "autocorThres", "autocorSmooth")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # repair_pitch() has warned already
        # the shared columns; with neither 'autocor' nor 'dom' the stage runs with 'dom' and its columns are blanked
        t = analyze_frames_numpy(sound, sr, pitchMethods=tuple(base) or ("dom",), _probe=probe, **kw)
    if not base:
        for k in ("dom", "domCand", "domCert"):
            t[k] = np.full_like(t[k], math.nan)
    nC, frames = s["nCands"], len(t["ampl"])
    for k in PITCH_KEYS:
        t[k] = np.full((frames, nC), math.nan)
    probe.update(d=d, s=s, cep={}, spec={})
    freq, bin_ = probe["freq"], sr / 2 / d["bins"]
    for f in np.nonzero(t["cond_entropy"] == 1)[0]:
        normed = probe["normed"][int(f)]                                      # utilities_analyze.R:72
        if "cep" in s["pitchMethods"]:                                        # :116-126
            tr = probe["cep"][int(f)] = {}
            cand, cert = get_pitch_cep(normed, sr, s["pitchFloor"], s["pitchCeiling"], s["cepThres"], s["cepSmooth"],
                                       s["cepZp"], nC, tr)
            t["cepCand"][f, :len(cand)], t["cepCert"][f, :len(cert)] = cand, cert
        if "spec" in s["pitchMethods"]:                                       # :129-144
            tr = probe["spec"][int(f)] = {}
            cand, cert = get_pitch_spec(normed, freq, bin_, s["pitchFloor"], s["pitchCeiling"], s["specSmooth"],
                                        s["specPeak"], s["specSinglePeakCert"], s["specThres"], s["specMerge"], nC,
                                        s["specHNRslope"], tr)
            t["specCand"][f, :len(cand)], t["specCert"][f, :len(cert)] = cand, cert
    return t


def _pitch_params(s):
    from . import _abi
    m = s["pitchMethods"]
    P = _abi.sg_pitch_params()
    P.a = _params(dict(s, pitchMethods=()))
    P.a.methods = sum(b for k, b in (("autocor", 1), ("dom", 2), ("cep", 4), ("spec", 8)) if k in m)
    c = s["cepSmooth"]
    P.cepThres, P.cepSmooth, P.cepZp = float(s["cepThres"]), math.nan if c is None else float(c), float(s["cepZp"])
    P.specThres, P.specPeak, P.specSinglePeakCert = float(s["specThres"]), float(s["specPeak"]), float(s["specSinglePeakCert"])
    P.specHNRslope, P.specSmooth, P.specMerge = float(s["specHNRslope"]), float(s["specSmooth"]), float(s["specMerge"])
    return P


def pitch_decisions_native(length, s):
    """sg_pitch_candidates_size and sg_pitch_candidates_cep_labels (host only): the library's pitch_decisions()."""
    L = native.lib()
    P = _pitch_params(s)
    frames, cols = C.c_int32(), C.c_int32()
    extra = (C.c_int32 * 24)()
    rc = L.sg_pitch_candidates_size(int(length), C.byref(P), C.byref(frames), C.byref(cols), extra)
    if rc < 0:
        _raise(rc, L.sg_analyze_frames_size_error().decode())
    d = dict(zip(PITCH_SIZE_KEYS, extra))
    d.update(frames=frames.value, cols=cols.value)
    lab = np.zeros(max(d["ncep"], 1))
    rc = L.sg_pitch_candidates_cep_labels(C.byref(P), lab.ctypes.data_as(C.POINTER(C.c_double)), d["ncep"])
    if rc < 0:
        _raise(rc, L.sg_analyze_frames_size_error().decode())
    d["cepf"] = lab[:d["ncep"]]
    return d


def _pitch_frames_native(length, P):
    """sg_pitch_candidates_size's frame count alone: the setup of the last parameters is
    cached in the library, so this is one cheap call per sound of a batch."""
    L = native.lib()
    fr, cl = C.c_int32(), C.c_int32()
    rc = L.sg_pitch_candidates_size(int(length), C.byref(P), C.byref(fr), C.byref(cl), None)
    if rc < 0:
        _raise(rc, L.sg_analyze_frames_size_error().decode())
    return fr.value


def _pitch_table(m, nC, length, sr, step):
    t = _table(m, nC, length, sr, step)
    for i, k in enumerate(PITCH_KEYS):
        t[k] = m[:, NFIXED + (2 + i) * nC:NFIXED + (3 + i) * nC].copy()
    return t


def pitch_candidates(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian", zp=0,
                     cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6, pitchFloor=75,
                     pitchCeiling=3500, nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7, autocorSmooth=None,
                     cepThres=0.3, cepSmooth=None, cepZp=0, specThres=0.3, specPeak=0.35, specSinglePeakCert=0.4,
                     specHNRslope=0.8, specSmooth=150, specMerge=1, device=0):
    """The per-frame stage of analyze() with all four pitch trackers on the GPU
    (sg_pitch_candidates, fp64): analyze_frames()'s dict plus cepCand, cepCert
    (getPitchCep, R/utilities_analyze.R:337-407), specCand and specCert (getPitchSpec,
    :424-558), frames x nCands, NaN for NA and for a method not asked for. pitchMethods:
    a non-empty subset of ('autocor', 'cep', 'spec', 'dom'); the default is analyze()'s.
    With pitchMethods within ('autocor', 'dom') the shared keys equal analyze_frames()'
    bit for bit. Not built: see pitch_candidates_numpy()."""
    sound, sr = _input(x, samplingRate)
    s = repair_pitch(sr, len(sound) / sr, **_pitch_args(locals()))
    return _run(sound, sr, s, pitch_decisions_native, _pitch_params, _pitch_table, "sg_pitch_candidates", device)


def pitch_candidates_batch(data, offsets, lengths, samplingRate, silence=0.04, windowLength=50, step=None, overlap=50,
                           wn="gaussian", zp=0, cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6,
                           pitchFloor=75, pitchCeiling=3500, nCands=1, domThres=0.1, domSmooth=220, autocorThres=0.7,
                           autocorSmooth=None, cepThres=0.3, cepSmooth=None, cepZp=0, specThres=0.3, specPeak=0.35,
                           specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150, specMerge=1, to_host=False,
                           device=0):
    """pitch_candidates(call i, samplingRate, ...) for a batch of sounds already in HBM,
    laid out and returned as analyze_frames_batch() does (sg_pitch_candidates_batch, one
    launch sequence, tables left in HBM). A row has 15 + 6 nCands columns: `columns`
    names the fixed ones, then nCands each of autocorCand, autocorCert, cepCand,
    cepCert, specCand, specCert. to_host=True returns the list of per-call dicts
    pitch_candidates() returns."""
    s = repair_pitch(samplingRate, None, **_pitch_args(locals()))
    return _run_batch(data, offsets, lengths, samplingRate, s, _pitch_frames_native, _pitch_params, _pitch_table,
                      ("autocorCand", "autocorCert") + PITCH_KEYS, "sg_pitch_candidates", to_host, device)


def pitch_matrices(table):
    """The pathfinder's inputs of R/analyze.R:578-591 from a pitch_candidates() table
    (host only): (pitchCands, pitchCert, pitchSource, names), each rows x frames with
    rows = max(1, the largest number of candidates a frame has), NaN-filled (pitchSource:
    small ints indexing `names`, -1 where there is no candidate). A frame's non-NA
    candidates are packed in the order analyzeFrame() rbinds them: dom, autocor[.],
    cep[.], spec[.].

    Known difference: the reference's 1:0 quirks (idx[1:0], pitchSpec_array[1:0, ]) can
    leave an extra all-NA row in a frame's pitch_array; such rows carry no candidate
    (:589-591 blank them) but can add an all-NA row to the matrices. They are not
    reproduced. The prior (:593-612) and everything after it is not built."""
    frames = len(table["ampl"])
    per = []
    for f in range(frames):
        rows = [(table["domCand"][f], table["domCert"][f], 0)]
        for src, key in ((1, "autocor"), (2, "cep"), (3, "spec")):
            if key + "Cand" in table:
                rows += [(c, a, src) for c, a in zip(table[key + "Cand"][f], table[key + "Cert"][f])]
        per.append([r for r in rows if not math.isnan(r[0])])
    n = max([len(p) for p in per] + [1])
    cands, cert = np.full((n, frames), math.nan), np.full((n, frames), math.nan)
    source = np.full((n, frames), -1, dtype=np.int8)
    for f, p in enumerate(per):
        for i, (c, a, src) in enumerate(p):
            cands[i, f], cert[i, f], source[i, f] = c, a, src
    return cands, cert, source, PITCH_SOURCES
