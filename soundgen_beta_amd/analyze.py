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
'cep' exists: both raise NotImplementedError there. pitch_candidates* (further down) run
all four: getPitchCep (R/utilities_analyze.R:337-407) and getPitchSpec (:424-558) restated
likewise and on the GPU (sg_anl_cep, sg_anl_bana), plus pitch_matrices (the pathfinder's
inputs, R/analyze.R:578-591). analyze* (at the end of this module) add what follows the
candidates (R/analyze.R:576-707, R/utilities_pitch_postprocessing.R): the prior,
findVoicedSegments, pathfinder, medianSmoother and the final columns, restated as
analyze_numpy / pitch_path_numpy and on the GPU (sg_anl_path, sg_anl_harm; sg_path.h).
summary = TRUE (R/analyze.R:770-796: one row per sound, the mean, median and sd of every
acoustic variable) is summarize_table_numpy and, on the GPU, sg_anl_summary (sg_summary.h):
analyze(summary=True), analyze_batch(summary=True), summarize_table; analyze_folder is
analyzeFolder() (:831-930) on top of analyze_batch.
The formant columns (formants=True; phonTools::findformants restated, unpinned against R) are
formants.py's: formants, formants_batch, find_formants_numpy, formants_numpy and
find_formants_frames are re-exported here. pathfinding = 'slow', the pitchAutocor / pitchCep /
pitchSpec columns (so also their summary cells), plots and savePath are out of scope.

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


def _host_check(rc):
    native.host_check(rc, native.lib().sg_analyze_frames_size_error, value_error=True)


def frame_decisions_native(length, s):
    """sg_analyze_frames_size (host only): the library's frame_decisions()."""
    L = native.lib()
    P = _params(s)
    o = [C.c_int32() for _ in range(6)]
    extra = (C.c_int32 * 8)()
    rc = L.sg_analyze_frames_size(int(length), C.byref(P), *[C.byref(v) for v in o], extra)
    _host_check(rc)
    keys = ("wl", "bins", "frames", "cols", "lag_first", "lag_last")
    d = {k: v.value for k, v in zip(keys, o)}
    d.update(zip(("rowLow", "rowHigh", "cut0", "ncut", "pitchFloor_idx", "domSmooth_bins", "autocorSmooth"), extra))
    return d


def ampl_starts_native(length, s, frames):
    L = native.lib()
    P = _params(s)
    out = np.zeros(max(frames, 1), dtype=np.int64)
    rc = L.sg_analyze_frames_ampl_starts(int(length), C.byref(P), out.ctypes.data_as(C.POINTER(C.c_int64)), frames)
    _host_check(rc)
    return out[:frames]


def _table(m, nC, length, sr, step):
    """frames x cols device rows -> the dict."""
    t = {k: m[:, i].copy() for i, k in enumerate(COLUMNS)}
    t["autocorCand"] = m[:, NFIXED:NFIXED + nC].copy()
    t["autocorCert"] = m[:, NFIXED + nC:NFIXED + 2 * nC].copy()
    t["time"], t["duration"] = frame_times(length, sr, step, m.shape[0])
    return t


def _check(rc, ctx):
    native.host_check(rc, lambda: native.lib().sg_last_error(ctx), value_error=True)


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


def _run_batch(data, offsets, lengths, samplingRate, s, frames_of, params, table, cand_keys, entry, to_host, device,
               tail=(), summary=False):
    """The *_batch forms likewise: frames_of(length, P) is the stage's frame count of a
    sound, cand_keys name the nCands-wide column groups behind the fixed columns, `tail`
    the single columns behind those, and the C entry points are entry + "_batch" and (in
    the text of the cross-check) entry + "_size". summary (analyze_batch only): the entry
    point is sg_analyze_summary_batch, which also fills one row of 44 cells per call."""
    L = native.lib()
    P = params(s)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    nC = s["nCands"]
    frames = [frames_of(int(n), P) for n in lens]
    cols = NFIXED + len(cand_keys) * nC + len(tail)
    ooff, p_ooff = native.out_offsets([f * cols for f in frames])
    ctx = native.default_context(device)
    fo = np.zeros(max(nc, 1), dtype=np.int32)
    out = native.device_out(data, ooff[-1])
    if summary:
        rows = native.device_out(data, max(nc, 1) * len(SUMMARY_COLUMNS))
        _check(L.sg_analyze_summary_batch(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                          C.c_void_p(out.data_ptr()), p_ooff, fo.ctypes.data_as(C.POINTER(C.c_int32)),
                                          C.c_void_p(rows.data_ptr())), ctx.ptr)
    else:
        _check(getattr(L, entry + "_batch")(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, C.byref(P),
                                            C.c_void_p(out.data_ptr()), p_ooff,
                                            fo.ctypes.data_as(C.POINTER(C.c_int32))), ctx.ptr)
    if [int(f) for f in fo[:nc]] != frames:
        raise native.SoundgenError(-1, "%s_batch: frame counts disagree with %s_size" % (entry, entry))
    if summary:
        rows = rows[:nc * len(SUMMARY_COLUMNS)].view(nc, len(SUMMARY_COLUMNS))
        if not to_host:
            return dict(out=rows, columns=SUMMARY_COLUMNS, frames=frames, tables=out, offsets=ooff[:-1].copy(), cols=cols)
        return _host_rows(rows)
    if not to_host:
        return dict(out=out, offsets=ooff[:-1].copy(), frames=frames, cols=cols,
                    columns=COLUMNS + sum(((k,) * nC for k in cand_keys), ()) + tuple(tail))
    return _host_tables(out, frames, cols, table, nC, lens, samplingRate, s["step"])


def _host_rows(rows):
    """The summary matrix of a batch (n_calls x 44, on the device) as the list of per-call dicts."""
    return [dict(zip(SUMMARY_COLUMNS, (float(v) for v in r))) for r in rows.cpu().numpy()]


def _host_tables(out, frames, cols, table, nC, lens, samplingRate, step):
    """The packed tables of a batch (on the device, call i's frames[i] x cols behind the ones before it) as the
    list of per-call dicts that `table` builds."""
    h = out.cpu().numpy()
    ooff = native.out_offsets([f * cols for f in frames])[0]
    return [table(h[ooff[i]:ooff[i + 1]].reshape(frames[i], cols), nC, int(lens[i]), samplingRate, step)
            for i in range(len(frames))]


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

    What follows these candidates (the prior, R/analyze.R:593-612, findVoicedSegments, the
    pathfinder, the smoothing) is analyze_numpy()'s. Not built: the pitchAutocor / pitchCep /
    pitchSpec columns (:659-667), which hinge on what as.numeric does with zero-length list
    elements and cannot be settled without R."""
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
    _host_check(rc)
    d = dict(zip(PITCH_SIZE_KEYS, extra))
    d.update(frames=frames.value, cols=cols.value)
    lab = np.zeros(max(d["ncep"], 1))
    rc = L.sg_pitch_candidates_cep_labels(C.byref(P), lab.ctypes.data_as(C.POINTER(C.c_double)), d["ncep"])
    _host_check(rc)
    d["cepf"] = lab[:d["ncep"]]
    return d


def _pitch_frames_native(length, P):
    """sg_pitch_candidates_size's frame count alone: the setup of the last parameters is
    cached in the library, so this is one cheap call per sound of a batch."""
    L = native.lib()
    fr, cl = C.c_int32(), C.c_int32()
    rc = L.sg_pitch_candidates_size(int(length), C.byref(P), C.byref(fr), C.byref(cl), None)
    _host_check(rc)
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
    bit for bit. analyze() goes on from these candidates to the pitch contour."""
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
    reproduced; they are immaterial to what follows (the pathfinder drops all-NA rows and
    findVoicedSegments counts non-NA entries). The prior (:593-612) and everything after it:
    analyze_numpy()."""
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


# ------------------------------------------- analyze(): the tail behind the candidates
SMOOTH_VARS = ("pitch", "dom")
TRACK_COLUMNS = ("pitch", "amplVoiced", "voiced", "harmonics")  # the device table's last four
PATHFINDING = ("none", "fast", "slow", "exact")  # the index is sg_analyze_params_full.pathfinding; 'exact' is not in the reference
PATH_MAX_WIN = 64  # interpolWin and floor(smoothing_ww / 2) on the GPU (kPathMaxWin)
SNAKE_MIN_STEP = 0.005  # the smallest snakeStep the GPU takes (its iterations are capped by range / snakeStep * 2)
_SLOW = "pathfinding = 'slow' is simulated annealing through optim() on R's random stream: not built"


def to_dB(x):
    """to_dB(), R/utilities_math.R:37-39; NaN for a ratio <= 0, as log10 gives."""
    x = np.asarray(x, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 10 * np.log10(x / (1 - x))


def dgamma(x, shape, rate, lconst=None):
    """stats::dgamma(x, shape, rate) restated as exp((shape - 1) ln x - rate x + shape
    ln(rate) - lgamma(shape)); 0 for x < 0. lconst: the last two terms, if already known."""
    if lconst is None:
        lconst = shape * math.log(rate) - math.lgamma(shape)
    if math.isnan(x):
        return math.nan
    if x < 0:
        return 0.0
    if x == 0:
        return 0.0 if shape > 1 else (rate if shape == 1 else math.inf)
    return math.exp((shape - 1) * math.log(x) - rate * x + lconst)


def prior_setup(priorMean, priorSD, pitchFloor, pitchCeiling):
    """R/analyze.R:599-605: (shape, rate, shape ln(rate) - lgamma(shape), prior_normalizer)."""
    shape = priorMean ** 2 / priorSD ** 2
    rate = priorMean / priorSD ** 2
    lconst = shape * math.log(rate) - math.lgamma(shape)
    grid = _r_seq_len(hz_to_semitones(pitchFloor), hz_to_semitones(pitchCeiling), 100)
    return shape, rate, lconst, max(dgamma(v, shape, rate, lconst) for v in grid)


def prior_multiplier(hz, prior):
    """pitchCert_multiplier (:606-610) of one candidate (Hz); prior: prior_setup()'s tuple."""
    shape, rate, lconst, norm = prior
    return dgamma(hz_to_semitones(hz), shape, rate, lconst) / norm


def find_voiced_segments(count, minVoicedCands, noRequired, nToleratedNA):
    """findVoicedSegments(), R/utilities_pitch_postprocessing.R:622-669, with its loop
    bounds as written: count[f] non-NA candidates in frame f -> [(start, end)], 1-based,
    inclusive. The last noRequired - 1 frames (and the very last one) cannot start a
    segment; the end is i - 1, or the last voiced frame of the sound."""
    v = np.asarray(count) >= minVoicedCands                                   # :628-630
    n = len(v)
    segs = []
    i = 1
    while i < n - noRequired + 1:                                             # :642
        found = False
        while i < n - noRequired + 1:                                         # :644-650
            if v[i - 1:i - 1 + noRequired].all():
                found = True
                break
            i += 1
        if found:                                                             # :652
            start, end = i, None
            while i < n - nToleratedNA + 1:                                   # :653-660
                if not v[i - 1:i + nToleratedNA].any():
                    end = i - 1
                    i -= 1
                    break
                i += 1
            if end is None:                                                   # :661-665
                segs.append((start, int(np.nonzero(v)[0][-1]) + 1))
                break
            segs.append((start, end))
        i += 1
    return segs


def _median(v):
    s = sorted(v)
    m = len(s)
    return s[(m - 1) // 2] if m % 2 else (s[m // 2 - 1] + s[m // 2]) / 2


def _mean(v):
    acc = 0.0
    for x in v:
        acc += x
    return acc / len(v) if len(v) else math.nan


def cost_jumps(cand1, cand2):
    """costJumps(), :283-285."""
    return 1 / (1 + 10 * math.exp(3 - 7 * abs(cand1 - cand2)))


def find_grad(path):
    """findGrad(), :534-562; lm()'s slopes over 2 or 3 points in closed form."""
    path = [float(v) for v in path]
    n = len(path)
    if n < 2:                                                                 # interpol == 1
        sl = sr = 0.0
    elif n == 2:
        sl = sr = path[1] - path[0]
    else:
        sl, sr = (path[2] - path[0]) / 2, (path[-1] - path[-3]) / 2
    ext = [path[0] - 2 * sl, path[0] - 1 * sl] + path + [path[-1] + 1 * sr, path[-1] + 2 * sr]
    return [ext[i - 2] - 4 * ext[i - 1] + 6 * ext[i] - 4 * ext[i + 1] + ext[i + 2] for i in range(2, n + 2)]


def force_per_path(pitch, cands, cert, certWeight, _pairs=None):
    """forcePerPath(), :495-521. cands / cert: per frame, the packed log2 candidates."""
    grad = find_grad(pitch)
    out = []
    for i, p in enumerate(pitch):
        external = 0.0
        for c, a in zip(cands[i], cert[i]):
            f = a * (1 / math.exp((c - p) ** 2))
            external += f if c > p else -f                                    # cands > pitch[i]: equal pushes with -cert
            if _pairs is not None and c != p:  # bit-equal: the point is still a copy of this candidate
                _pairs.append((c, p))
        out.append(certWeight * external + (1 - certWeight) * (-grad[i]))
    return out


def _trace_pick(scores, values, k, largest, out):
    """The chosen score against the best score of a different pitch value."""
    other = [s for s, v in zip(scores, values) if v != values[k] and not math.isnan(s)]
    if other:
        out.append((scores[k], max(other) if largest else min(other)))


def _which(scores, largest):
    best = -1
    for k, s in enumerate(scores):
        if math.isnan(s):
            continue
        if best < 0 or (s > scores[best] if largest else s < scores[best]):
            best = k
    return best


def _div(a, d):
    return a / d if d else (math.inf if a > 0 else math.nan)


def pathfinding_fast(C, A, cog, certWeight, tr):
    """pathfinding_fast(), :203-267, on the packed, sorted log2 candidates. point_current
    is never updated in either loop: every frame's choice depends on the start alone."""
    n = len(C)

    def run(order, p):
        f0 = order[0]
        start = math.nan
        if not math.isnan(p) and C[f0]:
            c = [_div(a, abs(v - p)) for v, a in zip(C[f0], A[f0])]           # :211, :241
            k = _which(c, True)
            if k >= 0:
                start = C[f0][k]
                _trace_pick(c, C[f0], k, True, tr["start"])
        path, total = {f0: start}, 0.0
        for f in order[1:]:
            if not C[f]:                                                      # length(cands) == 0: the frame is skipped
                path[f] = math.nan
                continue
            costs = [certWeight * abs(v - cog[f]) + (1 - certWeight) * (0.0 if math.isnan(start) else cost_jumps(start, v))
                     for v in C[f]]                                           # :220-229
            k = _which(costs, False)
            _trace_pick(costs, C[f], k, False, tr["choice"])
            path[f] = C[f][k]
            total += costs[k]
        return [path[f] for f in range(n)], total

    head = [v for v in cog[:min(5, n)] if not math.isnan(v)]
    pF = _median(head) if head else math.nan                                  # :209, na.rm = TRUE
    tail = cog[::-1][:min(5, n)]
    pB = math.nan if any(math.isnan(v) for v in tail) else _median(tail)      # :240, no na.rm
    fwd, costF = run(list(range(n)), pF)
    bwd, costB = run(list(range(n - 1, -1, -1)), pB)
    same = all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(fwd, bwd))
    if not same:
        tr["fb"].append((costF, costB))
    tr["direction"] = "forward" if costF < costB else "backward"
    return fwd if costF < costB else bwd


def _pick_none(C, cog, tr):
    """'none' (:110-113) as indices: which.min(|cand - centre of gravity|) per frame, None for an empty frame."""
    picks = []
    for f in range(len(C)):
        if not C[f]:
            picks.append(None)
            continue
        d = [abs(v - cog[f]) for v in C[f]]
        k = _which(d, False)
        _trace_pick(d, C[f], k, False, tr["choice"])
        picks.append(k)
    return picks


def cost_per_path(C, cog, picks, certWeight):
    """costPerPath(), :347-372, of the path that takes candidate picks[f] (0-based; None: no
    value, which both mean(..., na.rm = TRUE) leave out) of the packed, sorted log2
    candidates C[f]: certWeight * mean(|cand - cog|) + (1 - certWeight) * mean(costJumps of
    neighbouring frames). NaN where a mean has no term, as in the reference."""
    n = len(C)
    v = [math.nan if picks[f] is None else C[f][picks[f]] for f in range(n)]
    cert = [abs(v[f] - cog[f]) for f in range(n) if not math.isnan(v[f])]
    jump = [cost_jumps(v[f], v[f + 1]) for f in range(n - 1) if not (math.isnan(v[f]) or math.isnan(v[f + 1]))]
    return certWeight * _mean(cert) + (1 - certWeight) * _mean(jump)


def pathfinding_exact(C, cog, certWeight, tr):
    """pathfinding = 'exact', which the reference does not have: the picks (0-based indices,
    None for an empty frame) of the path that minimises costPerPath() (:347-372), the cost
    that 'slow' anneals, over the packed, sorted log2 candidates C of a segment of n >= 2
    frames. n_c frames have a candidate and n_j pairs of neighbouring frames both have one:
    the denominators of the reference's two means, which do not depend on the path. With wc =
    certWeight / n_c and wj = (1 - certWeight) / n_j the cost of a path is a sum along the
    chain, minimised by the recursion (in this order of operations, as sg_path.h's)
        D(f, i) = wc |C[f][i] - cog[f]|                      in the first frame of a run
        D(f, i) = wc |C[f][i] - cog[f]| + min_k (D(f - 1, k) + wj costJumps(C[f-1][k], C[f][i]))
    the lowest k winning ties; at the last frame of every maximal run of non-empty frames
    the lowest i with the least D is taken and the chosen k are followed back. n_j = 0 (every
    path costs NaN in the reference): the picks of 'none'. tr["exact"] receives every
    minimum taken, (the winner, the best of a different pitch value)."""
    tr.setdefault("exact", [])
    n = len(C)
    n_c = sum(1 for f in C if f)
    n_j = sum(1 for f in range(n - 1) if C[f] and C[f + 1])
    if n_j == 0:
        tr.setdefault("choice", [])
        return _pick_none(C, cog, tr)
    wc, wj = certWeight / n_c, (1 - certWeight) / n_j
    D, B = [None] * n, [None] * n
    for f in range(n):
        if not C[f]:
            continue
        D[f], B[f] = [], []
        for v in C[f]:
            node = wc * abs(v - cog[f])
            if f == 0 or not C[f - 1]:
                D[f].append(node)
                B[f].append(-1)
                continue
            t = [D[f - 1][k] + wj * cost_jumps(C[f - 1][k], v) for k in range(len(C[f - 1]))]
            k = _which(t, False)
            _trace_pick(t, C[f - 1], k, False, tr["exact"])
            D[f].append(node + t[k])
            B[f].append(k)
    picks = [None] * n
    at = -1
    for f in range(n - 1, -1, -1):
        if not C[f]:
            at = -1
            continue
        if at < 0:                                                            # the last frame of a run
            at = _which(D[f], False)
            _trace_pick(D[f], C[f], at, False, tr["exact"])
        picks[f] = at
        at = B[f][at]
    return picks


def _picks_of(C, path):
    """The index of each path value among its frame's candidates (the first of equal ones); None for NaN."""
    return [None if math.isnan(p) else C[f].index(p) for f, p in enumerate(path)]


def pathfinder_numpy(pitchCands, pitchCert, certWeight=0.5, pathfinding="fast", interpolWin=3, interpolTol=0.05,
                     interpolCert=0.3, snakeStep=0.05, _trace=None):
    """pathfinder(), R/utilities_pitch_postprocessing.R:28-132, for one voiced segment.
    pitchCands / pitchCert: per frame, the list of its non-NA candidates (Hz) and their
    certainties in pitch_matrices' order (the reference's NA-padded matrix columns; order()
    puts NA last and all-NA rows are dropped, so nrow is the largest count of a frame).
    Returns the pitch (Hz) per frame. The stated difference (see analyze_numpy): a frame
    that still has no candidate after interpolation keeps NaN, every other frame keeps its
    aligned choice, and the snake is not run on that segment. pathfinding = 'exact' is not in
    the reference: pathfinding_exact(), the minimum of the reference's costPerPath(), in the
    place of 'fast'. _trace (a dict) receives the sides (a, b) of the discrete comparisons
    (`exact`: the minima of pathfinding_exact), and C, cog (the packed, sorted log2 candidates
    and the centres of gravity), picks (the index taken per frame, None without a value)
    and cost (cost_per_path of the path handed to the snake)."""
    tr = _trace if _trace is not None else {}
    for k in ("band", "start", "choice", "fb", "maxiter", "delta", "force", "exact"):
        tr.setdefault(k, [])
    tr.update(interpolated=0, direction=None, iterations=0, rows=0)
    if pathfinding == "slow":
        raise NotImplementedError(_SLOW)
    n = len(pitchCands)
    C = [[math.log2(v) for v in f] for f in pitchCands]                       # :39
    A = [[float(a) for a in f] for f in pitchCert]
    cog = [_mean(f) for f in C]                                               # :43-49: `weights` is ignored
    if _num(interpolWin) and interpolWin > 0:                                 # interpolate(), :149-184
        W = int(interpolWin)
        for f in range(n):
            win = [v for v in cog[max(0, f - W):min(n - 1, f + W) + 1] if not math.isnan(v)]
            if not win:
                continue
            med = _median(win)
            lo, hi = (1 - interpolTol) * med, (1 + interpolTol) * med
            for c in C[f]:
                tr["band"] += [(c, lo), (c, hi)]
            if sum(1 for c in C[f] if c > lo and c < hi) == 0:
                C[f].append(med)
                A[f].append(float(interpolCert))
                cog[f] = _mean(C[f])
                tr["interpolated"] += 1
    for f in range(n):                                                        # :69-79 order(): stable
        o = sorted(range(len(C[f])), key=lambda k: C[f][k])
        C[f], A[f] = [C[f][k] for k in o], [A[f][k] for k in o]
    tr["rows"] = max(len(f) for f in C)
    tr.update(C=C, cog=cog)
    if tr["rows"] <= 1:                                                       # :87-89
        tr["picks"] = [0 if f else None for f in C]
        tr["cost"] = cost_per_path(C, cog, tr["picks"], certWeight)
        return [2.0 ** f[0] if f else math.nan for f in C]
    if n >= 2 and pathfinding == "fast":                                      # :93-100
        path = pathfinding_fast(C, A, cog, certWeight, tr)
        tr["picks"] = _picks_of(C, path)
    else:
        if n >= 2 and pathfinding == "exact":                                 # not in the reference
            tr["picks"] = pathfinding_exact(C, cog, certWeight, tr)
        else:                                                                 # :110-113
            tr["picks"] = _pick_none(C, cog, tr)
        path = [math.nan if k is None else C[f][k] for f, k in enumerate(tr["picks"])]
    tr["cost"] = cost_per_path(C, cog, tr["picks"], certWeight)
    if _num(snakeStep) and snakeStep > 0 and all(len(f) for f in C):          # snake(), :419-475
        flat = [v for f in C for v in f]
        q = (max(flat) - min(flat)) / snakeStep * 2                           # :426-427
        tr["maxiter"].append((q, float(np.round(q))))
        maxIter = math.floor(q)
        i, force_old = 1, 1e10
        while i < maxIter:
            force = force_per_path(path, C, A, certWeight, tr["force"])
            force_new = _mean([abs(v) for v in force])
            force_delta = (force_old - force_new) / force_old if force_old else math.nan
            force_old = force_new
            if not math.isnan(force_delta):
                tr["delta"].append((force_delta, snakeStep))
            if math.isnan(force_delta) or force_delta < snakeStep:
                break
            path = [p + snakeStep * v for p, v in zip(path, force)]
            i += 1
            tr["iterations"] += 1
    return [2.0 ** p for p in path]


def median_smoother(x, smoothing_ww, smoothingThres, _pairs=None):
    """medianSmoother(), :584-600, for one column: the medians read the unsmoothed copy
    and the test is abs(deviance - 1)."""
    x = np.array(x, float)
    temp = x.copy()
    hw = int(math.floor(smoothing_ww / 2))
    n = len(x)
    for i in range(n):
        win = temp[max(i - hw, 0):min(i + hw, n - 1) + 1]
        win = win[~np.isnan(win)]
        if not len(win) or math.isnan(x[i]):
            continue
        med = _median([float(v) for v in win])
        with np.errstate(invalid="ignore", divide="ignore"):
            deviance = float(12 * np.log2(np.float64(x[i]) / np.float64(med)))
        if math.isnan(deviance):
            continue
        if _pairs is not None:
            _pairs.append((abs(deviance - 1), smoothingThres))
        if abs(deviance - 1) > smoothingThres:
            x[i] = med
    return x


def repair_track(s, priorMean="default", priorSD=6, priorPlot=False, minVoicedCands="autom", shortestSyl=20,
                 shortestPause=60, interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast", certWeight=.5,
                 snakeStep=0.05, snakePlot=False, smooth=1, smoothVars=SMOOTH_VARS, plot=False):
    """The settings of analyze()'s tail (R/analyze.R:593-681) added to repair_pitch()'s
    dict s. What is out of scope raises here, before anything runs."""
    if plot or priorPlot or snakePlot:
        raise NotImplementedError("analyze(plot = TRUE / priorPlot = TRUE / snakePlot = TRUE): plotting is out of scope")
    if priorMean == "default":
        priorMean = hz_to_semitones(300)
    if isinstance(smoothVars, str):
        smoothVars = (smoothVars,)
    smoothVars = tuple(smoothVars or ())
    for v in smoothVars:
        if v not in SMOOTH_VARS:
            raise NotImplementedError("smoothVars = %r: only 'pitch' and 'dom' are smoothed" % (v,))
    if pathfinding not in PATHFINDING:
        raise ValueError("pathfinding must be one of %s" % (PATHFINDING,))
    prior = _num(priorMean) and _num(priorSD)                                 # :598
    if prior and not (priorMean > 0 and priorSD > 0):
        raise ValueError("analyze: priorMean and priorSD must be positive (dgamma gives NaN in the reference)")
    m = s["pitchMethods"]
    if not _num(minVoicedCands) or minVoicedCands < 1 or minVoicedCands > len(m):  # :615-624
        minVoicedCands = 2 if ("dom" in m and len(m) > 1) else 1
    for k, v in (("shortestSyl", shortestSyl), ("shortestPause", shortestPause), ("interpolTol", interpolTol),
                 ("interpolCert", interpolCert), ("certWeight", certWeight)):
        if not _num(v) or math.isnan(v):
            raise ValueError("analyze: %s must be a number" % k)
    if shortestPause < 0:
        raise ValueError("analyze: shortestPause must not be negative")
    if not (0 <= certWeight <= 1):
        raise ValueError("analyze: certWeight must lie in [0, 1]")
    if not _num(interpolWin):
        interpolWin = 0                                                       # !is.numeric(interpolWin): no interpolation
    if interpolWin != math.floor(interpolWin):
        raise ValueError("analyze: interpolWin must be a whole number (f - interpolWin indexes frames)")
    interpolWin = max(int(interpolWin), 0)
    if not _num(snakeStep) or math.isnan(snakeStep) or snakeStep <= 0:
        snakeStep = 0.0
    if not _num(smooth) or math.isnan(smooth) or smooth <= 0:
        smooth = 0.0
    s = dict(s)
    s.update(priorMean=float(priorMean) if prior else None, priorSD=float(priorSD) if prior else None,
             minVoicedCands=int(math.ceil(minVoicedCands)), shortestSyl=shortestSyl, shortestPause=shortestPause,
             noRequired=int(min(max(1, math.ceil(shortestSyl / s["step"])), 2 ** 30)),  # :633
             nToleratedNA=int(min(math.floor(shortestPause / s["step"]), 2 ** 30)),    # :636
             interpolWin=interpolWin, interpolTol=float(interpolTol), interpolCert=float(interpolCert),
             pathfinding=pathfinding, certWeight=float(certWeight), snakeStep=float(snakeStep), smooth=float(smooth),
             smoothVars=smoothVars)
    return s


def smoothing_hw(smooth, frames, length, samplingRate):
    """floor(smoothing_ww / 2) with smoothing_ww = round(smooth * nrow / duration / 10)
    (R/analyze.R:671-673; R's round goes half to even); 0 without smoothing."""
    if not smooth > 0 or frames <= 0:
        return 0
    duration = length / samplingRate
    return int(math.floor(float(np.round(smooth * (frames / duration) / 10)) / 2))


def track_decisions(length, s):
    """pitch_decisions() plus the integers of the tail for repair_track()'s dict s: what
    sg_analyze_size makes bit-equal."""
    d = pitch_decisions(length, s)
    d.update(cols=NFIXED + 6 * s["nCands"] + len(TRACK_COLUMNS), minVoicedCands=s["minVoicedCands"],
             noRequired=s["noRequired"], nToleratedNA=s["nToleratedNA"], interpolWin=s["interpolWin"],
             hw=smoothing_hw(s["smooth"], d["frames"], length, s["samplingRate"]))
    if s["pathfinding"] == "slow":
        raise native.SoundgenError(-4, "analyze: pathfinding = 'slow' (simulated annealing on R's random stream) is not built")
    if s["interpolWin"] > PATH_MAX_WIN or d["hw"] > PATH_MAX_WIN:
        raise native.SoundgenError(-4, "analyze: interpolWin and half the smoothing window may be at most %d frames"
                                   % PATH_MAX_WIN)
    if 0 < s["snakeStep"] < SNAKE_MIN_STEP:
        raise native.SoundgenError(-4, "analyze: snakeStep below %g is not supported" % SNAKE_MIN_STEP)
    return d


def _track(t, s, length, S=None, lab=None, probe=None):
    """R/analyze.R:576-703 on a pitch_candidates() table t (changed in place and returned)."""
    probe = {} if probe is None else probe
    probe.update(segments=[], smooth=[], harm=[])
    frames = len(t["ampl"])
    cands, cert, _, _ = pitch_matrices(t)                                     # :578-591
    per = [[(cands[r, f], cert[r, f]) for r in range(cands.shape[0]) if not math.isnan(cands[r, f])]
           for f in range(frames)]
    if s["priorMean"] is not None:                                            # :598-612
        prior = prior_setup(s["priorMean"], s["priorSD"], s["pitchFloor"], s["pitchCeiling"])
        per = [[(c, a * prior_multiplier(c, prior)) for c, a in f] for f in per]
    segs = find_voiced_segments([len(f) for f in per], s["minVoicedCands"], s["noRequired"], s["nToleratedNA"])  # :625-632
    pitch = np.full(frames, math.nan)
    for a, b in segs:                                                         # :635-654
        tr = {}
        pitch[a - 1:b] = pathfinder_numpy([[c for c, _ in f] for f in per[a - 1:b]], [[w for _, w in f] for f in per[a - 1:b]],
                                          s["certWeight"], s["pathfinding"], s["interpolWin"], s["interpolTol"],
                                          s["interpolCert"], s["snakeStep"], tr)
        tr.update(start_frame=a, end_frame=b)
        probe["segments"].append(tr)
    t["pitch"] = pitch
    if s["smooth"] > 0:                                                       # :670-681
        duration = length / s["samplingRate"]
        ww = float(np.round(s["smooth"] * (frames / duration) / 10))
        for k in s["smoothVars"]:
            t[k] = median_smoother(t[k], ww, 4 / s["smooth"], probe["smooth"])
    voiced = ~np.isnan(t["pitch"])                                            # :685-691
    t["amplVoiced"] = np.where(voiced, t["ampl"], math.nan)
    for k in ("quartile25", "quartile50", "quartile75"):
        t[k] = np.where(voiced, t[k], math.nan)
    t["voiced"] = voiced
    harm = np.full(frames, math.nan)
    if S is not None:                                                         # :694-699
        for f in np.nonzero(voiced)[0]:
            threshold = 1.25 * t["pitch"][f] / 1000
            probe["harm"] += [(float(v), threshold) for v in lab]
            harm[f] = np.sum(S[lab > threshold, f]) / np.sum(S[:, f])
    t["HNR"] = to_dB(t["HNR"])                                                # :702-703
    t["harmonics"] = to_dB(harm)
    return t


def _track_args(a):
    return {k: a[k] for k in ("priorMean", "priorSD", "priorPlot", "minVoicedCands", "shortestSyl", "shortestPause",
                              "interpolWin", "interpolTol", "interpolCert", "pathfinding", "certWeight", "snakeStep",
                              "snakePlot", "smooth", "smoothVars", "plot")}


def analyze_numpy(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian", zp=0,
                  cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6, pitchFloor=75, pitchCeiling=3500,
                  priorMean="default", priorSD=6, priorPlot=False, nCands=1, minVoicedCands="autom", domThres=0.1,
                  domSmooth=220, autocorThres=0.7, autocorSmooth=None, cepThres=0.3, cepSmooth=None, cepZp=0,
                  specThres=0.3, specPeak=0.35, specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150, specMerge=1,
                  shortestSyl=20, shortestPause=60, interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast",
                  certWeight=.5, snakeStep=0.05, snakePlot=False, smooth=1, smoothVars=SMOOTH_VARS, plot=False,
                  summary=False, _probe=None):
    """analyze() (R/analyze.R:153-707) restated on the host: pitch_candidates_numpy(), then
    statement by statement pitch_matrices (:578-591), the prior (:598-612; priorMean
    'default' is HzToSemitones(300), None skips it), minVoicedCands 'autom' (:615-624),
    findVoicedSegments, pathfinder per segment, medianSmoother (:670-681) and the final
    columns (:685-703). Returns pitch_candidates_numpy()'s dict with pitch, voiced,
    amplVoiced and harmonics added, HNR and harmonics in dB, dom (and pitch) smoothed and
    the quartiles blanked for unvoiced frames. summary=True (:770-796) returns
    summarize_table_numpy() of that table instead.

    Quirks kept (what the statements do):
        * mean(x, weights = ...) ignores `weights`: the centre of gravity is a plain mean;
        * point_current is never updated in either loop of pathfinding_fast;
        * the backward start's median has no na.rm, and its which.max indexes the
          na.omit-ed vector;
        * a candidate exactly equal to the snake's point pushes with -cert (cands >
          pitch[i] is false);
        * the smoother tests abs(deviance - 1), not abs(deviance);
        * analyze() passes interpolTol = 0.3, not the pathfinder's 0.05, and the
          tolerance multiplies a log2 value;
        * force_old starts at 1e10;
        * maxIter = floor(ran / snakeStep * 2), and the loop runs while i < maxIter.
    The one stated difference: a frame of a voiced segment can have no candidate when
    interpolate() is not run (interpolWin = 0 or not numeric; with interpolWin >= 1 every
    gap is filled, because a filled frame enters the next frame's median). In the reference 'fast' then skips the frame and assigns a misaligned, recycled
    path, and 'none' stops in apply(). Here the frame keeps NaN pitch and every other
    frame keeps its aligned choice; everything before that is restated as written
    (including the backward pass from a NaN median: no start, the last frame NaN,
    cost_pitchJump 0), and the snake is not run on that segment (in the reference its
    first force_new is NA and it breaks at once).
    Added to the reference: pathfinding = 'exact' (pathfinding_exact(): the path that
    minimises the reference's own costPerPath(), which 'slow' approximates by annealing;
    deterministic, by dynamic programming).
    Out of scope: pathfinding = 'slow' (simulated annealing through optim() on R's random
    stream) and smoothVars outside ('pitch', 'dom') raise NotImplementedError, as do the
    plots; the columns pitchAutocor / pitchCep / pitchSpec (:659-667, as.numeric of
    zero-length list elements, which cannot be settled without R), formants and savePath
    are not built.

    _probe (a dict) receives pitch_candidates_numpy()'s intermediates and `segments`
    (per voiced segment the sides (a, b) of every discrete comparison: `band` the
    interpolation band test per candidate, `start` the start which.max, `choice` each
    frame's which.min, best against the best of a different pitch value, `fb` forward
    against backward cost, `maxiter` ran / snakeStep * 2 against the nearest integer,
    `delta` each force_delta against snakeStep, `force` each cands > pitch[i]), `smooth`
    (the smoother's threshold tests) and `harm` (each label against the threshold)."""
    sound, sr = _input(x, samplingRate)
    a = locals()
    if pathfinding == "slow":
        raise NotImplementedError(_SLOW)
    s = repair_track(repair_pitch(sr, len(sound) / sr, **_pitch_args(a)), **_track_args(a))
    probe = {} if _probe is None else _probe
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # repair_pitch() has warned already
        t = pitch_candidates_numpy(sound, sr, _probe=probe, **_pitch_args(a))
    d = probe["d"]
    t = _track(t, s, len(sound), probe["S"], freq_labels(sr, d["wl"], d["bins"]), probe)
    return summarize_table_numpy(t) if summary else t


def pitch_path_numpy(table, step, samplingRate, pitchMethods=PITCH_DEFAULT_METHODS, pitchFloor=75, pitchCeiling=3500,
                     priorMean="default", priorSD=6, minVoicedCands="autom", shortestSyl=20, shortestPause=60,
                     interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast", certWeight=.5, snakeStep=0.05,
                     smooth=1, smoothVars=SMOOTH_VARS, _probe=None):
    """analyze_numpy()'s tail from a caller-given table shaped as pitch_candidates()'
    (ampl, HNR, dom, the quartiles, domCand / domCert, the *Cand / *Cert groups present,
    and `duration` in s): a copy with pitch, voiced, amplVoiced added, HNR in dB, dom
    smoothed, the quartiles blanked; harmonics is all NaN (it needs the spectrum).
    step (ms) and pitchMethods decide the segment settings as in analyze()."""
    if pathfinding == "slow":
        raise NotImplementedError(_SLOW)
    t = {k: np.array(v, float) for k, v in table.items()}
    s = _path_settings(t, step, samplingRate, locals())
    return _track(t, s, _path_length(t, samplingRate), probe=_probe)


def _path_length(t, samplingRate):
    return int(round(float(t["duration"][0]) * samplingRate)) if len(t["ampl"]) else 0


def _path_settings(t, step, samplingRate, a):
    nC = t["autocorCand"].shape[1] if "autocorCand" in t and np.ndim(t["autocorCand"]) == 2 else 1
    m = a["pitchMethods"]
    base = dict(samplingRate=samplingRate, step=float(step), pitchMethods=(m,) if isinstance(m, str) else tuple(m),
                pitchFloor=a["pitchFloor"], pitchCeiling=a["pitchCeiling"], nCands=nC)
    kw = {k: a[k] for k in ("priorMean", "priorSD", "minVoicedCands", "shortestSyl", "shortestPause", "interpolWin",
                            "interpolTol", "interpolCert", "pathfinding", "certWeight", "snakeStep", "smooth", "smoothVars")}
    return repair_track(base, **kw)


# ------------------------------------------------- analyze() on the GPU (sg_anl_path, sg_anl_harm)
TRACK_SIZE_KEYS = ("minVoicedCands", "noRequired", "nToleratedNA", "hw", "interpolWin")


def _track_params(s, pitch=True):
    """sg_analyze_params_full of repair_track()'s dict; pitch=False (pitch_path) fills
    only what the tail reads."""
    from . import _abi
    P = _abi.sg_analyze_params_full()
    if pitch:
        P.p = _pitch_params(s)
    else:
        m = s["pitchMethods"]
        P.p.a.samplingRate, P.p.a.step, P.p.a.nCands = float(s["samplingRate"]), float(s["step"]), float(s["nCands"])
        P.p.a.pitchFloor, P.p.a.pitchCeiling = float(s["pitchFloor"]), float(s["pitchCeiling"])
        P.p.a.methods = sum(b for k, b in (("autocor", 1), ("dom", 2), ("cep", 4), ("spec", 8)) if k in m)
    P.priorMean = math.nan if s["priorMean"] is None else s["priorMean"]
    P.priorSD = math.nan if s["priorSD"] is None else s["priorSD"]
    P.minVoicedCands = float(s["minVoicedCands"])
    P.shortestSyl, P.shortestPause = float(s["shortestSyl"]), float(s["shortestPause"])
    P.interpolWin, P.interpolTol, P.interpolCert = float(s["interpolWin"]), s["interpolTol"], s["interpolCert"]
    P.certWeight, P.snakeStep, P.smooth = s["certWeight"], s["snakeStep"], s["smooth"]
    P.pathfinding = PATHFINDING.index(s["pathfinding"])
    P.smoothVars = sum(b for k, b in (("pitch", 1), ("dom", 2)) if k in s["smoothVars"])
    return P


def track_decisions_native(length, s):
    """sg_analyze_size (host only): the library's track_decisions()."""
    L = native.lib()
    P = _track_params(s)
    frames, cols = C.c_int32(), C.c_int32()
    extra = (C.c_int32 * 8)()
    rc = L.sg_analyze_size(int(length), C.byref(P), C.byref(frames), C.byref(cols), extra)
    _host_check(rc)
    d = pitch_decisions_native(length, s)
    d.update(zip(TRACK_SIZE_KEYS, extra))
    d.update(frames=frames.value, cols=cols.value)
    return d


def _track_frames_native(length, P):
    L = native.lib()
    fr, cl = C.c_int32(), C.c_int32()
    rc = L.sg_analyze_size(int(length), C.byref(P), C.byref(fr), C.byref(cl), None)
    _host_check(rc)
    return fr.value


def _track_table(m, nC, length, sr, step):
    """frames x (15 + 6 nCands + 4) device rows -> the dict analyze_numpy() returns."""
    t = _pitch_table(m, nC, length, sr, step)
    c0 = NFIXED + 6 * nC
    for i, k in enumerate(TRACK_COLUMNS):
        t[k] = m[:, c0 + i].copy()
    t["voiced"] = t["voiced"] == 1
    return t


def analyze(x, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50, wn="gaussian", zp=0,
            cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6, pitchFloor=75, pitchCeiling=3500,
            priorMean="default", priorSD=6, priorPlot=False, nCands=1, minVoicedCands="autom", domThres=0.1,
            domSmooth=220, autocorThres=0.7, autocorSmooth=None, cepThres=0.3, cepSmooth=None, cepZp=0, specThres=0.3,
            specPeak=0.35, specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150, specMerge=1, shortestSyl=20,
            shortestPause=60, interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast", certWeight=.5,
            snakeStep=0.05, snakePlot=False, smooth=1, smoothVars=SMOOTH_VARS, plot=False, device=0,
            summary=False, formants=False, nFormants=3):
    """analyze() (R/analyze.R:153-707) on the GPU (sg_analyze, fp64): pitch_candidates()'
    dict plus pitch (the pathfinder's contour through the voiced segments, smoothed),
    voiced, amplVoiced and harmonics, with HNR and harmonics in dB, dom smoothed and the
    quartiles blanked for unvoiced frames. The candidates are made and consumed in one
    launch sequence (sg_anl_path: one 64-lane workgroup per sound; sg_anl_harm). The
    quirks kept, the one stated difference from the reference and what is out of scope
    (pathfinding = 'slow', pitchAutocor / pitchCep / pitchSpec, formants, plots, savePath)
    are listed at analyze_numpy(), which this is compared against. pathfinding = 'exact' is
    not in the reference: the path that minimises its costPerPath() (pathfinding_exact();
    sg_anl_path_exact), which 'slow' approximates; path_costs() reports what a path costs. plot defaults to False;
    True raises (with summary=True too, before anything runs). summary=True (R/analyze.R:
    770-796) returns the sound's summary row instead, a dict of the 44 floats named by
    SUMMARY_COLUMNS (see summarize_table_numpy): sg_anl_summary makes it from the table in
    the same launch sequence (sg_analyze_summary_sound) and only the row leaves the device.

    formants=True (default False: the table and the row are then what they were) adds the
    reference's formant columns f1_freq, f1_width, ..., 2 nFormants of them (R/analyze.R:486-502,
    formants.py; unpinned against phonTools), from a second launch sequence behind the gate
    (sg_formants_sound). With summary=True the 6 nFormants cells f1_freq_mean, f1_freq_median,
    f1_freq_sd, f1_width_mean, ... follow the 44, reduced on the host from the formant table
    (formants.formant_summary). nFormants is read only with formants=True."""
    sound, sr = _input(x, samplingRate)
    a = locals()
    s = repair_track(repair_pitch(sr, len(sound) / sr, **_pitch_args(a)), **_track_args(a))
    if formants:
        from . import formants as _fm
        nFormants = _fm._check_n(nFormants)
        _fm.formants_size(dict(s, pitchMethods=PITCH_METHODS), nFormants)  # refused before anything runs
        res = analyze(**dict({k: a[k] for k in list(_pitch_args(a)) + list(_track_args(a))}, x=sound, samplingRate=sr,
                             device=device, summary=summary))
        ft = _fm._dict(_fm._formants_sound(sound, s, nFormants, device), nFormants)
        res.update(_fm.formant_summary(ft, nFormants) if summary else ft)
        return res
    if summary:
        d = track_decisions_native(len(sound), s)
        if len(sound) <= d["wl"]:
            raise _too_short(len(sound), d["wl"])
        ctx = native.default_context(device)
        sound = np.ascontiguousarray(sound)
        row = np.zeros(len(SUMMARY_COLUMNS))
        dp = C.POINTER(C.c_double)
        P = _track_params(s)
        _check(native.lib().sg_analyze_summary_sound(ctx.ptr, sound.ctypes.data_as(dp), len(sound), C.byref(P), None,
                                                     row.ctypes.data_as(dp)), ctx.ptr)
        return dict(zip(SUMMARY_COLUMNS, (float(v) for v in row)))
    return _run(sound, sr, s, track_decisions_native, _track_params, _track_table, "sg_analyze", device)


def analyze_batch(data, offsets, lengths, samplingRate, silence=0.04, windowLength=50, step=None, overlap=50,
                  wn="gaussian", zp=0, cutFreq=6000, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6, pitchFloor=75,
                  pitchCeiling=3500, priorMean="default", priorSD=6, priorPlot=False, nCands=1, minVoicedCands="autom",
                  domThres=0.1, domSmooth=220, autocorThres=0.7, autocorSmooth=None, cepThres=0.3, cepSmooth=None, cepZp=0,
                  specThres=0.3, specPeak=0.35, specSinglePeakCert=0.4, specHNRslope=0.8, specSmooth=150, specMerge=1,
                  shortestSyl=20, shortestPause=60, interpolWin=3, interpolTol=0.3, interpolCert=0.3, pathfinding="fast",
                  certWeight=.5, snakeStep=0.05, snakePlot=False, smooth=1, smoothVars=SMOOTH_VARS, plot=False,
                  to_host=False, device=0, summary=False, formants=False, nFormants=3):
    """analyze(call i, samplingRate, ...) for a batch of sounds already in HBM, laid out
    and returned as pitch_candidates_batch() does (sg_analyze_batch, one launch sequence,
    tables left in HBM). A row has 15 + 6 nCands + 4 columns: `columns` names those of
    pitch_candidates_batch(), then pitch, amplVoiced, voiced (0 / 1) and harmonics. A
    call's table equals analyze()'s bit for bit. to_host=True returns the list of per-call
    dicts analyze() returns.

    summary=True (R/analyze.R:770-796, sg_analyze_summary_batch): sg_anl_summary follows in
    the same launch sequence and the tables never leave HBM. Returns a dict with `out` (an
    fp64 CUDA tensor of shape (n_calls, 44): row i is analyze(call i, summary=True) bit for
    bit, whatever the batch and the call's place in it), `columns` (SUMMARY_COLUMNS) and
    `frames`, and also the tables as above under `tables`, `offsets` and `cols`. A call
    with no frames (not longer than the window, or a failed call of length < 0) has a row
    of NaN. to_host=True then returns the list of per-call dicts of 44 named floats.

    formants=True (default False): sg_formants_batch runs behind the finished tables (formants.py).
    The returned dict gains `formants`, the dict formants_batch() returns (the formant tables
    next to the main ones, in HBM); with summary=True also `formant_cells` (a host array of
    shape (n_calls, 6 nFormants), reduced on the host from the formant tables) and
    `formant_columns`. to_host=True: the per-call dicts gain analyze(formants=True)'s keys."""
    a = locals()
    s = repair_track(repair_pitch(samplingRate, None, **_pitch_args(a)), **_track_args(a))
    if formants:
        from . import formants as _fm
        nFormants = _fm._check_n(nFormants)
        _fm.formants_size(dict(s, pitchMethods=PITCH_METHODS), nFormants)
        kw = dict(_pitch_args(a), **_track_args(a))
        res = analyze_batch(data, offsets, lengths, samplingRate, to_host=False, device=device, summary=summary, **kw)
        tabs = res["tables"] if summary else res["out"]
        out, foff = _fm.formants_behind(data, offsets, lengths, s, nFormants, tabs, res["offsets"], res["cols"], res["frames"],
                                        device)
        res["formants"] = dict(out=out, offsets=foff[:-1].copy(), frames=res["frames"], cols=2 * nFormants,
                               columns=_fm.formant_columns(nFormants))
        if not summary and not to_host:
            return res
        fts = [_fm._dict(m, nFormants) for m in _fm._host_tables(out, foff, res["frames"], nFormants)]
        if summary:
            cells = [_fm.formant_summary(ft, nFormants) for ft in fts]
            if not to_host:
                res["formant_columns"] = tuple(cells[0]) if cells else ()
                res["formant_cells"] = np.array([list(c.values()) for c in cells], float).reshape(len(cells), 6 * nFormants)
                return res
            return [dict(r, **c) for r, c in zip(_host_rows(res["out"]), cells)]
        tables = _host_tables(tabs, res["frames"], res["cols"], _track_table, s["nCands"], np.asarray(lengths, dtype=np.int64),
                              samplingRate, s["step"])
        return [dict(t, **ft) for t, ft in zip(tables, fts)]
    return _run_batch(data, offsets, lengths, samplingRate, s, _track_frames_native, _track_params, _track_table,
                      ("autocorCand", "autocorCert") + PITCH_KEYS, "sg_analyze", to_host, device, TRACK_COLUMNS,
                      summary=bool(summary))


def pitch_path(table, step, samplingRate, pitchMethods=PITCH_DEFAULT_METHODS, pitchFloor=75, pitchCeiling=3500,
               priorMean="default", priorSD=6, minVoicedCands="autom", shortestSyl=20, shortestPause=60, interpolWin=3,
               interpolTol=0.3, interpolCert=0.3, pathfinding="fast", certWeight=.5, snakeStep=0.05, smooth=1,
               smoothVars=SMOOTH_VARS, device=0):
    """pitch_path_numpy() on the GPU (sg_pitch_path: sg_anl_path alone): analyze()'s tail
    from a caller-given pitch_candidates()-shaped table (a host dict; a *Cand / *Cert
    group that is absent counts as all NaN). Returns a copy with pitch, voiced, amplVoiced
    added, HNR in dB, dom smoothed, the quartiles blanked; harmonics is all NaN."""
    return _pitch_path(table, step, samplingRate, locals(), device, False)


def path_costs(table, step, samplingRate, pitchMethods=PITCH_DEFAULT_METHODS, pitchFloor=75, pitchCeiling=3500,
               priorMean="default", priorSD=6, minVoicedCands="autom", shortestSyl=20, shortestPause=60, interpolWin=3,
               interpolTol=0.3, interpolCert=0.3, pathfinding="fast", certWeight=.5, snakeStep=0.05, smooth=1,
               smoothVars=SMOOTH_VARS, device=0):
    """pitch_path() plus what the pathfinder's choice cost (sg_pitch_path_costs): (table,
    segments), the table as pitch_path() returns it and, per voiced segment in order, a
    dict of start_frame and end_frame (1-based), rows (the largest number of candidates in
    a frame after interpolation) and cost: the reference's costPerPath() (cost_per_path())
    of the path handed to the snake, NaN where it is NaN in the reference (a one-frame
    segment; no two neighbouring frames with a value). Any pathfinding that pitch_path()
    takes: the difference between 'fast' and 'exact' is what 'fast' leaves on the table."""
    return _pitch_path(table, step, samplingRate, locals(), device, True)


def _pitch_path(table, step, samplingRate, a, device, costs):
    t = {k: np.array(v, float) for k, v in table.items()}
    s = _path_settings(t, step, samplingRate, a)
    frames, nC = len(t["ampl"]), s["nCands"]
    length = _path_length(t, samplingRate)
    m = np.full((frames, NFIXED + 6 * nC), math.nan)
    for i, k in enumerate(COLUMNS):
        if k in t:
            m[:, i] = t[k]
    for i, k in enumerate(("autocorCand", "autocorCert") + PITCH_KEYS):
        if k in t:
            m[:, NFIXED + i * nC:NFIXED + (i + 1) * nC] = np.reshape(t[k], (frames, nC))
    P = _track_params(s, pitch=False)
    out = np.zeros(max(frames, 1) * (m.shape[1] + len(TRACK_COLUMNS)))
    ctx = native.default_context(device)
    dp = C.POINTER(C.c_double)
    m = np.ascontiguousarray(m)
    if costs:
        seg, nseg = np.zeros(4 * max(frames, 1)), C.c_int32()
        _check(native.lib().sg_pitch_path_costs(ctx.ptr, m.ctypes.data_as(dp), frames, int(length), C.byref(P),
                                                out.ctypes.data_as(dp), seg.ctypes.data_as(dp), C.byref(nseg)), ctx.ptr)
    else:
        _check(native.lib().sg_pitch_path(ctx.ptr, m.ctypes.data_as(dp), frames, int(length), C.byref(P),
                                          out.ctypes.data_as(dp)), ctx.ptr)
    o = out[:frames * (m.shape[1] + 4)].reshape(frames, m.shape[1] + 4)
    for i, k in enumerate(COLUMNS):
        t[k] = o[:, i].copy()
    for i, k in enumerate(TRACK_COLUMNS):
        t[k] = o[:, m.shape[1] + i].copy()
    t["voiced"] = t["voiced"] == 1
    if costs:
        return t, [dict(start_frame=int(v[0]), end_frame=int(v[1]), rows=int(v[2]), cost=float(v[3]))
                   for v in seg[:4 * nseg.value].reshape(-1, 4)]
    return t


# ------------------------------------------------- analyze(summary = TRUE), analyzeFolder()
# vars (R/analyze.R:771-772) for the columns this table has: sort() of the column names (:706-707) under a
# case-insensitive collation such as en_US, less `voiced`
SUMMARY_VARS = ("ampl", "amplVoiced", "dom", "entropy", "harmonics", "HNR", "meanFreq", "peakFreq", "peakFreqCut", "pitch",
                "quartile25", "quartile50", "quartile75", "specSlope")
SUMMARY_COLUMNS = ("duration", "voiced") + tuple(v + "_" + k for v in SUMMARY_VARS for k in ("mean", "median", "sd"))


def summarize_table_numpy(table):
    """analyze()'s summary row (R/analyze.R:770-796) of an analyze()-shaped dict, restated
    on the host: a dict of the 44 floats named by SUMMARY_COLUMNS. duration is
    result$duration[1], in s (the reference's comment says ms; the value is not); voiced is
    mean(result$voiced); then <var>_mean, <var>_median, <var>_sd over the frames where the
    variable is not NA, in R's arithmetic (segment.py's r_mean, r_median, r_sd: NaN for no
    value, sd NaN for fewer than two; +-Inf, which HNR and harmonics can hold, are ordinary
    values: mean(c(Inf, 1)) is Inf, its sd NaN, its median finite).

    The variables are those of `result` that this table has, in the order sort() gives their
    names (:706-707) under a case-insensitive collation such as en_US; that order leaves
    `voiced` last, so myseq (:787) is aligned with vars (:771-772). Under the C locale HNR
    would come first: the names identify the cells, not the positions. The values are the
    final table's (HNR and harmonics in dB, dom and pitch smoothed, the quartiles blanked
    for unvoiced frames). Absent, with their columns: the pitchAutocor / pitchCep / pitchSpec
    and the formant groups. domCand, domCert, the *Cand / *Cert groups and cond_* are not
    columns of the reference's result and are not summarised. A table without frames (the
    reference stops before it has one) gives 44 NaN."""
    from .segment import r_mean, r_median, r_sd
    out = dict.fromkeys(SUMMARY_COLUMNS, math.nan)                            # :773-785
    frames = len(table["ampl"])
    if frames == 0:
        return out
    out["duration"] = float(np.asarray(table["duration"], float)[0])          # :788
    out["voiced"] = float(np.sum(np.asarray(table["voiced"]) != 0) / frames)  # :789
    with np.errstate(invalid="ignore", over="ignore"):
        for v in SUMMARY_VARS:                                                # :791-796
            x = np.asarray(table[v], float)
            x = x[~np.isnan(x)]                                               # na.rm = TRUE
            out[v + "_mean"], out[v + "_median"], out[v + "_sd"] = r_mean(x), r_median(x), r_sd(x)
    return out


def _whole_ratio(duration):
    """(len, samplingRate) as whole numbers with len / samplingRate == duration bit for bit:
    what summarize_table() hands the kernel, which divides them, when it is not told the
    rate. Exact for a duration that is a sample count over a whole rate up to 1e6 Hz."""
    from fractions import Fraction
    r = Fraction(float(duration)).limit_denominator(1000000)
    if r.numerator / r.denominator != float(duration):
        raise ValueError("summarize_table: the table's duration is not a sample count over a whole sampling rate; "
                         "pass samplingRate")
    return r.numerator, float(r.denominator)


def summarize_table(table, device=0, samplingRate=None):
    """summarize_table_numpy() on the GPU (sg_analyze_summary: sg_anl_summary alone, the
    counterpart of pitch_path()): the summary row of an analyze()-shaped host dict (a
    *Cand / *Cert group that is absent counts as all NaN; they are not summarised). The
    kernel writes duration as length / samplingRate: with samplingRate the length is
    round(duration * samplingRate); without it the two are the whole-number ratio that
    gives table['duration'][0] back bit for bit."""
    frames = len(table["ampl"])
    ac = np.asarray(table["autocorCand"], float) if "autocorCand" in table else None
    nC = ac.shape[1] if ac is not None and ac.ndim == 2 else 1
    cols = NFIXED + 6 * nC + len(TRACK_COLUMNS)
    m = np.full((frames, cols), math.nan)
    for i, k in enumerate(COLUMNS):
        if k in table:
            m[:, i] = table[k]
    for i, k in enumerate(("autocorCand", "autocorCert") + PITCH_KEYS):
        if k in table:
            m[:, NFIXED + i * nC:NFIXED + (i + 1) * nC] = np.reshape(table[k], (frames, nC))
    for i, k in enumerate(TRACK_COLUMNS):
        if k in table:
            m[:, NFIXED + 6 * nC + i] = table[k]
    if frames == 0:
        length, sr = 0, 1.0 if samplingRate is None else float(samplingRate)
    elif samplingRate is None:
        length, sr = _whole_ratio(np.asarray(table["duration"], float)[0])
    else:
        length, sr = _path_length(table, samplingRate), float(samplingRate)
    m = np.ascontiguousarray(m)
    row = np.zeros(len(SUMMARY_COLUMNS))
    ctx = native.default_context(device)
    dp = C.POINTER(C.c_double)
    _check(native.lib().sg_analyze_summary(ctx.ptr, m.ctypes.data_as(dp), frames, cols, nC, int(length), sr,
                                           row.ctypes.data_as(dp)), ctx.ptr)
    return dict(zip(SUMMARY_COLUMNS, (float(v) for v in row)))


def summary_columns_native():
    """The library's names of a summary row's cells (sg_analyze_summary_name; host only)."""
    L = native.lib()
    out = []
    while True:
        name = L.sg_analyze_summary_name(len(out))
        if name is None:
            return tuple(out)
        out.append(name.decode())


def folder_groups(myfolder, device=0):
    """The sounds of a folder on the device, as analyze_folder() documents it: (names, paths,
    groups). names: the files that end in '.wav', sorted; groups: one dict per sampling rate,
    in ascending order of the rates, with `samplingRate`, `files` (indices into names),
    `offsets`, `lengths` and `data` (the group's samples packed as a float32 CUDA tensor)."""
    import os

    import torch
    names = sorted(n for n in os.listdir(myfolder) if n.endswith(".wav"))     # :895
    paths = [os.path.join(myfolder, n) for n in names]
    sounds = [_input(p, None) for p in paths]
    groups = []
    for sr in sorted(set(r for _, r in sounds)):                              # :909-911, a group per rate
        idx = [i for i, (_, r) in enumerate(sounds) if r == sr]
        lens = np.array([len(sounds[i][0]) for i in idx], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        host = np.concatenate([sounds[i][0] for i in idx]).astype(np.float32)
        data = torch.from_numpy(host).to("cuda:%d" % device)
        groups.append(dict(samplingRate=sr, files=idx, offsets=offs, lengths=lens, data=data))
    return names, paths, groups


def analyze_folder(myfolder, verbose=True, samplingRate=None, silence=0.04, windowLength=50, step=None, overlap=50,
                   wn="gaussian", zp=0, cutFreq=6000, nFormants=3, pitchMethods=PITCH_DEFAULT_METHODS, entropyThres=0.6,
                   pitchFloor=75, pitchCeiling=3500, priorMean="default", priorSD=6, priorPlot=False, nCands=1,
                   minVoicedCands="autom", domThres=0.1, domSmooth=220, autocorThres=0.7, autocorSmooth=None, cepThres=0.3,
                   cepSmooth=None, cepZp=0, specThres=0.3, specPeak=0.35, specSinglePeakCert=0.4, specHNRslope=0.8,
                   specSmooth=150, specMerge=1, shortestSyl=20, shortestPause=60, interpolWin=3, interpolTol=0.3,
                   interpolCert=0.3, pathfinding="fast", annealPars=None, certWeight=.5, snakeStep=0.05, snakePlot=False,
                   smooth=1, smoothVars=SMOOTH_VARS, summary=True, plot=False, savePath=None, specPlot=None, pitchPlot=None,
                   candPlot=None, device=0, formants=False):
    """analyzeFolder() (R/analyze.R:831-930) on the GPU: analyze() for every .wav file of
    myfolder, by default (summary=True) one summary row per sound.

    The reference lists the folder with list.files(pattern = "*.wav"), a regular expression
    and not a glob; what a leading * means there is the regex library's choice. Stated
    difference: here the files are those whose names end in '.wav', in sorted() order of the
    names (list.files sorts them by the locale's collation). Each file is read with the
    module's WAV input (mono 16-bit PCM), the files are grouped by sampling rate (a batch
    has one rate), each group is uploaded packed as float32 (exact for 16-bit PCM) and runs
    through analyze_batch(), so the tables stay in HBM when only the rows are wanted.
    samplingRate is not read for files, as in the reference.

    summary=True: a list of dicts in file order, `sound` (the base name, :920-923) first,
    then the 44 cells of SUMMARY_COLUMNS; a row equals analyze(path, summary=True) bit for
    bit. summary=False: a dict from the file's full path (:926) to its analyze() table. As in
    analyze_batch(), the two repairs that need a sound's duration are not made, and a file not
    longer than the window gives a row of NaN (an empty table) where analyze() stops. verbose is
    accepted and prints nothing; annealPars (pathfinding = 'slow' raises) and the plot settings
    are accepted and not read; plot=True and a savePath raise before any file is read.
    formants=True (default False) is passed to analyze_batch() with nFormants: the rows (or the
    tables) gain analyze(formants=True)'s cells; nFormants is not read otherwise."""
    a = locals()
    if plot or priorPlot or snakePlot or savePath is not None:
        raise NotImplementedError("analyze_folder(plot = TRUE / savePath): plotting is out of scope")
    if pathfinding == "slow":
        raise NotImplementedError(_SLOW)
    kw = dict(_pitch_args(a), **_track_args(a))
    names, paths, groups = folder_groups(myfolder, device)
    results = [None] * len(paths)
    for g in groups:
        got = analyze_batch(g["data"], g["offsets"], g["lengths"], g["samplingRate"], to_host=True, device=device,
                            summary=bool(summary), formants=bool(formants), nFormants=nFormants, **kw)
        for i, r in zip(g["files"], got):
            results[i] = r
    if summary:                                                               # :918-923
        return [dict([("sound", n)] + list(r.items())) for n, r in zip(names, results)]
    return dict(zip(paths, results))                                          # :925-926


# ------------------------------------------------------------ parameter sweeps of analyze()
SWEEP_STAGES = ("spectrogram", "amplitude", "descriptives", "autocorrelation (full)", "autocorrelation (peaks only)",
                "cepstrum", "BaNa", "path", "harmonics", "summary")


def _sweep_params(samplingRate, rows):
    """The C array of sg_analyze_params_full for `rows`, dicts of analyze()'s arguments (absent:
    the default), each repaired as analyze_batch() repairs its own. What is out of scope raises
    here, the text naming the row. A row may carry its own samplingRate (the library then
    refuses the sweep)."""
    import inspect

    from . import _abi
    formals = inspect.signature(analyze_batch).parameters
    defaults = {k: p.default for k, p in formals.items() if p.default is not inspect.Parameter.empty}
    P = (_abi.sg_analyze_params_full * max(len(rows), 1))()
    for r, kw in enumerate(rows):
        unknown = [k for k in kw if k not in defaults and k != "samplingRate"]
        if unknown:
            raise ValueError("analyze_sweep: row %d: unused argument: %s" % (r, ", ".join(unknown)))
        a = dict(defaults, **kw)
        try:
            if a["formants"]:
                raise NotImplementedError("the formant columns are not part of a sweep")
            if "summary" in kw and not kw["summary"]:
                raise ValueError("a sweep gives summary rows: summary = FALSE has none")
            if a["pathfinding"] == "slow":
                raise NotImplementedError(_SLOW)
            s = repair_track(repair_pitch(a.get("samplingRate", samplingRate), None, **_pitch_args(a)), **_track_args(a))
        except (ValueError, NotImplementedError) as e:
            raise type(e)("analyze_sweep: row %d: %s" % (r, e)) from e
        P[r] = _track_params(s)
    return P


def sweep_plan(samplingRate, rows):
    """What the rows of an analyze_sweep() share (sg_analyze_sweep_plan; host only, no GPU):
    (frame_group, store_group, cand_group), three integer arrays with one entry per row,
    numbered by first appearance. Rows of one frame group share the spectrogram and the
    amplitudes; of one store group (-1: the row has no 'autocor') the autocorrelations; of one
    candidate group everything in front of the pathfinder. The keys are the resolved decisions,
    not the raw arguments."""
    L = native.lib()
    P = _sweep_params(samplingRate, rows)
    n = len(rows)
    g = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(3)]
    rc = L.sg_analyze_sweep_plan(P, n, *[v.ctypes.data_as(C.POINTER(C.c_int32)) for v in g])
    _host_check(rc)
    return tuple(v[:n] for v in g)


def sweep_size(lengths, samplingRate, rows):
    """sg_analyze_sweep_size (host only): the bytes of the largest frame group's spectrogram and
    candidate tables, of the largest autocorrelation store the sweep would build (0: none is
    shared), and of the largest tail workspace of one row: what workspace_cap is compared with.
    Refuses what analyze_sweep() refuses for these lengths."""
    L = native.lib()
    P = _sweep_params(samplingRate, rows)
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
    out = np.zeros(3, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    rc = L.sg_analyze_sweep_size(lens.ctypes.data_as(i64p), len(lens), P, len(rows), out.ctypes.data_as(i64p))
    _host_check(rc)
    return dict(frame_group=int(out[0]), store=int(out[1]), row=int(out[2]))


def analyze_sweep(data, offsets, lengths, samplingRate, rows, to_host=False, workspace_cap=0, device=0):
    """analyze(call i, samplingRate, summary = TRUE) under every row of `rows` for a batch of
    sounds already in HBM (the layout of analyze_batch()), as one launch sequence
    (sg_analyze_sweep): what optimizePars() evaluates for analyzeFolder. rows: a list of dicts of
    analyze()'s arguments (absent: the default). Each stage runs once per distinct set of the
    decisions it reads (sweep_plan()): the spectrogram and amplitudes per frame group, the
    autocorrelations per store group, the candidates per candidate group, and the pathfinder,
    the harmonics and the summary for all (row, sound) pairs of a chunk of rows in one launch
    each. Returns the fp64 CUDA tensor of shape (rows, sounds, 44), the cells named by
    SUMMARY_COLUMNS; row r of sound i equals analyze_batch(summary=True) under rows[r] bit for
    bit, whatever the other rows and sounds, their order and workspace_cap (bytes of a store
    and of the pair tables of a chunk of rows; 0: the library's default). to_host=True: a list
    per row of per-sound dicts. formants=True, plot=True, summary=False and pathfinding='slow'
    raise before anything runs; a row the library refuses refuses the sweep, the text naming
    the row."""
    P = _sweep_params(samplingRate, rows)
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    ctx = native.default_context(device)
    width = len(SUMMARY_COLUMNS)
    out = native.device_out(data, len(rows) * nc * width)
    _check(native.lib().sg_analyze_sweep(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, P, len(rows),
                                         int(workspace_cap), C.c_void_p(out.data_ptr())), ctx.ptr)
    out = out[:len(rows) * nc * width].reshape(len(rows), nc, width)
    return [_host_rows(m) for m in out] if to_host else out


def sweep_kernel_ms():
    """The device milliseconds of the stages of the last profiled analyze_sweep(), named by
    SWEEP_STAGES (sg_debug_analyze_sweep_kernel_ms)."""
    ms = np.zeros(len(SWEEP_STAGES))
    native.lib().sg_debug_analyze_sweep_kernel_ms(ms.ctypes.data_as(C.POINTER(C.c_double)))
    return dict(zip(SWEEP_STAGES, (float(v) for v in ms)))


_FORMANT_EXPORTS = ("formants", "formants_numpy", "find_formants_numpy", "formants_batch", "find_formants_frames")


def __getattr__(name):
    """formants.py's entry points under this module's name (formants.py imports this module)."""
    if name in _FORMANT_EXPORTS:
        from . import formants as _fm
        return getattr(_fm, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
