// sg_analyze.cpp — the host half of analyze()'s per-frame stage (R/analyze.R:233-575,
// R/utilities_analyze.R:22-324): every integer decision (the window and frames
// through sg_spectrogram.cpp; the frequency and lag labels after R's character
// round trip; rowLow / rowHigh :466-467; the cut band and pitchFloor_idx,
// utilities_analyze.R:52-53, :216; the amplitude windows :456-459; the smoothing
// widths, utilities_analyze.R:206, :268; the lag range :262-263), the refusals, and
// the autocorrelation filter (:403-407). sg_analyze_frames_size needs no device.
// pitch_setup adds the decisions of getPitchCep (utilities_analyze.R:346-367: the
// padded length, the effective cepSmooth, the band and its labels) and getPitchSpec
// (:438: the width) for sg_pitch_candidates_size, which needs no device either.
// track_setup adds those of analyze()'s tail (R/analyze.R:593-681): the prior's shape, rate
// and normaliser, minVoicedCands 'autom', noRequired and nToleratedNA of findVoicedSegments,
// the smoother's half width per sound, and the refusals, for sg_analyze_size.
// The numpy restatement (soundgen_beta_amd/analyze.py) makes the same decisions in
// the same operation order, so no product and sum may fuse here.
#pragma clang fp contract(off)
#include "sg_analyze.h"

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sg_formants.h"
#include "sg_rmath.h"

namespace sg {

namespace {

// as.numeric(as.character(v)): R prints 15 significant digits
double rt15(double v) {
  char b[48];
  std::snprintf(b, sizeof b, "%.15g", v);
  return std::strtod(b, nullptr);
}

// element i of seq(from, to, length.out = n): from + i by, the last one `to`
double seq_len_at(double from, double to, int64_t n, int64_t i) {
  if (i == 0 || n <= 1) return from;
  if (i == n - 1) return to;
  const double by = (to - from) / (double)(n - 1);
  return from + (double)i * by;
}

using cd = std::complex<double>;

// DFT of any length by its prime factors (decimation in time); sign -1 forward, +1 inverse (unscaled)
void fft_any(std::vector<cd>& a, int sign) {
  const int n = (int)a.size();
  if (n <= 1) return;
  int p = 2;
  while (n % p) ++p;
  const int m = n / p;
  std::vector<std::vector<cd>> sub(p, std::vector<cd>(m));
  for (int k = 0; k < m; ++k)
    for (int r = 0; r < p; ++r) sub[r][k] = a[(size_t)k * p + r];
  for (int r = 0; r < p; ++r) fft_any(sub[r], sign);
  for (int q = 0; q < n; ++q) {
    const int k = q % m;
    cd s = 0;
    for (int r = 0; r < p; ++r) {
      const double ang = sign * 2.0 * M_PI * (double)(((int64_t)r * q) % n) / (double)n;
      s += sub[r][k] * cd(std::cos(ang), std::sin(ang));
    }
    a[q] = s;
  }
}

bool in01(double v) { return v >= 0 && v <= 1; }

}  // namespace

namespace {

// anl_setup for the methods in `allowed` (bit 0 'autocor', 1 'dom', 2 'cep', 3 'spec')
AnlSetup anl_setup_m(const sg_analyze_params& p, int allowed) {
  AnlSetup S;
  sg_spectrogram_params q;
  std::memset(&q, 0, sizeof q);
  q.samplingRate = p.samplingRate;
  q.windowLength = p.windowLength;
  q.step = p.step;
  q.overlap = p.overlap;
  q.zp = 0;
  q.contrast = .2;
  q.percentNoise = 10;
  q.wn = p.wn;
  q.output = 0;
  S.spg = spg_setup(q);
  const double sr = S.spg.sr;
  const int wl = S.spg.wl, bins = S.spg.bins;
  if (!in01(p.silence) || !in01(p.entropyThres) || !in01(p.domThres) || !in01(p.autocorThres))
    throw SgError(SG_E_ARG, "analyze: silence, entropyThres, domThres and autocorThres must lie in [0, 1]");
  if (!(p.cutFreq > 0) || !(p.pitchFloor > 0) || !(p.pitchFloor <= p.pitchCeiling) || !(p.pitchCeiling <= sr / 2))
    throw SgError(SG_E_ARG, "analyze: cutFreq and pitchFloor must be positive and pitchFloor <= pitchCeiling <= samplingRate / 2");
  if (p.methods < 1 || (p.methods & ~allowed))
    throw SgError(SG_E_ARG, allowed == 3 ? "analyze: pitchMethods must be a non-empty subset of 'autocor', 'dom'"
                                         : "analyze: pitchMethods must be a non-empty subset of 'autocor', 'dom', 'cep', 'spec'");
  if (!(p.nCands >= 1) || p.nCands != std::floor(p.nCands)) throw SgError(SG_E_ARG, "analyze: nCands must be a whole number >= 1");
  const double zp = std::isnan(p.zp) ? 0.0 : p.zp;
  if (std::floor((zp - wl) / 2) * 2 > 0)
    throw SgError(SG_E_ARG, "analyze: zp pads the " + std::to_string(wl) + "-point frame; acf() then returns " +
                                std::to_string(wl + 1) + " values for the " + std::to_string(wl) +
                                "-row column of autocorBank (R/analyze.R:479) and the reference stops");
  S.silence = p.silence;
  S.entropyThres = p.entropyThres;
  S.domThres = p.domThres;
  S.autocorThres = p.autocorThres;
  S.do_autocor = p.methods & 1;
  S.do_dom = (p.methods >> 1) & 1;
  // Y = seq(0, samplingRate / 2 - samplingRate / wl, length.out = bins) / 1000, through rownames
  S.freq.resize(bins);
  const double top = (sr / 2) - (sr / wl);
  int cut1 = -1;
  S.cut0 = -1;
  for (int k = 0; k < bins; ++k) {
    const double lab = rt15(seq_len_at(0.0, top, bins, k) / 1000);
    if (!S.rowLow && lab > 0.05) S.rowLow = k + 1;
    if (!S.rowHigh && lab > 6) S.rowHigh = k + 1;
    if (!S.pf_idx && lab > p.pitchFloor / 1000) S.pf_idx = k + 1;
    S.freq[k] = 1000 * lab;
    if (S.freq[k] > p.pitchFloor && S.freq[k] < p.cutFreq) {
      if (S.cut0 < 0) S.cut0 = k;
      cut1 = k;
    }
  }
  if (!S.rowLow || !S.rowHigh)
    throw SgError(SG_E_ARG, "analyze: no frequency label above 6 kHz (samplingRate / 2 must exceed 6000 Hz): rowHigh is NA and "
                            "rowLow:rowHigh stops in the reference");
  S.ncut = S.cut0 < 0 ? 0 : cut1 - S.cut0 + 1;
  if (S.ncut < 2)
    throw SgError(SG_E_ARG, "analyze: fewer than 2 bins between pitchFloor and cutFreq; lm(amp ~ freq) stops in the reference");
  const double bin = sr / 2 / bins;
  const double dw = 2 * std::ceil(p.domSmooth / bin / 2) - 1;
  if (!(dw >= 1)) throw SgError(SG_E_ARG, "analyze: domSmooth must be positive");
  S.domW = dw > 1e9 ? 1000000000 : (int)dw;
  const double aw = std::isnan(p.autocorSmooth) ? 2 * std::ceil(7 * sr / 44100 / 2) - 1 : p.autocorSmooth;
  if (!(aw >= 1) || aw != std::floor(aw) || aw > 1e9 || ((int64_t)aw) % 2 == 0)
    throw SgError(SG_E_ARG, "analyze: autocorSmooth must be a whole odd number (zoo's even-width alignment is not restated)");
  S.acW = (int)aw;
  int j0 = 0, j1 = 0;  // rows (1-based) with pitchFloor < samplingRate / j < pitchCeiling
  for (int j = 1; j <= wl; ++j) {
    const double lf = rt15(sr / j);
    if (lf > p.pitchFloor && lf < p.pitchCeiling) {
      if (!j0) j0 = j;
      j1 = j;
    }
  }
  if (!j0) throw SgError(SG_E_ARG, "analyze: no lag between pitchFloor and pitchCeiling (max(numeric(0)) in the reference)");
  S.lag0 = j0 - 1;
  S.nlag = j1 - j0 + 1;
  S.lagf.resize(S.nlag);
  for (int i = 0; i < S.nlag; ++i) S.lagf[i] = rt15(sr / (j0 + i));
  if (S.acW > S.nlag)
    throw SgError(SG_E_ARG, "analyze: autocorSmooth = " + std::to_string(S.acW) + " is wider than the " +
                                std::to_string(S.nlag) + " lags between pitchFloor and pitchCeiling");
  if (p.nCands > kAnlMaxCands)
    throw SgError(SG_E_UNSUPPORTED, "analyze: nCands = " + std::to_string((long long)p.nCands) + "; at most " +
                                        std::to_string(kAnlMaxCands) + " candidates are kept");
  S.nCands = (int)p.nCands;
  S.cols = kAnlFixed + 2 * S.nCands;
  double m = 0;
  for (int k = 0; k < S.ncut; ++k) m += S.freq[S.cut0 + k];
  m /= S.ncut;
  S.xc.resize(S.ncut);
  for (int k = 0; k < S.ncut; ++k) {
    S.xc[k] = S.freq[S.cut0 + k] - m;
    S.sxx += S.xc[k] * S.xc[k];
  }
  return S;
}

// every prime factor of n is <= 31 (the radices of fft64)
bool smooth31(int n) {
  for (int p : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
    while (n % p == 0) n /= p;
  return n == 1;
}

}  // namespace

AnlSetup anl_setup(const sg_analyze_params& p) { return anl_setup_m(p, 3); }

AnlSetup anl_setup_any(const sg_analyze_params& p) { return anl_setup_m(p, 15); }

int formants_order(double samplingRate, int nFormants) {
  if (nFormants < 1 || nFormants > kFmtMaxFormants)
    throw SgError(SG_E_ARG, "formants: nFormants must lie in 1.." + std::to_string(kFmtMaxFormants));
  if (!(samplingRate > 0) || !(samplingRate < 1e9)) throw SgError(SG_E_ARG, "formants: samplingRate must be positive");
  const int order = fmt_order(samplingRate);
  if (order > kFmtMaxOrder)
    throw SgError(SG_E_UNSUPPORTED, "formants: the order round(samplingRate / 1000) + 3 = " + std::to_string(order) +
                                        " exceeds " + std::to_string(kFmtMaxOrder) +
                                        " (one root per lane of a wave): samplingRate must stay below 61.5 kHz");
  return order;
}

void formants_window(int wl, int order) {
  if (wl <= order)
    throw SgError(SG_E_ARG, "formants: windowLength gives frames of " + std::to_string(wl) + " samples; the prediction of order " +
                                std::to_string(order) + " needs more than " + std::to_string(order) +
                                " (the reference's solve() fails on every frame there and all rows are NA)");
}

PitchSetup pitch_setup(const sg_pitch_params& p) {
  PitchSetup S;
  static_cast<AnlSetup&>(S) = anl_setup_m(p.a, 15);
  const double sr = S.spg.sr;
  const int B = S.spg.bins;
  if (!in01(p.cepThres) || !in01(p.specThres) || !in01(p.specPeak) || !in01(p.specSinglePeakCert))
    throw SgError(SG_E_ARG, "analyze: cepThres, specThres, specPeak and specSinglePeakCert must lie in [0, 1]");
  if (!(p.specMerge >= 0)) throw SgError(SG_E_ARG, "analyze: specMerge must be non-negative");
  if (std::isnan(p.specSmooth) || std::isnan(p.cepZp)) throw SgError(SG_E_ARG, "analyze: specSmooth and cepZp must be numbers");
  S.do_cep = (p.a.methods >> 2) & 1;
  S.do_spec = (p.a.methods >> 3) & 1;
  S.cols = kAnlFixed + 6 * S.nCands;
  S.pitchFloor = p.a.pitchFloor;
  S.pitchCeiling = p.a.pitchCeiling;
  S.cepThres = p.cepThres;
  S.specThres = p.specThres;
  S.specPeak = p.specPeak;
  S.specSinglePeakCert = p.specSinglePeakCert;
  S.specMerge = p.specMerge;
  // getPitchCep :346-356
  double cw = std::isnan(p.cepSmooth) ? 2 * std::ceil(31 * sr / 44100 / 2) - 1 : p.cepSmooth;
  double Ld = B;
  if (!(p.cepZp < B)) {
    const double pad = std::trunc((p.cepZp - B) / 2);  // rep(0, x) truncates x
    if (pad > 1e6) throw SgError(SG_E_UNSUPPORTED, "analyze: cepZp is too large");
    S.cepPad = (int)pad;
    Ld = B + 2 * pad;
    cw = cw * std::nearbyint(p.cepZp / B);  // R's round(): half to even
  }
  S.cepL = (int)Ld;
  S.cepl = S.cepL / 2;
  S.cepW = cw >= 1 && cw <= 1e9 && cw == std::floor(cw) ? (int)cw : 0;
  // :361-367 freq = samplingRate / (1:l) / 2 * (length(frameZP) / length(frame))
  const double scale = Ld / (double)B;
  int k0 = 0, k1 = 0;
  for (int k = 1; k <= S.cepl; ++k) {
    const double f = sr / k / 2 * scale;
    if (f > p.a.pitchFloor && f < p.a.pitchCeiling) {
      if (!k0) k0 = k;
      k1 = k;
    }
  }
  S.cep0 = k0 ? k0 - 1 : 0;
  S.ncep = k0 ? k1 - k0 + 1 : 0;
  S.cepf.resize(S.ncep);
  for (int i = 0; i < S.ncep; ++i) S.cepf[i] = sr / (k0 + i) / 2 * scale;
  // getPitchSpec :438
  const double bin = sr / 2 / B;
  const double sw = 2 * std::ceil((p.specSmooth / bin + 1) * 20 / bin / 2) - 1;
  S.specW = sw > 1e9 ? 1000000000 : sw >= 1 ? (int)sw : 0;
  if (S.do_cep) {
    // the transform first: a cepZp beyond it is unsupported whatever cepSmooth it implies
    const int L = S.cepL, M = L % 2 ? L : L / 2;
    if (M < 1 || M > kSpgMaxBins || !smooth31(M))
      throw SgError(SG_E_UNSUPPORTED, "analyze: the cepstrum's " + std::to_string(L) + "-point transform is not supported (" +
                                          (L % 2 ? "L" : "L / 2") + " = " + std::to_string(M) +
                                          " must be at most 2048 with no prime factor above 31); R's fft() takes any length");
    if (!S.cepW || S.cepW % 2 == 0)
      throw SgError(SG_E_ARG, "analyze: the effective cepSmooth (cepSmooth * round(cepZp / bins) when cepZp pads the frame) "
                              "must be a whole odd number (zoo's even-width alignment is not restated)");
    if (!S.ncep)
      throw SgError(SG_E_ARG, "analyze: no row of the cepstrum between pitchFloor and pitchCeiling (rollapply gets an empty "
                              "series in the reference)");
  }
  if (S.do_spec && !S.specW)
    throw SgError(SG_E_ARG, "analyze: specSmooth gives getPitchSpec's rolling window a width below 1 (rollapply stops in the "
                            "reference)");
  return S;
}

PathPars track_path_pars(const sg_analyze_params_full& p, double* smooth) {
  PathPars P;
  std::memset(&P, 0, sizeof P);
  const sg_analyze_params& a = p.p.a;
  if (!(a.nCands >= 1) || a.nCands != std::floor(a.nCands)) throw SgError(SG_E_ARG, "analyze: nCands must be a whole number >= 1");
  if (a.nCands > kAnlMaxCands) throw SgError(SG_E_UNSUPPORTED, "analyze: at most " + std::to_string(kAnlMaxCands) + " candidates are kept");
  if (a.methods < 1 || (a.methods & ~15)) throw SgError(SG_E_ARG, "analyze: pitchMethods must be a non-empty subset of 'autocor', 'dom', 'cep', 'spec'");
  if (!(a.pitchFloor > 0) || !(a.pitchFloor <= a.pitchCeiling)) throw SgError(SG_E_ARG, "analyze: pitchFloor must be positive and at most pitchCeiling");
  P.nCands = (int)a.nCands;
  P.cols = kAnlFixed + 6 * P.nCands + kPathCols;
  if (p.pathfinding == 2)
    throw SgError(SG_E_UNSUPPORTED, "analyze: pathfinding = 'slow' (simulated annealing on R's random stream) is not built");
  if (p.pathfinding < 0 || p.pathfinding > 3)
    throw SgError(SG_E_ARG, "analyze: pathfinding must be 0 'none', 1 'fast', 2 'slow' or 3 'exact'");
  P.pathfinding = p.pathfinding;
  if (p.smoothVars & ~3) throw SgError(SG_E_ARG, "analyze: smoothVars must be a subset of 'pitch', 'dom'");
  // :598-605 the prior, when priorMean and priorSD are both numbers
  if (!std::isnan(p.priorMean) && !std::isnan(p.priorSD)) {
    if (!(p.priorMean > 0) || !(p.priorSD > 0) || std::isinf(p.priorMean) || std::isinf(p.priorSD))
      throw SgError(SG_E_ARG, "analyze: priorMean and priorSD must be positive (dgamma gives NaN in the reference)");
    P.do_prior = 1;
    P.shape = (p.priorMean * p.priorMean) / (p.priorSD * p.priorSD);
    P.rate = p.priorMean / (p.priorSD * p.priorSD);
    P.lconst = P.shape * std::log(P.rate) - std::lgamma(P.shape);
    const double from = std::log2(a.pitchFloor / 16.3516) * 12, to = std::log2(a.pitchCeiling / 16.3516) * 12;
    double mx = -INFINITY;
    for (int i = 0; i < 100; ++i) mx = std::max(mx, path_dgamma(seq_len_at(from, to, 100, i), P.shape, P.rate, P.lconst));
    if (!(mx > 0) || std::isinf(mx)) throw SgError(SG_E_ARG, "analyze: the prior vanishes over the whole pitch range");
    P.prior_norm = mx;
  }
  // :615-624 minVoicedCands 'autom'
  int nm = 0;
  for (int b = 0; b < 4; ++b) nm += (a.methods >> b) & 1;
  double mv = p.minVoicedCands;
  if (std::isnan(mv) || mv < 1 || mv > nm) mv = ((a.methods & 2) && nm > 1) ? 2 : 1;
  P.minVoiced = (int)std::ceil(mv);
  // findVoicedSegments :633-636
  const double step = std::isnan(a.step) ? a.windowLength * (1 - a.overlap / 100) : a.step;
  if (!(step > 0)) throw SgError(SG_E_ARG, "analyze: step must be positive");
  if (std::isnan(p.shortestSyl) || std::isnan(p.shortestPause) || p.shortestPause < 0)
    throw SgError(SG_E_ARG, "analyze: shortestSyl and shortestPause must be numbers, shortestPause not negative");
  P.noRequired = (int)std::min(std::max(1.0, std::ceil(p.shortestSyl / step)), 1073741824.0);
  P.nTolerated = (int)std::min(std::floor(p.shortestPause / step), 1073741824.0);
  if (std::isnan(p.interpolTol) || std::isnan(p.interpolCert)) throw SgError(SG_E_ARG, "analyze: interpolTol and interpolCert must be numbers");
  if (std::isnan(p.interpolWin) || p.interpolWin != std::floor(p.interpolWin))
    throw SgError(SG_E_ARG, "analyze: interpolWin must be a whole number (f - interpolWin indexes frames)");
  if (p.interpolWin > kPathMaxWin)
    throw SgError(SG_E_UNSUPPORTED, "analyze: interpolWin and half the smoothing window may be at most " + std::to_string(kPathMaxWin) + " frames");
  P.interpolWin = p.interpolWin > 0 ? (int)p.interpolWin : 0;
  P.interpolTol = p.interpolTol;
  P.interpolCert = p.interpolCert;
  if (!(p.certWeight >= 0 && p.certWeight <= 1)) throw SgError(SG_E_ARG, "analyze: certWeight must lie in [0, 1]");
  P.certWeight = p.certWeight;
  P.snakeStep = p.snakeStep > 0 ? p.snakeStep : 0.0;
  if (P.snakeStep > 0 && P.snakeStep < 0.005) throw SgError(SG_E_UNSUPPORTED, "analyze: snakeStep below 0.005 is not supported");
  *smooth = p.smooth > 0 ? p.smooth : 0.0;
  if (std::isinf(*smooth)) throw SgError(SG_E_ARG, "analyze: smooth must be finite");
  P.smooth_pitch = *smooth > 0 && (p.smoothVars & 1);
  P.smooth_dom = *smooth > 0 && (p.smoothVars & 2);
  P.smoothThres = *smooth > 0 ? 4 / *smooth : 0.0;
  return P;
}

TrackSetup track_setup(const sg_analyze_params_full& p) {
  TrackSetup S;
  static_cast<PitchSetup&>(S) = pitch_setup(p.p);
  S.path = track_path_pars(p, &S.smooth);
  S.cols = S.path.cols;
  const int bins = S.spg.bins;
  const double sr = S.spg.sr, top = (sr / 2) - (sr / S.spg.wl);
  S.lab.resize(bins);
  for (int k = 0; k < bins; ++k) S.lab[k] = rt15(seq_len_at(0.0, top, bins, k) / 1000);  // as anl_setup labels the bins
  return S;
}

int track_hw(double smooth, double samplingRate, int64_t len, int frames) {
  if (!(smooth > 0) || frames <= 0 || len <= 0) return 0;
  const double duration = (double)len / samplingRate;
  const double ww = std::nearbyint(smooth * ((double)frames / duration) / 10);  // R's round(): half to even
  const double hw = std::floor(ww / 2);
  if (hw > kPathMaxWin)
    throw SgError(SG_E_UNSUPPORTED, "analyze: interpolWin and half the smoothing window may be at most " + std::to_string(kPathMaxWin) + " frames");
  return (int)hw;
}

int anl_frames(const AnlSetup& S, int64_t len) { return len <= S.spg.wl ? 0 : spg_frames(S.spg, len); }

int64_t anl_ampl_start(const AnlSetup& S, int64_t len, int frames, int f) {
  return (int64_t)std::floor(seq_len_at(1.0, (double)(len - S.spg.wl), frames, f)) - 1;
}

std::vector<double> anl_filter(const AnlSetup& S) {
  const int wl = S.spg.wl, N = 2 * wl;
  const std::vector<double> w = spg_window(N, S.spg.wn);  // ftwindow_modif(2 * windowLength_points)
  std::vector<cd> a(N);
  for (int i = 0; i < N; ++i) a[i] = w[i];
  fft_any(a, -1);
  for (int i = 0; i < N; ++i) a[i] = std::norm(a[i]);  // abs(fft(filter)) ^ 2
  fft_any(a, +1);
  std::vector<double> f(wl);
  double mx = 0;
  for (int i = 0; i < wl; ++i) {
    f[i] = std::norm(a[i]);  // abs(fft(., inverse = TRUE)) ^ 2: the reference's second squaring
    mx = std::max(mx, f[i]);
  }
  std::vector<double> out(S.nlag);
  for (int i = 0; i < S.nlag; ++i) out[i] = f[S.lag0 + i] / mx;
  return out;
}

namespace {

bool same_frames(const SpgSetup& a, const SpgSetup& b) {
  return a.sr == b.sr && a.step == b.step && a.by == b.by && a.wl == b.wl && a.pad == b.pad && a.N == b.N && a.bins == b.bins &&
         a.wn == b.wn;
}

// what the autocorrelation of a frame and the gate in front of it read
bool same_store(const AnlSetup& a, const AnlSetup& b) {
  return a.silence == b.silence && a.entropyThres == b.entropyThres && a.rowLow == b.rowLow && a.rowHigh == b.rowHigh &&
         a.lag0 == b.lag0 && a.nlag == b.nlag;
}

// every field the per-frame kernels read (the label tables follow from the ones compared)
bool same_cands(const PitchSetup& a, const PitchSetup& b) {
  return same_store(a, b) && a.domThres == b.domThres && a.autocorThres == b.autocorThres && a.nCands == b.nCands &&
         a.do_autocor == b.do_autocor && a.do_dom == b.do_dom && a.cut0 == b.cut0 && a.ncut == b.ncut && a.pf_idx == b.pf_idx &&
         a.domW == b.domW && a.acW == b.acW && a.do_cep == b.do_cep && a.do_spec == b.do_spec && a.pitchFloor == b.pitchFloor &&
         a.pitchCeiling == b.pitchCeiling && a.cepThres == b.cepThres && a.specThres == b.specThres && a.specPeak == b.specPeak &&
         a.specSinglePeakCert == b.specSinglePeakCert && a.specMerge == b.specMerge && a.cepL == b.cepL && a.cepPad == b.cepPad &&
         a.cepW == b.cepW && a.cepl == b.cepl && a.cep0 == b.cep0 && a.ncep == b.ncep && a.specW == b.specW;
}

std::string sweep_row(int64_t r, int64_t c = -1) {
  return "sg_analyze_sweep: row " + std::to_string(r) + (c >= 0 ? ", sound " + std::to_string(c) : std::string()) + ": ";
}

}  // namespace

SweepPlan anl_sweep_plan(const sg_analyze_params_full* rows, int64_t n_rows) {
  SweepPlan W;
  W.S.reserve((size_t)n_rows);
  W.frame_group.resize((size_t)n_rows);
  W.store_group.resize((size_t)n_rows);
  W.cand_group.resize((size_t)n_rows);
  std::vector<int64_t> first_f, first_s, first_c;  // the row a group was first seen in
  for (int64_t r = 0; r < n_rows; ++r) {
    try {
      W.S.push_back(track_setup(rows[r]));
    } catch (const SgError& e) {
      throw SgError(e.code, sweep_row(r) + e.what());
    }
    if (rows[r].p.a.samplingRate != rows[0].p.a.samplingRate)
      throw SgError(SG_E_ARG, sweep_row(r) + "samplingRate is that of row 0");
    const TrackSetup& S = W.S.back();
    size_t f = 0, s = 0, c = 0;
    while (f < first_f.size() && !same_frames(W.S[first_f[f]].spg, S.spg)) ++f;
    if (f == first_f.size()) first_f.push_back(r);
    W.frame_group[r] = (int32_t)f;
    if (S.do_autocor) {
      while (s < first_s.size() && !(W.frame_group[first_s[s]] == (int32_t)f && same_store(W.S[first_s[s]], S))) ++s;
      if (s == first_s.size()) first_s.push_back(r);
      W.store_group[r] = (int32_t)s;
    } else {
      W.store_group[r] = -1;
    }
    while (c < first_c.size() && !(W.frame_group[first_c[c]] == (int32_t)f && same_cands(W.S[first_c[c]], S))) ++c;
    if (c == first_c.size()) first_c.push_back(r);
    W.cand_group[r] = (int32_t)c;
  }
  W.n_frame = (int)first_f.size();
  W.n_store = (int)first_s.size();
  W.n_cand = (int)first_c.size();
  return W;
}

void anl_sweep_bytes(const SweepPlan& W, const int64_t* lengths, int64_t n_calls, int64_t* bytes) {
  const int64_t n_rows = (int64_t)W.S.size();
  bytes[0] = bytes[1] = bytes[2] = 0;
  std::vector<int64_t> frames((size_t)W.n_frame, 0), persist((size_t)W.n_frame, 0);
  std::vector<int> seen_c((size_t)W.n_cand, 0), users((size_t)std::max(W.n_store, 1), 0);
  std::vector<int> seen_f((size_t)W.n_frame, 0);
  for (int64_t r = 0; r < n_rows; ++r) {
    const TrackSetup& S = W.S[r];
    const int f = W.frame_group[r];
    int64_t F = 0;
    for (int64_t c = 0; c < n_calls; ++c) {
      const int nf = anl_frames(S, lengths[c]);
      try {
        (void)track_hw(S.smooth, S.spg.sr, lengths[c], nf);
      } catch (const SgError& e) {
        throw SgError(e.code, sweep_row(r, c) + e.what());
      }
      F += nf;
    }
    if (!seen_f[f]) {
      seen_f[f] = 1;
      frames[f] = F;
      persist[f] = F * S.spg.bins * (int64_t)sizeof(double);
    }
    if (!seen_c[W.cand_group[r]]) {
      seen_c[W.cand_group[r]] = 1;
      persist[f] += F * (S.cols - kPathCols) * (int64_t)sizeof(double);
      if (W.store_group[r] >= 0) ++users[W.store_group[r]];
    }
    bytes[2] = std::max(bytes[2], F * (S.cols + path_scratch(S.nCands, S.path.pathfinding)) * (int64_t)sizeof(double));
  }
  for (int f = 0; f < W.n_frame; ++f) bytes[0] = std::max(bytes[0], persist[f]);
  for (int64_t r = 0; r < n_rows; ++r)
    if (W.store_group[r] >= 0 && users[W.store_group[r]] >= 2)
      bytes[1] = std::max(bytes[1], frames[W.frame_group[r]] * W.S[r].nlag * (int64_t)sizeof(double));
}

}  // namespace sg

namespace {
using sg::bad_arguments;
using sg::host_guarded;

// A size function is called once per sound of a batch: the setup make(p) of the thread's last
// parameters is kept, and unset while it is rebuilt (a throwing make leaves no stale pair)
template <class P, class S>
const S& memo(S (*make)(const P&), const P& p) {
  thread_local P last_p;
  thread_local S last_S;
  thread_local bool have = false;
  if (!have || std::memcmp(&p, &last_p, sizeof p) != 0) {
    have = false;
    last_S = make(p);
    last_p = p;
    have = true;
  }
  return last_S;
}
}  // namespace

extern "C" int sg_analyze_frames_size(int64_t len, const sg_analyze_params* p, int32_t* wl, int32_t* bins, int32_t* frames,
                                      int32_t* cols, int32_t* lag_first, int32_t* lag_last, int32_t* extra) {
  return host_guarded([&]() {
    if (!p || !wl || !bins || !frames || !cols || !lag_first || !lag_last) bad_arguments("sg_analyze_frames_size");
    const sg::AnlSetup& S = memo(sg::anl_setup, *p);
    *wl = S.spg.wl;
    *bins = S.spg.bins;
    *frames = sg::anl_frames(S, len);
    *cols = S.cols;
    *lag_first = S.lag0;
    *lag_last = S.lag0 + S.nlag - 1;
    if (extra) {
      const int32_t e[8] = {S.rowLow, S.rowHigh, S.cut0, S.ncut, S.pf_idx, S.domW, S.acW, 0};
      std::memcpy(extra, e, sizeof e);
    }
  });
}

extern "C" int sg_analyze_frames_ampl_starts(int64_t len, const sg_analyze_params* p, int64_t* starts, int32_t n) {
  return host_guarded([&]() {
    if (!p || (n > 0 && !starts)) bad_arguments("sg_analyze_frames_ampl_starts");
    const sg::AnlSetup& S = memo(sg::anl_setup, *p);
    const int frames = sg::anl_frames(S, len);
    if (n > frames) throw sg::SgError(SG_E_ARG, "sg_analyze_frames_ampl_starts: n exceeds the frame count");
    for (int f = 0; f < n; ++f) starts[f] = sg::anl_ampl_start(S, len, frames, f);
  });
}

extern "C" int sg_formants_size(const sg_analyze_params* p, int32_t nFormants, int32_t* order, int32_t* cols) {
  return host_guarded([&]() {
    if (!p || !order || !cols) bad_arguments("sg_formants_size");
    *order = sg::formants_order(p->samplingRate, nFormants);
    *cols = 2 * nFormants;
    sg::formants_window(sg::anl_setup_any(*p).spg.wl, *order);
  });
}

extern "C" int sg_pitch_candidates_size(int64_t len, const sg_pitch_params* p, int32_t* frames, int32_t* cols,
                                        int32_t* extra) {
  return host_guarded([&]() {
    if (!p || !frames || !cols) bad_arguments("sg_pitch_candidates_size");
    const sg::PitchSetup& S = memo(sg::pitch_setup, *p);
    *frames = sg::anl_frames(S, len);
    *cols = S.cols;
    if (extra) {
      const int32_t e[24] = {S.spg.wl, S.spg.bins, S.lag0, S.lag0 + S.nlag - 1, S.rowLow, S.rowHigh, S.cut0, S.ncut,
                             S.pf_idx, S.domW, S.acW, S.cepL, S.cepW, S.cepl, S.cep0, S.ncep, S.specW};
      std::memcpy(extra, e, sizeof e);
    }
  });
}

extern "C" int sg_pitch_candidates_cep_labels(const sg_pitch_params* p, double* labels, int32_t n) {
  return host_guarded([&]() {
    if (!p || (n > 0 && !labels)) bad_arguments("sg_pitch_candidates_cep_labels");
    const sg::PitchSetup& S = memo(sg::pitch_setup, *p);
    if (n > S.ncep) throw sg::SgError(SG_E_ARG, "sg_pitch_candidates_cep_labels: n exceeds the band");
    for (int i = 0; i < n; ++i) labels[i] = S.cepf[i];
  });
}

extern "C" int sg_analyze_size(int64_t len, const sg_analyze_params_full* p, int32_t* frames, int32_t* cols, int32_t* extra) {
  return host_guarded([&]() {
    if (!p || !frames || !cols) bad_arguments("sg_analyze_size");
    const sg::TrackSetup& S = memo(sg::track_setup, *p);
    *frames = sg::anl_frames(S, len);
    *cols = S.cols;
    const int hw = sg::track_hw(S.smooth, S.spg.sr, len, *frames);
    if (extra) {
      const int32_t e[8] = {S.path.minVoiced, S.path.noRequired, S.path.nTolerated, hw, S.path.interpolWin};
      std::memcpy(extra, e, sizeof e);
    }
  });
}

extern "C" int sg_analyze_sweep_plan(const sg_analyze_params_full* rows, int64_t n_rows, int32_t* frame_group,
                                     int32_t* store_group, int32_t* cand_group) {
  return host_guarded([&]() {
    if (n_rows < 0 || (n_rows > 0 && (!rows || !frame_group || !store_group || !cand_group)))
      bad_arguments("sg_analyze_sweep_plan");
    const sg::SweepPlan W = sg::anl_sweep_plan(rows, n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
      frame_group[r] = W.frame_group[r];
      store_group[r] = W.store_group[r];
      cand_group[r] = W.cand_group[r];
    }
  });
}

extern "C" int sg_analyze_sweep_size(const int64_t* lengths, int64_t n_calls, const sg_analyze_params_full* rows,
                                     int64_t n_rows, int64_t* bytes) {
  return host_guarded([&]() {
    if (n_rows < 0 || n_calls < 0 || !bytes || (n_rows > 0 && !rows) || (n_calls > 0 && !lengths))
      bad_arguments("sg_analyze_sweep_size");
    sg::anl_sweep_bytes(sg::anl_sweep_plan(rows, n_rows), lengths, n_calls, bytes);
  });
}

extern "C" const char* sg_analyze_frames_size_error(void) { return sg::g_host_err.c_str(); }

// analyze(summary = TRUE): the cells of a row (R/analyze.R:777-784), the variables in sg::sum_column's order
extern "C" const char* sg_analyze_summary_name(int32_t i) {
  static const char* const vars[sg::kSumVars] = {"ampl",     "amplVoiced",  "dom",   "entropy",    "harmonics",  "HNR",        "meanFreq",
                                                 "peakFreq", "peakFreqCut", "pitch", "quartile25", "quartile50", "quartile75", "specSlope"};
  static const char* const stats[3] = {"_mean", "_median", "_sd"};
  static_assert(SG_ANALYZE_SUMMARY_COLS == sg::kSumCols, "the header's row is sg_summary.h's");
  thread_local std::string name;
  if (i < 0 || i >= sg::kSumCols) return nullptr;
  if (i < 2) return i ? "voiced" : "duration";
  name = std::string(vars[(i - 2) / 3]) + stats[(i - 2) % 3];
  return name.c_str();
}
