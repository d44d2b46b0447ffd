// sg_spectrogram.cpp — the host half of spectrogram() (R/spectrogram.R:94-276):
// the integer decisions (step :118, windowLength_points :123, getFrameBank's
// frame starts :350-351 and zero padding :355), the validation of the limits the
// device code has, and ftwindow_modif's windows (:288-319; seewave_2.0.5.tar.gz::
// seewave/R/seewave.r:7293-7301, :7308-7314, :7417-7424, :7431-7437, :7444-7450,
// :7514-7519). sg_spectrogram_size needs no device. The numpy restatement
// (soundgen_beta_amd/spectrogram.py) makes the same decisions in the same
// operation order, so no product and sum may fuse here.
#pragma clang fp contract(off)
#include "sg_spectrogram.h"

#include <cmath>
#include <string>

#include "sg_frame_grid.h"
#include "sg_rmath.h"

namespace sg {

SpgSetup spg_setup(const sg_spectrogram_params& p) {
  SpgSetup S;
  S.sr = p.samplingRate;
  if (!(S.sr > 0) || !(p.windowLength > 0)) throw SgError(SG_E_ARG, "spectrogram: samplingRate and windowLength must be > 0");
  S.step = std::isnan(p.step) ? p.windowLength * (1 - p.overlap / 100) : p.step;
  S.by = S.step / 1000 * S.sr;
  if (!(S.by > 0)) throw SgError(SG_E_ARG, "spectrogram: step must be > 0");
  const double wl = std::floor(p.windowLength / 1000 * S.sr / 2) * 2;
  if (!(wl >= 4)) throw SgError(SG_E_UNSUPPORTED, "spectrogram: the window is shorter than 4 points");
  if (wl > 2.0 * kSpgMaxBins)
    throw SgError(SG_E_UNSUPPORTED, "spectrogram: the window has " + std::to_string((long long)wl) +
                                        " points; the device transform takes at most 4096 (windowLength is too long)");
  S.wl = (int)wl;
  const double zp = std::isnan(p.zp) ? 0.0 : p.zp;
  const double zpExtra = std::floor((zp - S.wl) / 2) * 2;
  if (zpExtra > 2.0 * kSpgMaxBins)
    throw SgError(SG_E_UNSUPPORTED, "spectrogram: zp pads the frame past 4096 points; choose a smaller zp");
  S.pad = zpExtra > 0 ? (int)zpExtra / 2 : 0;
  S.N = S.wl + 2 * S.pad;
  S.bins = S.N / 2;
  int rest = S.bins;
  for (int q : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
    while (rest % q == 0) rest /= q;
  if (S.bins > kSpgMaxBins || rest != 1)
    throw SgError(SG_E_UNSUPPORTED,
                  "spectrogram: a frame of " + std::to_string(S.N) + " points (" + std::to_string(S.bins) +
                      " bins) is not supported: bins must be <= 2048 and a product of 2 and the odd primes <= 31; "
                      "pad to a supported length with zp (e.g. a power of 2 above the window's " +
                      std::to_string(S.wl) + " points)");
  auto median_k = [](double v, const char* name) -> int {
    if (std::isnan(v) || !(v > 1)) return 0;
    if (v != std::floor(v) || v > 1e9) throw SgError(SG_E_ARG, std::string("spectrogram: ") + name + " must be a whole number");
    const int k = (int)v;
    if (k % 2 == 0)
      throw SgError(SG_E_ARG, std::string("spectrogram: ") + name +
                                  " must be odd (zoo::rollmedian's even-k path is not restated)");
    return k;
  };
  S.kFreq = median_k(p.smoothFreq, "smoothFreq");
  S.kTime = median_k(p.smoothTime, "smoothTime");
  if (p.wn < 0 || p.wn > 6 || p.method < 0 || p.method > 1 || p.output < 0 || p.output > 1)
    throw SgError(SG_E_ARG, "spectrogram: unknown wn, method or output");
  S.wn = p.wn;
  S.deriv = p.method;
  S.processed = p.output;
  S.qTime = p.qTime;
  S.percentNoise = p.percentNoise;
  S.noiseReduction = p.noiseReduction;
  if (S.qTime > 1 || (S.noiseReduction > 0 && !(S.percentNoise >= 0 && S.percentNoise <= 100)))
    throw SgError(SG_E_ARG, "spectrogram: qTime must lie in [0, 1] and percentNoise in [0, 100]");
  S.contrast_exp = std::exp(3 * p.contrast);
  S.brightness_exp = std::exp(3 * p.brightness);
  return S;
}

int spg_frames(const SpgSetup& S, int64_t len) {
  const int64_t n = grid_frames(S.by, S.wl, len);
  if (n > 2147483647LL) throw SgError(SG_E_UNSUPPORTED, "spectrogram: more than 2^31 frames");
  return (int)n;
}

int64_t spg_frame_start(const SpgSetup& S, int64_t len, int i) { return grid_frame_start(S.by, S.wl, len, i); }

void spg_list_frames(const SpgSetup& S, int64_t len, int nf, int32_t snd, const char* who, std::vector<SpgFrame>& fr) {
  if ((int64_t)fr.size() + nf > 2147483647LL)
    throw SgError(SG_E_UNSUPPORTED, std::string(who) + ": the frames of one launch exceed 2^31");
  for (int f = 0; f < nf; ++f) {
    const int64_t o = spg_frame_start(S, len, f);
    if (o < 0 || o + S.wl > len) throw SgError(SG_E_DEVICE, std::string(who) + ": a frame leaves its sound");
    fr.push_back(SpgFrame{o, snd, f});
  }
}

std::vector<double> spg_window(int wl, int wn) {
  std::vector<double> w(wl);
  const double n = (double)(wl - 1);
  const double pi = M_PI;
  switch (wn) {
    case 0: {  // bartlett.w: c((2 * (0:(m - 1))) / n, 2 - ((2 * (m:n)) / n)), m = n %/% 2
      const int m = (wl - 1) / 2;
      for (int i = 0; i < wl; ++i) w[i] = i < m ? (2 * (double)i) / n : 2 - ((2 * (double)i) / n);
      break;
    }
    case 1:
      for (int i = 0; i < wl; ++i) w[i] = 0.42 - 0.5 * std::cos(2 * pi * i / n) + 0.08 * std::cos(4 * pi * i / n);
      break;
    case 2:  // flattop.w: the source's sum ends at the 4 pi term (its next line is its own statement)
      for (int i = 0; i < wl; ++i) w[i] = 0.2156 - 0.4160 * std::cos(2 * pi * i / n) + 0.2781 * std::cos(4 * pi * i / n);
      break;
    case 3:
      for (int i = 0; i < wl; ++i) w[i] = 0.54 - 0.46 * std::cos(2 * pi * i / n);
      break;
    case 4:
      for (int i = 0; i < wl; ++i) w[i] = 0.5 - 0.5 * std::cos(2 * pi * i / n);
      break;
    case 5:
      for (int i = 0; i < wl; ++i) w[i] = 1.0;
      break;
    default: {  // gaussian.w: (exp(-12 * (((1:n) / n) - 0.5) ^ 2) - exp(-12)) / (1 - exp(-12))
      const double e12 = std::exp(-12.0);
      for (int i = 0; i < wl; ++i) {
        const double d = ((double)(i + 1) / (double)wl) - 0.5;
        w[i] = (std::exp(-12 * (d * d)) - e12) / (1 - e12);
      }
    }
  }
  return w;
}

}  // namespace sg

extern "C" int sg_spectrogram_size(int64_t len, const sg_spectrogram_params* p, int32_t* wl, int32_t* n_fft,
                                   int32_t* bins, int32_t* frames) {
  return sg::host_guarded([&]() {
    if (!p || !wl || !n_fft || !bins || !frames) sg::bad_arguments("sg_spectrogram_size");
    const sg::SpgSetup S = sg::spg_setup(*p);
    *wl = S.wl;
    *n_fft = S.N;
    *bins = S.bins;
    *frames = sg::spg_frames(S, len);
  });
}

extern "C" const char* sg_spectrogram_size_error(void) { return sg::g_host_err.c_str(); }
