// sg_ssm.cpp — the host half of ssm() (R/SSM.R:63-360): the integer decisions
// (step, win, kernelSize, nBands, maxFreq :111-128; selfsim's win clamp, numWins
// and winIdx :228-244), getCheckerboardKernel (:281-324) and the DCT rows of
// tuneR's spec2cep / lifter (tuneR_1.3.2.tar.gz::tuneR/R/spec2cep.R:13-24,
// lifter.R:21-29). sg_ssm_size needs no device. The numpy restatement
// (soundgen_beta_amd/ssm.py) makes the same decisions in the same operation order.
#include "sg_ssm.h"

#include <algorithm>
#include <cmath>

#include "sg_rmath.h"

namespace sg {

SsmSetup ssm_setup(const sg_ssm_params& p) {
  SsmSetup S;
  S.sr = p.samplingRate;
  S.windowLength = p.windowLength;
  if (!(S.sr > 0) || !(S.windowLength > 0)) throw SgError(SG_E_ARG, "ssm: samplingRate and windowLength must be > 0");
  S.step = std::isnan(p.step) ? p.windowLength * (1 - p.overlap / 100) : p.step;
  if (!(S.step > 0)) throw SgError(SG_E_ARG, "ssm: step must be > 0");
  if (!(p.ssmWin >= 0) || !(p.kernelLen >= 0) || !(p.kernelSD > 0))
    throw SgError(SG_E_ARG, "ssm: ssmWin, kernelLen must be >= 0 and kernelSD > 0");
  S.win0 = std::max(1, (int)r_round(p.ssmWin / S.step / 2) * 2 - 1);
  const double frame_points = S.sr * S.windowLength / 1000;
  // in windowLength frames, not steps: the reference's quirk (R/SSM.R:117-119)
  S.K = (int)r_round(p.kernelLen * S.sr / 1000 / frame_points / 2) * 2;
  const double nBands = std::isnan(p.nBands) ? 100 * S.windowLength / 20 : p.nBands;
  if (!(nBands >= 1) || nBands > 4096) throw SgError(SG_E_ARG, "ssm: nBands must lie in 1..4096");
  S.nb = (int)nBands;
  S.maxFreq = std::isnan(p.maxFreq) ? std::floor(S.sr / 2) : p.maxFreq;
  S.kernelSD = p.kernelSD;
  S.winpts = (int)r_round(S.windowLength / 1000 * S.sr);
  S.steppts = (int)r_round(S.step / 1000 * S.sr);
  if (S.winpts < 2 || S.steppts < 1) throw SgError(SG_E_ARG, "ssm: window shorter than 2 samples");
  if (p.input < 0 || p.input > 2 || p.simil < 0 || p.simil > 1) throw SgError(SG_E_ARG, "ssm: unknown input or simil");
  S.input = p.input;
  S.norm = p.norm != 0;
  S.simil = p.simil;
  S.normalize = p.normalize != 0;
  if (p.n_mfcc < 1 || !p.mfcc) throw SgError(SG_E_ARG, "ssm: MFCC is empty");
  S.mfcc.assign(p.mfcc, p.mfcc + p.n_mfcc);
  int mx = 0;
  for (int32_t v : S.mfcc) {
    if (v < 1 || v > S.nb) throw SgError(SG_E_ARG, "ssm: MFCC indices must lie in 1..nBands");
    mx = std::max(mx, (int)v);
  }
  if (mx < 2) throw SgError(SG_E_ARG, "ssm: max(MFCC) must be >= 2 (tuneR's lifter fails below that)");
  return S;
}

SsmDims ssm_dims(const SsmSetup& S, int64_t len) {
  SsmDims d;
  if (len <= 1) {
    d.win = S.win0;
    return d;
  }
  // tuneR powspec via signal::specgram: starts 0, steppts, ..., nn steppts
  d.nf = len > S.winpts ? (int)((double)(len - S.winpts - 1) / S.steppts + 1e-10) + 1 : 1;
  int win = S.win0;
  if (win > d.nf / 2) win = d.nf / 2;
  if (win % 2 == 0) win = std::max((int)std::ceil(win / 2.0) * 2 - 1, 1);
  d.win = win;
  const int numWins = (int)std::ceil((double)d.nf / win);
  // round(seq(1, ncol - win, length.out = numWins)), R's round: half to even
  const double from = 1.0, to = (double)(d.nf - win);
  d.idx.resize(numWins);
  if (numWins == 1) {
    d.idx[0] = 0;
  } else {
    const double by = (to - from) / (numWins - 1);
    for (int i = 0; i < numWins; ++i) d.idx[i] = (int32_t)r_round(i == numWins - 1 ? to : from + i * by) - 1;
  }
  return d;
}

std::vector<double> ssm_checkerboard(int size, double sd) {
  if (size < 2) throw SgError(SG_E_ARG, "ssm: kernelLen is shorter than two windows (kernelSize < 2)");
  std::vector<double> x(size), k((size_t)size * size);
  const double by = 2.0 / (size - 1);
  for (int i = 0; i < size; ++i) x[i] = i == size - 1 ? 1.0 : -1.0 + i * by;
  if (size < 50) {
    std::vector<double> d(size);
    for (int i = 0; i < size; ++i) {
      const double z = x[i] / sd;
      d[i] = std::exp(-0.5 * (z * z)) / (sd * std::sqrt(2 * M_PI));
    }
    for (int i = 0; i < size; ++i)
      for (int j = 0; j < size; ++j) k[(size_t)i * size + j] = d[i] * d[j];
  } else {  // mvtnorm::dmvnorm(sigma = diag(2) * kernelSD): kernelSD as a variance (quirk kept)
    for (int i = 0; i < size; ++i)
      for (int j = 0; j < size; ++j)
        k[(size_t)i * size + j] = std::exp(-0.5 * (x[i] * x[i] / sd + x[j] * x[j] / sd)) / (2 * M_PI * sd);
  }
  const int lo = size / 2, hi = (size + 1) / 2;
  for (int i = 0; i < lo; ++i)
    for (int j = hi; j < size; ++j) k[(size_t)i * size + j] = -k[(size_t)i * size + j];
  for (int i = hi; i < size; ++i)
    for (int j = 0; j < hi; ++j) k[(size_t)i * size + j] = -k[(size_t)i * size + j];
  const double mx = *std::max_element(k.begin(), k.end());
  for (double& v : k) v /= mx;
  return k;
}

void ssm_dct(const SsmSetup& S, std::vector<double>& dct, std::vector<double>& lift) {
  const int D = (int)S.mfcc.size(), nb = S.nb;
  dct.assign((size_t)D * nb, 0.0);
  lift.assign(D, 1.0);
  for (int d = 0; d < D; ++d) {
    const int i = S.mfcc[d] - 1;
    for (int b = 0; b < nb; ++b) {
      double v = std::cos((double)i * (2 * b + 1) / (2 * nb) * M_PI) * std::sqrt(2.0 / nb);
      if (i == 0) v /= std::sqrt(2.0);
      dct[(size_t)d * nb + b] = v;
    }
    lift[d] = i == 0 ? 1.0 : std::pow((double)i, 0.6);
  }
}

}  // namespace sg

extern "C" int sg_ssm_size(int64_t len, const sg_ssm_params* p, int32_t* n_frames, int32_t* n, int32_t* win,
                           int32_t* kernel_size) {
  return sg::host_guarded([&]() {
    if (!p || !n_frames || !n || !win || !kernel_size) sg::bad_arguments("sg_ssm_size");
    const sg::SsmSetup S = sg::ssm_setup(*p);
    const sg::SsmDims d = sg::ssm_dims(S, len);
    *n_frames = d.nf;
    *n = (int32_t)d.idx.size();
    *win = d.win;
    *kernel_size = S.K;
  });
}
