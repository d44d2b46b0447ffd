// sg_segment.cpp — the host half of segment() (R/segment.R:79-219): hilbert()'s padding
// and un-padding (seewave_2.0.5.tar.gz::seewave/R/seewave.r:3336-3363),
// windowLength_points (segment.R:127-130), the windows of env()'s msmooth
// (seewave.r:2489-2498: seq() with a fractional `by`, from:to from a fractional from, the
// truncating index), the time step and findSyllables' shortest run. No device is needed.
// The numpy restatement (soundgen_beta_amd/segment.py) makes the same decisions from the
// same fp64 operations in the same order.
#include <cfloat>
#include <cmath>
#include <string>

#include "sg_rmath.h"
#include "sg_segment_plan.h"

#pragma clang fp contract(off)

namespace sg {

SegPars seg_pars(const sg_segment_params& p) {
  if (!(p.samplingRate > 0) || !(p.windowLength > 0))
    throw SgError(SG_E_ARG, "segment: samplingRate and windowLength must be > 0");
  if (std::isnan(p.overlap) || std::isnan(p.shortestSyl) || std::isnan(p.sylThres) || std::isnan(p.interburstMult) ||
      std::isnan(p.burstThres) || std::isnan(p.peakToTrough))
    throw SgError(SG_E_ARG, "segment: an argument is not a number");
  if (p.interburst < 0) throw SgError(SG_E_ARG, "interburst is negative");
  if (p.workspace_cap < 0) throw SgError(SG_E_ARG, "segment: workspace_cap is negative");
  SegPars P;
  P.sylThres = p.sylThres;
  P.shortestSyl = p.shortestSyl;
  P.shortestPause = p.shortestPause;
  P.interburst = p.interburst;
  P.interburstMult = p.interburstMult;
  P.burstThres = p.burstThres;
  P.peakToTrough = p.peakToTrough;
  P.troughLeft = p.troughLeft != 0;
  P.troughRight = p.troughRight != 0;
  return P;
}

SegPlan seg_plan(const sg_segment_params& p, int64_t len, bool windows) {
  if (p.mode != 0 && p.mode != 1) throw SgError(SG_E_ARG, "segment: unknown mode");
  if (len < 2) throw SgError(SG_E_ARG, "segment: x must be a numeric vector longer than 1");
  SegPlan S;
  S.n1 = len;
  while (S.N < len) {  // 2^ceiling(log2(n)); n itself when log2(n) is whole
    S.N *= 2;
    ++S.p;
  }
  if (S.p > kSegMaxLog2)
    throw SgError(SG_E_UNSUPPORTED, "segment: the sound needs a transform of more than 2^22 points (" +
                                        std::to_string(len) + " samples)");
  const int64_t diffn = S.N - len;
  S.left = diffn / 2;
  // ht[floor(diffn / 2):(n1 + floor(diffn / 2) - 1)]: one sample early; 0:(n1 - 1) drops the 0
  S.shift = S.left > 0 ? S.left - 1 : 0;
  S.n_env = diffn == 1 ? len - 1 : len;
  if (p.mode == 1) return S;
  (void)seg_pars(p);
  const double ov = std::fmin(std::fmax(p.overlap, 0.0), 99.0);
  double wl = std::ceil(p.windowLength * p.samplingRate / 1000);
  if (wl > (double)len / 2) wl = (double)len / 2;
  if (wl == 0 || wl == 1) throw SgError(SG_E_ARG, "segment: 'smooth' window length cannot be equal to 0 or 1");
  S.wl = wl;
  const vec step = r_seq_by(1.0, (double)len - wl, wl - (ov * wl / 100));
  S.m = (int64_t)step.size();
  if (S.m < 1 || S.m > 2147483647LL) throw SgError(SG_E_ARG, "segment: no smoothing window");
  S.timestep = 1000 / p.samplingRate * ((double)len / (double)S.m);
  S.minCount = seg_min_count(p.shortestSyl, S.timestep);
  for (int64_t i = 0; i < S.m; ++i) {
    const double x = step[i], to = x + wl;
    const int64_t cnt = (int64_t)(std::fabs(to - x) + 1 + (double)FLT_EPSILON);  // length of from:to (seq_colon)
    // from:to is from + 0, from + 1, ... in fp64 and the index truncates: below a whole number by a
    // rounding error, from + j stays below one until the sum rounds to the whole number itself;
    // from there on the indices are one further and the window has skipped one value
    // (a sum that has rounded to its whole number stays there as j grows: the last point tells)
    const int64_t first = (int64_t)x;
    int64_t jump = cnt;
    if ((int64_t)(x + (double)(cnt - 1)) != first + cnt - 1)
      for (int64_t j = 0; j < cnt; ++j) {
        const int64_t off = (int64_t)(x + (double)j) - first - j;
        if (off < 0 || off > 1 || (off == 0 && jump < cnt))
          throw SgError(SG_E_UNSUPPORTED, "segment: a smoothing window that skips more than one value");
        if (off == 1 && jump == cnt) jump = j;
      }
    const int64_t last = first + cnt - 1 + (jump < cnt ? 1 : 0);
    if (first < 1 || last > S.n_env) throw SgError(SG_E_ARG, "segment: a smoothing window leaves the envelope (NA in R)");
    if (i == 0) S.points = cnt;
    if (windows) {
      S.first.push_back((int32_t)(first - 1));
      S.count.push_back((int32_t)cnt);
      S.jump.push_back((int32_t)jump);
    }
  }
  return S;
}

int64_t seg_out_cells(const sg_segment_params& p, const SegPlan& S) { return p.mode == 1 ? S.n_env : seg_cells(S.m); }

}  // namespace sg

extern "C" {

int sg_segment_size(int64_t len, const sg_segment_params* p, int32_t* log2n, int32_t* n_env, int32_t* points,
                    int64_t* cells) {
  return sg::host_guarded([&] {
    if (!p || !log2n || !n_env || !points || !cells) sg::bad_arguments("sg_segment_size");
    const sg::SegPlan S = sg::seg_plan(*p, len, false);
    *log2n = S.p;
    *n_env = (int32_t)(p->mode == 1 ? S.n_env : S.m);
    *points = (int32_t)S.points;
    *cells = sg::seg_out_cells(*p, S);
  });
}

const char* sg_segment_size_error(void) { return sg::g_host_err.c_str(); }

int sg_segment_windows(int64_t len, const sg_segment_params* p, int64_t* first, int64_t* points, int64_t* jump,
                       int32_t n, double* timestep) {
  return sg::host_guarded([&] {
    if (!p || !first || !points || !jump || !timestep || p->mode != 0) sg::bad_arguments("sg_segment_windows");
    const sg::SegPlan S = sg::seg_plan(*p, len, true);
    if (n != S.m) throw sg::SgError(SG_E_ARG, "sg_segment_windows: n is not the envelope's length");
    for (int32_t i = 0; i < n; ++i) {
      first[i] = S.first[i];
      points[i] = S.count[i];
      jump[i] = S.jump[i];
    }
    *timestep = S.timestep;
  });
}

}  // extern "C"
