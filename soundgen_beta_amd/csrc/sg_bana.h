// sg_bana.h — the candidate logic of getPitchSpec (R/utilities_analyze.R:461-555, a
// modified BaNa: Ba et al. 2012, "BaNa: A hybrid approach for noise resilient pitch
// detection", IEEE SSP) once the spectral peaks are known: the single-peak branch,
// the ratios of the five lowest peaks against BaNaRatios, the range filter, the
// sort, the merge loop, the certainty, the stable ranking, specThres and nCands.
// One function for the device (one thread of sg_anl_bana runs it) and the host
// (tests/cpp/bana_pins.cpp); no HIP header is needed on the host side, no dynamic
// memory anywhere.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SG_BANA_HD __host__ __device__
#else
#define SG_BANA_HD
#endif

namespace sg {

constexpr int kBanaRows = 9;    // BaNaRatios (R/sysdata.rda)
constexpr int kBanaPeaks = 5;   // "analyze five lowest harmonics" (:475)
constexpr int kBanaCands = 10;  // pairs A > B of five peaks; the table's rows do not overlap

struct BanaPars {
  double pitchFloor, pitchCeiling, specSinglePeakCert, specThres, specMerge;
  int nCands;
};

// BaNaRatios: a ratio strictly inside (value_low, value_high) says the lower peak is
// harmonic number divide_lower_by. Row order as in the data frame.
SG_BANA_HD inline double bana_low(int r) {
  const double v[kBanaRows] = {1.9, 2.8, 1.42, 3.8, 1.29, 4.8, 2.4, 1.59, 1.15};
  return v[r];
}
SG_BANA_HD inline double bana_high(int r) {
  const double v[kBanaRows] = {2.1, 3.2, 1.59, 4.2, 1.42, 5.2, 2.6, 1.8, 1.29};
  return v[r];
}
SG_BANA_HD inline double bana_div(int r) {
  const double v[kBanaRows] = {1, 1, 2, 1, 3, 1, 2, 3, 4};
  return v[r];
}

// pf: the frequencies (Hz) of the lowest min(npeaks, 5) peaks, ascending; npeaks:
// how many peaks the frame has (0, 1 and >= 2 are the three branches). cand / cert
// receive up to P.nCands candidates, best first; the number written is returned
// (0: NULL, or the all-NA row R makes of an emptied table).
SG_BANA_HD inline int bana_candidates(const double* pf, int npeaks, const BanaPars& P, double* cand, double* cert) {
#if defined(__clang__)
#pragma clang fp contract(off)  // the certainty's products and sums as R makes them, on both sides
#endif
  double pc[kBanaCands], pa[kBanaCands];
  int ai[kBanaCands];
  int n = 0;
  if (npeaks <= 0) return 0;
  if (npeaks == 1) {  // :461-472
    if (!(pf[0] < P.pitchCeiling && pf[0] > P.pitchFloor)) return 0;
    pc[0] = pf[0];
    pa[0] = P.specSinglePeakCert;
    n = 1;
  } else {
    const int np = npeaks < kBanaPeaks ? npeaks : kBanaPeaks;  // :475
    // :487-507 for (i in 2:np) for (j in 1:(np - 1)), kept where A > B
    for (int i = 1; i < np; ++i)
      for (int j = 0; j < i; ++j) {
        const double ratio = pf[i] / pf[j];
        for (int r = 0; r < kBanaRows; ++r)
          if (ratio > bana_low(r) && ratio < bana_high(r) && n < kBanaCands) {
            const double c = pf[j] / bana_div(r);
            if (c > P.pitchFloor && c < P.pitchCeiling) pc[n++] = c;  // :511-512
          }
      }
    if (n == 0) return 0;
    for (int i = 1; i < n; ++i) {  // sort(): ascending
      const double v = pc[i];
      int k = i;
      for (; k > 0 && pc[k - 1] > v; --k) pc[k] = pc[k - 1];
      pc[k] = v;
    }
    for (int i = 0; i < n; ++i) ai[i] = 1;
    int c = 0;  // :521-536
    while (c + 1 < n) {
      if (fabs(log2(pc[c] / pc[c + 1])) < P.specMerge / 12) {
        ai[c] += 1;
        pc[c] = (pc[c] + pc[c + 1]) / 2;  // mean() of the running value and the next
        for (int k = c + 1; k + 1 < n; ++k) {
          pc[k] = pc[k + 1];
          ai[k] = ai[k + 1];
        }
        --n;
      } else {
        ++c;
      }
    }
    for (int i = 0; i < n; ++i)  // :537-539
      pa[i] = P.specSinglePeakCert + (1 / (1 + exp(-(double)(ai[i] - 1))) - 0.5) * 2 * (1 - P.specSinglePeakCert);
    for (int i = 1; i < n; ++i) {  // order(pitchAmpl, decreasing = TRUE): stable
      const double v = pa[i], w = pc[i];
      int k = i;
      for (; k > 0 && pa[k - 1] < v; --k) {
        pa[k] = pa[k - 1];
        pc[k] = pc[k - 1];
      }
      pa[k] = v;
      pc[k] = w;
    }
  }
  int m = 0;  // :550-555
  for (int i = 0; i < n && m < P.nCands; ++i)
    if (pa[i] > P.specThres) {
      cand[m] = pc[i];
      cert[m] = pa[i];
      ++m;
    }
  return m;
}

}  // namespace sg
