// sg_summary.h — analyze(summary = TRUE) (R/analyze.R:770-796): one row of 2 + 3 * 14 cells
// per sound from its finished table: duration, the proportion of voiced frames, then the
// mean, median and sd of every acoustic variable over the frames where it is not NA.
// sum_sound() drives it for one sound with `nl` cooperating lanes: the 256 lanes of
// sg_anl_summary's workgroup on the device, one lane (and a sync that does nothing) on the
// host (tests/cpp/summary_pins.cpp). No HIP header is needed on the host side, no dynamic
// memory anywhere, and no bound on the frame count.
//
// Layout. The table is row-major, 25 or more doubles a row. The work is cut into kSumSlots
// x G items, G = max(1, nl / kSumSlots): item (v, g) owns variable v in the rows g, g + G,
// g + 2 G, ... A wave's 64 lanes are therefore 16 variables x 4 consecutive rows: each load
// instruction reads one contiguous 4-row span of the table (and the workgroup's 256 lanes
// 16 consecutive rows), 14 of whose 25+ columns are used. Every pass over the table has
// that shape.
//
// Mean and sd are R's (summary.c, cov.c) in fp64: the sum / n, refined once by the mean of
// the residuals; then the two-pass variance about the refined mean over n - 1. An item adds
// its rows in order and one lane folds a variable's G partial sums in order, so the result
// depends on (nl, frames) alone: a sound's row is the same bit for bit alone, in any batch,
// at any position. There are no floating-point atomics.
//
// The median is exact for any frame count: a radix select over the order-preserving 64-bit
// image of the doubles, eight 8-bit digits from the top, one 256-bin histogram per variable
// (integer adds, atomic on the device), narrowing to the value of rank (n - 1) / 2. For an
// even n one more pass counts the values <= that one and finds the smallest above it: the
// upper middle is the same value again if the count passes n / 2, the smallest above it
// otherwise. The two middles are averaged as R's mean() of two values. -0.0 is imaged as 0.0
// (x + 0.0), so the image cannot order the two zeros: a median that is a zero comes out as
// +0.0, equal as a number to what R's sort leaves there. +-Inf are ordinary values: plain
// IEEE arithmetic gives mean(c(Inf, 1)) = Inf, sd NaN, and a finite median.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SG_SUM_HD __host__ __device__
#else
#define SG_SUM_HD
#endif

namespace sg {

constexpr int kSumVars = 14;                // summarised variables
constexpr int kSumCols = 2 + 3 * kSumVars;  // duration, voiced, then mean / median / sd of each
constexpr int kSumSlots = 16;               // the variables, `voiced`, and one idle slot
constexpr int kSumVoiced = kSumVars;        // the slot that sums `voiced`
constexpr int kSumMaxGroups = 16;           // G for the device's 256 lanes
constexpr int kSumBins = 256;               // one 8-bit digit of the image per pass

// What the lanes of a workgroup share (LDS on the device)
struct SumShared {
  double part[kSumSlots * kSumMaxGroups];    // an item's partial sum
  uint64_t upart[kSumSlots * kSumMaxGroups];  // an item's count (and, in the last pass, its smallest image above)
  uint64_t umin[kSumSlots * kSumMaxGroups];
  double m[kSumSlots];        // the mean the next pass subtracts
  uint64_t n[kSumSlots];      // non-NA values
  uint64_t prefix[kSumSlots];  // the digits of the lower middle's image found so far
  uint64_t rank[kSumSlots];   // its rank among the values that share those digits
  uint32_t hist[kSumVars * kSumBins];
};

// The summarised variables in the reference's order: result's columns 3.. are sorted by name
// (R/analyze.R:706-707) under a case-insensitive collation, which puts `voiced` last, so
// myseq (:787) is aligned with vars (:771-772). c0: the first of the four columns behind the
// candidates (pitch, amplVoiced, voiced, harmonics).
SG_SUM_HD inline int sum_column(int v, int c0) {
  switch (v) {
    case 0: return 0;        // ampl
    case 1: return c0 + 1;   // amplVoiced
    case 2: return 3;        // dom
    case 3: return 1;        // entropy
    case 4: return c0 + 3;   // harmonics
    case 5: return 2;        // HNR
    case 6: return 6;        // meanFreq
    case 7: return 4;        // peakFreq
    case 8: return 5;        // peakFreqCut
    case 9: return c0;       // pitch
    case 10: return 7;       // quartile25
    case 11: return 8;       // quartile50
    case 12: return 9;       // quartile75
    case 13: return 10;      // specSlope
    case kSumVoiced: return c0 + 2;
    default: return -1;
  }
}

// the order-preserving image of a non-NaN double (with -0.0 taken as 0.0) and its inverse
SG_SUM_HD inline uint64_t sum_image(double x) {
  x = x + 0.0;
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
SG_SUM_HD inline double sum_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

SG_SUM_HD inline void sum_count(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, 1u);
#else
  __atomic_fetch_add(p, 1u, __ATOMIC_RELAXED);  // lanes may be host threads
#endif
}

SG_SUM_HD inline bool sum_finite(double x) { return x - x == 0.0; }

// mean() of the two middles (summary.c real_mean on two values)
SG_SUM_HD inline double sum_mean2(double a, double b) {
  double s = (a + b) / 2;
  if (sum_finite(s)) s = s + ((a - s) + (b - s)) / 2;
  return s;
}

// One sound: rows = nf rows of `cols` doubles (cols = 15 + 6 nCands + 4), len samples at
// samplingRate; out receives kSumCols doubles. nf <= 0 (a sound not longer than the window,
// or a failed call): kSumCols NaN. Every lane of the workgroup must call it (it syncs).
template <class Sync>
SG_SUM_HD inline void sum_sound(const double* rows, int64_t nf, int cols, int64_t len, double samplingRate, double* out,
                                int lane, int nl, SumShared& sh, Sync sync) {
  if (nf <= 0) {  // workgroup-uniform
    for (int c = lane; c < kSumCols; c += nl) out[c] = NAN;
    return;
  }
  const int c0 = cols - 4;
  const int G = nl / kSumSlots < 1 ? 1 : (nl / kSumSlots > kSumMaxGroups ? kSumMaxGroups : nl / kSumSlots);
  const int items = kSumSlots * G;
  // passes 0..2: the sum, the residuals about sum / n, the squares about the refined mean
  for (int pass = 0; pass < 3; ++pass) {
    for (int it = lane; it < items; it += nl) {
      const int v = it % kSumSlots, g = it / kSumSlots, col = sum_column(v, c0);
      double s = 0;
      uint64_t cnt = 0;
      if (col >= 0 && (pass == 0 || v < kSumVars)) {
        const double m = pass ? sh.m[v] : 0.0;
        for (int64_t r = g; r < nf; r += G) {
          const double x = rows[r * cols + col];
          if (x != x) continue;
          const double d = x - m;
          s += pass == 2 ? d * d : (pass == 1 ? d : x);
          ++cnt;
        }
      }
      sh.part[v * G + g] = s;
      sh.upart[v * G + g] = cnt;
    }
    sync();
    for (int v = lane; v < kSumSlots; v += nl) {
      if (v > kSumVoiced) continue;
      double s = 0;
      uint64_t n = 0;
      for (int g = 0; g < G; ++g) {
        s += sh.part[v * G + g];
        n += sh.upart[v * G + g];
      }
      if (pass == 0) {
        sh.n[v] = n;
        if (v == kSumVoiced) {
          out[0] = (double)len / samplingRate;  // result$duration[1], in s
          out[1] = s / (double)nf;              // mean(result$voiced)
        } else {
          sh.m[v] = s / (double)n;  // 0 / 0 is NaN: no value
          sh.prefix[v] = 0;
          sh.rank[v] = n ? (n - 1) / 2 : 0;
        }
      } else if (v < kSumVars) {
        if (pass == 1) {
          const double m1 = sh.m[v], m2 = m1 + s / (double)n;
          out[2 + 3 * v] = sum_finite(m1) ? m2 : m1;  // real_mean refines a finite mean only
          sh.m[v] = m2;                             // cov.c refines whatever it has
        } else {
          out[2 + 3 * v + 2] = n < 2 ? NAN : sqrt(s / (double)(n - 1));
        }
      }
    }
    sync();
  }
  // the lower middle: eight digits of its image, from the top
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = lane; i < kSumVars * kSumBins; i += nl) sh.hist[i] = 0;
    sync();
    for (int it = lane; it < items; it += nl) {
      const int v = it % kSumSlots, g = it / kSumSlots;
      if (v >= kSumVars) continue;
      const int col = sum_column(v, c0);
      const uint64_t pre = sh.prefix[v];
      for (int64_t r = g; r < nf; r += G) {
        const double x = rows[r * cols + col];
        if (x != x) continue;
        const uint64_t k = sum_image(x);
        if (shift < 56 && (k >> (shift + 8)) != (pre >> (shift + 8))) continue;
        sum_count(&sh.hist[v * kSumBins + (int)((k >> shift) & 255)]);
      }
    }
    sync();
    for (int v = lane; v < kSumVars; v += nl) {
      if (!sh.n[v]) continue;
      uint64_t rank = sh.rank[v];
      int d = 0;
      for (; d < kSumBins - 1; ++d) {
        const uint64_t h = sh.hist[v * kSumBins + d];
        if (rank < h) break;
        rank -= h;
      }
      sh.rank[v] = rank;
      sh.prefix[v] |= (uint64_t)d << shift;
    }
    sync();
  }
  // the upper middle of an even count
  for (int it = lane; it < items; it += nl) {
    const int v = it % kSumSlots, g = it / kSumSlots;
    uint64_t le = 0, above = ~0ull;
    if (v < kSumVars) {
      const int col = sum_column(v, c0);
      const uint64_t a = sh.prefix[v];
      for (int64_t r = g; r < nf; r += G) {
        const double x = rows[r * cols + col];
        if (x != x) continue;
        const uint64_t k = sum_image(x);
        if (k <= a)
          ++le;
        else if (k < above)
          above = k;
      }
    }
    sh.upart[v * G + g] = le;
    sh.umin[v * G + g] = above;
  }
  sync();
  for (int v = lane; v < kSumVars; v += nl) {
    const uint64_t n = sh.n[v];
    double med = NAN;
    if (n) {
      uint64_t le = 0, above = ~0ull;
      for (int g = 0; g < G; ++g) {
        le += sh.upart[v * G + g];
        if (sh.umin[v * G + g] < above) above = sh.umin[v * G + g];
      }
      const double a = sum_value(sh.prefix[v]);
      med = n % 2 ? a : sum_mean2(a, le > n / 2 ? a : sum_value(above));
    }
    out[2 + 3 * v + 1] = med;
  }
}

}  // namespace sg
