// sg_segment.h — segment() behind its smoothed envelope (R/segment.R:146-212,
// R/utilities_segment.R): the threshold, findSyllables (rle, the strict length test, the
// start quirks), mergeSyllables, the interburst window, findBursts and the eleven summary
// columns, as plain functions. seg_sound() drives them for one sound with `nl`
// cooperating lanes: the 64 lanes of sg_seg_tail's workgroup on the device, one lane (and
// a sync that does nothing) on the host (tests/cpp/segment_pins.cpp). No HIP header is
// needed on the host side, no dynamic memory anywhere. The numpy restatement is
// soundgen_beta_amd/segment.py; the reference's quirks are listed there.
//
// A sound's cells (doubles), seg_cells(m) of them for m envelope values:
//   [0] m  [1] rows of the syllable table  [2] 1 if a syllable was found (0: the table is
//   the one row syllable = 0, NaN elsewhere, and its fourth column is `dur`)  [3] bursts
//   [4] timestep (ms)  [5] threshold  [6] interburst (ms)  [7] n = floor(interburst / timestep)
//   [8 .. 18] the summary row: nSyl, sylLen_mean, sylLen_median, sylLen_sd, pauseLen_mean,
//             pauseLen_median, pauseLen_sd, nBursts, interburst_mean, interburst_median,
//             interburst_sd (NaN for NA)
//   seg_env0()    the envelope, m values
//   seg_syl0(m)   the syllable table, rows x (syllable, start, end, sylLen, pauseLen); room
//                 for ceil(m / 2) rows (runs above the threshold alternate with runs below)
//   seg_bur0(m)   the burst table, bursts x (time, ampl, interburstInt); room for m rows
//   seg_scr0(m)   m cells of scratch (the medians' sorted copies)
//
// Order of the sums, part of the results: mean(envelope) -- lane l adds its values l, l +
// nl, ... in order, then every lane folds the nl partial sums in lane order (it depends on
// nl alone, not on the launch); the summary's means and sds -- one lane, in row order, the
// mean refined once as R's mean() does, in fp64 where R has long double. Every time and
// length is made of the same fp64 operations as the restatement's, unfused.
//
// The default cap of the transform workspace of one chunk of a batch (sg_segment.hip
// splits a batch into as many chunks as this needs; a sound larger than the cap runs alone):
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_SEG_HD __host__ __device__
#else
#define SG_SEG_HD
#endif

namespace sg {

constexpr int64_t kSegWorkspaceCap = int64_t(1) << 30;  // bytes: 2^26 complex doubles, sixteen 2^22-point sounds
constexpr int kSegMaxLog2 = 22;                         // N = 2^p = N1 N2, both <= 2048 (fft64's LDS frame)
constexpr int kSegHead = 8, kSegSummary = 11;
constexpr int kSegM = 0, kSegRows = 1, kSegFound = 2, kSegBursts = 3, kSegTimestep = 4, kSegThreshold = 5,
              kSegInterburst = 6, kSegN = 7;

SG_SEG_HD inline int64_t seg_env0() { return kSegHead + kSegSummary; }
SG_SEG_HD inline int64_t seg_max_syl(int64_t m) { return (m + 1) / 2; }
SG_SEG_HD inline int64_t seg_syl0(int64_t m) { return seg_env0() + m; }
SG_SEG_HD inline int64_t seg_bur0(int64_t m) { return seg_syl0(m) + 5 * seg_max_syl(m); }
SG_SEG_HD inline int64_t seg_scr0(int64_t m) { return seg_bur0(m) + 3 * m; }
SG_SEG_HD inline int64_t seg_cells(int64_t m) { return seg_scr0(m) + m; }

// A (sound, parameter row) pair of a sweep keeps the head, the two tables and the scratch,
// not the envelope and not the summary row (that one goes to the sweep's output)
SG_SEG_HD inline int64_t seg_pair_syl0() { return kSegHead; }
SG_SEG_HD inline int64_t seg_pair_bur0(int64_t m) { return seg_pair_syl0() + 5 * seg_max_syl(m); }
SG_SEG_HD inline int64_t seg_pair_scr0(int64_t m) { return seg_pair_bur0(m) + 3 * m; }
SG_SEG_HD inline int64_t seg_pair_cells(int64_t m) { return seg_pair_scr0(m) + m; }

// findSyllables' shortest run, ceiling(shortestSyl / timestep): the planner's statement and
// the sweep's, which makes it per pair on the device
SG_SEG_HD inline int64_t seg_min_count(double shortestSyl, double timestep) {
  return (int64_t)fmin(ceil(shortestSyl / timestep), 4e18);
}

// What every sound of a launch shares; timestep and the shortest run come per sound
struct SegPars {
  double sylThres, shortestSyl;
  double shortestPause;  // NaN: mergeSyl = FALSE
  double interburst;     // NaN: median(sylLen) * interburstMult, or shortestSyl without a syllable
  double interburstMult, burstThres, peakToTrough;
  int troughLeft, troughRight;
};

SG_SEG_HD inline bool seg_isnan(double v) { return v != v; }

// v as it is rounded, for a product that must not fuse with the sum behind it: the library is
// built with -ffp-contract=fast, under which the device compiler fuses across the contract(off)
// pragmas below. The empty statement holds no instruction; the compiler cannot see through it.
SG_SEG_HD inline double seg_rounded(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
  return v;
}

// v[0 .. n) ascending (heapsort: no recursion, no memory)
SG_SEG_HD inline void seg_sort(double* v, int64_t n) {
  for (int64_t start = n / 2 - 1, end = n; end > 1;) {
    int64_t root;
    if (start >= 0) {
      root = start--;
    } else {
      --end;
      const double t = v[0];
      v[0] = v[end];
      v[end] = t;
      root = 0;
      if (end <= 1) break;
    }
    for (;;) {
      int64_t c = 2 * root + 1;
      if (c >= end) break;
      if (c + 1 < end && v[c] < v[c + 1]) ++c;
      if (!(v[root] < v[c])) break;
      const double t = v[root];
      v[root] = v[c];
      v[c] = t;
      root = c;
    }
  }
}

// mean(), median() and sd() of column `col` of the first n rows of a table of `stride`
// columns (no NA among them); scr: n cells
SG_SEG_HD inline double seg_mean(const double* t, int stride, int col, int64_t n) {
  if (n <= 0) return NAN;
  double s = 0;
  for (int64_t i = 0; i < n; ++i) s += t[i * stride + col];
  s /= (double)n;
  double r = 0;
  for (int64_t i = 0; i < n; ++i) r += t[i * stride + col] - s;
  return s + r / (double)n;
}
SG_SEG_HD inline double seg_median(const double* t, int stride, int col, int64_t n, double* scr) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (n <= 0) return NAN;
  for (int64_t i = 0; i < n; ++i) scr[i] = t[i * stride + col];
  seg_sort(scr, n);
  const int64_t h = (n + 1) / 2;
  return n % 2 ? scr[h - 1] : (scr[h - 1] + scr[h]) / 2;
}
SG_SEG_HD inline double seg_sd(const double* t, int stride, int col, int64_t n) {
  if (n < 2) return NAN;
  const double m = seg_mean(t, stride, col, n);
  double s = 0;
  for (int64_t i = 0; i < n; ++i) {
    const double d = t[i * stride + col] - m;
    s += d * d;
  }
  return sqrt(s / (double)(n - 1));
}

// findSyllables (utilities_segment.R:18-69) and mergeSyllables (:80-91) for one lane: the
// table at syl; returns its rows and whether a syllable was found
SG_SEG_HD inline int64_t seg_syllables(const double* env, int64_t m, double thr, double timestep, int64_t minCount,
                                       double shortestPause, double* syl, int* found) {
#if defined(__clang__)
#pragma clang fp contract(off)  // start + count * timestep: a product and a sum, as R makes them
#endif
  int64_t rows = 0;
  const bool begins_above = env[0] > thr;
  for (int64_t i = 0; i < m;) {  // rle: the run [i, j)
    const bool above = env[i] > thr;
    int64_t j = i + 1;
    while (j < m && (env[j] > thr) == above) ++j;
    const int64_t count = j - i;
    if (above && count > minCount) {
      // sum(count[1:(idx - 1)]): the i values in front; for idx == 1, 1:0 is c(1, 0): count[1]
      double start = (double)(i == 0 ? count : i) * timestep;
      if (rows == 0 && begins_above) start = 0;  // syllables$start[1] = 0: the first KEPT one
      syl[5 * rows + 1] = start;
      syl[5 * rows + 2] = start + seg_rounded((double)count * timestep);
      ++rows;
    }
    i = j;
  }
  if (rows == 0) {
    *found = 0;
    syl[0] = 0;
    syl[1] = syl[2] = syl[3] = syl[4] = NAN;
    return 1;
  }
  *found = 1;
  if (!seg_isnan(shortestPause)) {  // row w swallows its successors while the gap is short
    int64_t w = 0;
    for (int64_t r = 1; r < rows; ++r) {
      if (syl[5 * r + 1] - syl[5 * w + 2] < shortestPause) {
        syl[5 * w + 2] = syl[5 * r + 2];
      } else {
        ++w;
        syl[5 * w + 1] = syl[5 * r + 1];
        syl[5 * w + 2] = syl[5 * r + 2];
      }
    }
    rows = w + 1;
  }
  for (int64_t r = 0; r < rows; ++r) {
    syl[5 * r] = (double)(r + 1);
    syl[5 * r + 3] = syl[5 * r + 2] - syl[5 * r + 1];
    syl[5 * r + 4] = r + 1 < rows ? syl[5 * (r + 1) + 1] - syl[5 * r + 2] : NAN;
  }
  return rows;
}

// findBursts' test of point i (1-based) (utilities_segment.R:122-165)
SG_SEG_HD inline bool seg_is_burst(const double* env, int64_t m, int64_t n, int64_t i, double vmax, const SegPars& P) {
  const double v = env[i - 1];
  if (!(v / vmax > P.burstThres)) return false;  // cond2
  const bool left = i > n, right = i < m - n - 1;
  const int64_t ll = left ? i - n : 1, lr = right ? i + n : m;
  double mx = env[ll - 1];
  for (int64_t k = ll; k <= lr; ++k) mx = fmax(mx, env[k - 1]);
  if (!(v == mx)) return false;  // cond1
  if (P.troughLeft) {
    double mn = 0;
    if (left) {
      mn = v;
      for (int64_t k = i - n; k <= i; ++k) mn = fmin(mn, env[k - 1]);
    }
    if (!(v / mn > P.peakToTrough)) return false;
  }
  if (P.troughRight) {
    double mn = 0;
    if (right) {
      mn = v;
      for (int64_t k = i; k <= i + n; ++k) mn = fmin(mn, env[k - 1]);
    }
    if (!(v / mn > P.peakToTrough)) return false;
  }
  return true;
}

// One sound whose envelope (m values at env) lies apart from what is written: o = the
// kSegHead head cells, sum = the summary row, syl / bur / scr = the tables and the scratch
// with the room the layout above gives them. red: nl doubles shared by the lanes. A parameter
// sweep (sg_seg_sweep_tail) reads one envelope for many parameter rows this way.
template <class Sync>
SG_SEG_HD inline void seg_sound_at(const SegPars& P, double timestep, int64_t minCount, int64_t m, const double* env,
                                   double* o, double* sum, double* syl, double* bur, double* scr, int lane, int nl,
                                   double* red, Sync sync) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (m <= 0) {  // a sound the reference stops on: nothing but the counts
    if (lane == 0) {
      for (int k = 0; k < kSegHead; ++k) o[k] = 0;
      for (int k = 0; k < kSegSummary; ++k) sum[k] = NAN;
      sum[0] = sum[7] = 0;
    }
    return;
  }
  double s = 0, mx = -INFINITY;
  for (int64_t i = lane; i < m; i += nl) {
    s += env[i];
    mx = fmax(mx, env[i]);
  }
  red[lane] = s;
  sync();
  double tot = 0;
  for (int l = 0; l < nl; ++l) tot += red[l];
  sync();
  red[lane] = mx;
  sync();
  double vmax = -INFINITY;
  for (int l = 0; l < nl; ++l) vmax = fmax(vmax, red[l]);
  sync();
  const double thr = tot / (double)m * P.sylThres;
  int64_t rows = 0;
  int found = 0;
  if (lane == 0) {
    rows = seg_syllables(env, m, thr, timestep, minCount, P.shortestPause, syl, &found);
    double ib = P.interburst;
    if (seg_isnan(ib)) ib = found ? seg_median(syl, 5, 3, rows, scr) * P.interburstMult : P.shortestSyl;
    const double q = floor(ib / timestep);
    o[kSegM] = (double)m;
    o[kSegRows] = (double)rows;
    o[kSegFound] = (double)found;
    o[kSegTimestep] = timestep;
    o[kSegThreshold] = thr;
    o[kSegInterburst] = ib;
    o[kSegN] = q;
    red[0] = q < (double)m ? q : (double)m;  // beyond m every n decides alike
  }
  sync();
  const int64_t n = (int64_t)red[0];
  for (int64_t i = lane + 1; i <= m; i += nl) bur[3 * (i - 1)] = seg_is_burst(env, m, n, i, vmax, P) ? 1.0 : 0.0;
  sync();
  if (lane != 0) return;
  // the flags sit in the first cell of rows 0 .. m - 1: row nb <= i - 1 is written after flag i was read
  int64_t nb = 0;
  for (int64_t i = 1; i <= m; ++i) {
    if (bur[3 * (i - 1)] == 0.0) continue;
    bur[3 * nb] = (double)i * timestep;
    bur[3 * nb + 1] = env[i - 1];
    ++nb;
  }
  for (int64_t k = 0; k < nb; ++k) bur[3 * k + 2] = k + 1 < nb ? bur[3 * (k + 1)] - bur[3 * k] : NAN;
  o[kSegBursts] = (double)nb;
  sum[0] = (double)rows;
  sum[1] = found ? seg_mean(syl, 5, 3, rows) : NAN;
  sum[2] = found ? seg_median(syl, 5, 3, rows, scr) : NAN;
  sum[3] = found ? seg_sd(syl, 5, 3, rows) : NAN;
  sum[4] = found ? seg_mean(syl, 5, 4, rows - 1) : NAN;  // na.rm: the last row is the NA
  sum[5] = found && rows > 1 ? seg_median(syl, 5, 4, rows - 1, scr) : NAN;
  sum[6] = NAN;  // sd(pauseLen) without na.rm: the last pauseLen is NA
  sum[7] = (double)nb;
  sum[8] = seg_mean(bur, 3, 2, nb - 1);
  sum[9] = seg_median(bur, 3, 2, nb - 1, scr);
  sum[10] = seg_sd(bur, 3, 2, nb - 1);
}

// One sound: o = its cells with the envelope in place
template <class Sync>
SG_SEG_HD inline void seg_sound(const SegPars& P, double timestep, int64_t minCount, int64_t m, double* o, int lane,
                                int nl, double* red, Sync sync) {
  const int64_t mm = m > 0 ? m : 0;
  seg_sound_at(P, timestep, minCount, m, o + seg_env0(), o, o + kSegHead, o + seg_syl0(mm), o + seg_bur0(mm),
               o + seg_scr0(mm), lane, nl, red, sync);
}

}  // namespace sg
