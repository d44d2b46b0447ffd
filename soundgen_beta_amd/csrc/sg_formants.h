// sg_formants.h — the formant tracks of analyze() (R/analyze.R:486-502): per analysed frame,
// phonTools::findformants(frame, fs, verify = FALSE) with its defaults, restated from
// phonTools 0.2-2.1 as documented. phonTools is not in the reference tree: PARITY UNPINNED,
// as for sg_dtw_symmetric2. Every constant taken from phonTools stands in this file, so a
// later pin against R touches this file alone.
//
//   order      round(fs / 1000) + 3, R's half-even round
//   frame      pre-emphasis y[i] = x[i] + coeff x[i - 1], coeff = -exp(-2 pi 50 / fs); minus
//              its mean; times the Hann window 0.5 (1 - cos(2 pi i / (n - 1)))
//   lags       r[k] = sum_i y[i] y[i + k], k = 0..order, unnormalised
//   predictor  T a = -r[1..order], T the Toeplitz matrix of r[0..order - 1]. phonTools calls
//              solve() (LU); here Levinson-Durbin, which agrees to about 1e-12 in the
//              coefficients. r[0] <= 0, a non-finite value or a prediction error <= 0: NA row
//   roots      all roots of z^p + a1 z^(p - 1) + ... + ap (R: polyroot(rev(coeffs))), by the
//              Aberth-Ehrlich iteration from p points on a circle, every root corrected from
//              the previous iterate of all the others, until every root has settled
//              (fmt_aberth_step) or kFmtMaxIter steps are spent (NA row)
//   formants   f = round(atan2(Im z, Re z) fs / (2 pi), 2), bw = -(fs / pi) log|z|, ordered by
//              f (order(): ties by root index), kept where bw < 600 & f > 200 & f < fs / 2;
//              analyze() takes the first nFormants kept rows, NA where there are fewer
// Stated difference: R's round(x, 2) multiplies in long double; here nearbyint(100 x) / 100
// in fp64. The two differ only where 100 x lies within an ulp of a half-integer.
//
// fmt_frame() is the whole chain behind the lags for one frame. It is written for `nlanes`
// lanes that run it together on one FmtShared (the device: the 64 lanes of a wave, lane j
// holding root j; the host: one lane that walks every index), with ops.sync() between a
// write and the reads of other lanes, ops.sum() the sum over the lanes and ops.all() their
// conjunction. Everything a lane branches on is the same in all lanes.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SG_FMT_HD __host__ __device__
#else
#define SG_FMT_HD
#endif

namespace sg {

// ---- phonTools::findformants' constants
constexpr double kFmtPreemphHz = 50.0;   // the pre-emphasis cutoff
constexpr double kFmtMaxBw = 600.0;      // maxbw
constexpr double kFmtMinFormant = 200.0; // minformant
constexpr int kFmtOrderExtra = 3;        // order = round(fs / 1000) + 3
// ---- this restatement's
constexpr int kFmtMaxOrder = 64;         // one root per lane of a wave
constexpr int kFmtMaxFormants = 8;       // nFormants
constexpr double kFmtRadius = 0.9;       // the circle of the initial points
constexpr int kFmtMaxIter = 64;          // Aberth iterations before a frame is given up
constexpr double kFmtTol = 4 * 2.220446049250313e-16;  // |correction| <= kFmtTol |z| in every lane
constexpr double kFmtSettle = 2.220446049250313e-16;   // |correction|^2 <= kFmtSettle |z|^2: the noise rule may apply
constexpr double kFmtTwoPi = 6.283185307179586476925286766559;

// round(fs / 1000) + 3 with R's half-even round (nearbyint under the default rounding mode)
SG_FMT_HD inline int fmt_order(double fs) { return (int)nearbyint(fs / 1000) + kFmtOrderExtra; }
SG_FMT_HD inline double fmt_preemph_coeff(double fs) { return -exp(-kFmtTwoPi * kFmtPreemphHz / fs); }
// sample i of the pre-emphasised frame from x[i] and x[i - 1] (prev is not read for i == 0)
SG_FMT_HD inline double fmt_preemph(double cur, double prev, int i, double coeff) { return i == 0 ? cur : cur + coeff * prev; }
// the Hann window at i of n (n >= 2)
SG_FMT_HD inline double fmt_hann(int i, int n) { return 0.5 * (1 - cos(kFmtTwoPi * (double)i / (double)(n - 1))); }
// steps 2-4 on sample i, given the pre-emphasised frame's mean
SG_FMT_HD inline double fmt_shape(double y, double mean, int i, int n) { return (y - mean) * fmt_hann(i, n); }

// what the lanes of one frame share (LDS on the device)
struct FmtShared {
  double r[kFmtMaxOrder + 1];            // the lags
  double a[kFmtMaxOrder], b[kFmtMaxOrder];  // a1..ap; Levinson's next row, later every root's last |correction|^2
  double zr[kFmtMaxOrder], zi[kFmtMaxOrder];  // the roots
  double wr[kFmtMaxOrder], wi[kFmtMaxOrder];  // their corrections; later formant and bandwidth
  double out[2 * kFmtMaxFormants];
};

// Levinson-Durbin for T a = -r[1..p] into sh.a; false where the frame gets an NA row
template <class Ops>
SG_FMT_HD inline bool fmt_levinson(FmtShared& sh, int p, int lane, int nlanes, const Ops& ops) {
  const double* r = sh.r;
  double E = r[0];
  if (!(E > 0) || !(E <= 1.79769313486231570815e308)) return false;
  for (int m = 1; m <= p; ++m) {
    double part = 0;
    for (int l = lane; l < m - 1; l += nlanes) part += sh.a[l] * r[m - 1 - l];
    const double acc = r[m] + ops.sum(part);
    const double k = -acc / E;  // the reflection coefficient
    for (int l = lane; l < m - 1; l += nlanes) sh.b[l] = sh.a[l] + k * sh.a[m - 2 - l];
    ops.sync();
    for (int l = lane; l < m - 1; l += nlanes) sh.a[l] = sh.b[l];
    if (lane == (m - 1) % nlanes) sh.a[m - 1] = k;
    ops.sync();
    E *= 1 - k * k;
    if (!(E > 0) || !(E <= 1.79769313486231570815e308)) return false;
  }
  return true;
}

// the initial points: p of them equally spaced on the circle, a quarter step off the real axis
template <class Ops>
SG_FMT_HD inline void fmt_aberth_start(FmtShared& sh, int p, int lane, int nlanes, const Ops& ops) {
  for (int l = lane; l < p; l += nlanes) {
    const double ang = kFmtTwoPi * ((double)l + 0.25) / (double)p;
    sh.zr[l] = kFmtRadius * cos(ang);
    sh.zi[l] = kFmtRadius * sin(ang);
    sh.b[l] = INFINITY;  // no correction yet (fmt_aberth_step)
  }
  ops.sync();
}

// One Aberth step: every root's correction w = N / (1 - N S), N = P(z) / P'(z) by Horner,
// S = sum_{k != l} 1 / (z_l - z_k), from the previous iterate; then z -= w. True when every
// root has settled (a NaN never does). A root settles, for good, when |w| <= kFmtTol |z|, or
// when its corrections have reached the rounding noise of P / P' and stopped shrinking: |w| <=
// sqrt(kFmtSettle) |z|, where a converging correction shrinks by orders of magnitude per step,
// and |w| >= half the previous |w|. Without the second rule a root whose noise lies above
// kFmtTol |z| (a pair close to its conjugate, a long frame) passes only by chance: on 50 ms
// frames at 44.1 kHz more than half of the frames ran into kFmtMaxIter.
template <class Ops>
SG_FMT_HD inline bool fmt_aberth_step(FmtShared& sh, int p, int lane, int nlanes, const Ops& ops) {
  for (int l = lane; l < p; l += nlanes) {
    const double x = sh.zr[l], y = sh.zi[l];
    double pr = 1, pi = 0, dr = 0, di = 0;
    for (int i = 0; i < p; ++i) {  // P' = P' z + P; P = P z + a[i + 1]
      const double tr = dr * x - di * y + pr, ti = dr * y + di * x + pi;
      dr = tr;
      di = ti;
      const double ur = pr * x - pi * y + sh.a[i], ui = pr * y + pi * x;
      pr = ur;
      pi = ui;
    }
    const double dd = dr * dr + di * di;
    const double nr = (pr * dr + pi * di) / dd, ni = (pi * dr - pr * di) / dd;
    double sr = 0, si = 0;
    for (int k = 0; k < p; ++k) {
      if (k == l) continue;
      const double ex = x - sh.zr[k], ey = y - sh.zi[k];
      const double inv = 1 / (ex * ex + ey * ey);  // one division per pair
      sr += ex * inv;
      si -= ey * inv;
    }
    const double qr = 1 - (nr * sr - ni * si), qi = -(nr * si + ni * sr);
    const double qq = qr * qr + qi * qi;
    sh.wr[l] = (nr * qr + ni * qi) / qq;
    sh.wi[l] = (ni * qr - nr * qi) / qq;
  }
  ops.sync();
  bool ok = true;
  for (int l = lane; l < p; l += nlanes) {
    const double wr = sh.wr[l], wi = sh.wi[l];
    const double x = sh.zr[l] - wr, y = sh.zi[l] - wi;
    sh.zr[l] = x;
    sh.zi[l] = y;
    const double w2 = wr * wr + wi * wi, z2 = x * x + y * y;
    const double prev = sh.b[l];  // the last |w|^2; negative once the root has settled
    const bool settled = prev < 0 || w2 <= (kFmtTol * kFmtTol) * z2 || (w2 <= kFmtSettle * z2 && w2 >= 0.25 * prev);
    sh.b[l] = settled ? -1.0 : w2;
    ok = ok && settled;
  }
  ops.sync();
  return ops.all(ok);
}

SG_FMT_HD inline double fmt_freq(double re, double im, double fs) { return atan2(im, re) * (fs / kFmtTwoPi); }
SG_FMT_HD inline double fmt_round2(double f) { return nearbyint(100 * f) / 100; }
SG_FMT_HD inline double fmt_bandwidth(double re, double im, double fs) { return -(fs / (kFmtTwoPi / 2)) * (0.5 * log(re * re + im * im)); }
SG_FMT_HD inline bool fmt_keep(double f, double bw, double fs) { return bw < kFmtMaxBw && f > kFmtMinFormant && f < fs / 2; }

// Step 8 on the roots in sh.zr / sh.zi: sh.out receives the first nFormants kept (formant,
// bandwidth) pairs in ascending order of formant, ties by root index, NaN behind them.
// With all == true, all_out (2 p doubles) receives every kept pair.
template <class Ops>
SG_FMT_HD inline void fmt_select(FmtShared& sh, int p, double fs, int nFormants, int lane, int nlanes, const Ops& ops,
                                 double* all_out = nullptr, int* n_all = nullptr) {
  for (int l = lane; l < p; l += nlanes) {
    const double re = sh.zr[l], im = sh.zi[l];
    sh.wr[l] = fmt_round2(fmt_freq(re, im, fs));
    sh.wi[l] = fmt_bandwidth(re, im, fs);
  }
  for (int c = lane; c < 2 * nFormants; c += nlanes) sh.out[c] = NAN;
  ops.sync();
  int kept = 0;
  for (int l = lane; l < p; l += nlanes) {
    const double f = sh.wr[l], bw = sh.wi[l];
    if (!fmt_keep(f, bw, fs)) continue;
    ++kept;
    int pos = 0;  // the kept entries that order() puts before this one
    for (int k = 0; k < p; ++k) {
      const double g = sh.wr[k];
      if (fmt_keep(g, sh.wi[k], fs) && (g < f || (g == f && k < l))) ++pos;
    }
    if (pos < nFormants) {
      sh.out[2 * pos] = f;
      sh.out[2 * pos + 1] = bw;
    }
    if (all_out) {
      all_out[2 * pos] = f;
      all_out[2 * pos + 1] = bw;
    }
  }
  if (n_all) *n_all = kept;  // one lane on the host
  ops.sync();
}

// The chain behind the lags for one frame: sh.r holds r[0..p] (published). Leaves the row in
// sh.out (published). Returns the Aberth iterations taken; 0 where Levinson-Durbin refuses
// the frame and -1 where the iteration hits kFmtMaxIter: an NA row in both cases.
template <class Ops>
SG_FMT_HD inline int fmt_frame(FmtShared& sh, int p, double fs, int nFormants, int lane, int nlanes, const Ops& ops) {
  int it = 0;
  bool done = false;
  if (fmt_levinson(sh, p, lane, nlanes, ops)) {
    fmt_aberth_start(sh, p, lane, nlanes, ops);
    while (!done && it < kFmtMaxIter) {
      done = fmt_aberth_step(sh, p, lane, nlanes, ops);
      ++it;
    }
  }
  if (!done) {
    for (int c = lane; c < 2 * nFormants; c += nlanes) sh.out[c] = NAN;
    ops.sync();
    return it == 0 ? 0 : -1;
  }
  fmt_select(sh, p, fs, nFormants, lane, nlanes, ops);
  return it;
}

// ---- findformants on a whole sound (matchPars: R/matchPars.R:130): the same steps over all N
// samples. The sound is cut into chunks of kFmtSoundChunk samples; the mean and every lag are
// sums of per-chunk sums, folded in chunk order (sg_formants.hip: sg_fmt_sound_*).
// Inside a chunk a lag's sum is split into segments, summed in index order and folded in
// segment order: as many segments as a workgroup of kFmtSoundThreads threads can give to
// each group of kFmtSoundLagWidth lags, of an odd number of samples (the device's LDS banks).
constexpr int kFmtSoundChunk = 4096;
constexpr int kFmtSoundThreads = 256;
constexpr int kFmtSoundLagWidth = 8;
SG_FMT_HD inline int64_t fmt_sound_chunks(int64_t n) { return n <= 0 ? 0 : (n + kFmtSoundChunk - 1) / kFmtSoundChunk; }
SG_FMT_HD inline int fmt_sound_groups(int p) { return (p + kFmtSoundLagWidth) / kFmtSoundLagWidth; }  // covering 0..p
SG_FMT_HD inline int fmt_sound_segments(int p) { return kFmtSoundThreads / fmt_sound_groups(p); }
SG_FMT_HD inline int fmt_sound_seglen(int p) { return ((kFmtSoundChunk + fmt_sound_segments(p) - 1) / fmt_sound_segments(p)) | 1; }
// the window and steps 2-4 with the sample's index in a sound longer than an int holds
SG_FMT_HD inline double fmt_hann(int64_t i, int64_t n) { return 0.5 * (1 - cos(kFmtTwoPi * (double)i / (double)(n - 1))); }
SG_FMT_HD inline double fmt_shape(double y, double mean, int64_t i, int64_t n) { return (y - mean) * fmt_hann(i, n); }

// the one lane of the host
struct FmtHostOps {
  void sync() const {}
  double sum(double v) const { return v; }
  bool all(bool b) const { return b; }
};

// The lags of a frame of n samples on the host, steps 2-5: y (n doubles of work space), r[0..p]
inline void fmt_lags_host(const double* x, int n, double fs, int p, double* y, double* r) {
  const double coeff = fmt_preemph_coeff(fs);
  double mean = 0;
  for (int i = 0; i < n; ++i) {
    y[i] = fmt_preemph(x[i], i ? x[i - 1] : 0.0, i, coeff);
    mean += y[i];
  }
  mean /= n;
  for (int i = 0; i < n; ++i) y[i] = fmt_shape(y[i], mean, i, n);
  for (int k = 0; k <= p; ++k) {
    double s = 0;
    for (int i = 0; i + k < n; ++i) s += y[i] * y[i + k];
    r[k] = s;
  }
}

// The lags of a whole sound of n samples on the host, in the device's chunk order: the mean
// from the chunks' sums of the pre-emphasised samples, folded in chunk order; lag k from the
// chunks' partial sums over the i of the chunk (y[i + k] read across the chunk's end, nothing
// past the sound's), folded in chunk order; a chunk's partial sum in the device's segments.
// y: n doubles of work space; r[0..p]. What is left to differ from the device: the order
// inside a chunk's sum for the mean, and the device's fused multiply-adds.
inline void fmt_sound_lags_host(const double* x, int64_t n, double fs, int p, double* y, double* r) {
  const double coeff = fmt_preemph_coeff(fs);
  const int64_t nchunks = fmt_sound_chunks(n);
  double mean = 0;
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t i0 = c * kFmtSoundChunk, i1 = i0 + kFmtSoundChunk < n ? i0 + kFmtSoundChunk : n;
    double s = 0;
    for (int64_t i = i0; i < i1; ++i) {
      y[i] = i == 0 ? x[i] : x[i] + coeff * x[i - 1];
      s += y[i];
    }
    mean += s;
  }
  mean /= (double)n;
  for (int64_t i = 0; i < n; ++i) y[i] = fmt_shape(y[i], mean, i, n);
  for (int k = 0; k <= p; ++k) r[k] = 0;
  const int S = fmt_sound_segments(p), L = fmt_sound_seglen(p);
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t i0 = c * kFmtSoundChunk, i1 = i0 + kFmtSoundChunk < n ? i0 + kFmtSoundChunk : n;
    for (int k = 0; k <= p; ++k) {
      double s = 0;
      for (int g = 0; g < S; ++g) {
        const int64_t a = i0 + (int64_t)g * L < i1 ? i0 + (int64_t)g * L : i1, b = a + L < i1 ? a + L : i1;
        double t = 0;
        for (int64_t i = a; i < b && i + k < n; ++i) t += y[i] * y[i + k];
        s += t;
      }
      r[k] += s;
    }
  }
}

}  // namespace sg
