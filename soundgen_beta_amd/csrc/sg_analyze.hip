// sg_analyze.hip — the per-frame stage of analyze() on the device (R/analyze.R:233-575,
// R/utilities_analyze.R:22-324), fp64 throughout. A frame's row of the output table
// holds the columns of sg::AnlCol, then autocorCand[nCands] and autocorCert[nCands];
// NaN is R's NA.
//
//   (spectrogram_device, output = 'original': the normalisation statistics and the
//    |X| frames, to scratch. analyze() normalises and getFrameBank normalises again;
//    the second pass divides by exactly 1, so it runs once.)
//   sg_anl_ampl   :455-462 RMS of the wl + 1 normalised samples of a frame's
//                 amplitude window; the sound's min(ampl) (an order-preserving key)
//   sg_anl_spec   one workgroup per frame, its magnitudes in LDS: getEntropy over
//                 rowLow:rowHigh (:466-470), the two gates (:472-473), analyzeFrame's
//                 descriptives (utilities_analyze.R:45-69) for cond_silence frames,
//                 getDom (:190-233) for cond_entropy frames
//   sg_anl_acf    one workgroup per cond_entropy frame: the windowed frame rebuilt
//                 in LDS, acf() at the lags getPitchAutocor reads (direct sums, four
//                 consecutive lags per thread), / the filter table (:479-481), then
//                 getPitchAutocor (:250-324) and the dom certainty (:151-159)
// pitch_candidates (sg_pitch_candidates*) runs the same sequence on rows that also hold
// cepCand, cepCert, specCand, specCert (nCands each) and adds, each only if its method
// is asked for, one workgroup per cond_entropy frame:
//   sg_anl_cep    getPitchCep (utilities_analyze.R:337-407): frame / max zero-padded,
//                 a second transform through fft64, |C_k| / max, the peaks, the 1.8 rule
//   sg_anl_bana   getPitchSpec (:424-558): the five lowest spectral peaks, then
//                 sg::bana_candidates (sg_bana.h) in one thread
// analyze (sg_analyze*) runs all of that on rows that end in pitch, amplVoiced, voiced and
// harmonics, then the tail (R/analyze.R:576-707, R/utilities_pitch_postprocessing.R):
//   sg_anl_path   one 64-lane workgroup per sound (sg::path_sound, sg_path.h): the prior,
//                 findVoicedSegments, pathfinder per segment, medianSmoother, voiced /
//                 amplVoiced, the blanked quartiles, HNR in dB
//   sg_anl_path_exact  the same with pathfinding 'exact' (the minimum of costPerPath(), not in the
//                 reference) and the segment list of sg_pitch_path_costs compiled in: launched in
//                 sg_anl_path's place only for those two
//   sg_anl_harm   one workgroup per frame with a pitch: the share of |X| above 1.25 *
//                 pitch, in dB
// and, where the caller asks for analyze(summary = TRUE) (R/analyze.R:770-796), behind them
//   sg_anl_summary one 256-lane workgroup per sound (sg::sum_sound, sg_summary.h): duration,
//                 the proportion of voiced frames, and the mean, median and sd of the 14
//                 acoustic variables over their non-NA frames, from the finished table
// A parameter sweep (sg_analyze_sweep: what optimizePars() evaluates for analyzeFolder) runs the
// same kernels once per distinct set of the decisions each reads (sg_analyze.h, SweepPlan): the
// spectrogram and sg_anl_ampl per frame group; sg_anl_spec, sg_anl_cep, sg_anl_bana per candidate
// group into that group's candidate table; sg_anl_acf<T, true> once per store group, keeping the
// gated frames' corrected autocorrelations in HBM, and for the store's other candidate groups
//   sg_anl_acf_peaks  one workgroup per cond_entropy frame: the stored values to LDS, then the
//                 peak picker (SG_ACF_PEAKS, the tail of sg_anl_acf) under the group's own
//                 autocorThres, autocorSmooth and nCands
// and then, for all (row, sound) pairs of a chunk of rows in one launch each,
//   sg_anl_sweep_path  sg::path_sound_at from the shared candidate table into the pair's own
//   sg_anl_sweep_path_exact  the same for the pairs of the rows with pathfinding 'exact'
//   sg_anl_sweep_harm  sg_anl_harm on grid (frames, rows of the chunk)
// and sg_anl_summary once per row. A pair's cells are those of sg_analyze_summary_batch bit for bit.
// On the host the two sequences (analyze_device, analyze_sweep) share what they decide alike: the frames of a
// launch and both of their refusals (list_frames), the spectrogram behind them (list_spectra), and the five
// candidate stages of one table with their LDS sizes and the cepstrum's roots (candidate_stages), which
// analyze_device runs once and a sweep once per candidate group; each brings its own clock.
// Cumulative sums run in index order: a thread sums a contiguous run, one thread
// folds the 256 run sums in order, and the runs are rescanned from their offsets,
// so a frame's result does not depend on the launch it is in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sg_analyze.h"
#include "sg_bana.h"
#include "sg_dev64.h"
#include "sg_fft64_dev.h"
#include "sg_launch.h"
#include "sg_path.h"
#include "sg_rmath.h"
#include "sg_summary.h"

namespace {

using sg::DevBuf;
using sg::SpgStat;
using sg::upload;

constexpr int kT = 256;
static_assert(SG_F64_THREADS == kT, "fft64 strides by SG_F64_THREADS");

struct AnlSound {
  int64_t base, len;  // samples [base, base + len) of the input buffer
  int64_t z0;         // first cell of its |X| frames in scratch
  int64_t row0;       // first double of its table in the output buffer
  int32_t nf, pad;
};

struct AnlFrame {
  int64_t o;       // first sample of the frame within the sound
  int64_t a;       // first sample of its amplitude window
  int32_t snd, f;  // sound, frame within the sound
};

// the launch's constants
struct AnlK {
  int wl, B, cols, nCands;
  int fill;  // the columns sg_anl_spec blanks: cols, less the four that sg_anl_path writes for every frame
  int rowLow, rowHigh;  // 0-based, inclusive
  int cut0, ncut, pf_idx, domW, acW, lag0, nlag;
  int do_dom, do_autocor;
  double silence, entropyThres, domThres, autocorThres, sxx;
};

// the smallest int over the workgroup
__device__ __forceinline__ int block_min_int(int v, int* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  return red[0];
}

// dst[i] = src[0] + ... + src[i] for i < n, summed in index order (see the header)
__device__ __forceinline__ void block_cumsum(const double* src, int n, double* dst, double* red) {
  const int run = (n + kT - 1) / kT;
  const int i0 = min((int)threadIdx.x * run, n), i1 = min(i0 + run, n);
  double acc = 0;
  for (int i = i0; i < i1; ++i) acc += src[i];
  __syncthreads();
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int t = 0; t < kT; ++t) {
      const double v = red[t];
      red[t] = s;
      s += v;
    }
  }
  __syncthreads();
  acc = red[threadIdx.x];
  for (int i = i0; i < i1; ++i) {
    acc += src[i];
    dst[i] = acc;
  }
  __syncthreads();
}

// the first i < n with cum[i] > v (strict) or cum[i] >= v; n if none
__device__ __forceinline__ int first_crossing(const double* cum, int n, double v, bool strict, int* redi) {
  int best = n;
  for (int i = threadIdx.x; i < n; i += kT)
    if (strict ? cum[i] > v : cum[i] >= v) {
      best = i;
      break;
    }
  return block_min_int(best, redi);
}

// a centred window of 2 h + 1 values of a[] whose first maximum is its middle, v = a[c]: the values before it are
// smaller, those behind it not larger; NaN passes
__device__ __forceinline__ bool peak_at(const double* a, int c, int h, double v) {
  bool ok = true;
  for (int j = c - h; j < c && ok; ++j) ok = a[j] < v || a[j] != a[j];
  for (int j = c + 1; j <= c + h && ok; ++j) ok = a[j] <= v || a[j] != a[j];
  return ok;
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_anl_ampl(const T* __restrict__ x, const AnlFrame* __restrict__ frames,
                                                  const AnlSound* __restrict__ snds, const SpgStat* __restrict__ stat,
                                                  int wl, int cols, double* __restrict__ out,
                                                  unsigned long long* __restrict__ minampl) {
  __shared__ double red[kT];
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  const SpgStat st = stat[F.snd];
  const T* xc = x + S.base + F.a;  // host: F.a + wl < S.len
  double acc = 0;
  for (int i = threadIdx.x; i <= wl; i += kT) {
    const double v = sg::spg_normalise((double)xc[i], st);
    acc += v * v;
  }
  acc = block_reduce<kT>(acc, 0, red);
  if (threadIdx.x == 0) {
    const double a = sqrt(acc / (double)(wl + 1));
    out[S.row0 + (int64_t)F.f * cols + sg::kAmpl] = a;
    if (a == a) atomicMin(&minampl[F.snd], dkey(a));
  }
}

__global__ __launch_bounds__(kT) void sg_anl_spec(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                  const double* __restrict__ Z, const double* __restrict__ freq,
                                                  const double* __restrict__ xcut, const unsigned long long* __restrict__ minampl,
                                                  AnlK K, double* __restrict__ out) {
  __shared__ double fr[sg::kSpgMaxBins];
  __shared__ double cum[sg::kSpgMaxBins];
  __shared__ double red[kT];
  __shared__ int redi[kT];
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  const int B = K.B;
  const double* z = Z + S.z0 + (int64_t)F.f * B;
  double* row = out + S.row0 + (int64_t)F.f * K.cols;
  for (int b = threadIdx.x; b < B; b += kT) fr[b] = z[b];
  __syncthreads();
  // getEntropy(s[rowLow:rowHigh, f], 'weiner'): NA for sum == 0; x <= 0 -> 1e-10; exp(mean(log)) / mean
  double s0 = 0, s1 = 0, sl = 0;
  for (int b = K.rowLow + threadIdx.x; b <= K.rowHigh; b += kT) {
    const double v = fr[b];
    s0 += v;
    const double y = v <= 0 ? 1e-10 : v;
    s1 += y;
    sl += log(y);
  }
  s0 = block_reduce<kT>(s0, 0, red);
  s1 = block_reduce<kT>(s1, 0, red);
  sl = block_reduce<kT>(sl, 0, red);
  const double nb = (double)(K.rowHigh - K.rowLow + 1);
  const double entropy = s0 == 0 ? NAN : exp(sl / nb) / (s1 / nb);
  const double ampl = row[sg::kAmpl];
  const double sil = fmax(K.silence, dunkey(minampl[F.snd]));  // silence = max(silence, min(ampl))
  const bool c_sil = ampl > sil;
  const bool c_ent = c_sil && entropy < K.entropyThres;  // NA entropy: not tracked
  if (threadIdx.x == 0) {
    row[sg::kEntropy] = entropy;
    row[sg::kCondSilence] = c_sil ? 1.0 : 0.0;
    row[sg::kCondEntropy] = c_ent ? 1.0 : 0.0;
    for (int c = sg::kHNR; c <= sg::kDomCert; ++c) row[c] = NAN;
    for (int c = sg::kAnlFixed; c < K.fill; ++c) row[c] = NAN;
  }
  if (!c_sil) return;  // workgroup-uniform
  // which.max(frame): the first maximum
  double mx = -INFINITY;
  for (int b = threadIdx.x; b < B; b += kT) mx = fmax(mx, fr[b]);
  mx = block_reduce<kT>(mx, 2, red);
  int am = B;
  for (int b = threadIdx.x; b < B; b += kT)
    if (fr[b] == mx) {
      am = b;
      break;
    }
  am = block_min_int(am, redi);
  // meanFreq: the first index whose cumulative sum exceeds half the total
  block_cumsum(fr, B, cum, red);
  const double amplitude = cum[B - 1];
  const int imean = first_crossing(cum, B, amplitude / 2, true, redi);
  // the cut band
  block_cumsum(fr + K.cut0, K.ncut, cum, red);
  const double amp_cut = cum[K.ncut - 1];
  const int i25 = first_crossing(cum, K.ncut, 0.25 * amp_cut, false, redi);
  const int i50 = first_crossing(cum, K.ncut, 0.5 * amp_cut, false, redi);
  const int i75 = first_crossing(cum, K.ncut, 0.75 * amp_cut, false, redi);
  // lm(amp ~ freq): sum((x - mean x)(y - mean y)) / sum((x - mean x)^2)
  const double ybar = amp_cut / (double)K.ncut;
  double sxy = 0;
  for (int k = threadIdx.x; k < K.ncut; k += kT) sxy += xcut[k] * (fr[K.cut0 + k] - ybar);
  sxy = block_reduce<kT>(sxy, 0, red);
  if (threadIdx.x == 0) {
    row[sg::kPeakFreq] = am < B ? freq[am] : NAN;
    row[sg::kPeakFreqCut] = am < K.ncut ? freq[K.cut0 + am] : NAN;  // meanSpec_cut$freq[which.max(frame)]
    row[sg::kMeanFreq] = imean < B ? freq[imean] : NAN;
    row[sg::kQ25] = i25 < K.ncut ? freq[K.cut0 + i25] : NAN;
    row[sg::kQ50] = i50 < K.ncut ? freq[K.cut0 + i50] : NAN;
    row[sg::kQ75] = i75 < K.ncut ? freq[K.cut0 + i75] : NAN;
    row[sg::kSlope] = sxy / K.sxx;
  }
  if (!c_ent || !K.do_dom) return;
  // getDom on frame / max(frame): a centred window of domW bins whose first maximum
  // is its middle and exceeds domThres; the first such bin (1-based) above pitchFloor_idx
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += kT) cum[b] = fr[b] / mx;
  __syncthreads();
  const int h = K.domW / 2;
  int best = B;
  for (int c = h + threadIdx.x; c < B - h && best == B; c += kT) {
    if (c + 1 <= K.pf_idx) continue;
    const double v = cum[c];
    if (!(v > K.domThres)) continue;
    if (peak_at(cum, c, h, v)) best = c;
  }
  best = block_min_int(best, redi);
  if (threadIdx.x == 0 && best < B) {
    row[sg::kDom] = freq[best];
    row[sg::kDomCand] = freq[best];
    row[sg::kDomCert] = cum[best];
  }
}

// What getPitchAutocor (:250-324) makes of a frame's nl corrected autocorrelations and the dom
// certainty behind it (:151-159): HNR = max(a$amp); the peaks (a centred window of acW rows whose
// first maximum is its middle and exceeds autocorThres), the 0.975 rule, the 1.8 rule, the
// ordered candidates, the HNR >= 1 clamp. The tail of sg_anl_acf and the body of
// sg_anl_acf_peaks; it reads the names of the kernel it stands in: amp (nl doubles of LDS), pk
// (room for nl ints of LDS), npk (an int of LDS), red (kT doubles of LDS), nl, K, lagf, row. The
// peak list is unordered; every use is decided by (value, index), not by the list's order. Every
// value written is a copy of one of amp[] or lagf[] and every decision a comparison, so the
// result does not depend on who computed amp[].
// A macro and not a function: as a __device__ function (forced inline or not, the constants by
// reference, by value or as scalars: twenty variants) sg_anl_acf compiled to 46 VGPRs where
// the one-piece kernel has 44; as text it is the one-piece kernel. (peak_at, the window test
// alone, costs it nothing: the same registers, LDS and occupancy in all four kernels that call it.)
#define SG_ACF_PEAKS                                                                                      \
  if (threadIdx.x == 0) npk = 0;                                                                          \
  __syncthreads();                                                                                        \
  double hn = -INFINITY;                                                                                  \
  for (int i = threadIdx.x; i < nl; i += kT) hn = fmax(hn, amp[i]);                                       \
  hn = block_reduce<kT>(hn, 2, red);                                                                      \
  const int h = K.acW / 2;                                                                                \
  for (int c = h + threadIdx.x; c < nl - h; c += kT) {                                                    \
    const double v = amp[c];                                                                              \
    if (!(v > K.autocorThres)) continue;                                                                  \
    if (peak_at(amp, c, h, v)) pk[atomicAdd(&npk, 1)] = c; /* at most nl - 2 h entries */                 \
  }                                                                                                       \
  __syncthreads();                                                                                        \
  if (threadIdx.x != 0) return;                                                                           \
  const int P = npk;                                                                                      \
  double HNR = hn > -INFINITY ? hn : NAN;                                                                 \
  if (P > 0) {                                                                                            \
    double pmax = -INFINITY;                                                                              \
    for (int q = 0; q < P; ++q) pmax = fmax(pmax, amp[pk[q]]);                                            \
    int ibest = nl; /* which(amp > 0.975 * max(amp))[1] */                                                \
    for (int q = 0; q < P; ++q)                                                                           \
      if (amp[pk[q]] > 0.975 * pmax && pk[q] < ibest) ibest = pk[q];                                      \
    const double cutf = lagf[ibest] / 1.8; /* peaks with freq > bestFreq / 1.8 */                         \
    /* order(amp, decreasing = TRUE): the larger first, the earlier row on ties */                        \
    double lastv = INFINITY;                                                                              \
    int lasti = -1;                                                                                       \
    for (int n = 0; n < K.nCands; ++n) {                                                                  \
      int bi = -1;                                                                                        \
      double bv = -INFINITY;                                                                              \
      for (int q = 0; q < P; ++q) {                                                                       \
        const int i = pk[q];                                                                              \
        const double v = amp[i];                                                                          \
        if (!(lagf[i] > cutf)) continue;                                                                  \
        if (!(v < lastv || (v == lastv && i > lasti))) continue; /* already taken */                      \
        if (bi < 0 || v > bv || (v == bv && i < bi)) {                                                    \
          bi = i;                                                                                         \
          bv = v;                                                                                         \
        }                                                                                                 \
      }                                                                                                   \
      if (bi < 0) break;                                                                                  \
      row[sg::kAnlFixed + n] = lagf[bi];                                                                  \
      row[sg::kAnlFixed + K.nCands + n] = bv;                                                             \
      lastv = bv;                                                                                         \
      lasti = bi;                                                                                         \
    }                                                                                                     \
  }                                                                                                       \
  if (HNR >= 1.0) HNR = 0.9999;                                                                           \
  row[sg::kHNR] = HNR;                                                                                    \
  if (row[sg::kDom] == row[sg::kDom] && HNR == HNR) row[sg::kDomCert] = 1.0 / (1.0 + exp(3.0 * HNR - 1.0));

// LDS: wl + 4 doubles (the demeaned windowed frame and 4 zeros, later the peak list), nlag
// doubles (the corrected autocorrelation). kStore (a sweep's first candidate group of a store
// group): the frame's nlag corrected values also go to store + blockIdx.x * nlag, for
// sg_anl_acf_peaks
template <typename T, bool kStore>
__global__ __launch_bounds__(kT) void sg_anl_acf(const T* __restrict__ x, const AnlFrame* __restrict__ frames,
                                                 const AnlSound* __restrict__ snds, const SpgStat* __restrict__ stat,
                                                 const double* __restrict__ win, const double* __restrict__ filt,
                                                 const double* __restrict__ lagf, AnlK K, double* __restrict__ out,
                                                 double* __restrict__ store) {
  extern __shared__ double lds_acf[];
  __shared__ double red[kT];
  __shared__ int npk;
  double* xw = lds_acf;
  double* amp = lds_acf + K.wl + 4;
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  double* row = out + S.row0 + (int64_t)F.f * K.cols;
  if (row[sg::kCondEntropy] != 1.0) return;  // workgroup-uniform; written by sg_anl_spec
  const SpgStat st = stat[F.snd];
  const T* xc = x + S.base + F.o;  // host: F.o + wl <= S.len
  const int wl = K.wl, nl = K.nlag;
  double acc = 0;
  if (threadIdx.x < 4) xw[wl + threadIdx.x] = 0.0;  // the zeros the lag groups run into
  for (int i = threadIdx.x; i < wl; i += kT) {
    const double v = sg::spg_normalise((double)xc[i], st) * win[i];
    xw[i] = v;
    acc += v;
  }
  const double mean = block_reduce<kT>(acc, 0, red) / (double)wl;
  acc = 0;
  for (int i = threadIdx.x; i < wl; i += kT) {
    const double v = xw[i] - mean;  // acf() demeans
    xw[i] = v;
    acc += v * v;
  }
  const double c0 = block_reduce<kT>(acc, 0, red) / (double)wl;  // lag 0; the barrier inside publishes xw
  const double se = sqrt(c0);
  // Four consecutive lags per thread: xw[t] is a broadcast, and the window w0..w3 =
  // xw[t + k .. t + k + 3] slides by one new value per step, so 4 multiply-adds cost 2
  // LDS reads. Every lag's sum still runs over t in order; the shorter lags of a group
  // run into the 4 zeros behind the frame, which add nothing.
  for (int g = threadIdx.x; 4 * g < nl; g += kT) {
    const int k = K.lag0 + 4 * g;
    const int n = wl - k;  // >= 1; the terms of the group's first lag
    const double* y = xw + k;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    double w0 = y[0], w1 = y[1], w2 = y[2], w3 = y[3];
    int t = 0;
    for (; t + 4 <= n; t += 4) {  // reads up to y[n + 3] = xw[wl + 3]
      double a = xw[t];
      s0 += a * w0; s1 += a * w1; s2 += a * w2; s3 += a * w3;
      w0 = y[t + 4];
      a = xw[t + 1];
      s0 += a * w1; s1 += a * w2; s2 += a * w3; s3 += a * w0;
      w1 = y[t + 5];
      a = xw[t + 2];
      s0 += a * w2; s1 += a * w3; s2 += a * w0; s3 += a * w1;
      w2 = y[t + 6];
      a = xw[t + 3];
      s0 += a * w3; s1 += a * w0; s2 += a * w1; s3 += a * w2;
      w3 = y[t + 7];
    }
    for (; t < n; ++t) {  // reads up to y[n + 2]
      const double a = xw[t];
      s0 += a * y[t]; s1 += a * y[t + 1]; s2 += a * y[t + 2]; s3 += a * y[t + 3];
    }
    const double s[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * g + r;
      if (i < nl) {
        double a = (s[r] / (double)wl) / (se * se);
        a = a > 1.0 ? 1.0 : (a < -1.0 ? -1.0 : a);  // as acf()'s C code clamps
        amp[i] = a / filt[i];
        if (kStore) store[(int64_t)blockIdx.x * nl + i] = amp[i];
      }
    }
  }
  int* pk = reinterpret_cast<int*>(xw);  // xw is dead behind the first barrier below: at most nl - 2 h <= wl entries
  SG_ACF_PEAKS
}

// A sweep's later candidate groups of a store group: the frame's corrected autocorrelations
// from the store sg_anl_acf<T, true> filled, then SG_ACF_PEAKS under this group's autocorThres,
// autocorSmooth and nCands. The gate is the store group's, so the frame was stored.
// LDS: nlag doubles, then nlag ints (the peak list)
__global__ __launch_bounds__(kT) void sg_anl_acf_peaks(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                       const double* __restrict__ store, const double* __restrict__ lagf,
                                                       AnlK K, double* __restrict__ out) {
  extern __shared__ double lds_pk[];
  __shared__ double red[kT];
  __shared__ int npk;
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  double* row = out + S.row0 + (int64_t)F.f * K.cols;
  if (row[sg::kCondEntropy] != 1.0) return;  // workgroup-uniform; written by sg_anl_spec
  const int nl = K.nlag;
  const double* src = store + (int64_t)blockIdx.x * nl;
  double* amp = lds_pk;
  int* pk = reinterpret_cast<int*>(lds_pk + nl);
  for (int i = threadIdx.x; i < nl; i += kT) amp[i] = src[i];
  SG_ACF_PEAKS  // its first barrier publishes amp[]
}
#undef SG_ACF_PEAKS

// the constants of the two trackers pitch_candidates adds
struct PitchK {
  int B, cols, nCands;
  int L, M, odd, pad;  // the cepstrum's transform: L points, as M = L / 2 packed pairs (L even) or M = L complex points
  int l, c0, nc, cepW, specW;
  double cepThres, specPeak;
  sg::BanaPars bana;  // carries pitchFloor
};

// getPitchCep (R/utilities_analyze.R:337-407) for one cond_entropy frame: abs(fft(c(zp,
// frame / max(frame), zp))) / its maximum, the rows with pitchFloor < label < pitchCeiling,
// the peaks, the 1.8 rule, the order, the discount. Row i (1-based) of the reference's
// table holds DFT bin i - 1 and is labelled samplingRate / i / 2 * (L / B); cepf holds
// the labels of the band's rows, which are bins [c0, c0 + nc).
// LDS: fft64_lds_bytes(M), then l + 1 doubles (|C_k|, k <= L / 2: by conjugate symmetry
// they hold the maximum over all L bins)
__global__ __launch_bounds__(kT) void sg_anl_cep(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                 const double* __restrict__ Z, const double2* __restrict__ TN,
                                                 const double* __restrict__ cepf, PitchK K, double* __restrict__ out) {
  extern __shared__ double2 lds_cep[];
  __shared__ double red[kT];
  __shared__ int npk;
  const int M = K.M, B = K.B, nl = K.nc;
  const Fft64Lds L = fft64_carve(lds_cep, M);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  double* cep = static_cast<double*>(L.end);
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  double* row = out + S.row0 + (int64_t)F.f * K.cols;
  if (row[sg::kCondEntropy] != 1.0) return;  // workgroup-uniform; written by sg_anl_spec
  const double* z = Z + S.z0 + (int64_t)F.f * B;
  double mx = -INFINITY;
  for (int i = threadIdx.x; i < B; i += kT) mx = fmax(mx, z[i]);
  mx = block_reduce<kT>(mx, 2, red);
  if (K.odd) {
    for (int n = threadIdx.x; n < M; n += kT) {
      const int j = n - K.pad;
      a[n] = make_double2(j >= 0 && j < B ? z[j] / mx : 0.0, 0.0);
    }
  } else {
    load_packed64(a, M, K.pad, B, [z, mx](int j) { return z[j] / mx; });
  }
  if (threadIdx.x == 0) npk = 0;
  __syncthreads();
  fft64(a, b, M, TN, rt, false);
  if (K.odd) {
    for (int k = threadIdx.x; k <= K.l; k += kT) cep[k] = hypot(a[k].x, a[k].y);
  } else {
    // |X_k| of the packed frame; X_M = Re Z_0 - Im Z_0, its own branch: without the rounding of W_L^M
    for (int k = threadIdx.x; k <= M; k += kT) {
      if (k == M) {
        cep[k] = fabs(a[0].x - a[0].y);
        continue;
      }
      const double2 X = untangle64(a, k, M, TN);
      cep[k] = hypot(X.x, X.y);
    }
  }
  __syncthreads();
  double cm = -INFINITY;
  for (int k = threadIdx.x; k <= K.l; k += kT) cm = fmax(cm, cep[k]);
  cm = block_reduce<kT>(cm, 2, red);
  double* amp = cep + K.c0;  // host: c0 + nc <= l
  for (int i = threadIdx.x; i < nl; i += kT) amp[i] = amp[i] / cm;
  __syncthreads();
  // the peaks, as in sg_anl_acf: an unordered list, every use decided by (value, index)
  int* pk = reinterpret_cast<int*>(lds_cep);  // a and b are dead
  const int h = K.cepW / 2;
  for (int c = h + threadIdx.x; c < nl - h; c += kT) {
    const double v = amp[c];
    if (!(v > K.cepThres)) continue;
    if (peak_at(amp, c, h, v)) pk[atomicAdd(&npk, 1)] = c;  // at most nc <= l <= 2 M entries of 4 bytes in 32 M bytes
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int P = npk;
  if (P == 0) return;
  // absCepPeak = idx[which.max(cep[idx])]: the first maximum in index order
  double pmax = -INFINITY;
  int ibest = nl;
  for (int q = 0; q < P; ++q) {
    const int i = pk[q];
    const double v = amp[i];
    if (v > pmax || (v == pmax && i < ibest)) {
      pmax = v;
      ibest = i;
    }
  }
  const double cutf = cepf[ibest] / 1.8;
  double lastv = INFINITY;
  int lasti = -1;
  const int c1 = sg::kAnlFixed + 2 * K.nCands;
  for (int n = 0; n < K.nCands; ++n) {  // order(cep, decreasing = TRUE): the earlier row on ties
    int bi = -1;
    double bv = -INFINITY;
    for (int q = 0; q < P; ++q) {
      const int i = pk[q];
      const double v = amp[i];
      if (!(cepf[i] > cutf)) continue;
      if (!(v < lastv || (v == lastv && i > lasti))) continue;  // already taken
      if (bi < 0 || v > bv || (v == bv && i < bi)) {
        bi = i;
        bv = v;
      }
    }
    if (bi < 0) break;
    const double cand = cepf[bi];
    // :400-401 the discount, after the ordering; HzToSemitones(h) = log2(h / 16.3516) * 12
    const double st = log2((cand / K.bana.pitchFloor) / 16.3516) * 12;
    const double den = __dadd_rn(1.0, 5 / __dadd_rn(1.0, exp(__dsub_rn(2.0, __dmul_rn(.25, st)))));
    row[c1 + n] = cand;
    row[c1 + K.nCands + n] = bv / den;
    lastv = bv;
    lasti = bi;
  }
}

// getPitchSpec (R/utilities_analyze.R:424-558) for one cond_entropy frame: the peaks
// of frame / max(frame) in centred windows of specW bins above specPeak (HNR = NULL,
// :134), the five lowest of them found in index order, then sg::bana_candidates
__global__ __launch_bounds__(kT) void sg_anl_bana(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                  const double* __restrict__ Z, const double* __restrict__ freq,
                                                  PitchK K, double* __restrict__ out) {
  __shared__ double fr[sg::kSpgMaxBins];
  __shared__ double red[kT];
  __shared__ int redi[kT];
  const int B = K.B;
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  double* row = out + S.row0 + (int64_t)F.f * K.cols;
  if (row[sg::kCondEntropy] != 1.0) return;  // workgroup-uniform
  const double* z = Z + S.z0 + (int64_t)F.f * B;
  double mx = -INFINITY;
  for (int i = threadIdx.x; i < B; i += kT) mx = fmax(mx, z[i]);
  mx = block_reduce<kT>(mx, 2, red);
  for (int i = threadIdx.x; i < B; i += kT) fr[i] = z[i] / mx;
  __syncthreads();
  const int h = K.specW / 2;
  int pidx[sg::kBanaPeaks];
  int np = 0, last = -1;
  for (int r = 0; r < sg::kBanaPeaks; ++r) {  // the lowest peak above the last one found
    int best = B;
    for (int c = h + threadIdx.x; c < B - h && best == B; c += kT) {
      if (c <= last) continue;
      const double v = fr[c];
      if (!(v > K.specPeak)) continue;
      if (peak_at(fr, c, h, v)) best = c;
    }
    best = block_min_int(best, redi);  // every thread gets it: the loop is workgroup-uniform
    if (best == B) break;
    pidx[np++] = best;
    last = best;
  }
  if (threadIdx.x != 0 || np == 0) return;
  double pf[sg::kBanaPeaks], cand[sg::kAnlMaxCands], cert[sg::kAnlMaxCands];
  for (int i = 0; i < sg::kBanaPeaks; ++i) pf[i] = i < np ? freq[pidx[i]] : 0.0;
  const int m = sg::bana_candidates(pf, np, K.bana, cand, cert);
  const int c1 = sg::kAnlFixed + 4 * K.nCands;
  for (int n = 0; n < m; ++n) {
    row[c1 + n] = cand[n];
    row[c1 + K.nCands + n] = cert[n];
  }
}

static_assert(sg::kPathAmpl == sg::kAmpl && sg::kPathHNR == sg::kHNR && sg::kPathDom == sg::kDom && sg::kPathQ25 == sg::kQ25 &&
                  sg::kPathQ75 == sg::kQ75 && sg::kPathDomCand == sg::kDomCand && sg::kPathDomCert == sg::kDomCert &&
                  sg::kPathFixed == sg::kAnlFixed,
              "sg_path.h names the columns of sg::AnlCol");

constexpr int kPathT = 64;  // one wave per sound
constexpr int kPathMaxW = 2 + 3 * sg::kAnlMaxCands;  // sg::path_width() at its largest

struct PathSound {
  int64_t row0;  // first double of its table in the output buffer
  int64_t scr0;  // first double of its frames' scratch
  int32_t nf, hw;
  int64_t seg0;  // first double of its segment list (sg::path_seg_cells), where the launch has one
};

struct WgSync {
  __device__ void operator()() const { __syncthreads(); }
};

// analyze()'s tail for one sound per workgroup (sg::path_sound, sg_path.h): lanes stride
// over frames; one lane scans for voiced segments and interpolates; the per-frame sort,
// the choices, the snake's iterations and the smoother are lane-parallel. The candidates
// live in global scratch (a sound has no frame bound), sized by the launch's frame total.
__global__ __launch_bounds__(kPathT) void sg_anl_path(const PathSound* __restrict__ snds, sg::PathPars P,
                                                      double* __restrict__ out, double* __restrict__ scr) {
  __shared__ double red[kPathT];
  __shared__ int64_t sh[3];
  const PathSound S = snds[blockIdx.x];
  if (S.nf <= 0) return;  // workgroup-uniform
  sg::path_sound(P, S.nf, S.hw, out + S.row0, scr + S.scr0, (int)threadIdx.x, kPathT, red, sh, WgSync());
}

// sg_anl_path with pathfinding 'exact' and the segment list compiled in (sg::kPathExact | sg::kPathSegs), a kernel of
// its own so that sg_anl_path stays what it was: launched for 'exact' (the scratch is then sg::path_scratch()
// doubles per frame: the back-pointers; D of two frames in dd) and for sg_pitch_path_costs (segs: the sounds'
// segment lists, else nullptr)
__global__ __launch_bounds__(kPathT) void sg_anl_path_exact(const PathSound* __restrict__ snds, sg::PathPars P,
                                                            double* __restrict__ out, double* __restrict__ scr,
                                                            double* __restrict__ segs) {
  __shared__ double red[kPathT];
  __shared__ double dd[2 * kPathMaxW];
  __shared__ int64_t sh[3];
  const PathSound S = snds[blockIdx.x];
  if (S.nf <= 0) {  // workgroup-uniform
    if (segs && threadIdx.x == 0) segs[S.seg0] = 0;
    return;
  }
  sg::path_sound<WgSync, sg::kPathExact | sg::kPathSegs>(P, S.nf, S.hw, out + S.row0, scr + S.scr0, (int)threadIdx.x, kPathT,
                                                         red, sh, WgSync(), dd, segs ? segs + S.seg0 : nullptr);
}

// the one of the two a launch needs
void launch_path(dim3 grid, hipStream_t s, const PathSound* d_ps, const sg::PathPars& P, double* d_out, double* d_scr,
                 double* d_segs) {
  if (P.pathfinding == 3 || d_segs)
    hipLaunchKernelGGL(sg_anl_path_exact, grid, dim3(kPathT), 0, s, d_ps, P, d_out, d_scr, d_segs);
  else
    hipLaunchKernelGGL(sg_anl_path, grid, dim3(kPathT), 0, s, d_ps, P, d_out, d_scr);
}

// `harmonics` (R/analyze.R:694-703) for the frame of a workgroup, its row of `cols` doubles at row and its |X| at z:
// the share of |X| above 1.25 * pitch (labels in kHz, strictly above), in dB; the path kernel has left NaN where
// pitch is NaN
__device__ __forceinline__ void harm_frame(double* row, int cols, const double* z, const double* lab, int B, double* red) {
  const double pitch = row[cols - sg::kPathCols + sg::kPathPitch];
  if (pitch != pitch) return;  // workgroup-uniform
  const double threshold = 1.25 * pitch / 1000;
  double above = 0, all = 0;
  for (int b = threadIdx.x; b < B; b += kT) {
    const double v = z[b];
    all += v;
    if (lab[b] > threshold) above += v;
  }
  above = block_reduce<kT>(above, 0, red);
  all = block_reduce<kT>(all, 0, red);
  if (threadIdx.x == 0) row[cols - sg::kPathCols + sg::kPathHarmonics] = sg::path_to_dB(above / all);
}

__global__ __launch_bounds__(kT) void sg_anl_harm(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                  const double* __restrict__ Z, const double* __restrict__ lab, int B,
                                                  int cols, double* __restrict__ out) {
  __shared__ double red[kT];
  const AnlFrame F = frames[blockIdx.x];
  const AnlSound S = snds[F.snd];
  harm_frame(out + S.row0 + (int64_t)F.f * cols, cols, Z + S.z0 + (int64_t)F.f * B, lab, B, red);
}

constexpr int kSumT = 256;
static_assert(kSumT == sg::kSumSlots * sg::kSumMaxGroups, "sg::SumShared holds one cell per lane");

// analyze(summary = TRUE) for one sound per workgroup (sg::sum_sound, sg_summary.h). A sound
// without frames (not longer than the window, or a failed call) gets NaN.
__global__ __launch_bounds__(kSumT) void sg_anl_summary(const sg::SumSound* __restrict__ snds, int cols, double samplingRate,
                                                        const double* __restrict__ tables, double* __restrict__ out) {
  __shared__ sg::SumShared sh;
  const sg::SumSound S = snds[blockIdx.x];
  sg::sum_sound(tables + S.row0, S.nf, cols, S.len, samplingRate, out + (int64_t)blockIdx.x * sg::kSumCols, (int)threadIdx.x,
                kSumT, sh, WgSync());
}

// A sweep (sg_analyze_sweep). A pair is (row of the chunk, sound): workgroup b of a tail kernel
// is pair b = row_in_chunk * n_calls + sound. Its candidates are the sound's table of the row's
// candidate group, which the tail leaves untouched; its own table and scratch lie in the chunk's
// workspace.
struct SweepPair {
  int64_t src0;  // first double of the sound's candidate table
  int64_t dst0;  // first double of the pair's table in the workspace
  int64_t scr0;  // first double of its frames' scratch there
  int32_t nf, hw, cols, row;  // frames, half the smoothing window, doubles of a row of its table, the row's PathPars
};

// sg_anl_path for a pair: sg::path_sound_at from the shared candidates into the pair's table
__global__ __launch_bounds__(kPathT) void sg_anl_sweep_path(const SweepPair* __restrict__ pairs,
                                                            const sg::PathPars* __restrict__ pars,
                                                            const double* __restrict__ cands, double* __restrict__ work) {
  __shared__ double red[kPathT];
  __shared__ int64_t sh[3];
  const SweepPair R = pairs[blockIdx.x];
  if (R.nf <= 0) return;  // workgroup-uniform
  const sg::PathPars P = pars[R.row];
  sg::path_sound_at(P, R.nf, R.hw, cands + R.src0, P.cols - sg::kPathCols, work + R.dst0, work + R.scr0, (int)threadIdx.x,
                    kPathT, red, sh, WgSync());
}

// sg_anl_path_exact for a pair: the pairs of a chunk whose row has pathfinding 'exact'. Both kernels go over all
// the pairs of a chunk (sg_anl_sweep_harm and the summary index them by row and sound); each is launched only for a
// chunk that has a pair for it, and in a chunk that has both each gets a copy of the pairs in which the other's have
// no frames.
__global__ __launch_bounds__(kPathT) void sg_anl_sweep_path_exact(const SweepPair* __restrict__ pairs,
                                                                  const sg::PathPars* __restrict__ pars,
                                                                  const double* __restrict__ cands, double* __restrict__ work) {
  __shared__ double red[kPathT];
  __shared__ double dd[2 * kPathMaxW];
  __shared__ int64_t sh[3];
  const SweepPair R = pairs[blockIdx.x];
  if (R.nf <= 0) return;  // workgroup-uniform
  const sg::PathPars P = pars[R.row];
  sg::path_sound_at<WgSync, sg::kPathExact>(P, R.nf, R.hw, cands + R.src0, P.cols - sg::kPathCols, work + R.dst0, work + R.scr0,
                                            (int)threadIdx.x, kPathT, red, sh, WgSync(), dd);
}

// sg_anl_harm for frame blockIdx.x of the frame group under row blockIdx.y of the chunk; snds: any candidate
// group's of the frame group (for z0)
__global__ __launch_bounds__(kT) void sg_anl_sweep_harm(const AnlFrame* __restrict__ frames, const AnlSound* __restrict__ snds,
                                                        const SweepPair* __restrict__ pairs, int n_calls,
                                                        const double* __restrict__ Z, const double* __restrict__ lab, int B,
                                                        double* __restrict__ work) {
  __shared__ double red[kT];
  const AnlFrame F = frames[blockIdx.x];
  const SweepPair R = pairs[(int64_t)blockIdx.y * n_calls + F.snd];
  harm_frame(work + R.dst0 + (int64_t)F.f * R.cols, R.cols, Z + snds[F.snd].z0 + (int64_t)F.f * B, lab, B, red);
}

// the launch's constants from the setup: `cols` doubles a row, of which sg_anl_spec blanks the first `fill`
AnlK launch_consts(const sg::AnlSetup& A, int cols, int fill) {
  AnlK K;
  K.wl = A.spg.wl;
  K.B = A.spg.bins;
  K.cols = cols;
  K.fill = fill;
  K.nCands = A.nCands;
  K.rowLow = A.rowLow - 1;
  K.rowHigh = A.rowHigh - 1;
  K.cut0 = A.cut0;
  K.ncut = A.ncut;
  K.pf_idx = A.pf_idx;
  K.domW = A.domW;
  K.acW = A.acW;
  K.lag0 = A.lag0;
  K.nlag = A.nlag;
  K.do_dom = A.do_dom;
  K.do_autocor = A.do_autocor;
  K.silence = A.silence;
  K.entropyThres = A.entropyThres;
  K.domThres = A.domThres;
  K.autocorThres = A.autocorThres;
  K.sxx = A.sxx;
  return K;
}

PitchK launch_consts(const sg::PitchSetup& Q, int cols) {
  PitchK X;
  X.B = Q.spg.bins;
  X.cols = cols;
  X.nCands = Q.nCands;
  X.L = Q.cepL;
  X.odd = Q.cepL % 2;
  X.M = X.odd ? Q.cepL : Q.cepL / 2;
  X.pad = Q.cepPad;
  X.l = Q.cepl;
  X.c0 = Q.cep0;
  X.nc = Q.ncep;
  X.cepW = Q.cepW;
  X.specW = Q.specW;
  X.cepThres = Q.cepThres;
  X.specPeak = Q.specPeak;
  X.bana = sg::BanaPars{Q.pitchFloor, Q.pitchCeiling, Q.specSinglePeakCert, Q.specThres, Q.specMerge, Q.nCands};
  return X;
}

// the checks of a setup against its frame, before anything is launched
void check_setup(const sg::AnlSetup& A, const sg::PitchSetup* pitch) {
  const int B = A.spg.bins, wl = A.spg.wl;
  if (A.rowLow < 1 || A.rowHigh > B || A.rowLow > A.rowHigh || A.cut0 < 0 || A.cut0 + A.ncut > B || A.lag0 < 0 ||
      A.lag0 + A.nlag > wl || B > sg::kSpgMaxBins || A.nCands > sg::kAnlMaxCands)
    throw sg::SgError(SG_E_DEVICE, "analyze: the setup leaves the frame");
  if (pitch && pitch->do_cep) {
    const sg::PitchSetup& Q = *pitch;
    const int M = Q.cepL % 2 ? Q.cepL : Q.cepL / 2;
    if (Q.cepL != B + 2 * Q.cepPad || Q.cepPad < 0 || M < 1 || M > sg::kSpgMaxBins || Q.cepl != Q.cepL / 2 || Q.cep0 < 0 ||
        Q.ncep < 1 || Q.cep0 + Q.ncep > Q.cepl || (int)Q.cepf.size() != Q.ncep || Q.cepW < 1)
      throw sg::SgError(SG_E_DEVICE, "analyze: the cepstrum's setup leaves the frame");
  }
}

// a row of the tail: the candidates' columns and sg_path.h's four, as the path's constants have it; `also`: what else
// the caller requires
void check_tail_row(const sg::PathPars& P, int cols, int nCands, bool also) {
  if (P.cols != cols || cols != sg::kAnlFixed + 6 * nCands + sg::kPathCols || sg::path_width(nCands) > kPathMaxW || !also)
    throw sg::SgError(SG_E_DEVICE, "analyze: the tail's setup leaves the row");
}

// The frames of the sounds of one launch sequence, sound after sound, and where each sound's lie
struct FrameList {
  std::vector<AnlFrame> fr;
  std::vector<int64_t> lens;  // a sound's samples; 0 without frames: a sound of exactly wl samples has a spectrogram frame but no analysis
  std::vector<int64_t> zoff;  // the first cell of its |X| frames
  std::vector<int64_t> foff;  // its first frame in fr
  std::vector<int32_t> nfs;
  int64_t cells = 0;  // of all |X| frames
};

// per_sound(c, frames, first frame) runs before sound c's frames are listed: analyze_device refuses a smoothing
// window there, so that of two refusals the one of the earlier sound is reported
template <class PerSound>
FrameList list_frames(const sg::AnlSetup& A, const int64_t* lengths, int64_t n_calls, PerSound&& per_sound) {
  const sg::SpgSetup& P = A.spg;
  FrameList L;
  L.lens.resize(n_calls), L.zoff.resize(n_calls), L.foff.resize(n_calls), L.nfs.resize(n_calls);
  for (int64_t c = 0; c < n_calls; ++c) {
    const int nf = sg::anl_frames(A, lengths[c]);
    L.lens[c] = nf ? lengths[c] : 0;
    L.zoff[c] = L.cells;
    L.foff[c] = (int64_t)L.fr.size();
    L.nfs[c] = nf;
    per_sound(c, nf, L.foff[c]);
    if (L.foff[c] + nf > 2147483647LL) throw sg::SgError(SG_E_UNSUPPORTED, "analyze: the frames of one launch exceed 2^31");
    for (int f = 0; f < nf; ++f) {
      const int64_t o = sg::spg_frame_start(P, lengths[c], f), a = sg::anl_ampl_start(A, lengths[c], nf, f);
      if (o < 0 || o + P.wl > lengths[c] || a < 0 || a + P.wl + 1 > lengths[c])
        throw sg::SgError(SG_E_DEVICE, "analyze: a frame leaves its sound");
      L.fr.push_back(AnlFrame{o, a, (int32_t)c, f});
    }
    L.cells += (int64_t)nf * P.bins;
  }
  return L;
}

// the listed sounds' |X| frames to d_Z (at L.zoff) and their statistics to d_stat
template <typename T>
void list_spectra(const sg::SpgSetup& P, const T* d_x, const int64_t* offsets, const FrameList& L, double* d_Z,
                  SpgStat* d_stat, hipStream_t s) {
  const int64_t n_calls = (int64_t)L.nfs.size();
  std::vector<int32_t> b_o(n_calls), f_o(n_calls);
  sg::spectrogram_device<T>(P, d_x, offsets, L.lens.data(), n_calls, d_Z, L.zoff.data(), b_o.data(), f_o.data(), s, nullptr,
                            d_stat);
  for (int64_t c = 0; c < n_calls; ++c)
    if (f_o[c] != L.nfs[c]) throw sg::SgError(SG_E_DEVICE, "analyze: the spectrogram's frame count differs");
}

// What the candidate tables of a frame group share: device memory, but for F
template <typename T>
struct FrameGroup {
  const T* x;
  const AnlFrame* fr;
  int64_t F;
  const SpgStat* stat;
  const double* Z;
  const double* freq;
  const double* win;  // nullptr: uploaded by the first table that computes autocorrelations
  unsigned long long* minampl;
};

enum CandStage { kCsAmpl = 0, kCsSpec, kCsAcf, kCsPeaks, kCsCep, kCsBana };
// sg_anl_acf alone; sg_anl_acf that also fills d_store; sg_anl_acf_peaks from d_store
enum AcfRun { kAcfPlain, kAcfStore, kAcfFromStore };

// The candidate stages for one table of a frame group: rows of `cols` doubles, of which sg_anl_spec blanks the first
// `fill`, sound c's at d_out + snds[c].row0. pitch: nullptr without the cepstral and the spectral tracker.
// mark(stage, false) at every stage's boundary in stage order, launched or not (kCsAcf for either autocorrelation
// kernel; kCsCep and kCsBana only with pitch), then mark(stage, true) right before the stage's launch, behind the host
// work that prepares it: the caller's clock stamps at the one or at the other.
template <typename T, class Mark>
void candidate_stages(DevBuf& db, hipStream_t s, FrameGroup<T>& G, const sg::AnlSetup& A, const sg::PitchSetup* pitch, int cols,
                      int fill, const AnlSound* d_snd, double* d_out, AcfRun acf, double* d_store, Mark&& mark) {
  const int wl = A.spg.wl;
  const dim3 gF((unsigned)G.F), bT(kT);
  const AnlK K = launch_consts(A, cols, fill);
  const double* d_xc = upload(db, A.xc, s);
  auto launch = [&](int stage, auto&& go) {
    mark(stage, true);
    go();
    HIPCHK(hipGetLastError());
  };
  mark(kCsAmpl, false);
  launch(kCsAmpl, [&]() { hipLaunchKernelGGL(sg_anl_ampl<T>, gF, bT, 0, s, G.x, G.fr, d_snd, G.stat, wl, cols, d_out, G.minampl); });
  mark(kCsSpec, false);
  launch(kCsSpec, [&]() { hipLaunchKernelGGL(sg_anl_spec, gF, bT, 0, s, G.fr, d_snd, G.Z, G.freq, d_xc, G.minampl, K, d_out); });
  mark(kCsAcf, false);
  if (A.do_autocor) {
    const double* d_lagf = upload(db, A.lagf, s);
    if (acf == kAcfFromStore) {
      const int lds = A.nlag * (int)(sizeof(double) + sizeof(int));
      launch(kCsPeaks, [&]() {
        sg::lds_opt_in(&sg_anl_acf_peaks, lds, "sg_anl_acf_peaks");
        hipLaunchKernelGGL(sg_anl_acf_peaks, gF, bT, (size_t)lds, s, G.fr, d_snd, d_store, d_lagf, K, d_out);
      });
    } else {
      if (!G.win) G.win = upload(db, sg::spg_window(wl, A.spg.wn), s);
      const double* d_filt = upload(db, sg::anl_filter(A), s);
      const int lds = (wl + 4 + A.nlag) * (int)sizeof(double);
      const auto kernel = acf == kAcfStore ? &sg_anl_acf<T, true> : &sg_anl_acf<T, false>;
      launch(kCsAcf, [&]() {
        sg::lds_opt_in(kernel, lds, "sg_anl_acf");
        hipLaunchKernelGGL(kernel, gF, bT, (size_t)lds, s, G.x, G.fr, d_snd, G.stat, G.win, d_filt, d_lagf, K, d_out,
                           acf == kAcfStore ? d_store : nullptr);
      });
    }
  }
  mark(kCsCep, false);
  if (!pitch) return;
  const sg::PitchSetup& Q = *pitch;
  const PitchK X = launch_consts(Q, cols);
  if (Q.do_cep) {
    const int N = X.odd ? 2 * X.M : X.L;  // fft64 reads W_N^t, t < 2 M
    double2* d_TN = db.get<double2>((size_t)N);
    const double* d_cepf = upload(db, Q.cepf, s);
    sg::fill_roots64(d_TN, N, s);
    const int lds = fft64_lds_bytes(X.M) + (X.l + 1) * (int)sizeof(double);
    sg::lds_opt_in(&sg_anl_cep, lds, "sg_anl_cep");
    launch(kCsCep, [&]() { hipLaunchKernelGGL(sg_anl_cep, gF, bT, (size_t)lds, s, G.fr, d_snd, G.Z, d_TN, d_cepf, X, d_out); });
  }
  mark(kCsBana, false);
  if (Q.do_spec) launch(kCsBana, [&]() { hipLaunchKernelGGL(sg_anl_bana, gF, bT, 0, s, G.fr, d_snd, G.Z, G.freq, X, d_out); });
}

sg::StageTimes<sg::kAnlStages> g_anl_ms;  // of the last profiled launch sequence
sg::StageTimes<sg::kSweepStages> g_sweep_ms;
int g_sweep_store = 1;  // sg_set_analyze_sweep_store
sg::StageTimes<1> g_summary_ms;
sg::StageTimes<sg::kPitchStages> g_pitch_ms;
sg::StageTimes<sg::kTrackStages> g_track_ms;

}  // namespace

namespace sg {

void summary_device(const std::vector<SumSound>& snds, int cols, double samplingRate, const double* d_tables,
                    double* d_summary, hipStream_t s, double* kernel_ms) {
  StageClock clk(s, kernel_ms, 1);
  clk.zero();
  if (snds.empty()) return;
  if (cols < kAnlFixed + 6 + kPathCols || (cols - kAnlFixed - kPathCols) % 6)
    throw SgError(SG_E_DEVICE, "analyze: the summary's setup leaves the row");
  DevBuf db;
  const SumSound* d_ss = upload(db, snds, s);
  clk.stamp();
  hipLaunchKernelGGL(sg_anl_summary, dim3((unsigned)snds.size()), dim3(kSumT), 0, s, d_ss, cols, samplingRate, d_tables,
                     d_summary);
  HIPCHK(hipGetLastError());
  clk.stamp();
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
}

template <typename T>
void analyze_device(const AnlSetup& A, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                    double* d_out, const int64_t* out_off, int32_t* frames_out, hipStream_t s, double* kernel_ms,
                    const PitchSetup* pitch, const TrackSetup* track, double* d_summary, double* summary_ms) {
  const SpgSetup& P = A.spg;
  const int B = P.bins;
  std::vector<PathSound> ps(track ? n_calls : 0);
  const int pstride = track ? path_scratch(track->path.nCands, track->path.pathfinding) : 0;
  const FrameList L = list_frames(A, lengths, n_calls, [&](int64_t c, int nf, int64_t f0) {
    frames_out[c] = nf;
    if (track)  // the smoothing window is refused before anything is launched
      ps[c] = PathSound{out_off[c], f0 * pstride, nf, track_hw(track->smooth, P.sr, lengths[c], nf), 0};
  });
  std::vector<AnlSound> snds(n_calls);
  std::vector<SumSound> ss(d_summary ? n_calls : 0);
  for (int64_t c = 0; c < n_calls; ++c) {
    snds[c] = AnlSound{offsets[c], L.lens[c], L.zoff[c], out_off[c], L.nfs[c], 0};
    if (d_summary) ss[c] = SumSound{out_off[c], lengths[c], L.nfs[c], 0};
  }
  StageClock clk(s, kernel_ms, track ? kTrackStages : pitch ? kPitchStages : kAnlStages);
  clk.zero();
  const int64_t F = (int64_t)L.fr.size();
  if (d_summary && !track) throw SgError(SG_E_DEVICE, "analyze: the summary needs the tail's columns");
  if (F == 0) {  // nothing to analyse; the summary rows are still written (NaN)
    if (d_summary) summary_device(ss, A.cols, P.sr, d_out, d_summary, s, summary_ms);
    return;
  }
  check_setup(A, pitch);
  DevBuf db;
  double* d_Z = db.get<double>((size_t)L.cells);
  SpgStat* d_stat = db.get<SpgStat>((size_t)n_calls);
  clk.stamp();
  list_spectra<T>(P, d_x, offsets, L, d_Z, d_stat, s);
  const AnlSound* d_snd = upload(db, snds, s);
  const AnlFrame* d_fr = upload(db, L.fr, s);
  FrameGroup<T> G{d_x, d_fr, F, d_stat, d_Z, upload(db, A.freq, s), nullptr,
                  upload(db, std::vector<unsigned long long>(n_calls, dkey(INFINITY)), s)};
  // stages 1 to 5 (amplitudes; descriptives and dom; autocorrelation; cepstrum; BaNa): a stamp at every boundary, so a
  // stage's figure carries the host work that prepares its launch
  candidate_stages<T>(db, s, G, A, pitch, A.cols, track ? A.cols - kPathCols : A.cols, d_snd, d_out, kAcfPlain, nullptr,
                      [&](int, bool launching) {
                        if (!launching) clk.stamp();
                      });
  if (pitch) {
    clk.stamp();
    if (track) {  // 6: voiced segments, pathfinder, smoother, final columns
      check_tail_row(track->path, A.cols, A.nCands, (int)track->lab.size() == B);
      const PathSound* d_ps = upload(db, ps, s);
      double* d_scr = db.get<double>((size_t)F * pstride);
      const double* d_lab = upload(db, track->lab, s);
      launch_path(dim3((unsigned)n_calls), s, d_ps, track->path, d_out, d_scr, nullptr);
      HIPCHK(hipGetLastError());
      clk.stamp();  // 7: harmonics
      hipLaunchKernelGGL(sg_anl_harm, dim3((unsigned)F), dim3(kT), 0, s, d_fr, d_snd, d_Z, d_lab, B, A.cols, d_out);
      HIPCHK(hipGetLastError());
      clk.stamp();
    }
  }
  if (d_summary) {  // on the same stream behind sg_anl_harm; it synchronises
    summary_device(ss, A.cols, P.sr, d_out, d_summary, s, summary_ms);
    clk.finish();
    return;
  }
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
}

// sg_formants.hip runs the stage for its gate
template void analyze_device<double>(const AnlSetup&, const double*, const int64_t*, const int64_t*, int64_t, double*,
                                     const int64_t*, int32_t*, hipStream_t, double*, const PitchSetup*, const TrackSetup*, double*,
                                     double*);

void path_device(const PathPars& P, int frames, int hw, double* d_rows, hipStream_t s, double* kernel_ms, double* d_segs) {
  double ms = 0;
  StageClock clk(s, kernel_ms ? &ms : nullptr, 1);
  for (int k = 0; kernel_ms && k < kTrackStages; ++k) kernel_ms[k] = 0;
  if (frames <= 0) return;
  check_tail_row(P, P.cols, P.nCands, P.nCands >= 1 && P.nCands <= kAnlMaxCands && hw >= 0);
  DevBuf db;
  const PathSound* d_ps = upload(db, std::vector<PathSound>(1, PathSound{0, 0, frames, hw, 0}), s);
  double* d_scr = db.get<double>((size_t)frames * path_scratch(P.nCands, P.pathfinding));
  clk.stamp();
  launch_path(dim3(1), s, d_ps, P, d_rows, d_scr, d_segs);
  HIPCHK(hipGetLastError());
  clk.stamp();
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
  if (kernel_ms) kernel_ms[kTrackStages - 2] = ms;
}

}  // namespace sg

namespace {

using sg::guarded;

// The single-sound and the batch entry point of analyze_frames (pitch == nullptr, ms =
// g_anl_ms' sink) and of pitch_candidates (pitch == &S, ms = g_pitch_ms' sink), behind their
// argument checks
int frames_single(sg_ctx* ctx, const sg::AnlSetup& S, const sg::PitchSetup* pitch, double* ms, const double* wave,
                  int64_t len, double* out, const sg::TrackSetup* track = nullptr) {
  HIPCHK(hipSetDevice(ctx->device));
  const int64_t cells = (int64_t)sg::anl_frames(S, len) * S.cols;
  sg::single_sound(ctx, wave, len, cells, out, [&](const double* d, double* d_o) {
    const int64_t off = 0;
    int32_t f = 0;
    sg::analyze_device<double>(S, d, &off, &len, 1, d_o, &off, &f, ctx->stream, ms, pitch, track);
  });
  return SG_OK;
}

int frames_batch(sg_ctx* ctx, const sg::AnlSetup& S, const sg::PitchSetup* pitch, double* ms, const float* d_wave,
                 const int64_t* offsets, const int64_t* lengths, int64_t n_calls, double* d_out, const int64_t* out_off,
                 int32_t* frames_out, const sg::TrackSetup* track = nullptr) {
  if (n_calls == 0) return SG_OK;
  HIPCHK(hipSetDevice(ctx->device));
  sg::analyze_device<float>(S, d_wave, offsets, lengths, n_calls, d_out, out_off, frames_out, ctx->stream, ms, pitch, track);
  return SG_OK;
}

// the stages of sg_debug_analyze_sweep_kernel_ms
enum SweepStage { kSwSpg = 0, kSwAmpl, kSwSpec, kSwAcf, kSwPeaks, kSwCep, kSwBana, kSwPath, kSwHarm, kSwSummary };
static_assert(kSwSummary + 1 == sg::kSweepStages, "ten stages");
static_assert(kSwSpec - kSwAmpl == kCsSpec && kSwAcf - kSwAmpl == kCsAcf && kSwPeaks - kSwAmpl == kCsPeaks &&
                  kSwCep - kSwAmpl == kCsCep && kSwBana - kSwAmpl == kCsBana,
              "stage kSwAmpl + k is candidate_stages' stage k");

// sg_analyze_sweep: n_rows parameter rows over n_calls sounds (the header's text). Frame groups run one after
// another; within one, the candidate groups in the order of their store groups, so that a store's users follow each
// other and one buffer serves every store; then the tail over chunks of the frame group's rows. Every kernel's work
// on a frame or a pair is what sg_analyze_summary_batch's kernels do on it, whatever shares the launch.
void analyze_sweep(sg_ctx* ctx, const float* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                   const sg_analyze_params_full* prow, int64_t n_rows, int64_t workspace_cap, double* d_out) {
  using namespace sg;
  const SweepPlan W = anl_sweep_plan(prow, n_rows);  // every refusal comes before the first launch
  int64_t bytes[3];
  anl_sweep_bytes(W, lengths, n_calls, bytes);  // the smoothing window of every (row, sound)
  std::vector<PathPars> pars((size_t)n_rows);
  for (int64_t r = 0; r < n_rows; ++r) {
    const TrackSetup& S = W.S[r];
    check_setup(S, &S);
    check_tail_row(S.path, S.cols, S.nCands, (int)S.lab.size() == S.spg.bins);
    pars[r] = S.path;
  }
  const int64_t cap = workspace_cap > 0 ? workspace_cap : kSweepWorkspaceCap;
  const bool use_store = g_sweep_store != 0;
  hipStream_t s = ctx->stream;
  HIPCHK(hipSetDevice(ctx->device));
  StageClock clk(s, g_sweep_ms.sink(ctx), kSweepStages);
  clk.zero();
  auto timed = [&](int stage, auto&& launch) {  // what follows up to the next stamp (an upload at most) counts with it
    clk.stamp(stage);
    launch();
    HIPCHK(hipGetLastError());
  };
  DevBuf top;
  const PathPars* d_pars = upload(top, pars, s);
  for (int fg = 0; fg < W.n_frame; ++fg) {
    // the frame group's candidate groups, ordered by store group (-1 first), then by number; its rows behind them
    std::vector<int> cgs;
    std::vector<int64_t> rep;  // a row of each
    for (int64_t r = 0; r < n_rows; ++r)
      if (W.frame_group[r] == fg && std::find(cgs.begin(), cgs.end(), W.cand_group[r]) == cgs.end()) {
        cgs.push_back(W.cand_group[r]);
        rep.push_back(r);
      }
    std::vector<size_t> order(cgs.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(),
                     [&](size_t a, size_t b) { return W.store_group[rep[a]] < W.store_group[rep[b]]; });
    std::vector<int64_t> frows;
    for (size_t i : order)
      for (int64_t r = 0; r < n_rows; ++r)
        if (W.cand_group[r] == cgs[i]) frows.push_back(r);
    const TrackSetup& A = W.S[frows[0]];
    const SpgSetup& P = A.spg;
    const int B = P.bins;
    const FrameList L = list_frames(A, lengths, n_calls, [](int64_t, int, int64_t) {});
    const std::vector<int64_t>& foff = L.foff;
    const std::vector<int32_t>& nfs = L.nfs;
    const int64_t F = (int64_t)L.fr.size();
    DevBuf db;
    // where each candidate group's tables lie in the one buffer, and its view of the sounds
    std::vector<int64_t> cand0(cgs.size());
    int64_t cand_cells = 0;
    for (size_t i : order) {
      cand0[i] = cand_cells;
      cand_cells += F * (W.S[rep[i]].cols - kPathCols);
    }
    // the tail: chunks of consecutive rows whose pair tables and scratch fit the cap, at least one row
    const int64_t cap_cells = std::max<int64_t>(1, cap / (int64_t)sizeof(double));
    auto row_cells = [&](int64_t r) { return F * (W.S[r].cols + path_scratch(W.S[r].nCands, W.S[r].path.pathfinding)); };
    std::vector<size_t> chunk_end;
    int64_t work = 0, work_cells = 0;
    size_t first = 0;
    for (size_t k = 0; k < frows.size(); ++k) {
      const int64_t need = row_cells(frows[k]);
      if (k > first && (work + need > cap_cells || k - first >= 65535 || (int64_t)(k - first + 1) * n_calls > 2147483647LL)) {
        chunk_end.push_back(k);
        first = k;
        work = 0;
      }
      work += need;
      work_cells = std::max(work_cells, work);
    }
    chunk_end.push_back(frows.size());
    double* d_cand = db.get<double>((size_t)(cand_cells + work_cells));  // the candidate tables, then a chunk's workspace
    double* d_work = d_cand + cand_cells;
    double* d_Z = nullptr;
    const AnlFrame* d_fr = nullptr;
    const AnlSound* d_zs = nullptr;  // the sounds' |X| frames (z0) for sg_anl_sweep_harm: any candidate group's view
    const double* d_lab = nullptr;
    if (F > 0) {
      d_Z = db.get<double>((size_t)L.cells);
      SpgStat* d_stat = db.get<SpgStat>((size_t)n_calls);
      timed(kSwSpg, [&]() { list_spectra<float>(P, d_x, offsets, L, d_Z, d_stat, s); });
      d_fr = upload(db, L.fr, s);
      d_lab = upload(db, A.lab, s);
      const double* d_freq = upload(db, A.freq, s);
      const double* d_win = upload(db, spg_window(P.wl, P.wn), s);
      FrameGroup<float> G{d_x, d_fr, F, d_stat, d_Z, d_freq, d_win,
                          upload(db, std::vector<unsigned long long>(n_calls, dkey(INFINITY)), s)};
      // one buffer for the stores that are built: shared by two candidate groups or more, and within the cap
      std::vector<int> users((size_t)std::max(W.n_store, 1), 0);
      int64_t store_cells = 0;
      for (size_t i : order)
        if (W.store_group[rep[i]] >= 0) ++users[W.store_group[rep[i]]];
      auto built = [&](int64_t r) {
        return use_store && W.store_group[r] >= 0 && users[W.store_group[r]] >= 2 &&
               F * W.S[r].nlag * (int64_t)sizeof(double) <= cap;
      };
      for (size_t i : order)
        if (built(rep[i])) store_cells = std::max(store_cells, F * W.S[rep[i]].nlag);
      double* d_store = store_cells ? db.get<double>((size_t)store_cells) : nullptr;
      int filled = -1;  // the store group whose values d_store holds
      for (size_t i : order) {
        const TrackSetup& S = W.S[rep[i]];
        const int cols = S.cols - kPathCols;
        std::vector<AnlSound> snds(n_calls);
        for (int64_t c = 0; c < n_calls; ++c)
          snds[c] = AnlSound{offsets[c], L.lens[c], L.zoff[c], cand0[i] + foff[c] * cols, nfs[c], 0};
        d_zs = upload(db, snds, s);
        const int sgp = W.store_group[rep[i]];
        const AcfRun acf = !built(rep[i]) ? kAcfPlain : filled == sgp ? kAcfFromStore : kAcfStore;
        if (acf == kAcfStore) filled = sgp;
        // a stamp only where a stage launches, under the stage's label
        candidate_stages<float>(db, s, G, S, &S, cols, cols, d_zs, d_cand, acf, d_store, [&](int stage, bool launching) {
          if (launching) clk.stamp(kSwAmpl + stage);
        });
      }
    }
    size_t k0 = 0;
    for (size_t k1 : chunk_end) {
      std::vector<SweepPair> pairs;
      pairs.reserve((k1 - k0) * (size_t)n_calls);
      int64_t at = 0;
      for (size_t k = k0; k < k1; ++k) {
        const int64_t r = frows[k];
        const TrackSetup& S = W.S[r];
        const int ccols = S.cols - kPathCols, pstride = path_scratch(S.nCands, S.path.pathfinding);
        const size_t i = (size_t)(std::find(cgs.begin(), cgs.end(), W.cand_group[r]) - cgs.begin());
        for (int64_t c = 0; c < n_calls; ++c) {
          SweepPair R;
          R.src0 = cand0[i] + foff[c] * ccols;
          R.dst0 = at;
          R.scr0 = at + (int64_t)nfs[c] * S.cols;
          R.nf = nfs[c];
          R.hw = track_hw(S.smooth, P.sr, lengths[c], nfs[c]);
          R.cols = S.cols;
          R.row = (int32_t)r;
          at = R.scr0 + (int64_t)nfs[c] * pstride;
          pairs.push_back(R);
        }
      }
      if (at > work_cells) throw SgError(SG_E_DEVICE, "analyze: a chunk leaves its workspace");
      const SweepPair* d_pairs = upload(db, pairs, s);
      const dim3 gP((unsigned)pairs.size());
      if (F > 0) {
        bool plain = false, exact = false;
        for (size_t k = k0; k < k1; ++k) (W.S[frows[k]].path.pathfinding == 3 ? exact : plain) = true;
        const SweepPair *d_plain = d_pairs, *d_exact = d_pairs;
        if (plain && exact) {  // a copy for either kernel in which the other's pairs have no frames
          std::vector<SweepPair> a = pairs, b = pairs;
          for (size_t i = 0; i < pairs.size(); ++i) (W.S[pairs[i].row].path.pathfinding == 3 ? a : b)[i].nf = 0;
          d_plain = upload(db, a, s);
          d_exact = upload(db, b, s);
        }
        timed(kSwPath, [&]() {
          if (plain) hipLaunchKernelGGL(sg_anl_sweep_path, gP, dim3(kPathT), 0, s, d_plain, d_pars, d_cand, d_work);
          if (exact) hipLaunchKernelGGL(sg_anl_sweep_path_exact, gP, dim3(kPathT), 0, s, d_exact, d_pars, d_cand, d_work);
        });
        timed(kSwHarm, [&]() {
          hipLaunchKernelGGL(sg_anl_sweep_harm, dim3((unsigned)F, (unsigned)(k1 - k0)), dim3(kT), 0, s, d_fr, d_zs, d_pairs,
                             (int)n_calls, d_Z, d_lab, B, d_work);
        });
      }
      // sg_anl_summary itself, once per row: its workgroups write consecutive rows of the output, and a second
      // kernel around sg::sum_sound costs the first one registers (41 -> 48 VGPRs)
      std::vector<SumSound> ss(pairs.size());
      for (size_t b = 0; b < pairs.size(); ++b) ss[b] = SumSound{pairs[b].dst0, lengths[b % (size_t)n_calls], pairs[b].nf, 0};
      const SumSound* d_ss = upload(db, ss, s);
      timed(kSwSummary, [&]() {
        for (size_t k = k0; k < k1; ++k)
          hipLaunchKernelGGL(sg_anl_summary, dim3((unsigned)n_calls), dim3(kSumT), 0, s, d_ss + (k - k0) * (size_t)n_calls,
                             W.S[frows[k]].cols, P.sr, d_work, d_out + frows[k] * n_calls * kSumCols);
      });
      k0 = k1;
    }
    clk.stamp(-1);
    HIPCHK(hipStreamSynchronize(s));  // before the frame group's buffers go
  }
  clk.finish();
}

}  // namespace

extern "C" {

int sg_analyze_frames(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params* p, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_analyze_frames: bad arguments");
    const sg::AnlSetup S = sg::anl_setup(*p);
    if (len <= S.spg.wl)
      throw sg::SgError(SG_E_ARG, "sg_analyze_frames: the sound is not longer than the window (the reference's amplitude "
                                  "window sound[a:(a + wl)] leaves it)");
    return frames_single(ctx, S, nullptr, g_anl_ms.sink(ctx), wave, len, out);
  });
}

int sg_analyze_frames_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                            int64_t n_calls, const sg_analyze_params* p, double* d_out, const int64_t* out_off,
                            int32_t* frames_out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p) sg::bad_arguments("sg_analyze_frames_batch");
    sg::batch_args("sg_analyze_frames_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off, frames_out});
    const sg::AnlSetup S = sg::anl_setup(*p);
    return frames_batch(ctx, S, nullptr, g_anl_ms.sink(ctx), d_wave, offsets, lengths, n_calls, d_out, out_off, frames_out);
  });
}

int sg_pitch_candidates(sg_ctx* ctx, const double* wave, int64_t len, const sg_pitch_params* p, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_pitch_candidates: bad arguments");
    const sg::PitchSetup S = sg::pitch_setup(*p);
    if (len <= S.spg.wl)
      throw sg::SgError(SG_E_ARG, "sg_pitch_candidates: the sound is not longer than the window (the reference's amplitude "
                                  "window sound[a:(a + wl)] leaves it)");
    return frames_single(ctx, S, &S, g_pitch_ms.sink(ctx), wave, len, out);
  });
}

int sg_pitch_candidates_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                              int64_t n_calls, const sg_pitch_params* p, double* d_out, const int64_t* out_off,
                              int32_t* frames_out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p) sg::bad_arguments("sg_pitch_candidates_batch");
    sg::batch_args("sg_pitch_candidates_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off, frames_out});
    const sg::PitchSetup S = sg::pitch_setup(*p);
    return frames_batch(ctx, S, &S, g_pitch_ms.sink(ctx), d_wave, offsets, lengths, n_calls, d_out, out_off, frames_out);
  });
}

int sg_analyze(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params_full* p, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_analyze: bad arguments");
    const sg::TrackSetup S = sg::track_setup(*p);
    if (len <= S.spg.wl)
      throw sg::SgError(SG_E_ARG, "sg_analyze: the sound is not longer than the window (the reference's amplitude window "
                                  "sound[a:(a + wl)] leaves it)");
    return frames_single(ctx, S, &S, g_track_ms.sink(ctx), wave, len, out, &S);
  });
}

int sg_analyze_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_analyze_params_full* p, double* d_out, const int64_t* out_off, int32_t* frames_out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p) sg::bad_arguments("sg_analyze_batch");
    sg::batch_args("sg_analyze_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off, frames_out});
    const sg::TrackSetup S = sg::track_setup(*p);
    return frames_batch(ctx, S, &S, g_track_ms.sink(ctx), d_wave, offsets, lengths, n_calls, d_out, out_off, frames_out, &S);
  });
}

// sg_pitch_path (segments == nullptr) and sg_pitch_path_costs behind their argument checks
static int pitch_path_run(sg_ctx* ctx, const char* who, const double* table, int32_t frames, int64_t len,
                          const sg_analyze_params_full* p, double* out, double* segments, int32_t* n_segments) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || frames < 0 || len < 0 || (frames > 0 && (!table || !out)) ||
        (n_segments && frames > 0 && !segments))
      throw sg::SgError(SG_E_ARG, std::string(who) + ": bad arguments");
    double smooth = 0;
    const sg::PathPars P = sg::track_path_pars(*p, &smooth);
    const int hw = sg::track_hw(smooth, p->p.a.samplingRate, len, frames);
    if (n_segments) *n_segments = 0;
    if (frames == 0) return (int)SG_OK;
    if (!(p->p.a.samplingRate > 0)) throw sg::SgError(SG_E_ARG, std::string(who) + ": samplingRate must be positive");
    HIPCHK(hipSetDevice(ctx->device));
    const int in_cols = P.cols - sg::kPathCols;
    for (int32_t f = 0; f < frames; ++f) {  // the caller's rows, widened, staged in `out`
      for (int c = 0; c < in_cols; ++c) out[(int64_t)f * P.cols + c] = table[(int64_t)f * in_cols + c];
      for (int c = in_cols; c < P.cols; ++c) out[(int64_t)f * P.cols + c] = NAN;
    }
    sg::DevBuf db;
    double* d_rows = sg::upload_sound(db, out, (int64_t)frames * P.cols, ctx->stream);
    double* d_segs = n_segments ? db.get<double>((size_t)sg::path_seg_cells(frames)) : nullptr;
    sg::path_device(P, frames, hw, d_rows, ctx->stream, g_track_ms.sink(ctx), d_segs);
    HIPCHK(hipMemcpy(out, d_rows, (size_t)frames * P.cols * sizeof(double), hipMemcpyDeviceToHost));
    if (n_segments) {
      std::vector<double> h((size_t)sg::path_seg_cells(frames));
      HIPCHK(hipMemcpy(h.data(), d_segs, h.size() * sizeof(double), hipMemcpyDeviceToHost));
      const int64_t n = (int64_t)h[0];
      if (!(n >= 0 && n <= frames)) throw sg::SgError(SG_E_DEVICE, "analyze: the segment list leaves its buffer");
      for (int64_t k = 0; k < n * sg::kPathSegCells; ++k) segments[k] = h[1 + k];
      *n_segments = (int32_t)n;
    }
    return (int)SG_OK;
  });
}

int sg_pitch_path(sg_ctx* ctx, const double* table, int32_t frames, int64_t len, const sg_analyze_params_full* p,
                  double* out) {
  return pitch_path_run(ctx, "sg_pitch_path", table, frames, len, p, out, nullptr, nullptr);
}

int sg_pitch_path_costs(sg_ctx* ctx, const double* table, int32_t frames, int64_t len, const sg_analyze_params_full* p,
                        double* out, double* segments, int32_t* n_segments) {
  if (!n_segments) return guarded(ctx, [&]() -> int { throw sg::SgError(SG_E_ARG, "sg_pitch_path_costs: bad arguments"); });
  return pitch_path_run(ctx, "sg_pitch_path_costs", table, frames, len, p, out, segments, n_segments);
}

int sg_analyze_summary(sg_ctx* ctx, const double* table, int32_t frames, int32_t cols, int32_t nCands, int64_t len,
                       double samplingRate, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !out || frames < 0 || (frames > 0 && !table)) throw sg::SgError(SG_E_ARG, "sg_analyze_summary: bad arguments");
    if (nCands < 1 || nCands > sg::kAnlMaxCands || cols != sg::kAnlFixed + 6 * nCands + sg::kPathCols)
      throw sg::SgError(SG_E_ARG, "sg_analyze_summary: a row has 15 + 6 nCands + 4 columns, nCands in 1..8");
    if (!(samplingRate > 0)) throw sg::SgError(SG_E_ARG, "sg_analyze_summary: samplingRate must be positive");
    HIPCHK(hipSetDevice(ctx->device));
    sg::DevBuf db;
    const double* d_rows = frames > 0 ? sg::upload_sound(db, table, (int64_t)frames * cols, ctx->stream) : db.get<double>(1);
    double* d_sum = db.get<double>(sg::kSumCols);
    // a failed call (len < 0) has no table: NaN, as in a batch
    const std::vector<sg::SumSound> one(1, sg::SumSound{0, len, len < 0 ? 0 : frames, 0});
    sg::summary_device(one, cols, samplingRate, d_rows, d_sum, ctx->stream, g_summary_ms.sink(ctx));
    HIPCHK(hipMemcpy(out, d_sum, sg::kSumCols * sizeof(double), hipMemcpyDeviceToHost));
    return (int)SG_OK;
  });
}

int sg_analyze_summary_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                             int64_t n_calls, const sg_analyze_params_full* p, double* d_tables, const int64_t* out_off,
                             int32_t* frames_out, double* d_summary) {
  return guarded(ctx, [&]() {
    if (!ctx || !p) sg::bad_arguments("sg_analyze_summary_batch");
    sg::batch_args("sg_analyze_summary_batch", n_calls, {d_wave, offsets, lengths, d_tables, out_off, frames_out, d_summary});
    const sg::TrackSetup S = sg::track_setup(*p);
    if (n_calls == 0) return (int)SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::analyze_device<float>(S, d_wave, offsets, lengths, n_calls, d_tables, out_off, frames_out, ctx->stream,
                              g_track_ms.sink(ctx), &S, &S, d_summary, g_summary_ms.sink(ctx));
    return (int)SG_OK;
  });
}

int sg_analyze_summary_sound(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params_full* p, double* out,
                             double* summary) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !summary) throw sg::SgError(SG_E_ARG, "sg_analyze_summary_sound: bad arguments");
    const sg::TrackSetup S = sg::track_setup(*p);
    if (len <= S.spg.wl)
      throw sg::SgError(SG_E_ARG, "sg_analyze_summary_sound: the sound is not longer than the window (the reference's "
                                  "amplitude window sound[a:(a + wl)] leaves it)");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t cells = (int64_t)sg::anl_frames(S, len) * S.cols, off = 0;
    sg::DevBuf db;
    const double* d = sg::upload_sound(db, wave, len, ctx->stream);
    double* d_o = db.get<double>((size_t)cells);
    double* d_sum = db.get<double>(sg::kSumCols);
    int32_t f = 0;
    sg::analyze_device<double>(S, d, &off, &len, 1, d_o, &off, &f, ctx->stream, g_track_ms.sink(ctx), &S, &S,
                               d_sum, g_summary_ms.sink(ctx));
    if (out) HIPCHK(hipMemcpy(out, d_o, (size_t)cells * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(summary, d_sum, sg::kSumCols * sizeof(double), hipMemcpyDeviceToHost));
    return (int)SG_OK;
  });
}

int sg_analyze_sweep(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_analyze_params_full* rows, int64_t n_rows, int64_t workspace_cap, double* d_out) {
  return guarded(ctx, [&]() {
    if (!ctx || n_rows < 0 || workspace_cap < 0 || (n_rows > 0 && !rows) || (n_calls > 0 && n_rows > 0 && !d_out))
      sg::bad_arguments("sg_analyze_sweep");
    sg::batch_args("sg_analyze_sweep", n_calls, {d_wave, offsets, lengths});
    if (n_rows == 0) return (int)SG_OK;
    if (n_calls == 0) {
      (void)sg::anl_sweep_plan(rows, n_rows);  // the rows are still judged
      return (int)SG_OK;
    }
    analyze_sweep(ctx, d_wave, offsets, lengths, n_calls, rows, n_rows, workspace_cap, d_out);
    return (int)SG_OK;
  });
}

int sg_set_analyze_sweep_store(int32_t mode) {
  if (mode != 0 && mode != 1) return SG_E_ARG;
  g_sweep_store = mode;
  return SG_OK;
}

int sg_debug_analyze_sweep_kernel_ms(double* out) { return g_sweep_ms.read(out); }

int sg_debug_summary_kernel_ms(double* out) { return g_summary_ms.read(out); }

int sg_debug_track_kernel_ms(double* out) { return g_track_ms.read(out); }

int sg_debug_pitch_kernel_ms(double* out) { return g_pitch_ms.read(out); }

int sg_debug_analyze_kernel_ms(double* out) { return g_anl_ms.read(out); }

}  // extern "C"
