// sg_spectrogram.hip — spectrogram() on the device (R/spectrogram.R:94-276):
// getFrameBank, the STFT magnitudes and the denoising chain of a batch of sounds,
// fp64 throughout. A matrix is kept frame after frame (cell (f, b) at f bins + b):
// the frame kernel writes a frame's bins contiguously, and every per-frame pass
// (the median along bins, the frame quantile, the entropy) reads them so, while
// the passes that walk along frames (the derivative's second term, the median
// along frames, the noise spectrum) run one thread per bin and stay coalesced. It
// is also R's column-major image of the bins x frames matrix that is returned.
//
//   sg_spg_stats      getFrameBank's normalisation (:345-348): sum, min and max per
//                     chunk of 64 Ki samples, then the squared deviations for
//                     scale(); sg_spg_stats_fold folds a sound's chunks in a fixed order
//   sg_spg_roots      W_N^t, t < N: a table fft64 reads (fill_roots64: the launch's frame
//                     length here, the cepstrum's transform in sg_analyze.hip)
//   sg_spg_frames     one workgroup per frame: |X_k| for k < N / 2 (spg_forward_frame,
//                     sg_spectrogram_dev.h; the window is a host table in R's operation order)
//   sg_spg_deriv      :180-185 sqrt(dZ_dt^2 + dZ_df^2): along bins / along frames
//   sg_spg_medbins    :192-196 smoothTime: rollmedian(fill = 0) along a frame's bins
//   sg_spg_medframes  :197-201 smoothFreq: rollmedian(fill = 0) along a bin's frames
//   sg_spg_prep       :202-206 each frame minus the type-7 quantile of its bins (a
//                     bitonic sort of the frame in LDS), and the sound's smallest
//                     positive cell and NaN flag (:209-212; order-preserving keys)
//   sg_spg_log        :211-213 log, the floor, minus the minimum; the sound's maximum
//   sg_spg_entropy    :217 getEntropy ('weiner') per frame
//   sg_spg_entq       :218 the two order statistics of a sound's entropies that
//                     quantile() blends, by rank counting (any number of frames)
//   sg_spg_noise      :221-223 the mean spectrum of the frames with entropy >= q
//   sg_spg_sub        :225-228 the recycled subtraction, the clamp; the new maximum
//   sg_spg_final      :231-241 power, / max, brightness, the clamp at 1
// The medians are exact for every odd k (rank counting in the window, O(k^2) per
// cell) and meant for small k.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sg_dev64.h"
#include "sg_launch.h"
#include "sg_rmath.h"
#include "sg_spectrogram_dev.h"

namespace {

using sg::DevBuf;
using sg::upload;

struct SpgSound {
  int64_t base, len;  // samples [base, base + len) of the input buffer
  int64_t cell0[2];   // first cell of its matrix in the output buffer [0] / the work buffer [1]
  int32_t f0, nf;     // frames [f0, f0 + nf) of the launch
  int32_t ch0, pad;   // first of its ceil(len / kStatChunk) chunks
};

// a select, not an index: a dynamic index would put the struct into scratch
__device__ __forceinline__ int64_t cell0(const SpgSound& S, int w) { return w ? S.cell0[1] : S.cell0[0]; }

using sg::SpgFrame;

struct SpgChunk {
  int32_t snd, c;
};

using sg::SpgStat;

// per sound: the smallest positive cell, the maxima after the log and after the
// subtraction (order-preserving keys), the NaN flag, the entropies' order statistics
struct SpgRange {
  unsigned long long minpos, max1, max2;
  double elo, ehi;   // sorted valid entropies at floor / ceiling of quantile()'s index
  int32_t nan, nvalid;
};

constexpr int kT = 256;  // threads of every workgroup here (SG_F64_THREADS for the frames)
static_assert(SG_F64_THREADS == kT, "fft64 strides by SG_F64_THREADS");
constexpr int kStatChunk = 1 << 16;

// quantile(type 7) from the two order statistics at floor / ceiling of index = 1 + (n - 1) p
__device__ __forceinline__ double q7(double xlo, double xhi, int n, double p) {
  const double index = 1.0 + (double)(n > 1 ? n - 1 : 0) * p;
  const double lo = floor(index);
  double qs = xlo;
  if (index > lo && xhi != qs) {
    const double h = index - lo;
    qs = __dadd_rn(__dmul_rn(1.0 - h, qs), __dmul_rn(h, xhi));  // R's two products and a sum, unfused
  }
  return qs;
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_spg_stats(const T* __restrict__ x, const SpgChunk* __restrict__ chunks,
                                                   const SpgSound* __restrict__ snds, const SpgStat* __restrict__ stat,
                                                   int pass, double* __restrict__ part) {
  __shared__ double red[kT];
  const SpgChunk J = chunks[blockIdx.x];
  const SpgSound S = snds[J.snd];
  const T* xc = x + S.base;
  const int64_t i0 = (int64_t)J.c * kStatChunk, i1 = S.len < i0 + kStatChunk ? S.len : i0 + kStatChunk;
  if (pass == 0) {
    double acc = 0, lo = INFINITY, hi = -INFINITY;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kT) {
      const double v = (double)xc[i];
      acc += v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    acc = block_reduce<kT>(acc, 0, red);
    lo = block_reduce<kT>(lo, 1, red);
    hi = block_reduce<kT>(hi, 2, red);
    if (threadIdx.x == 0) {
      part[3 * (int64_t)blockIdx.x] = acc;
      part[3 * (int64_t)blockIdx.x + 1] = lo;
      part[3 * (int64_t)blockIdx.x + 2] = hi;
    }
  } else {
    const double mean = stat[J.snd].mean;
    double acc = 0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kT) {
      const double d = (double)xc[i] - mean;
      acc += d * d;
    }
    acc = block_reduce<kT>(acc, 0, red);
    if (threadIdx.x == 0) part[3 * (int64_t)blockIdx.x] = acc;
  }
}

// one thread per sound walks its chunks in order
__global__ __launch_bounds__(64) void sg_spg_stats_fold(const double* __restrict__ part, const SpgSound* __restrict__ snds,
                                                        int n_snds, int pass, SpgStat* __restrict__ stat) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= n_snds) return;
  const SpgSound S = snds[c];
  const int nch = (int)((S.len + kStatChunk - 1) / kStatChunk);
  SpgStat st = stat[c];
  if (pass == 0) {
    double acc = 0, lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < nch; ++k) {
      acc += part[3 * (int64_t)(S.ch0 + k)];
      lo = fmin(lo, part[3 * (int64_t)(S.ch0 + k) + 1]);
      hi = fmax(hi, part[3 * (int64_t)(S.ch0 + k) + 2]);
    }
    st.mean = S.len > 0 ? acc / (double)S.len : 0.0;
    st.mn = lo;
    st.mx = hi;
    st.scaled = lo > 0 ? 1 : 0;  // if (min(sound) > 0) sound = scale(sound)
    st.sd = 1;
    st.m = fmax(fabs(hi), fabs(lo));
  } else if (st.scaled) {
    double acc = 0;
    for (int k = 0; k < nch; ++k) acc += part[3 * (int64_t)(S.ch0 + k)];
    st.sd = sqrt(acc / (double)(S.len - 1));
    st.m = fmax(fabs((st.mx - st.mean) / st.sd), fabs((st.mn - st.mean) / st.sd));
  }
  stat[c] = st;
}

__global__ __launch_bounds__(kT) void sg_spg_roots(double2* __restrict__ TN, int N) {
  const int t = blockIdx.x * kT + threadIdx.x;
  if (t < N) TN[t] = root64(t, N);
}

// Test hook (sg_debug_fft64): fft64 alone, one workgroup per frame of M complex
// points, unscaled. LDS: fft64_lds_bytes(M).
__global__ __launch_bounds__(kT) void sg_fft64_probe(const double2* __restrict__ in, const double2* __restrict__ TN,
                                                     int M, int inv, double2* __restrict__ out) {
  extern __shared__ double2 lds64[];
  Fft64Lds L = fft64_carve(lds64, M);
  const double2* x = in + (int64_t)blockIdx.x * M;
  for (int n = threadIdx.x; n < M; n += kT) L.a[n] = x[n];
  __syncthreads();
  fft64(L.a, L.b, M, TN, L.rt, inv != 0);
  double2* y = out + (int64_t)blockIdx.x * M;
  for (int k = threadIdx.x; k < M; k += kT) y[k] = L.a[k];
}

// |X_k|, k < M = N / 2, of every frame (spg_forward_frame). LDS: fft64_lds_bytes(M).
template <typename T>
__global__ __launch_bounds__(kT) void sg_spg_frames(const T* __restrict__ x, const SpgFrame* __restrict__ frames,
                                                    const SpgSound* __restrict__ snds, const SpgStat* __restrict__ stat,
                                                    const double* __restrict__ win, const double2* __restrict__ TN,
                                                    int wl, int pad, int M, double* __restrict__ out) {
  extern __shared__ double2 lds64[];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const SpgStat st = stat[F.snd];
  double* row = out + S.cell0[0] + (int64_t)F.f * M;
  // host: F.o + wl <= S.len
  spg_forward_frame(lds64, x + S.base + F.o, &st, win, TN, wl, pad, M, M,
                    [row](int k, double re, double im) { row[k] = hypot(re, im); });
}

__global__ __launch_bounds__(kT) void sg_spg_deriv(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                   const double* __restrict__ src, int sw, double* __restrict__ dst,
                                                   int dw, int B) {
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const double* r = src + cell0(S, sw) + (int64_t)F.f * B;
  double* d = dst + cell0(S, dw) + (int64_t)F.f * B;
  for (int b = threadIdx.x; b < B; b += kT) {
    const double z = r[b];
    const double dt = b > 0 ? z - r[b - 1] : 0.0;  // dZ_dt: along the frame's bins (:182)
    const double df = F.f > 0 ? z - r[b - B] : 0.0;  // dZ_df: along frames (:184)
    d[b] = sqrt(dt * dt + df * df);
  }
}

// the median of the k = 2 h + 1 values p[0], p[stride], ...: the value whose rank
// interval [#less, #less + #equal) holds h; NaN if a NaN leaves no such value
__device__ __forceinline__ double window_median(const double* p, int64_t stride, int k) {
  const int h = k / 2;
  for (int c = 0; c < k; ++c) {
    const double v = p[c * stride];
    int lt = 0, eq = 0;
    for (int j = 0; j < k; ++j) {
      const double u = p[j * stride];
      lt += u < v ? 1 : 0;
      eq += u == v ? 1 : 0;
    }
    if (lt <= h && h < lt + eq) return v;
  }
  return NAN;
}

__global__ __launch_bounds__(kT) void sg_spg_medbins(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                     const double* __restrict__ src, int sw, double* __restrict__ dst,
                                                     int dw, int B, int k) {
  __shared__ double rowl[sg::kSpgMaxBins];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const double* r = src + cell0(S, sw) + (int64_t)F.f * B;
  double* d = dst + cell0(S, dw) + (int64_t)F.f * B;
  for (int b = threadIdx.x; b < B; b += kT) rowl[b] = r[b];
  __syncthreads();
  const int h = k / 2;
  for (int b = threadIdx.x; b < B; b += kT) d[b] = (b < h || b >= B - h) ? 0.0 : window_median(rowl + b - h, 1, k);
}

__global__ __launch_bounds__(kT) void sg_spg_medframes(const SpgFrame* __restrict__ frames,
                                                       const SpgSound* __restrict__ snds, const double* __restrict__ src,
                                                       int sw, double* __restrict__ dst, int dw, int B, int k) {
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const double* r = src + cell0(S, sw) + (int64_t)F.f * B;
  double* d = dst + cell0(S, dw) + (int64_t)F.f * B;
  const int h = k / 2;
  const bool edge = F.f < h || F.f >= S.nf - h;
  for (int b = threadIdx.x; b < B; b += kT) d[b] = edge ? 0.0 : window_median(r + b - (int64_t)h * B, B, k);
}

// q > 0: the frame minus quantile(frame, q) in place; always: the sound's smallest
// positive cell and its NaN flag
__global__ __launch_bounds__(kT) void sg_spg_prep(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                  double* __restrict__ buf, int w, int B, double q,
                                                  SpgRange* __restrict__ range) {
  __shared__ double srt[sg::kSpgMaxBins];
  __shared__ double red[kT];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  double* r = buf + cell0(S, w) + (int64_t)F.f * B;
  double qs = 0;
  if (q > 0) {
    int n2 = 1;
    while (n2 < B) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += kT) srt[i] = i < B ? r[i] : INFINITY;
    __syncthreads();
    for (int kk = 2; kk <= n2; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < n2; i += kT) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const double u = srt[i], v = srt[ixj];
            if ((i & kk) == 0 ? u > v : u < v) {
              srt[i] = v;
              srt[ixj] = u;
            }
          }
        }
        __syncthreads();
      }
    }
    const double index = 1.0 + (double)(B - 1) * q;
    qs = q7(srt[(int)floor(index) - 1], srt[(int)ceil(index) - 1], B, q);
  }
  double lo = INFINITY;
  int bad = 0;
  for (int b = threadIdx.x; b < B; b += kT) {
    double v = r[b];
    if (q > 0) {
      v -= qs;
      r[b] = v;
    }
    if (v > 0) lo = fmin(lo, v);
    bad |= isnan(v) ? 1 : 0;
  }
  lo = block_reduce<kT>(lo, 1, red);
  const double nb = block_reduce<kT>((double)bad, 2, red);
  if (threadIdx.x == 0) {
    if (lo < INFINITY) atomicMin(&range[F.snd].minpos, dkey(lo));
    if (nb > 0) atomicOr(&range[F.snd].nan, 1);
  }
}

// Z1[positives] = log(Z1[positives]); Z1[nonpositives] = min(Z1[positives]); Z1 = Z1 - min(Z1):
// the smallest log is log(the smallest positive), and min() of a matrix with a NaN is NaN
__global__ __launch_bounds__(kT) void sg_spg_log(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                 double* __restrict__ buf, int w, int B, SpgRange* __restrict__ range) {
  __shared__ double red[kT];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  double* r = buf + cell0(S, w) + (int64_t)F.f * B;
  const int bad = range[F.snd].nan;
  const double lmin = log(dunkey(range[F.snd].minpos));  // +Inf when nothing is positive
  double hi = -INFINITY;
  for (int b = threadIdx.x; b < B; b += kT) {
    const double x = r[b];
    const double v = bad ? NAN : ((x > 0 ? log(x) : lmin) - lmin);
    r[b] = v;
    hi = fmax(hi, v);
  }
  hi = block_reduce<kT>(hi, 2, red);
  if (threadIdx.x == 0 && hi > -INFINITY) atomicMax(&range[F.snd].max1, dkey(hi));
}

// getEntropy(frame, 'weiner'): NaN (R's NA) for sum(x) == 0; x <= 0 -> 1e-10;
// exp(mean(log(x))) / mean(x)
__global__ __launch_bounds__(kT) void sg_spg_entropy(const SpgFrame* __restrict__ frames,
                                                     const SpgSound* __restrict__ snds, const double* __restrict__ buf,
                                                     int w, int B, double* __restrict__ entr) {
  __shared__ double red[kT];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const double* r = buf + cell0(S, w) + (int64_t)F.f * B;
  double s0 = 0, s1 = 0, sl = 0;
  for (int b = threadIdx.x; b < B; b += kT) {
    const double x = r[b];
    s0 += x;
    const double y = x <= 0 ? 1e-10 : x;
    s1 += y;
    sl += log(y);
  }
  s0 = block_reduce<kT>(s0, 0, red);
  s1 = block_reduce<kT>(s1, 0, red);
  sl = block_reduce<kT>(sl, 0, red);
  if (threadIdx.x == 0) entr[S.f0 + F.f] = s0 == 0 ? NAN : exp(sl / (double)B) / (s1 / (double)B);
}

// quantile(entr, p, na.rm = TRUE)'s two order statistics by rank counting:
// blockIdx.y = sound, a thread per frame of it; tiles of the entropies through LDS
__global__ __launch_bounds__(kT) void sg_spg_entq(const SpgSound* __restrict__ snds, const double* __restrict__ entr,
                                                  double p, SpgRange* __restrict__ range) {
  __shared__ double tile[kT];
  const SpgSound S = snds[blockIdx.y];
  if ((int64_t)blockIdx.x * kT >= S.nf) return;  // workgroup-uniform
  const double* e = entr + S.f0;
  const int i = blockIdx.x * kT + threadIdx.x;
  const double v = i < S.nf ? e[i] : NAN;
  int lt = 0, eq = 0, nv = 0;
  for (int t0 = 0; t0 < S.nf; t0 += kT) {
    __syncthreads();
    tile[threadIdx.x] = t0 + (int)threadIdx.x < S.nf ? e[t0 + threadIdx.x] : NAN;
    __syncthreads();
    const int n = S.nf - t0 < kT ? S.nf - t0 : kT;
    for (int j = 0; j < n; ++j) {
      const double u = tile[j];
      nv += u == u ? 1 : 0;
      lt += u < v ? 1 : 0;
      eq += u == v ? 1 : 0;
    }
  }
  SpgRange* R = range + blockIdx.y;
  if (i == 0) R->nvalid = nv;
  if (nv == 0 || !(v == v)) return;
  const double index = 1.0 + (double)(nv - 1) * p;
  const int lo = (int)floor(index) - 1, hi = (int)ceil(index) - 1;
  if (lt <= lo && lo < lt + eq) R->elo = v;  // equal values write the same bits
  if (lt <= hi && hi < lt + eq) R->ehi = v;
}

// noise_spectrum = colMeans(Z1[which(entr >= q), ]): blockIdx.y = sound, a thread per bin,
// frames in order; nsel[sound] = the number of selected frames
__global__ __launch_bounds__(kT) void sg_spg_noise(const SpgSound* __restrict__ snds, const double* __restrict__ entr,
                                                   const SpgRange* __restrict__ range, double p,
                                                   const double* __restrict__ buf, int w, int B,
                                                   double* __restrict__ noise, int32_t* __restrict__ nsel) {
  const SpgSound S = snds[blockIdx.y];
  const SpgRange R = range[blockIdx.y];
  const int b = blockIdx.x * kT + threadIdx.x;
  if (b >= B) return;
  int cnt = 0;
  double acc = 0;
  if (R.nvalid > 0) {
    const double q = q7(R.elo, R.ehi, R.nvalid, p);
    const double* m = buf + cell0(S, w);
    for (int f = 0; f < S.nf; ++f) {
      if (entr[S.f0 + f] >= q) {  // false for NaN: which() drops NA
        acc += m[(int64_t)f * B + b];
        ++cnt;
      }
    }
  }
  noise[(int64_t)blockIdx.y * B + b] = cnt ? acc / (double)cnt : 0.0;
  if (b == 0) nsel[blockIdx.y] = cnt;
}

// Z1 - noiseReduction * noise_spectrum with R's recycling down the columns of the
// frames x bins matrix: cell (f, b) takes noise[(f + b nf) mod B]; then Z1[Z1 <= 0] = 0
__global__ __launch_bounds__(kT) void sg_spg_sub(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                 double* __restrict__ buf, int w, int B, double nr,
                                                 const double* __restrict__ noise, const int32_t* __restrict__ nsel,
                                                 SpgRange* __restrict__ range) {
  __shared__ double red[kT];
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  double* r = buf + cell0(S, w) + (int64_t)F.f * B;
  const double* nz = noise + (int64_t)F.snd * B;
  const bool sub = nsel[F.snd] > 0;
  double hi = -INFINITY;
  for (int b = threadIdx.x; b < B; b += kT) {
    double v = r[b];
    if (sub) v = __dsub_rn(v, __dmul_rn(nr, nz[((int64_t)F.f + (int64_t)b * S.nf) % B]));
    if (v <= 0) v = 0;
    r[b] = v;
    hi = fmax(hi, v);
  }
  hi = block_reduce<kT>(hi, 2, red);
  if (threadIdx.x == 0 && hi > -INFINITY) atomicMax(&range[F.snd].max2, dkey(hi));
}

// Z1 ^ contrast_exp, / max (the power is monotone: max(Z1 ^ c) = max(Z1) ^ c), / brightness_exp,
// and the clamp at 1 for brightness_exp < 1
__global__ __launch_bounds__(kT) void sg_spg_final(const SpgFrame* __restrict__ frames, const SpgSound* __restrict__ snds,
                                                   const double* src, int sw, double* dst,  // may be one buffer
                                                   int dw, int B, double ce, double be, int use2,
                                                   const SpgRange* __restrict__ range) {
  const SpgFrame F = frames[blockIdx.x];
  const SpgSound S = snds[F.snd];
  const double* r = src + cell0(S, sw) + (int64_t)F.f * B;
  double* d = dst + cell0(S, dw) + (int64_t)F.f * B;
  const SpgRange R = range[F.snd];
  double mx = dunkey(use2 ? R.max2 : R.max1);
  if (ce != 1.0) mx = pow(mx, ce);
  for (int b = threadIdx.x; b < B; b += kT) {
    double v = r[b];
    if (ce != 1.0) v = pow(v, ce);
    v = v / mx;
    if (be != 1.0) v = v / be;
    if (be < 1.0 && v > 1.0) v = 1.0;
    d[b] = R.nan ? NAN : v;
  }
}

sg::StageTimes<sg::kSpgStages> g_spg_ms;  // of the last profiled launch sequence

}  // namespace

namespace sg {

void fill_roots64(double2* d_TN, int N, hipStream_t s) {
  hipLaunchKernelGGL(sg_spg_roots, dim3((unsigned)((N + kT - 1) / kT)), dim3(kT), 0, s, d_TN, N);
  HIPCHK(hipGetLastError());
}

namespace {

// The chunks of sound c (len samples) appended to the launch's list; returns the first of them
int32_t stat_chunks(std::vector<SpgChunk>& chunks, int64_t c, int64_t len) {
  const int32_t ch0 = (int32_t)chunks.size();
  if ((int64_t)chunks.size() + len / kStatChunk + 1 > 2147483647LL)
    throw SgError(SG_E_UNSUPPORTED, "spectrogram: the frames of one launch exceed 2^31");
  for (int64_t k = 0; k * kStatChunk < len; ++k) chunks.push_back(SpgChunk{(int32_t)c, (int32_t)k});
  return ch0;
}

// The normalisation statistics of n_calls sounds on stream s, nothing awaited: both passes over the chunks, each
// folded per sound. d_stat holds kSpgStatIdentity on entry; d_part: 3 doubles per chunk
template <typename T>
void stats_launch(const T* d_x, const SpgChunk* d_ch, size_t nchunks, const SpgSound* d_snd, int64_t n_calls, SpgStat* d_stat,
                  double* d_part, hipStream_t s) {
  for (int pass = 0; pass < 2; ++pass) {
    if (nchunks) {
      hipLaunchKernelGGL(sg_spg_stats<T>, dim3((unsigned)nchunks), dim3(kT), 0, s, d_x, d_ch, d_snd, d_stat, pass, d_part);
      HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(sg_spg_stats_fold, dim3(((unsigned)n_calls + 63) / 64), dim3(64), 0, s, d_part, d_snd, (int)n_calls, pass,
                       d_stat);
    HIPCHK(hipGetLastError());
  }
}

}  // namespace

template <typename T>
void spectrogram_device(const SpgSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths,
                        int64_t n_calls, double* d_out, const int64_t* out_off, int32_t* bins_out,
                        int32_t* frames_out, hipStream_t s, double* kernel_ms, SpgStat* d_stat_out) {
  const int B = S.bins;
  if (S.processed && S.kTime > B)  // zoo::rollmedian stops for k > length
    throw SgError(SG_E_ARG, "spectrogram: smoothTime is larger than the " + std::to_string(B) + " bins of a frame");
  std::vector<SpgSound> snds(n_calls);
  std::vector<SpgFrame> fr;
  std::vector<SpgChunk> chunks;
  int64_t cells = 0;
  int nfmax = 0;
  for (int64_t c = 0; c < n_calls; ++c) {
    const int nf = spg_frames(S, lengths[c]);
    SpgSound& Q = snds[c];
    Q.base = offsets[c];
    Q.len = nf ? lengths[c] : 0;
    Q.cell0[0] = out_off[c];
    Q.cell0[1] = cells;
    Q.f0 = (int32_t)fr.size();
    Q.nf = nf;
    Q.ch0 = (int32_t)chunks.size();
    Q.pad = 0;
    bins_out[c] = B;
    frames_out[c] = nf;
    if (!nf) continue;
    if (S.processed && S.kFreq > nf)
      throw SgError(SG_E_ARG, "spectrogram: smoothFreq is larger than the " + std::to_string(nf) + " frames of call " +
                                  std::to_string((long long)c));
    stat_chunks(chunks, c, Q.len);
    spg_list_frames(S, lengths[c], nf, (int32_t)c, "spectrogram", fr);
    cells += (int64_t)nf * B;
    nfmax = std::max(nfmax, nf);
  }
  StageClock clk(s, kernel_ms, kSpgStages);
  clk.zero();
  const int64_t F = (int64_t)fr.size();
  if (F == 0) return;
  const unsigned NS = (unsigned)n_calls;
  DevBuf db;
  const SpgSound* d_snd = upload(db, snds, s);
  const SpgFrame* d_fr = upload(db, fr, s);
  const SpgChunk* d_ch = upload(db, chunks, s);
  const double* d_win = upload(db, spg_window(S.wl, S.wn), s);
  // the keys of +Inf (no positive cell yet) and -Inf (no maximum yet)
  const unsigned long long kinf = dkey(INFINITY), kninf = dkey(-INFINITY);
  SpgRange* d_range = upload(db, std::vector<SpgRange>(n_calls, SpgRange{kinf, kninf, kninf, 0.0, 0.0, 0, 0}), s);
  SpgStat* d_stat = upload(db, std::vector<SpgStat>(n_calls, kSpgStatIdentity), s);
  double* d_part = db.get<double>(3 * chunks.size());
  double2* d_TN = db.get<double2>((size_t)S.N);
  const dim3 gF((unsigned)F), bT(kT);
  clk.stamp();
  stats_launch<T>(d_x, d_ch, chunks.size(), d_snd, n_calls, d_stat, d_part, s);
  if (d_stat_out)  // for a caller that goes on with the normalised samples (sg_analyze.hip)
    HIPCHK(hipMemcpyAsync(d_stat_out, d_stat, (size_t)n_calls * sizeof(SpgStat), hipMemcpyDeviceToDevice, s));
  clk.stamp();  // 1: frames
  fill_roots64(d_TN, S.N, s);
  const int lds = fft64_lds_bytes(B);
  lds_opt_in(&sg_spg_frames<T>, lds, "sg_spg_frames");
  hipLaunchKernelGGL(sg_spg_frames<T>, gF, bT, (size_t)lds, s, d_x, d_fr, d_snd, d_stat, d_win, d_TN, S.wl, S.pad, B,
                     d_out);
  HIPCHK(hipGetLastError());
  if (S.processed) {
    // cur: where the matrices are (0: the output buffer, 1: the work buffer)
    double* bufs[2] = {d_out, nullptr};
    int cur = 0;
    auto other = [&]() -> int {
      if (!bufs[1]) bufs[1] = db.get<double>((size_t)cells);
      return 1 - cur;
    };
    clk.stamp();  // 2: derivative
    if (S.deriv) {
      const int o = other();
      hipLaunchKernelGGL(sg_spg_deriv, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, bufs[o], o, B);
      HIPCHK(hipGetLastError());
      cur = o;
    }
    clk.stamp();  // 3: median along bins
    if (S.kTime > 1) {
      const int o = other();
      hipLaunchKernelGGL(sg_spg_medbins, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, bufs[o], o, B, S.kTime);
      HIPCHK(hipGetLastError());
      cur = o;
    }
    clk.stamp();  // 4: median along frames
    if (S.kFreq > 1) {
      const int o = other();
      hipLaunchKernelGGL(sg_spg_medframes, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, bufs[o], o, B, S.kFreq);
      HIPCHK(hipGetLastError());
      cur = o;
    }
    clk.stamp();  // 5: frame quantile, smallest positive cell
    hipLaunchKernelGGL(sg_spg_prep, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, B, S.qTime > 0 ? S.qTime : 0.0, d_range);
    HIPCHK(hipGetLastError());
    clk.stamp();  // 6: log
    hipLaunchKernelGGL(sg_spg_log, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, B, d_range);
    HIPCHK(hipGetLastError());
    const bool nr = S.noiseReduction > 0;
    double* d_entr = nullptr;
    double* d_noise = nullptr;
    int32_t* d_nsel = nullptr;
    const double p = 1 - S.percentNoise / 100;
    clk.stamp();  // 7: entropy
    if (nr) {
      d_entr = db.get<double>((size_t)F);
      d_noise = db.get<double>((size_t)n_calls * B);
      d_nsel = db.get<int32_t>((size_t)n_calls);
      hipLaunchKernelGGL(sg_spg_entropy, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, B, d_entr);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // 8: entropy quantile
    if (nr) {
      hipLaunchKernelGGL(sg_spg_entq, dim3((unsigned)((nfmax + kT - 1) / kT), NS), bT, 0, s, d_snd, d_entr, p, d_range);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // 9: noise spectrum
    if (nr) {
      hipLaunchKernelGGL(sg_spg_noise, dim3((unsigned)((B + kT - 1) / kT), NS), bT, 0, s, d_snd, d_entr, d_range, p,
                         bufs[cur], cur, B, d_noise, d_nsel);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // 10: subtraction
    if (nr) {
      hipLaunchKernelGGL(sg_spg_sub, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, B, S.noiseReduction, d_noise, d_nsel,
                         d_range);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // 11: power and scale, into the output buffer
    hipLaunchKernelGGL(sg_spg_final, gF, bT, 0, s, d_fr, d_snd, bufs[cur], cur, d_out, 0, B, S.contrast_exp,
                       S.brightness_exp, nr ? 1 : 0, d_range);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();  // 'original' stops after the frames: stamps 0, 1, 2; 'processed' records all 13
}

template <typename T>
void spg_stats_device(const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls, SpgStat* d_stat,
                      hipStream_t s) {
  if (n_calls == 0) return;
  std::vector<SpgSound> snds(n_calls);
  std::vector<SpgChunk> chunks;
  for (int64_t c = 0; c < n_calls; ++c) {
    const int64_t len = lengths[c] > 0 ? lengths[c] : 0;
    snds[c] = SpgSound{offsets[c], len, {0, 0}, 0, 0, stat_chunks(chunks, c, len), 0};
  }
  DevBuf db;
  const SpgSound* d_snd = upload(db, snds, s);
  const SpgChunk* d_ch = upload(db, chunks, s);
  const SpgStat* d_init = upload(db, std::vector<SpgStat>(n_calls, kSpgStatIdentity), s);
  double* d_part = db.get<double>(3 * chunks.size());
  HIPCHK(hipMemcpyAsync(d_stat, d_init, (size_t)n_calls * sizeof(SpgStat), hipMemcpyDeviceToDevice, s));
  stats_launch<T>(d_x, d_ch, chunks.size(), d_snd, n_calls, d_stat, d_part, s);
  HIPCHK(hipStreamSynchronize(s));  // db goes away
}

template void spg_stats_device<float>(const float*, const int64_t*, const int64_t*, int64_t, SpgStat*, hipStream_t);
template void spg_stats_device<double>(const double*, const int64_t*, const int64_t*, int64_t, SpgStat*, hipStream_t);
template void spectrogram_device<float>(const SpgSetup&, const float*, const int64_t*, const int64_t*, int64_t, double*,
                                        const int64_t*, int32_t*, int32_t*, hipStream_t, double*, SpgStat*);
template void spectrogram_device<double>(const SpgSetup&, const double*, const int64_t*, const int64_t*, int64_t,
                                         double*, const int64_t*, int32_t*, int32_t*, hipStream_t, double*, SpgStat*);

}  // namespace sg

// The C entry points that touch the device live here, not in sg_api.cpp: the
// host-only sanitizer build links sg_api.cpp without this file's device code.
using sg::guarded;

extern "C" {

int sg_spectrogram(sg_ctx* ctx, const double* wave, int64_t len, const sg_spectrogram_params* p, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_spectrogram: bad arguments");
    const sg::SpgSetup S = sg::spg_setup(*p);
    if (len < S.wl || len < 2)
      throw sg::SgError(SG_E_ARG, "sg_spectrogram: the sound is shorter than the window (R would index past its end)");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t cells = (int64_t)sg::spg_frames(S, len) * S.bins;
    sg::single_sound(ctx, wave, len, cells, out, [&](const double* d, double* d_o) {
      const int64_t off = 0;
      int32_t b = 0, f = 0;
      sg::spectrogram_device<double>(S, d, &off, &len, 1, d_o, &off, &b, &f, ctx->stream, g_spg_ms.sink(ctx));
    });
    return SG_OK;
  });
}

int sg_spectrogram_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                         int64_t n_calls, const sg_spectrogram_params* p, double* d_out, const int64_t* out_off,
                         int32_t* bins_out, int32_t* frames_out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p) sg::bad_arguments("sg_spectrogram_batch");
    sg::batch_args("sg_spectrogram_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off, bins_out, frames_out});
    const sg::SpgSetup S = sg::spg_setup(*p);
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::spectrogram_device<float>(S, d_wave, offsets, lengths, n_calls, d_out, out_off, bins_out, frames_out,
                                  ctx->stream, g_spg_ms.sink(ctx));
    return SG_OK;
  });
}

// Test hook (not part of the reference surface): fft64 on nframes frames of M complex
// points from host memory. The refusals come first and need no context.
int sg_debug_fft64(sg_ctx* ctx, int32_t M, int32_t inverse, int32_t nframes, const double* in, double* out) {
  return guarded(ctx, [&]() {
    int rest = M < 1 || M > sg::kSpgMaxBins ? 0 : M;
    for (int p : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
      while (rest > 1 && rest % p == 0) rest /= p;
    if (rest != 1)
      throw sg::SgError(SG_E_UNSUPPORTED, "sg_debug_fft64: M must be 31-smooth and in 1.." +
                                              std::to_string(sg::kSpgMaxBins));
    if (!ctx || !in || !out || nframes < 0) throw sg::SgError(SG_E_ARG, "sg_debug_fft64: bad arguments");
    if (nframes == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)nframes * M;
    DevBuf db;
    double2* d_in = db.get<double2>(n);
    double2* d_out = db.get<double2>(n);
    double2* d_TN = db.get<double2>((size_t)2 * M);
    HIPCHK(hipMemcpyAsync(d_in, in, n * sizeof(double2), hipMemcpyHostToDevice, s));
    sg::fill_roots64(d_TN, 2 * M, s);
    const int lds = fft64_lds_bytes(M);
    sg::lds_opt_in(&sg_fft64_probe, lds, "sg_fft64_probe");
    hipLaunchKernelGGL(sg_fft64_probe, dim3((unsigned)nframes), dim3(kT), (size_t)lds, s, d_in, d_TN, (int)M,
                       (int)inverse, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(out, d_out, n * sizeof(double2), hipMemcpyDeviceToHost));
    return SG_OK;
  });
}

int sg_debug_spectrogram_kernel_ms(double* out) { return g_spg_ms.read(out); }

}  // extern "C"
