// sg_fft64_dev.h — the fp64 transforms that five files share on the device: sg_fft.hip (the fp64
// formant filter frames, sg_fft_frames64), sg_spectrogram.hip (spectrogram()'s frames),
// sg_invert.hip (stft(), istft(), invert_spectrogram()), sg_analyze.hip (the cepstral tracker)
// and sg_segment.hip (the rows and columns of segment()'s whole-sound transform). One frame per
// SG_F64_THREADS-thread workgroup. Included by .hip files only.
//
//   fft64            the complex transform: an M-point mixed-radix Stockham FFT (radices 2, 4 and
//                    the odd primes <= 31, M <= 2048), and the contract of its table of roots
//   fft64_lds_bytes  the dynamic LDS of an M-point frame (host and device), and
//   fft64_carve      its layout: two M-point buffers, the radix roots, then the caller's own
//   load_packed64    N = 2M real points, zero-padded, as z_n = s(2n - pad) + i s(2n + 1 - pad)
//   untangle64       X_k, 0 <= k <= M, of those N real points from the M-point transform of z
// The inverse packing (the Hermitian extension fed to the inverse transform) is not here:
// sg_inv_frames and sg_fft_frames64 extend differently and round differently.
//
// Stockham autosort, out of place between two M-point LDS buffers. Per stage of
// radix R: (a) every input times its twiddle, in place; (b) odd R: one work item
// per (butterfly, output pair k, R - k) from the symmetric sums x_m +- x_{R-m} (all
// threads busy for R = 19, 29), R = 2, 4: one item per butterfly. (Grouping several
// outputs per item so each input pair is read once measured no better: r04d, +2 %
// at 3, +21 % at 2 per item.)
//
// Roots: TN[t] = W_N^t = exp(-2 pi i t / N), t < N = 2M, an fp64 table in global
// memory (L2-resident), every entry root64(t, N) -- sg_roots64 fills one per
// window length of a plan, sg_spg_roots (fill_roots64, sg_spectrogram.h) one per
// spectrogram launch and one per launch of the cepstral tracker.
#pragma once
#include <hip/hip_runtime.h>

constexpr int SG_F64_THREADS = 256;  // threads per fp64 frame (r04: 128 / 512 / 1,024 slower)
constexpr int SG_F64_MAX_RADIX = 31;   // fft64's largest radix
constexpr int SG_F64_ROOT_SLOTS = 32;  // W_R^t, t < R, of the stage under way: the largest radix, rounded up
static_assert(SG_F64_MAX_RADIX <= SG_F64_ROOT_SLOTS, "a stage's roots fill rt[0 .. R)");
namespace {
// Bytes of dynamic LDS an M-point frame needs, and how they are laid out: a, b (M points each),
// rt (SG_F64_ROOT_SLOTS), and `end`, the first byte behind them, for what the kernel adds
__host__ __device__ constexpr int fft64_lds_bytes(int M) { return (2 * M + SG_F64_ROOT_SLOTS) * (int)sizeof(double2); }
struct Fft64Lds {
  double2 *a, *b, *rt;
  void* end;
};
__device__ __forceinline__ Fft64Lds fft64_carve(double2* lds, int M) {
  return Fft64Lds{lds, lds + M, lds + 2 * M, lds + 2 * M + SG_F64_ROOT_SLOTS};
}
// W_N^t as the tables hold it (sincospi: exact at the quadrant points)
__device__ __forceinline__ double2 root64(int t, int N) {
  double sn, cs;
  sincospi(-2.0 * (double)t / (double)N, &sn, &cs);
  return make_double2(cs, sn);
}
__device__ __forceinline__ double2 cmul64(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ double2 conj_if(double2 w, bool c) { return c ? make_double2(w.x, -w.y) : w; }
// one radix-R stage of an M-point frame, src -> dst; TN = W_N^t, t < N = 2M; rt = W_R^t.
// CM, CNS > 0: frame size and stage stride as compile-time constants (the dominant
// geometry, M = 1102 = 2 x 19 x 29): every division and modulo folds to shifts and
// multiplies, the odd butterflies' root index steps by k instead of (m k) mod R.
template <int R, int CM = 0, int CNS = 0>
__device__ void stage64(double2* __restrict__ src, double2* __restrict__ dst, int M_, int Ns_,
                        const double2* __restrict__ TN, const double2* __restrict__ rt, bool inv) {
  const int M = CM ? CM : M_, Ns = CNS ? CNS : Ns_;
  const int nR = M / R, tstep2 = 2 * (M / (Ns * R));  // W_{Ns R}^e = W_N^(2 e M / (Ns R))
  if (Ns > 1) {  // (a) input j + r nR of butterfly j times W_{Ns R}^(r (j mod Ns)), in place
    for (int q = threadIdx.x; q < M; q += SG_F64_THREADS) {
      const int r = q / nR, jm = (q - r * nR) % Ns;
      if (r != 0 && jm != 0) src[q] = cmul64(src[q], conj_if(TN[r * jm * tstep2], inv));
    }
    __syncthreads();
  }
  if constexpr (R == 2 || R == 4) {
    for (int j = threadIdx.x; j < nR; j += SG_F64_THREADS) {
      const int jm = j % Ns;
      const double2* x = src + j;
      double2* y = dst + (j - jm) * R + jm;
      if constexpr (R == 2) {
        const double2 u = x[0], v = x[nR];
        y[0] = make_double2(u.x + v.x, u.y + v.y);
        y[Ns] = make_double2(u.x - v.x, u.y - v.y);
      } else {
        const double2 a = x[0], b = x[nR], c = x[2 * nR], d = x[3 * nR];
        const double2 s0 = make_double2(a.x + c.x, a.y + c.y), d0 = make_double2(a.x - c.x, a.y - c.y);
        const double2 s1 = make_double2(b.x + d.x, b.y + d.y), d1 = make_double2(b.x - d.x, b.y - d.y);
        // forward: y1 = d0 - i d1, y3 = d0 + i d1 (inverse: swapped)
        const double2 mm = make_double2(d0.x + d1.y, d0.y - d1.x), mp = make_double2(d0.x - d1.y, d0.y + d1.x);
        y[0] = make_double2(s0.x + s1.x, s0.y + s1.y);
        y[Ns] = inv ? mp : mm;
        y[2 * Ns] = make_double2(s0.x - s1.x, s0.y - s1.y);
        y[3 * Ns] = inv ? mm : mp;
      }
    }
  } else {
    // y_k = x_0 + sum_m A_m c_mk -/+ i sum_m B_m s_mk (forward -, inverse +), y_{R-k} the
    // other sign; A_m = x_m + x_{R-m}, B_m = x_m - x_{R-m}; item k = 0: y_0 = x_0 + sum A_m
    constexpr int H = (R - 1) / 2;
    for (int i = threadIdx.x; i < nR * (H + 1); i += SG_F64_THREADS) {
      const int k = i % (H + 1), j = i / (H + 1), jm = j % Ns;
      const double2* x = src + j;
      double2* y = dst + (j - jm) * R + jm;
      const double2 x0 = x[0];
      double2 P = make_double2(0.0, 0.0), Q = make_double2(0.0, 0.0);
      int t = 0;  // (m k) mod R
#pragma unroll 2
      for (int m = 1; m <= H; ++m) {
        t += k;
        if (t >= R) t -= R;
        const double2 u = x[m * nR], v = x[(R - m) * nR];
        const double2 w = k == 0 ? make_double2(1.0, 0.0) : rt[t];  // (cos, -sin) of 2 pi m k / R
        P.x = fma(u.x + v.x, w.x, P.x);
        P.y = fma(u.y + v.y, w.x, P.y);
        Q.x = fma(u.x - v.x, -w.y, Q.x);
        Q.y = fma(u.y - v.y, -w.y, Q.y);
      }
      const double2 ya = make_double2(x0.x + P.x + Q.y, x0.y + P.y - Q.x);
      const double2 yb = make_double2(x0.x + P.x - Q.y, x0.y + P.y + Q.x);
      if (k == 0) {
        y[0] = ya;
      } else {
        y[k * Ns] = inv ? yb : ya;
        y[(R - k) * Ns] = inv ? ya : yb;
      }
    }
  }
  __syncthreads();
}
// M-point complex DFT of *a (result in *a, *b scratch); TN: W_N^t (t < 2M), global; rt: LDS
// (SG_F64_ROOT_SLOTS points: every rt[threadIdx.x] below is written for threadIdx.x < R <= SG_F64_MAX_RADIX)
__device__ void fft64(double2*& a, double2*& b, int M, const double2* __restrict__ TN,
                                   double2* __restrict__ rt, bool inv) {
  if (M == 1102) {  // 2 x 19 x 29, the stage order of the loop below, sizes folded
    stage64<2, 1102, 1>(a, b, M, 1, TN, rt, inv);
    if (threadIdx.x < 19) rt[threadIdx.x] = TN[threadIdx.x * (2 * 1102 / 19)];
    __syncthreads();
    stage64<19, 1102, 2>(b, a, M, 2, TN, rt, inv);  // ends with a barrier: its root reads are done
    if (threadIdx.x < 29) rt[threadIdx.x] = TN[threadIdx.x * (2 * 1102 / 29)];
    __syncthreads();
    stage64<29, 1102, 38>(a, b, M, 38, TN, rt, inv);
    double2* t = a; a = b; b = t;  // three stages: the result is in b -> swap as the loop does
    return;
  }
  int rest = M, Ns = 1;
  while (rest > 1) {
    int R = rest % 4 == 0 ? 4 : rest % 2 == 0 ? 2 : 0;
    if (!R)
      for (int p : {3, 5, 7, 11, 13, 17, 19, 23, 29, SG_F64_MAX_RADIX})
        if (rest % p == 0) { R = p; break; }
    if (R != 2 && R != 4) {  // odd radix: W_R^t = W_N^(t 2M / R), t < R
      if (threadIdx.x < R) rt[threadIdx.x] = TN[threadIdx.x * (2 * M / R)];
      __syncthreads();
    }
    switch (R) {
#define SG_S64(RR) case RR: stage64<RR>(a, b, M, Ns, TN, rt, inv); break;
      SG_S64(2) SG_S64(3) SG_S64(4) SG_S64(5) SG_S64(7) SG_S64(11) SG_S64(13) SG_S64(17) SG_S64(19) SG_S64(23)
      SG_S64(29) SG_S64(31)
#undef SG_S64
      default: return;  // the planner only sends 31-smooth M
    }
    double2* t = a; a = b; b = t;
    Ns *= R;
    rest /= R;
  }
}
// N = 2M real points s(j - pad), j - pad in [0, len), zeros around them, packed for fft64:
// a[n] = s(2n - pad) + i s(2n + 1 - pad), n < M. sample(j), 0 <= j < len, gives s(j).
template <class Sample>
__device__ __forceinline__ void load_packed64(double2* a, int M, int pad, int len, Sample&& sample) {
  for (int n = threadIdx.x; n < M; n += SG_F64_THREADS) {
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * n + h - pad;
      v[h] = j >= 0 && j < len ? sample(j) : 0.0;
    }
    a[n] = make_double2(v[0], v[1]);
  }
}
// X_k, 0 <= k <= M, of the N real points from a = fft64 of their packing:
// X_k = E_k + W_N^k O_k, E = (Z_k + conj Z_{M-k}) / 2, O = -i (Z_k - conj Z_{M-k}) / 2; Z_M = Z_0, W_N^M = TN[M]
__device__ __forceinline__ double2 untangle64(const double2* a, int k, int M, const double2* __restrict__ TN) {
  const double2 p = a[k == M ? 0 : k], q = a[(k == 0 || k == M) ? 0 : M - k], w = TN[k];
  const double2 e = make_double2(0.5 * (p.x + q.x), 0.5 * (p.y - q.y));
  const double2 o = make_double2(0.5 * (p.y + q.y), -0.5 * (p.x - q.x));
  return make_double2(e.x + (o.x * w.x - o.y * w.y), e.y + (o.x * w.y + o.y * w.x));
}
}  // namespace
