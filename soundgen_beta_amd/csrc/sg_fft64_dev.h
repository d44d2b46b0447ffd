// sg_fft64_dev.h — the fp64 complex transform that sg_fft.hip (the fp64 formant
// filter frames, sg_fft_frames64), sg_spectrogram.hip (spectrogram()'s frames) and
// sg_segment.hip (the rows and columns of segment()'s whole-sound transform)
// share on the device: an M-point mixed-radix Stockham FFT (radices 2, 4 and the
// odd primes <= 31, M <= 2048) of one frame per SG_F64_THREADS-thread workgroup,
// and the contract of its table of roots. Included by .hip files only.
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
namespace {
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
// M-point complex DFT of *a (result in *a, *b scratch); TN: W_N^t (t < 2M), global; rt: LDS (32)
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
      for (int p : {3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
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
}  // namespace
