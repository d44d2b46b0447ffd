// sg_mel_dev.h — what sg_mel.hip (compareSounds) and sg_ssm.hip (ssm) share on
// the device side of tuneR's melfcc front end: the zero-padded real FFT of one
// windowed frame in LDS and its power spectrum, and a mel band of it. Included by
// .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sg {

struct MelBand {
  int32_t k0, n;  // first bin and count of the band's non-zero weights
  int32_t w0;     // offset of its weights
  int32_t pad;
};

// |X_k|^2, k < M, of the real 2M-point transform of the frame packed in A as
// z[n] = xw[2n] + i xw[2n+1] (A and B: M double2 each in LDS, A filled and
// synchronised by the caller). Complex M-point radix-2 Stockham, forward
// (e^{-2 pi i / M}): Y[b 2Ns + k] = a + w b', Y[.. + Ns] = a - w b'; then the
// untangling X_k = E_k + e^{-2 pi i k / N} O_k, E = (Z_k + conj Z_{M-k}) / 2,
// O = -i (Z_k - conj Z_{M-k}) / 2. Returns the M powers (in LDS, synchronised).
__device__ __forceinline__ double* mel_frame_power(double2* A, double2* B, const double2* __restrict__ tw,
                                                   const double2* __restrict__ twN, int M, int logM) {
  double2* X = A;
  double2* Y = B;
  for (int s = 0, Ns = 1; s < logM; ++s, Ns <<= 1) {
    for (int j = threadIdx.x; j < M / 2; j += blockDim.x) {
      const int k = j & (Ns - 1);
      const double2 w = tw[k * (M / (2 * Ns))];
      const double2 a = X[j], b0 = X[j + M / 2];
      const double2 b = make_double2(b0.x * w.x - b0.y * w.y, b0.x * w.y + b0.y * w.x);
      const int o = (j - k) * 2 + k;
      Y[o] = make_double2(a.x + b.x, a.y + b.y);
      Y[o + Ns] = make_double2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
    double2* t = X;
    X = Y;
    Y = t;
  }
  double* P = reinterpret_cast<double*>(Y);
  for (int k = threadIdx.x; k < M; k += blockDim.x) {
    const double2 z = X[k], zc = X[(M - k) & (M - 1)];
    const double ex = 0.5 * (z.x + zc.x), ey = 0.5 * (z.y - zc.y);
    const double ox = 0.5 * (z.y + zc.y), oy = -0.5 * (z.x - zc.x);
    const double2 w = twN[k];
    const double re = ex + (w.x * ox - w.y * oy), im = ey + (w.x * oy + w.y * ox);
    P[k] = re * re + im * im;
  }
  __syncthreads();
  return P;
}

// one Slaney mel band of the power spectrum P (sparse triangle)
__device__ __forceinline__ double mel_band(const MelBand bd, const double* __restrict__ wts, const double* P) {
  double acc = 0;
  for (int i = 0; i < bd.n; ++i) acc += wts[bd.w0 + i] * P[bd.k0 + i];
  return acc;
}

}  // namespace sg
