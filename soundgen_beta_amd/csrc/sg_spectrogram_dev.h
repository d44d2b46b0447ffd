// sg_spectrogram_dev.h — the analysis operator A of one frame on the device, the body of the
// frame kernels of spectrogram() (sg_spg_frames, sg_spectrogram.hip) and of stft() and
// invert_spectrogram() (sg_inv_stft, sg_inv_project, sg_invert.hip). Included by .hip files only.
#pragma once
#include "sg_fft64_dev.h"
#include "sg_spectrogram.h"

namespace {
// N = wl + 2 pad points, the wl windowed samples xc[0 .. wl) in the middle, through the packed
// real transform (sg_fft64_dev.h); sink(k, re, im) receives X_k, k < rows <= M + 1 = N / 2 + 1,
// from the thread k mod SG_F64_THREADS. stat: the sound's normalisation, applied on the fly
// in R's operation order; nullptr: the samples as they are. lds: fft64_lds_bytes(M) bytes.
template <typename T, class Sink>
__device__ __forceinline__ void spg_forward_frame(double2* lds, const T* __restrict__ xc, const sg::SpgStat* stat,
                                                  const double* __restrict__ win, const double2* __restrict__ TN, int wl,
                                                  int pad, int M, int rows, Sink&& sink) {
  Fft64Lds L = fft64_carve(lds, M);
  const sg::SpgStat st = stat ? *stat : sg::kSpgStatIdentity;
  load_packed64(L.a, M, pad, wl, [&](int j) {
    double s = (double)xc[j];
    if (stat) s = sg::spg_normalise(s, st);
    return s * win[j];
  });
  __syncthreads();
  fft64(L.a, L.b, M, TN, L.rt, false);
  for (int k = threadIdx.x; k < rows; k += SG_F64_THREADS) {
    const double2 X = untangle64(L.a, k, M, TN);
    sink(k, X.x, X.y);
  }
}
}  // namespace
