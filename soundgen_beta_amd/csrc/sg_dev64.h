// sg_dev64.h — the fp64 device helpers that more than one of sg_mel.hip,
// sg_ssm.hip, sg_spectrogram.hip, sg_analyze.hip and sg_segment.hip use: the order-preserving
// keys behind their atomic minima and maxima, and the reductions whose order is
// part of the results. Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// a double's bits and back, as __double_as_longlong and __longlong_as_double move them, for
// host code too. Plain inline like those two: forced inline, the compiler knows the sign
// bit in dkey and turns its | into an xor (the same key, another instruction stream)
__host__ __device__ static inline long long double_bits(double x) {
  long long t;
  __builtin_memcpy(&t, &x, sizeof t);
  return t;
}
__host__ __device__ static inline double bits_double(long long x) {
  double t;
  __builtin_memcpy(&t, &x, sizeof t);
  return t;
}

// a double as an unsigned key with the doubles' order (atomicMin / atomicMax), and back
__host__ __device__ __forceinline__ unsigned long long dkey(double v) {
  const unsigned long long b = (unsigned long long)double_bits(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double dunkey(unsigned long long k) {
  return bits_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the sum over a wavefront, a butterfly: every lane gets the result
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// op 0: sum, 1: min, 2: max over a workgroup of NT threads (red: NT doubles of LDS), in
// a fixed order; every thread gets the result
template <int NT>
__device__ __forceinline__ double block_reduce(double v, int op, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double a = red[threadIdx.x], b = red[threadIdx.x + o];
      red[threadIdx.x] = op == 0 ? a + b : op == 1 ? fmin(a, b) : fmax(a, b);
    }
    __syncthreads();
  }
  return red[0];
}

}  // namespace
