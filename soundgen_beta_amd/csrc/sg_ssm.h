// sg_ssm.h — ssm() (R/SSM.R:63-360): host decisions (sg_ssm.cpp) and the device
// launch sequence (sg_ssm.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "soundgen_hip.h"

namespace sg {

// What ssm() decides from its arguments alone (R/SSM.R:111-128), validated
struct SsmSetup {
  double sr = 0, windowLength = 0, step = 0, maxFreq = 0, kernelSD = 0;
  int nb = 0;               // melfcc(nbands)
  int winpts = 0, steppts = 0;  // powspec's round(wintime sr), round(steptime sr)
  int win0 = 1;             // max(1, round(ssmWin / step / 2) * 2 - 1), before selfsim's clamp
  int K = 0;                // kernelSize
  int input = 0, norm = 0, simil = 0, normalize = 1;
  std::vector<int32_t> mfcc;  // 1-based
};
SsmSetup ssm_setup(const sg_ssm_params& p);

// selfsim()'s windows for one sound (R/SSM.R:228-244): the frame count, win after
// the clamp and the odd-making rule, and the 0-based first frame of each window
struct SsmDims {
  int nf = 0, win = 1;
  std::vector<int32_t> idx;
};
SsmDims ssm_dims(const SsmSetup& S, int64_t len);

// getCheckerboardKernel(size, kernelSD = sd) (R/SSM.R:281-324), size x size
std::vector<double> ssm_checkerboard(int size, double sd);
// the requested rows of spec2cep's dctm2 (D x nb, row-major) and their lifter weights
void ssm_dct(const SsmSetup& S, std::vector<double>& dct, std::vector<double>& lift);

// The launch sequence for n_calls sounds at d_x + offsets[c] (device memory, T =
// float or double); outputs to host memory as sg_ssm_batch documents them.
// kernel_ms (7 doubles or nullptr): the device time of each stage
template <typename T>
void ssm_device(const SsmSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                int32_t* n_out, double* novelty_out, const int64_t* novelty_off, double* ssm_out,
                const int64_t* ssm_off, hipStream_t s, double* kernel_ms);
// unnormalised Gram matrix of n vectors of L doubles through sg_ssm_gram (test hook)
void ssm_debug_gram(const double* feat, int L, int n, double* out, hipStream_t s);

}  // namespace sg
