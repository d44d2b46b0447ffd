// sg_segment_plan.h — segment()'s host decisions (sg_segment.cpp) and its device launch
// sequence (sg_segment.hip). sg_segment.h holds what runs behind the envelope.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "sg_segment.h"
#include "soundgen_hip.h"

namespace sg {

constexpr int kSegStages = 6;

// What segment() decides from its arguments and a sound's length alone: hilbert()'s
// padding and un-padding (seewave.r:3336-3363), windowLength_points (segment.R:127-130),
// env()'s smoothing windows (seewave.r:2489-2498), the time step (segment.R:139-140) and
// findSyllables' shortest run
struct SegPlan {
  int64_t n1 = 0;
  int p = 0;          // the transform has N = 2^p points
  int64_t N = 1;
  int64_t left = 0;   // zeros in front of the sound
  int64_t shift = 0;  // envelope value k is |ht[shift + k]|
  int64_t n_env = 0;  // values of the un-padded transform
  double wl = 0;      // windowLength_points, possibly ending in .5
  int64_t m = 0;      // smoothed values
  int64_t points = 0; // of a smoothing window (the first one's; all are alike in practice)
  double timestep = 0;
  int64_t minCount = 0;  // ceiling(shortestSyl / timestep)
  // per window: 0-based first envelope index, points, and the point from which the indices are
  // one further (== points: none; see seg_plan)
  std::vector<int32_t> first, count, jump;
};

// p's fields behind the envelope, validated (SG_E_ARG as the reference stops)
SegPars seg_pars(const sg_segment_params& p);
// mode 1: the hilbert fields alone. windows = false leaves first / count empty.
SegPlan seg_plan(const sg_segment_params& p, int64_t len, bool windows);
// cells of a sound's output
int64_t seg_out_cells(const sg_segment_params& p, const SegPlan& S);

// The launch sequence for n_calls sounds at d_x + offsets[c] (device memory, T = float or
// double) into d_out + out_off[c] (device memory). plans[c].n1 == 0 marks a sound the
// reference stops on (batch only). kernel_ms: kSegStages doubles or nullptr.
template <typename T>
void segment_device(const sg_segment_params& p, const std::vector<SegPlan>& plans, const T* d_x, const int64_t* offsets,
                    int64_t n_calls, double* d_out, const int64_t* out_off, hipStream_t s, double* kernel_ms);

}  // namespace sg
