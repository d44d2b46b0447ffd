// sg_spectrogram.h — spectrogram() (R/spectrogram.R:94-276): host decisions
// (sg_spectrogram.cpp) and the device launch sequence (sg_spectrogram.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "soundgen_hip.h"

namespace sg {

constexpr int kSpgStages = 12;   // sg_debug_spectrogram_kernel_ms
constexpr int kSpgMaxBins = 2048;  // fft64's M, and the frame quantile's LDS sort

// What spectrogram() decides from its arguments alone, validated
struct SpgSetup {
  double sr = 0, step = 0;
  double by = 0;          // seq()'s fractional step / 1000 * samplingRate
  int wl = 0;             // windowLength_points
  int pad = 0;            // zpExtra / 2 zeros on either side of a frame (0 when zpExtra <= 0)
  int N = 0, bins = 0;    // FFT length wl + 2 pad, N / 2
  int kTime = 0, kFreq = 0;  // rolling medians along bins / along frames; 0: off
  double qTime = 0, percentNoise = 0, noiseReduction = 0;
  double contrast_exp = 1, brightness_exp = 1;
  int wn = 6, deriv = 0, processed = 1;
};
SpgSetup spg_setup(const sg_spectrogram_params& p);
// frames of a sound of len samples (0 for len <= 1 or len < wl; more than 2^31 are refused), and
// the 0-based first sample of frame i: sg_frame_grid.h's grid at S.by and S.wl
int spg_frames(const SpgSetup& S, int64_t len);
int64_t spg_frame_start(const SpgSetup& S, int64_t len, int i);
// ftwindow_modif(wl, wn) in R's operation order
std::vector<double> spg_window(int wl, int wn);

// A frame of a launch, as the frame kernels of spectrogram(), stft() and invert_spectrogram() read it
struct SpgFrame {
  int64_t o;       // first sample within the sound
  int32_t snd, f;  // sound (of the launch's table), frame within the sound
};
// The nf = spg_frames(S, len) frames of sound snd appended to fr. Refuses, in the name of the
// feature `who`, a frame that leaves its sound and more than 2^31 frames in one launch.
void spg_list_frames(const SpgSetup& S, int64_t len, int nf, int32_t snd, const char* who, std::vector<SpgFrame>& fr);

// getFrameBank's normalisation of a sound (device): x -> ((x - mean) / sd) / m when scaled, else x / m
struct SpgStat {
  double mean, sd, m, mn, mx;
  int32_t scaled, pad;
};
// the statistics that leave a sample as it is, bit for bit: what a sound has before its own are known
constexpr SpgStat kSpgStatIdentity{0, 1, 1, 0, 0, 0, 0};
#if defined(__HIPCC__)
__host__ __device__
#endif
inline double spg_normalise(double s, const SpgStat& st) {
  if (st.scaled) s = (s - st.mean) / st.sd;
  return s / st.m;
}

// The normalisation statistics alone, as spectrogram_device computes them (the same kernels in
// the same order: bit-equal), for a caller that rebuilds frames without a spectrogram
// (sg_formants.hip). lengths[c] <= 0: an untouched entry. Synchronises the stream.
template <typename T>
void spg_stats_device(const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls, SpgStat* d_stat,
                      hipStream_t s);

// TN[t] = W_N^t = root64(t, N), t < N (device memory): a table of roots as fft64
// (sg_fft64_dev.h) reads it, filled on stream s (the kernel sg_spg_roots)
void fill_roots64(double2* d_TN, int N, hipStream_t s);

// The launch sequence for n_calls sounds at d_x + offsets[c] (device memory, T =
// float or double); matrices to d_out + out_off[c] (device memory). kernel_ms
// (kSpgStages doubles or nullptr): the device time of each stage. d_stat_out (device,
// n_calls entries, or nullptr) receives every sound's normalisation statistics
template <typename T>
void spectrogram_device(const SpgSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths,
                        int64_t n_calls, double* d_out, const int64_t* out_off, int32_t* bins_out,
                        int32_t* frames_out, hipStream_t s, double* kernel_ms, SpgStat* d_stat_out = nullptr);

}  // namespace sg
