// sg_frame_grid.h — getFrameBank's frame grid (R/spectrogram.R:350-351), seq(1, max(1, len - wl), by),
// stated once for the host and the device: spectrogram(), analyze(), formants(), stft() / istft() /
// invert_spectrogram() and time_stretch() place their frames by it (through spg_frames and
// spg_frame_start, sg_spectrogram.h). No HIP header is needed on the host side
// (tests/cpp/ola_pins.cpp builds it with the host compiler).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_HD __host__ __device__
#else
#define SG_HD
#endif

namespace sg {

// seq()'s count: from + (0:n) by, n = as.integer((to - from) / by + 1e-10); 0 for len <= 1 or
// len < wl. A count past any caller's limit saturates instead of leaving int64_t.
SG_HD inline int64_t grid_frames(double by, int wl, int64_t len) {
  if (len <= 1 || len < wl) return 0;
  const double to = (double)(len - wl > 1 ? len - wl : 1);
  const double n = floor((to - 1.0) / by + 1e-10);
  return n < 4e18 ? (int64_t)n + 1 : INT64_MAX;
}
// The 0-based first sample of frame i: floor(pmin(1 + i by, to)) - 1 (indexing truncates). The
// product and the sum stay unfused, as R and the numpy restatement compute them, whatever the
// including file compiles with.
SG_HD inline int64_t grid_frame_start(double by, int wl, int64_t len, int64_t i) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double to = (double)(len - wl > 1 ? len - wl : 1);
  const double prod = (double)i * by;
  const double v = 1.0 + prod;
  return (int64_t)floor(v < to ? v : to) - 1;
}

}  // namespace sg
