// sg_invert.h — stft(), istft() and invert_spectrogram(): the integer side of the
// operator pair (A, A+) that sg_invert.hip runs, for the host and for the device:
// which frames of a sound (getFrameBank's grid, sg_frame_grid.h) cover a sample, the sizes of what a
// sound leaves in HBM and of the workspace an iteration needs, and the refusals that
// are this feature's own. No HIP header is needed on the host side
// (tests/cpp/ola_pins.cpp builds it alone).
//
//   N = wl + 2 pad, M = N / 2, s_i = the 0-based first sample of frame i.
//   A   frame i = w[t] x[s_i + t], zero-padded; bins 0 .. M of its N-point DFT, unscaled.
//   A+  the M + 1 bins extended Hermitian, Re(inverse DFT) / N, the pad dropped, then
//       x^[t] = sum_i w[t - s_i] y_i[t - s_i] / sum_i w[t - s_i]^2 over the frames that
//       cover t, in frame order; 0 where that denominator is 0. No other floor.
#pragma once
#include "sg_frame_grid.h"

namespace sg {

constexpr int kInvStages = 6;  // sg_debug_invert_kernel_ms: statistics, forward (+ projection), start, inverse, overlap-add, error fold
constexpr int kInvTile = 256;  // output samples per workgroup of sg_inv_ola
constexpr int64_t kInvWorkspaceCap = (int64_t)1 << 30;  // bytes a chunk's workspace may take when the caller gives 0

// The frames [first, last] of F with s_i <= t < s_i + wl; last < first: none covers t.
// start(i) = s_i, non-decreasing in i (equal starts happen: by < 1, the clamp at len - wl).
// s_i = floor(1 + i by) - 1 <= t  <=>  i < (t + 1) / by, and s_i >= u  <=>  i >= u / by: the two
// quotients give a first guess, which the rounding of 1 + i by, the quotient's own and the
// clamp may each move by a frame, so both ends are walked to where the starts say.
struct InvCover {
  int64_t first, last;
};
template <class Start>
SG_HD inline InvCover inv_cover(int64_t t, int wl, int64_t F, double by, Start start) {
  InvCover c{0, -1};
  if (F <= 0 || t < 0) return c;
  const double top = (double)(F - 1);
  double g = ceil((double)(t + 1) / by) - 1.0;
  int64_t hi = (int64_t)(g < 0 ? 0 : g > top ? top : g);
  while (hi + 1 < F && start(hi + 1) <= t) ++hi;
  while (hi >= 0 && start(hi) > t) --hi;
  const int64_t u = t - wl + 1;  // s_i >= u  <=>  t < s_i + wl
  int64_t lo = 0;
  if (u > 0) {
    g = ceil((double)u / by);
    lo = (int64_t)(g < 0 ? 0 : g > top ? top : g);
    while (lo > 0 && start(lo - 1) >= u) --lo;
    while (lo < F && start(lo) < u) ++lo;
  }
  c.first = lo;
  c.last = hi;
  return c;
}

// What a sound of `frames` frames takes in HBM. A matrix has rows = bins (the reference's
// shape: DC in, Nyquist out) or bins + 1 rows, frame after frame.
SG_HD inline bool inv_rows_ok(int rows, int bins) { return rows == bins || rows == bins + 1; }
// bytes of workspace a sound needs inside istft / invert_spectrogram: the bins + 1 complex bins
// of every frame, its wl windowed samples, and the two error sums of a frame
SG_HD inline int64_t inv_workspace_bytes(int64_t frames, int wl, int bins) {
  return frames * ((int64_t)(bins + 1) * 16 + (int64_t)wl * 8 + 16);
}

}  // namespace sg
