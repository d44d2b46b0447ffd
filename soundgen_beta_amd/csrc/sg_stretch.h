// sg_stretch.h — time_stretch(), shift_pitch() and resample(): the integer side of the phase
// vocoder between A and A+ (sg_invert.h) and of the band-limited resampler, for the host and
// for the device: the output length of a ratio and the taps of an output sample, the reduction
// of a tap's numerator mod 2 D, the split of a position between two analysis frames, and the
// sizes. No HIP header is needed on the host side (tests/cpp/stretch_pins.cpp builds it alone).
//
//   Resampler. up and down reduced by their gcd, D = max(up, down), Z = kStrZ zero crossings:
//     y[r] = sum_m x[m] (up / D) sinc(num / D) (1 + cos(pi num / (Z D))) / 2,   num = r down - m up,
//   over 0 <= m < n with |num| < Z D, in ascending m. sin(pi num / D) is taken on num reduced
//   mod 2 D to sign * sin(pi rem / D), 0 <= rem <= D / 2: exactly 0 at the multiples of D.
//   Vocoder. A position q in [0, F_in - 1] lies between the frames i = min(floor(q), F_in - 1)
//   and i1 = min(i + 1, F_in - 1), a = q - i of the way, h = s_i1 - s_i samples apart.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_STR_HD __host__ __device__
#else
#define SG_STR_HD
#endif

namespace sg {

constexpr int kStrStages = 5;      // sg_debug_stretch_kernel_ms: resampler, forward, vocoder, inverse, overlap-add
constexpr int kStrZ = 16;          // zero crossings of the windowed sinc on either side
constexpr int kStrMaxRatio = 64;   // D / min(up, down) at most: 2 Z 64 = 2,048 taps a sample
constexpr int kStrTile = 256;      // output samples per workgroup of sg_str_resample
constexpr int kStrSpan = 2048;     // input samples a workgroup stages at a time
constexpr int64_t kStrLimit = (int64_t)1 << 31;

SG_STR_HD inline int64_t str_gcd(int64_t a, int64_t b) {
  while (b != 0) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// floor(a / b), b > 0
SG_STR_HD inline int64_t str_floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

struct StrRatio {
  int64_t up, down, D;  // reduced
};
// 0, or why the ratio is refused: 1 not positive, 2 a term >= 2^31, 3 D / min above kStrMaxRatio
SG_STR_HD inline int str_ratio(int64_t up, int64_t down, StrRatio* r) {
  if (up <= 0 || down <= 0) return 1;
  if (up >= kStrLimit || down >= kStrLimit) return 2;
  const int64_t g = str_gcd(up, down);
  r->up = up / g;
  r->down = down / g;
  r->D = r->up > r->down ? r->up : r->down;
  const int64_t lo = r->up < r->down ? r->up : r->down;
  if (r->D > kStrMaxRatio * lo) return 3;
  return 0;
}
// ceil(n up / down) of a reduced ratio, or -1 where it reaches 2^31 (n >= 0). n = q down + rem:
// n up / down = q up + rem up / down, and neither term overflows below the limit.
SG_STR_HD inline int64_t str_n_out(int64_t n, const StrRatio& R) {
  if (n < 0) return -1;
  const int64_t q = n / R.down, rem = n % R.down;
  if (q >= kStrLimit) return -1;
  const int64_t whole = q * R.up;  // < 2^62
  const int64_t out = whole + (rem * R.up + R.down - 1) / R.down;
  return out >= kStrLimit ? -1 : out;
}
// the most taps an output sample has: the integers of an open interval of length 2 Z D / up
SG_STR_HD inline int64_t str_tap_count(const StrRatio& R) { return (2 * kStrZ * R.D + R.up - 1) / R.up; }

// The inputs [lo, hi] of output sample r: 0 <= m < n with |r down - m up| < Z D; hi < lo: none.
struct StrTaps {
  int64_t lo, hi;
};
SG_STR_HD inline StrTaps str_taps(int64_t r, const StrRatio& R, int64_t n) {
  const int64_t c = r * R.down, W = (int64_t)kStrZ * R.D;
  StrTaps t;
  t.lo = str_floordiv(c - W, R.up) + 1;    // m up > c - W
  t.hi = -str_floordiv(-(c + W), R.up) - 1;  // m up < c + W: m <= ceil((c + W) / up) - 1
  if (t.lo < 0) t.lo = 0;
  if (t.hi > n - 1) t.hi = n - 1;
  return t;
}

// sin(pi num / D) = sign sin(pi rem / D) with 0 <= rem <= D / 2 (rem = 0: a multiple of D)
struct StrRem {
  int64_t rem;
  int sign;
};
// from the residue v of num in [0, 2 D), which the resampler steps from tap to tap
SG_STR_HD inline StrRem str_fold2d(int64_t v, int64_t D) {
  StrRem s{v, 1};
  if (s.rem >= D) {  // sin(x + pi) = -sin x
    s.rem -= D;
    s.sign = -1;
  }
  if (2 * s.rem > D) s.rem = D - s.rem;  // sin(pi - x) = sin x
  return s;
}
SG_STR_HD inline StrRem str_mod2d(int64_t num, int64_t D) {
  int64_t v = num % (2 * D);
  if (v < 0) v += 2 * D;
  return str_fold2d(v, D);
}

// A position between two analysis frames. ok: q is a number in [0, F_in - 1].
SG_STR_HD inline bool str_position_ok(double q, int64_t F_in) { return F_in >= 1 && q >= 0.0 && q <= (double)(F_in - 1); }
struct StrSplit {
  int64_t i, i1, h;
  double a;
};
template <class Start>
SG_STR_HD inline StrSplit str_split(double q, int64_t F_in, Start start) {
  StrSplit s;
  const double fl = floor(q);
  s.i = (int64_t)fl;
  if (s.i > F_in - 1) s.i = F_in - 1;
  s.a = q - (double)s.i;
  s.i1 = s.i + 1 < F_in ? s.i + 1 : F_in - 1;
  s.h = start(s.i1) - start(s.i);
  return s;
}

// bytes of workspace a sound takes inside time_stretch: the bins + 1 complex bins of every input
// frame, and of every output frame with its wl windowed samples and its record
constexpr int kStrFrameRecord = 48;
SG_STR_HD inline int64_t str_workspace_bytes(int64_t frames_in, int64_t frames_out, int wl, int bins) {
  return frames_in * ((int64_t)(bins + 1) * 16) + frames_out * ((int64_t)(bins + 1) * 16 + (int64_t)wl * 8 + kStrFrameRecord);
}

}  // namespace sg
