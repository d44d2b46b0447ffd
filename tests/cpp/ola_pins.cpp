// ola_pins — sg_invert.h (the integer side of stft / istft / invert_spectrogram: what the lanes
// of sg_inv_ola run to find the frames that cover a sample) compiled for the host as a
// stand-alone program. Built with and without -fsanitize=address,undefined by
// tests/test_invert.py.
//
// Coverage against brute force -- for every sample t of the sound, the first and the last
// frame with s_i <= t < s_i + wl, or none -- over
//   wl 8, 44, 62;  len wl, wl + 1, wl + 7, 1000;  by 0.4, 1, 3.7, 20.8, wl, wl + 5
// (a fractional step, equal starts, a step longer than the window: uncovered samples, the tail
// behind the last frame, the clamp at len - wl), the starts read from a table sized exactly
// (the sanitizer sees a read past it). Then the sizes, worked out by hand.
// Prints "ok <cases> <samples>" and returns 0, or the first disagreement and 1.
#include <cstdio>
#include <vector>

#include "sg_invert.h"

static int fail(const char* what, int wl, long long len, double by, long long t, long long a, long long b) {
  std::printf("%s: wl %d len %lld by %g t %lld: %lld != %lld\n", what, wl, len, by, t, a, b);
  return 1;
}

int main() {
  long long cases = 0, samples = 0;
  for (int wl : {8, 44, 62}) {
    const long long lens[4] = {wl, wl + 1, wl + 7, 1000};
    const double bys[6] = {0.4, 1.0, 3.7, 20.8, (double)wl, (double)wl + 5};
    for (long long len : lens)
      for (double by : bys) {
        const int64_t F = sg::grid_frames(by, wl, len);
        if (F < 1) return fail("frames", wl, len, by, 0, F, 1);
        std::vector<int64_t> s((size_t)F);
        for (int64_t i = 0; i < F; ++i) {
          s[(size_t)i] = sg::grid_frame_start(by, wl, len, i);
          if (s[(size_t)i] < 0 || s[(size_t)i] + wl > len) return fail("start", wl, len, by, i, s[(size_t)i], len);
          if (i > 0 && s[(size_t)i] < s[(size_t)i - 1]) return fail("order", wl, len, by, i, s[(size_t)i], s[(size_t)i - 1]);
        }
        const int64_t* tab = s.data();
        for (int64_t t = 0; t < len; ++t) {
          int64_t first = 0, last = -1;
          bool any = false;
          for (int64_t i = 0; i < F; ++i)
            if (tab[i] <= t && t < tab[i] + wl) {
              if (!any) first = i;
              last = i;
              any = true;
            }
          const sg::InvCover c = sg::inv_cover(t, wl, F, by, [tab](int64_t i) { return tab[i]; });
          if (!any) {
            if (c.last >= c.first) return fail("uncovered", wl, len, by, t, c.first, c.last);
          } else if (c.first != first || c.last != last) {
            return fail(c.first != first ? "first" : "last", wl, len, by, t, c.first != first ? c.first : c.last,
                        c.first != first ? first : last);
          }
          ++samples;
        }
        ++cases;
      }
  }
  // by hand. len = wl: to = max(1, 0) = 1, one frame at 0. len = wl + 1: the same, sample wl uncovered.
  if (sg::grid_frames(3.7, 44, 44) != 1 || sg::grid_frames(3.7, 44, 45) != 1 || sg::grid_frame_start(3.7, 44, 45, 0) != 0) return 2;
  if (sg::grid_frames(3.7, 44, 43) != 0 || sg::grid_frames(1.0, 8, 1) != 0) return 2;
  // len = wl + 7: to = 7; by = 1: floor(6 / 1) + 1 = 7 frames at 0 .. 6; by = 3.7: floor(6 / 3.7) + 1 = 2 at 0 and floor(4.7) - 1 = 3
  if (sg::grid_frames(1.0, 44, 51) != 7 || sg::grid_frame_start(1.0, 44, 51, 6) != 6) return 3;
  if (sg::grid_frames(3.7, 44, 51) != 2 || sg::grid_frame_start(3.7, 44, 51, 1) != 3) return 3;
  // wl = 44, len = 1000, by = 20.8: to = 956, floor(955 / 20.8 = 45.9) + 1 = 46 frames; the last at floor(1 + 45 * 20.8 = 937) - 1
  if (sg::grid_frames(20.8, 44, 1000) != 46 || sg::grid_frame_start(20.8, 44, 1000, 45) != 936) return 4;
  // zp = 64 on wl = 44: pad 10, N = 64, 32 bins: 33 complex bins (528 B), 44 samples (352 B), two sums (16 B) per frame
  if (sg::inv_workspace_bytes(46, 44, 32) != 46 * 896 || sg::inv_workspace_bytes(0, 44, 32) != 0) return 5;
  if (!sg::inv_rows_ok(32, 32) || !sg::inv_rows_ok(33, 32) || sg::inv_rows_ok(34, 32) || sg::inv_rows_ok(31, 32)) return 5;
  std::printf("ok %lld %lld\n", cases, samples);
  return 0;
}
