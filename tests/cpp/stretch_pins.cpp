// stretch_pins — sg_stretch.h (the integer side of time_stretch / shift_pitch / resample: what
// the lanes of sg_str_resample run to find their taps, and what the host runs to split a
// position between two analysis frames) compiled for the host as a stand-alone program. Built
// with and without -fsanitize=address,undefined by tests/test_stretch.py.
//
// Over the ratios 1:1, 3:2, 2:3, 1:64, 64:1, 160:147 and 4000:5480 (given unreduced where they
// reduce) and the lengths 1, 2, 33 and 1000, against brute force:
//   n_out = ceil(n up / down), by searching for the smallest r with r down >= n up;
//   the taps [lo, hi] of every output sample, by testing every m of the sound, read from a
//   table sized exactly (the sanitizer sees a read past it), and that the ends do not decrease
//   with r (the workgroup's span rests on it);
//   the reduction mod 2 D of every tap's numerator, against the definition in floating point;
//   the most taps a sample has.
// Then the position split at q = 0, an integer, F_in - 1 and one ulp either side of an integer,
// the refusals and the sizes, worked out by hand.
// Prints "ok <cases> <taps>" and returns 0, or the first disagreement and 1.
#include <cmath>
#include <cstdio>
#include <vector>

#include "sg_stretch.h"

static int fail(const char* what, long long up, long long down, long long n, long long r, long long a, long long b) {
  std::printf("%s: %lld:%lld n %lld r %lld: %lld != %lld\n", what, up, down, n, r, a, b);
  return 1;
}

int main() {
  const long long ratios[7][2] = {{1, 1}, {3, 2}, {2, 3}, {1, 64}, {64, 1}, {160, 147}, {4000, 5480}};
  const long long lens[4] = {1, 2, 33, 1000};
  long long cases = 0, taps = 0;
  for (const auto& q : ratios)
    for (long long n : lens) {
      sg::StrRatio R;
      if (sg::str_ratio(q[0], q[1], &R) != 0) return fail("ratio", q[0], q[1], n, 0, 1, 0);
      if (R.up * q[1] != R.down * q[0] || sg::str_gcd(R.up, R.down) != 1 || R.D != (R.up > R.down ? R.up : R.down))
        return fail("reduced", q[0], q[1], n, 0, R.up, R.down);
      long long want = 0;
      while (want * R.down < n * R.up) ++want;
      const long long n_out = sg::str_n_out(n, R);
      if (n_out != want) return fail("n_out", R.up, R.down, n, 0, n_out, want);
      std::vector<char> in((size_t)n, 1);  // the sound, sized exactly
      const char* tab = in.data();
      const long long W = (long long)sg::kStrZ * R.D;
      long long most = 0, plo = 0, phi = -1;
      for (long long r = 0; r < n_out; ++r) {
        long long lo = 0, hi = -1;
        bool any = false;
        for (long long m = 0; m < n; ++m) {
          const long long num = r * R.down - m * R.up;
          if (num > -W && num < W) {
            if (!any) lo = m;
            hi = m;
            any = true;
          }
        }
        const sg::StrTaps t = sg::str_taps(r, R, n);
        if (!any) return fail("no taps", R.up, R.down, n, r, t.lo, t.hi);  // every output sample has one
        if (t.lo != lo || t.hi != hi) return fail(t.lo != lo ? "lo" : "hi", R.up, R.down, n, r, t.lo != lo ? t.lo : t.hi, t.lo != lo ? lo : hi);
        if (t.lo < plo || t.hi < phi) return fail("order", R.up, R.down, n, r, t.lo, plo);
        plo = t.lo;
        phi = t.hi;
        if (hi - lo + 1 > most) most = hi - lo + 1;
        for (long long m = t.lo; m <= t.hi; ++m) {
          if (!tab[m]) return 1;
          const long long num = r * R.down - m * R.up;
          const sg::StrRem s = sg::str_mod2d(num, R.D);
          if (s.rem < 0 || 2 * s.rem > R.D || (s.sign != 1 && s.sign != -1)) return fail("rem", R.up, R.down, n, r, s.rem, R.D);
          // sign sin(pi rem / D) = sin(pi num / D): both sides in long double, the left on a small argument
          const long double pi = 3.14159265358979323846264338327950288L;
          const long double a = s.sign * sinl(pi * (long double)s.rem / (long double)R.D);
          const long double b = sinl(pi * (long double)(num % (2 * R.D)) / (long double)R.D);
          if (fabsl(a - b) > 1e-15L) return fail("mod 2D", R.up, R.down, n, r, num, s.rem);
          if (num % R.D == 0 && s.rem != 0) return fail("multiple of D", R.up, R.down, n, r, num, s.rem);
          ++taps;
        }
      }
      if (most > sg::str_tap_count(R)) return fail("tap count", R.up, R.down, n, 0, most, sg::str_tap_count(R));
      ++cases;
    }
  // by hand
  sg::StrRatio R;
  if (sg::str_ratio(4000, 5480, &R) != 0 || R.up != 100 || R.down != 137 || R.D != 137) return 2;
  if (sg::str_ratio(1, 64, &R) != 0 || sg::str_tap_count(R) != 2048 || sg::str_n_out(200, R) != 4) return 2;
  if (sg::str_ratio(64, 1, &R) != 0 || sg::str_tap_count(R) != 32 || sg::str_n_out(200, R) != 12800) return 2;
  if (sg::str_ratio(1, 65, &R) != 3 || sg::str_ratio(65, 1, &R) != 3 || sg::str_ratio(130, 2, &R) != 3) return 3;
  if (sg::str_ratio(0, 1, &R) != 1 || sg::str_ratio(1, -1, &R) != 1) return 3;
  if (sg::str_ratio(sg::kStrLimit, 1, &R) != 2 || sg::str_ratio(1, sg::kStrLimit, &R) != 2) return 3;
  if (sg::str_ratio(sg::kStrLimit - 1, sg::kStrLimit - 1, &R) != 0 || R.up != 1 || R.down != 1) return 3;
  if (sg::str_ratio(3, 2, &R) != 0) return 3;
  // 3 n / 2 reaches 2^31 at n = 1431655765 (ceil(2147483647.5)): refused; one sample fewer is 2^31 - 1
  if (sg::str_n_out(1431655765, R) != -1 || sg::str_n_out(1431655764, R) != 2147483646) return 4;
  if (sg::str_n_out((long long)1 << 62, R) != -1 || sg::str_n_out(-1, R) != -1 || sg::str_n_out(0, R) != 0) return 4;
  // 3:2, r = 10: c = 20, W = 48: m 3 in (-28, 68): m = -9 .. 22, clamped to the sound
  {
    const sg::StrTaps t = sg::str_taps(10, R, 1000), u = sg::str_taps(10, R, 5);
    if (t.lo != 0 || t.hi != 22 || u.lo != 0 || u.hi != 4) return 5;
    const sg::StrTaps v = sg::str_taps(100, R, 1000);  // c = 200: m 3 in (152, 248): 51 .. 82
    if (v.lo != 51 || v.hi != 82) return 5;
  }
  if (sg::str_floordiv(-7, 2) != -4 || sg::str_floordiv(7, 2) != 3 || sg::str_floordiv(-8, 2) != -4 || sg::str_floordiv(0, 5) != 0) return 5;
  // the position split over the starts 0, 5, 10, 15, 15 (the clamp repeats the last)
  {
    const int64_t s[5] = {0, 5, 10, 15, 15};
    const auto start = [&s](int64_t i) { return s[i]; };  // an index past 4 is a read past the table
    sg::StrSplit p = sg::str_split(0.0, 5, start);
    if (p.i != 0 || p.i1 != 1 || p.h != 5 || p.a != 0.0) return 6;
    p = sg::str_split(2.0, 5, start);
    if (p.i != 2 || p.i1 != 3 || p.h != 5 || p.a != 0.0) return 6;
    p = sg::str_split(4.0, 5, start);  // F_in - 1: i1 = i, h = 0
    if (p.i != 4 || p.i1 != 4 || p.h != 0 || p.a != 0.0) return 6;
    p = sg::str_split(3.0, 5, start);  // equal starts before the last frame: h = 0 with i1 > i
    if (p.i != 3 || p.i1 != 4 || p.h != 0) return 6;
    const double below = std::nextafter(2.0, 0.0), above = std::nextafter(2.0, 3.0);
    p = sg::str_split(below, 5, start);
    if (p.i != 1 || p.i1 != 2 || p.a != below - 1.0 || !(p.a < 1.0)) return 7;
    p = sg::str_split(above, 5, start);
    if (p.i != 2 || p.i1 != 3 || p.a != above - 2.0 || !(p.a > 0.0)) return 7;
    p = sg::str_split(0.25, 1, start);  // one frame: everything is frame 0 (0.25 is refused before, see below)
    if (p.i != 0 || p.i1 != 0 || p.h != 0) return 7;
    if (!sg::str_position_ok(0.0, 5) || !sg::str_position_ok(4.0, 5) || sg::str_position_ok(std::nextafter(4.0, 5.0), 5) ||
        sg::str_position_ok(-1e-300, 5) || sg::str_position_ok(NAN, 5) || sg::str_position_ok(0.25, 1) ||
        !sg::str_position_ok(0.0, 1) || sg::str_position_ok(0.0, 0))
      return 8;
  }
  // wl = 44, zp = 64: 32 bins, 33 complex bins (528 B) a frame; 10 frames in, 14 out: 10 * 528 + 14 * (528 + 352 + 48)
  if (sg::str_workspace_bytes(10, 14, 44, 32) != 10 * 528 + 14 * 928 || sg::str_workspace_bytes(0, 0, 44, 32) != 0) return 9;
  std::printf("ok %lld %lld\n", cases, taps);
  return 0;
}
