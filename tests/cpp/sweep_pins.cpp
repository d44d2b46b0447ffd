// sweep_pins — sg::seg_sound_at (sg_segment.h: what the lanes of sg_seg_sweep_tail run, the
// envelope held apart from the pair's cells) against sg::seg_sound (the envelope inside the
// sound's cells), both compiled for the host with one lane and a sync that does nothing, on
// envelopes the test generates; and sg::seg_min_count against the count the test made.
// Built with and without -fsanitize=address,undefined by tests/test_optimize.py.
//
// usage: sweep_pins FILE. A case of FILE is segment_pins' (numbers as C hex floats, "nan"):
//   m timestep minCount sylThres shortestSyl shortestPause interburst interburstMult burstThres
//   peakToTrough troughLeft troughRight
//   m envelope values
// Every buffer has exactly the cells the device gives it: the envelope m, the pair
// seg_pair_cells(m), the summary 11. Prints one line per case, the 11 summary cells as hex
// floats, and stops with status 1 at the first cell that differs from seg_sound's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sg_segment.h"

static bool rd(FILE* f, double* v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

static bool same(const double* a, const double* b, int64_t n) {
  return n <= 0 || std::memcmp(a, b, (size_t)n * sizeof(double)) == 0;  // bit for bit, NaN included
}

struct NoSync {
  void operator()() const {}
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double h[12];
  int64_t cases = 0;
  while (rd(f, &h[0])) {
    for (int i = 1; i < 12; ++i)
      if (!rd(f, &h[i])) return 3;
    const int64_t m = (int64_t)h[0];
    if (m < 0 || m > (1 << 24)) return 3;
    sg::SegPars P;
    P.sylThres = h[3];
    P.shortestSyl = h[4];
    P.shortestPause = h[5];
    P.interburst = h[6];
    P.interburstMult = h[7];
    P.burstThres = h[8];
    P.peakToTrough = h[9];
    P.troughLeft = (int)h[10];
    P.troughRight = (int)h[11];
    std::vector<double> o((size_t)sg::seg_cells(m), NAN), env((size_t)m), pair((size_t)sg::seg_pair_cells(m), NAN),
        sum((size_t)sg::kSegSummary, NAN);
    for (int64_t i = 0; i < m; ++i) {
      if (!rd(f, &env[(size_t)i])) return 3;
      o[(size_t)(sg::seg_env0() + i)] = env[(size_t)i];
    }
    const int64_t minCount = m > 0 ? sg::seg_min_count(P.shortestSyl, h[1]) : 0;
    if (m > 0 && minCount != (int64_t)h[2]) {
      std::fprintf(stderr, "case %lld: seg_min_count %lld, the test's %lld\n", (long long)cases, (long long)minCount,
                   (long long)h[2]);
      return 1;
    }
    double red[1];
    sg::seg_sound(P, h[1], (int64_t)h[2], m, o.data(), 0, 1, red, NoSync());
    sg::seg_sound_at(P, h[1], minCount, m, env.data(), pair.data(), sum.data(), pair.data() + sg::seg_pair_syl0(),
                     pair.data() + sg::seg_pair_bur0(m), pair.data() + sg::seg_pair_scr0(m), 0, 1, red, NoSync());
    const int64_t rows = (int64_t)o[sg::kSegRows], nb = (int64_t)o[sg::kSegBursts];
    if (!same(o.data(), pair.data(), sg::kSegHead) || !same(o.data() + sg::kSegHead, sum.data(), sg::kSegSummary) ||
        !same(o.data() + sg::seg_syl0(m), pair.data() + sg::seg_pair_syl0(), 5 * rows) ||
        !same(o.data() + sg::seg_bur0(m), pair.data() + sg::seg_pair_bur0(m), 3 * nb)) {
      std::fprintf(stderr, "case %lld: seg_sound_at differs from seg_sound\n", (long long)cases);
      return 1;
    }
    for (int k = 0; k < sg::kSegSummary; ++k) std::printf("%a ", sum[(size_t)k]);
    std::printf("\n");
    ++cases;
  }
  std::fclose(f);
  return 0;
}
