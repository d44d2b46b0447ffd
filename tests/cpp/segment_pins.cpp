// segment_pins — sg::seg_sound (sg_segment.h: segment() behind its envelope, what the 64
// lanes of sg_seg_tail run) compiled for the host with one lane and a sync that does
// nothing, on envelopes the test generates. Built with and without
// -fsanitize=address,undefined by tests/test_segment.py.
//
// usage: segment_pins FILE. A case of FILE (numbers as C hex floats, "nan" for NaN):
//   m timestep minCount sylThres shortestSyl shortestPause interburst interburstMult burstThres
//   peakToTrough troughLeft troughRight
//   m envelope values
// Prints one line per case: the 8 head cells, the 11 summary cells, rows x 5 syllable cells,
// bursts x 3 burst cells, as hex floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_segment.h"

static bool rd(FILE* f, double* v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

struct NoSync {
  void operator()() const {}
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double h[12];
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
    // exactly the cells the device gets: the sanitizer sees an access past the buffer
    std::vector<double> o((size_t)sg::seg_cells(m), NAN);
    for (int64_t i = 0; i < m; ++i)
      if (!rd(f, &o[(size_t)(sg::seg_env0() + i)])) return 3;
    double red[1];
    sg::seg_sound(P, h[1], (int64_t)h[2], m, o.data(), 0, 1, red, NoSync());
    for (int k = 0; k < sg::kSegHead + sg::kSegSummary; ++k) std::printf("%a ", o[k]);
    const int64_t rows = (int64_t)o[sg::kSegRows], nb = (int64_t)o[sg::kSegBursts];
    for (int64_t k = 0; k < 5 * rows; ++k) std::printf("%a ", o[(size_t)(sg::seg_syl0(m) + k)]);
    for (int64_t k = 0; k < 3 * nb; ++k) std::printf("%a ", o[(size_t)(sg::seg_bur0(m) + k)]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
