// summary_pins — sg::sum_sound (sg_summary.h: analyze(summary = TRUE), what the 256 lanes of
// sg_anl_summary run) compiled for the host with one lane and a sync that does nothing, on
// tables the test generates. Built with and without -fsanitize=address,undefined by
// tests/test_analyze_summary.py.
//
// usage: summary_pins FILE. A case of FILE (numbers as C hex floats, "nan", "inf", "-inf"):
//   frames nCands len samplingRate
//   frames * (15 + 6 nCands + 4) cells, row after row
// Prints one line per case: the 44 cells of the row as hex floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_summary.h"

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
  double h[4];
  while (rd(f, &h[0])) {
    for (int i = 1; i < 4; ++i)
      if (!rd(f, &h[i])) return 3;
    const long long frames = (long long)h[0], len = (long long)h[2];
    const int nCands = (int)h[1];
    if (frames < 0 || nCands < 1 || nCands > 8) return 3;
    const int cols = 15 + 6 * nCands + 4;
    // exactly the cells the device gets: the sanitizer sees an access past either buffer
    std::vector<double> rows((size_t)frames * cols), out(sg::kSumCols, 0.0);
    for (double& v : rows)
      if (!rd(f, &v)) return 3;
    static sg::SumShared sh;
    sg::sum_sound(rows.data(), frames, cols, len, h[3], out.data(), 0, 1, sh, NoSync());
    for (double v : out) std::printf("%a ", v);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
