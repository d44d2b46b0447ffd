// path_at_pins — sg::path_sound_at (sg_path.h: what the lanes of sg_anl_sweep_path run, the
// candidates in a table apart that stays untouched) against sg::path_sound (the table rewritten
// in place), both compiled for the host with one lane and a sync that does nothing, on
// candidate tables the test generates. Built with and without -fsanitize=address,undefined by
// tests/test_analyze_sweep.py.
//
// usage: path_at_pins FILE. A case of FILE is path_pins' (numbers as C hex floats, "nan"):
//   nCands frames hw minVoiced noRequired nTolerated interpolWin pathfinding do_prior smooth_pitch smooth_dom
//   shape rate lconst prior_norm interpolTol interpolCert certWeight snakeStep smoothThres
//   frames * (15 + 6 nCands) cells, row after row
// Every buffer has exactly the cells the device gives it: the shared table frames * (15 + 6
// nCands), the pair's table frames * (15 + 6 nCands + 4), either scratch frames * path_stride().
// Prints one line per case (per frame pitch, dom, HNR, voiced as hex floats) and stops with
// status 1 at the first case whose tables differ in a bit or whose source table was touched.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sg_path.h"

static bool rd(FILE* f, double* v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

static bool same(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

struct NoSync {
  void operator()() const {}
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double h[20];
  long cases = 0;
  while (rd(f, &h[0])) {
    for (int i = 1; i < 20; ++i)
      if (!rd(f, &h[i])) return 3;
    sg::PathPars P;
    P.nCands = (int)h[0];
    const int frames = (int)h[1], hw = (int)h[2];
    if (P.nCands < 1 || P.nCands > 8 || frames < 0 || hw < 0) return 3;
    P.minVoiced = (int)h[3];
    P.noRequired = (int)h[4];
    P.nTolerated = (int)h[5];
    P.interpolWin = (int)h[6];
    P.pathfinding = (int)h[7];
    P.do_prior = (int)h[8];
    P.smooth_pitch = (int)h[9];
    P.smooth_dom = (int)h[10];
    P.shape = h[11];
    P.rate = h[12];
    P.lconst = h[13];
    P.prior_norm = h[14];
    P.interpolTol = h[15];
    P.interpolCert = h[16];
    P.certWeight = h[17];
    P.snakeStep = h[18];
    P.smoothThres = h[19];
    const int in_cols = sg::kPathFixed + 6 * P.nCands;
    P.cols = in_cols + sg::kPathCols;
    std::vector<double> src((size_t)frames * in_cols), in_place((size_t)frames * P.cols, NAN), pair((size_t)frames * P.cols, NAN);
    std::vector<double> scr1((size_t)frames * sg::path_stride(P.nCands), NAN), scr2(scr1);
    for (int r = 0; r < frames; ++r)
      for (int c = 0; c < in_cols; ++c) {
        if (!rd(f, &src[(size_t)r * in_cols + c])) return 3;
        in_place[(size_t)r * P.cols + c] = src[(size_t)r * in_cols + c];
      }
    const std::vector<double> before(src);
    double red[1];
    int64_t sh[3] = {0, 0, 0};
    if (frames > 0) {
      sg::path_sound(P, frames, hw, in_place.data(), scr1.data(), 0, 1, red, sh, NoSync());
      sg::path_sound_at(P, frames, hw, src.data(), in_cols, pair.data(), scr2.data(), 0, 1, red, sh, NoSync());
    }
    if (!same(src, before)) {
      std::fprintf(stderr, "case %ld: path_sound_at wrote to the source table\n", cases);
      return 1;
    }
    if (!same(in_place, pair)) {
      std::fprintf(stderr, "case %ld: path_sound_at differs from path_sound\n", cases);
      return 1;
    }
    for (int r = 0; r < frames; ++r) {
      const double* row = &pair[(size_t)r * P.cols];
      std::printf("%a %a %a %a ", row[in_cols + sg::kPathPitch], row[sg::kPathDom], row[sg::kPathHNR], row[in_cols + sg::kPathVoiced]);
    }
    std::printf("\n");
    ++cases;
  }
  std::fclose(f);
  return 0;
}
