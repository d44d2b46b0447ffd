// path_exact_pins — sg::path_sound (sg_path.h) with pathfinding 'exact' and the segment list compiled in
// (sg::kPathExact | sg::kPathSegs: what the 64 lanes of sg_anl_path_exact run), built for the host with one lane
// and a sync that does nothing, on candidate tables the test generates. Built with and without
// -fsanitize=address,undefined by tests/test_path_exact.py.
//
// usage: path_exact_pins FILE. A case of FILE: as for path_pins (tests/cpp/path_pins.cpp); pathfinding may be 0, 1
// or 3. Prints two lines per case: per frame pitch, dom, HNR, amplVoiced, voiced, quartile25; then per voiced
// segment its first frame, last frame, nrow and path cost. All as hex floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_path.h"

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
  double h[20];
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
    // exactly the cells the device gets: the sanitizer sees an access past any of the buffers
    std::vector<double> rows((size_t)frames * P.cols, NAN);
    std::vector<double> scr((size_t)frames * sg::path_scratch(P.nCands, P.pathfinding), NAN);
    std::vector<double> dd((size_t)2 * sg::path_width(P.nCands), NAN), segs((size_t)sg::path_seg_cells(frames), NAN);
    for (int r = 0; r < frames; ++r)
      for (int c = 0; c < in_cols; ++c)
        if (!rd(f, &rows[(size_t)r * P.cols + c])) return 3;
    double red[1];
    int64_t sh[3] = {0, 0, 0};
    segs[0] = 0;
    if (frames > 0)
      sg::path_sound<NoSync, sg::kPathExact | sg::kPathSegs>(P, frames, hw, rows.data(), scr.data(), 0, 1, red, sh, NoSync(),
                                                             dd.data(), segs.data());
    for (int r = 0; r < frames; ++r) {
      const double* row = &rows[(size_t)r * P.cols];
      std::printf("%a %a %a %a %a %a ", row[in_cols + sg::kPathPitch], row[sg::kPathDom], row[sg::kPathHNR],
                  row[in_cols + sg::kPathAmplVoiced], row[in_cols + sg::kPathVoiced], row[sg::kPathQ25]);
    }
    std::printf("\n");
    const int nseg = (int)segs[0];
    if (nseg < 0 || nseg > frames) return 4;
    for (int k = 0; k < nseg * sg::kPathSegCells; ++k) std::printf("%a ", segs[1 + k]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
