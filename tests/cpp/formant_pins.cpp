// The host build of soundgen_beta_amd/csrc/sg_formants.h on frames dumped by tests/test_formants.py.
// Input (argv[1]): doubles in the machine's byte order: nframes, n, fs, nFormants, then nframes x n samples.
// Output: per frame one line: the iterations fmt_frame returns, then 2 nFormants values (%.17g; nan for NA).
#include <cstdio>
#include <vector>

#include "sg_formants.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  double head[4];
  if (std::fread(head, sizeof(double), 4, f) != 4) return 2;
  const int nframes = (int)head[0], n = (int)head[1], nF = (int)head[3];
  const double fs = head[2];
  const int p = sg::fmt_order(fs);
  if (nframes < 0 || p < 1 || p > sg::kFmtMaxOrder || n <= p || nF < 1 || nF > sg::kFmtMaxFormants) return 3;
  std::vector<double> x(n), y(n);
  sg::FmtShared sh;
  const sg::FmtHostOps ops;
  for (int i = 0; i < nframes; ++i) {
    if (std::fread(x.data(), sizeof(double), n, f) != (size_t)n) return 2;
    sg::fmt_lags_host(x.data(), n, fs, p, y.data(), sh.r);
    const int it = sg::fmt_frame(sh, p, fs, nF, 0, 1, ops);
    std::printf("%d", it);
    for (int c = 0; c < 2 * nF; ++c) std::printf(" %.17g", sh.out[c]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
