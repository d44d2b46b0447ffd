// bana_pins — sg::bana_candidates (sg_bana.h: getPitchSpec's candidate logic, the
// function one thread of sg_anl_bana runs) compiled for the host, against cases the
// test worked out with the numpy restatement. Built with -fsanitize=address,undefined
// by tests/test_pitch_candidates.py.
//
// usage: bana_pins FILE. A line of FILE (numbers as C hex floats):
//   npeaks  f_1 .. f_min(npeaks, 5)  pitchFloor pitchCeiling specSinglePeakCert specThres specMerge nCands
//   m  cand_1 .. cand_m  cert_1 .. cert_m
// Prints "cases N bad K"; a case is bad when the count differs or a value is off by
// more than 1e-15 relative (both sides run the same operations in fp64).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sg_bana.h"

static bool rd(FILE* f, double* v) {
  char tok[64];
  if (std::fscanf(f, "%63s", tok) != 1) return false;
  *v = std::strtod(tok, nullptr);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  long cases = 0, bad = 0;
  double v;
  while (rd(f, &v)) {
    const int npeaks = (int)v;
    const int have = npeaks < sg::kBanaPeaks ? npeaks : sg::kBanaPeaks;
    std::vector<double> pf(have > 0 ? have : 1, 0.0);  // exactly `have` values: the sanitizer sees a read past them
    for (int i = 0; i < have; ++i)
      if (!rd(f, &pf[i])) return 3;
    double a[6];
    for (double& x : a)
      if (!rd(f, &x)) return 3;
    const sg::BanaPars P{a[0], a[1], a[2], a[3], a[4], (int)a[5]};
    if (!rd(f, &v)) return 3;
    const int m = (int)v;
    std::vector<double> want(2 * (m > 0 ? m : 0) + 1);
    for (int i = 0; i < 2 * m; ++i)
      if (!rd(f, &want[i])) return 3;
    std::vector<double> cand(P.nCands, NAN), cert(P.nCands, NAN);  // nCands slots, as a row of the table has
    const int got = sg::bana_candidates(pf.data(), npeaks, P, cand.data(), cert.data());
    bool ok = got == m;
    for (int i = 0; ok && i < m; ++i) {
      ok = std::fabs(cand[i] - want[i]) <= 1e-15 * std::fabs(want[i]) &&
           std::fabs(cert[i] - want[m + i]) <= 1e-15 * std::fabs(want[m + i]);
    }
    if (!ok) {
      ++bad;
      if (bad <= 5) std::fprintf(stderr, "case %ld: got %d candidates, want %d\n", cases, got, m);
    }
    ++cases;
  }
  std::fclose(f);
  std::printf("cases %ld bad %ld\n", cases, bad);
  return bad ? 1 : 0;
}
