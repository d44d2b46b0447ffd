// sine_bank_check — sg::sine_bank_args_check (sg_sine_check.h), the range check the test hook
// sg_debug_sine_bank makes before its first HIP call, alone on the host. Built with and
// without -fsanitize=address,undefined by tests/test_sine_bank.py: the check reads exactly
// the records it is given (each case's tasks and jobs sit in heap blocks of their own size,
// so a read past them is the sanitizer's to find) and forms no sum that overflows.
//
// usage: sine_bank_check FILE. FILE (native byte order): int64 ncases, then per case
//   int64 ntasks, namps, wlen, njobs; double env; ntasks records of SgWTask; njobs of SgTabJob.
// Prints one line per case: "ok", or the check's complaint.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "sg_sine_check.h"

template <class T>
static bool rd(FILE* f, T* v, size_t n) {
  return n == 0 || std::fread(v, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t ncases = 0;
  if (!rd(f, &ncases, 1) || ncases < 0 || ncases > 100000) return 2;
  for (int64_t c = 0; c < ncases; ++c) {
    int64_t h[4];
    double env;
    if (!rd(f, h, 4) || !rd(f, &env, 1) || h[0] < 0 || h[0] > 100000 || h[3] < 0 || h[3] > 100000) return 2;
    std::vector<SgWTask> tasks((size_t)h[0]);
    std::vector<SgTabJob> jobs((size_t)h[3]);
    if (!rd(f, tasks.data(), tasks.size()) || !rd(f, jobs.data(), jobs.size())) return 2;
    const char* why = sg::sine_bank_args_check(tasks.empty() ? nullptr : tasks.data(), h[0], h[1], h[2],
                                               jobs.empty() ? nullptr : jobs.data(), h[3], env);
    std::printf("%s\n", why ? why : "ok");
  }
  std::fclose(f);
  return 0;
}
