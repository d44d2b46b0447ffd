// sine_bank_layout — the size and the field offsets of the sine bank's descriptors
// SgWTask and SgTabJob (sg_dev.h) and the constants their test relies on, as the
// host compiler lays them out. tests/test_sine_bank.py builds this with g++ and
// compares the lines with its ctypes mirrors of the two records.
//
// Prints "NAME sizeof N", then "NAME FIELD OFFSET" per field in declaration order,
// then "const NAME VALUE" lines.
#include <cstddef>
#include <cstdio>

#include "sg_dev.h"

#define FIELD(S, f) std::printf(#S " " #f " %zu\n", offsetof(S, f))
#define CONST(c) std::printf("const " #c " %.17g\n", (double)(c))

int main() {
  std::printf("SgWTask sizeof %zu\n", sizeof(SgWTask));
  FIELD(SgWTask, w_off);
  FIELD(SgWTask, a_off);
  FIELD(SgWTask, d_off);
  FIELD(SgWTask, dk0);
  FIELD(SgWTask, c0);
  FIELD(SgWTask, c1);
  FIELD(SgWTask, c2);
  FIELD(SgWTask, c3);
  FIELD(SgWTask, c4);
  FIELD(SgWTask, invD);
  FIELD(SgWTask, rdx);
  FIELD(SgWTask, tc0);
  FIELD(SgWTask, xby);
  FIELD(SgWTask, mbase);
  FIELD(SgWTask, R);
  FIELD(SgWTask, j0);
  FIELD(SgWTask, len);
  FIELD(SgWTask, dj0);
  FIELD(SgWTask, dj1);
  FIELD(SgWTask, syl);
  FIELD(SgWTask, flags);
  FIELD(SgWTask, Rn);
  std::printf("SgTabJob sizeof %zu\n", sizeof(SgTabJob));
  FIELD(SgTabJob, a_off);
  FIELD(SgTabJob, Rn);
  FIELD(SgTabJob, t0);
  FIELD(SgTabJob, n);
  FIELD(SgTabJob, logn);
  FIELD(SgTabJob, syl);
  FIELD(SgTabJob, flags);
  CONST(SG_TASK_CONST);
  CONST(SG_TASK_LIN);
  CONST(SG_TASK_ENV);
  CONST(SG_TASK_HP);
  CONST(SG_TASK_MAX);
  CONST(SG_RUN_TASKS);
  CONST(SG_ROWS_F32);
  CONST(SG_TAB_TASKS);
  CONST(SG_TAB_LOGN_MIN);
  CONST(SG_TAB_LOGN_MAX);
  CONST(SG_TAB_TOL);
  return 0;
}
