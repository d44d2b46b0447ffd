// sg_sine_check.h -- the range check of the test hook sg_debug_sine_bank (soundgen_hip.h),
// host only and free of the HIP runtime: sg_exec.cpp runs it before the hook's first HIP
// call, tests/cpp/sine_bank_check.cpp runs it alone (tests/test_sine_bank.py, with and
// without the sanitizers).
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <unordered_set>

#include "sg_dev.h"

namespace sg {

// What the sine-bank kernels index with a task's or a job's fields, checked on the
// host (no HIP call): nullptr when every record is in range, else what is not.
inline const char* sine_bank_args_check(const SgWTask* t, int64_t ntasks, int64_t namps, int64_t wlen,
                                        const SgTabJob* jobs, int64_t njobs, double env) {
  constexpr int64_t kMaxTasks = int64_t(1) << 20, kMaxElems = int64_t(1) << 26;
  if (!t || ntasks < 1 || ntasks > kMaxTasks) return "ntasks out of range";
  if (wlen < 1 || wlen > kMaxElems) return "wlen out of range";
  if (namps < 1 || namps > kMaxElems) return "namps out of range";
  if (njobs < 0 || njobs > ntasks || (njobs > 0 && !jobs)) return "njobs out of range";
  if (!std::isfinite(env)) return "env not finite";
  constexpr int32_t known = SG_TASK_CONST | SG_TASK_LIN | SG_TASK_ENV | SG_TASK_HP;
  std::unordered_set<int32_t> seen;  // the syllables closed so far
  for (int64_t i = 0; i < ntasks; ++i) {
    const SgWTask& T = t[i];
    if (T.len < 1 || T.len > SG_TASK_MAX) return "len outside 1..SG_TASK_MAX";
    if (T.R <= 0 || T.R % 16 != 0) return "R not a positive multiple of 16";
    if (T.Rn <= 0 || T.Rn > T.R || T.Rn % SG_ROW_CHUNK != 0) return "Rn not a multiple of 4 in (0, R]";
    if (T.j0 < 0) return "j0 negative";
    if (T.mbase < 0 || T.mbase > (1 << 30)) return "mbase outside 0..2^30";
    // w_off + j0 in [0, wlen - len] without forming a sum that can overflow
    if (T.w_off < -(int64_t)T.j0 || T.w_off > wlen - (int64_t)T.len - (int64_t)T.j0) return "samples outside the scratch";
    if (T.a_off < 0 || T.a_off > namps - (int64_t)T.R) return "a_off outside the amplitudes";
    if (T.d_off < 0 || T.d_off > namps - (int64_t)T.R) return "d_off outside the amplitudes";
    if (T.dj0 < 0 || T.dj0 > T.dj1) return "window not 0 <= dj0 <= dj1";
    if (T.syl < 0) return "syl negative";
    if (T.flags & ~known) return "unknown flag";
    if ((T.flags & SG_TASK_ENV) && (T.flags & SG_TASK_LIN)) return "SG_TASK_ENV with SG_TASK_LIN";
    for (double c : {T.c0, T.c1, T.c2, T.c3, T.c4, T.invD, (double)T.rdx, (double)T.tc0, (double)T.xby})
      if (!std::isfinite(c)) return "coefficient not finite";
    if (i > 0 && T.syl != t[i - 1].syl) {
      seen.insert(t[i - 1].syl);
      if (seen.count(T.syl)) return "tasks of one syllable apart";
    }
  }
  int64_t next = 0;  // first task past the job before
  for (int64_t q = 0; q < njobs; ++q) {
    const SgTabJob& J = jobs[q];
    if (J.flags != 0) return "job flags not 0";
    if (J.n < 1 || J.n > SG_TAB_TASKS) return "job n outside 1..SG_TAB_TASKS";
    if (J.t0 < next || (int64_t)J.t0 + J.n > ntasks) return "job tasks out of range or not ascending";
    if (J.logn < SG_TAB_LOGN_MIN || J.logn > SG_TAB_LOGN_MAX) return "job logn out of range";
    if (J.Rn < 4 || J.Rn > SG_ROWS_F32) return "job Rn outside 4..SG_ROWS_F32";
    if (J.a_off < 0 || J.a_off > namps - (int64_t)J.Rn) return "job a_off outside the amplitudes";
    for (int64_t i = J.t0; i < (int64_t)J.t0 + J.n; ++i)
      if (t[i].flags != (SG_TASK_CONST | SG_TASK_LIN) || t[i].R > SG_ROWS_F32 || t[i].a_off != J.a_off || t[i].Rn != J.Rn)
        return "job task not CONST | LIN on the job's column";
    next = (int64_t)J.t0 + J.n;
  }
  return nullptr;
}

}  // namespace sg
