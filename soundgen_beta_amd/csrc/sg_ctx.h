// sg_ctx.h -- the device context behind the C ABI's sg_ctx handle (sg_api.cpp
// owns its life cycle; every entry point, in sg_api.cpp and in the .hip files of
// the analysis features, uses its stream and, through guarded() of sg_launch.h,
// its error text).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "sg_exec.h"

struct sg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;  // finalize stream of the slice pipeline
  std::string err;
  bool profiling = false;
  std::vector<sg::SgProfEvent> prof_events;
};
