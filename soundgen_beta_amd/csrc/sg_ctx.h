// sg_ctx.h -- the device context behind the C ABI's sg_ctx handle (sg_api.cpp
// owns its life cycle; sg_ssm.hip's entry points use its stream and error text).
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
