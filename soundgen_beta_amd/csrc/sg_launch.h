// sg_launch.h — what every host-side launch sequence (the synthesis executor sg_exec.cpp and
// its launchers; the analysis features sg_mel.hip, sg_ssm.hip, sg_spectrogram.hip, sg_analyze.hip,
// sg_segment.hip) and the C entry points (theirs and sg_api.cpp's) share: the HIP error check, the buffers of a
// launch sequence, the opt-in for dynamic LDS, what an entry point needs around its launch sequence (guarded,
// batch_args, with_samples, StageTimes; the exception ladder itself is sg_rmath.h's), the per-stage device
// clock and the single-sound round trip. Host code that needs the HIP runtime.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "sg_ctx.h"
#include "sg_rmath.h"
#include "soundgen_hip.h"

#define HIPCHK(x)                                                                                        \
  do {                                                                                                   \
    hipError_t _e = (x);                                                                                 \
    if (_e != hipSuccess) throw sg::SgError(SG_E_DEVICE, std::string(#x) + ": " + hipGetErrorString(_e)); \
  } while (0)

// after a kernel launch: launch failures (bad configuration, LDS over the opted-in size) are loud
#define SG_LAUNCHED(name)                                                                       \
  do {                                                                                          \
    const hipError_t _e = hipGetLastError();                                                    \
    if (_e != hipSuccess) throw sg::SgError(SG_E_DEVICE, std::string("launch " name ": ") + hipGetErrorString(_e)); \
  } while (0)

namespace sg {

// Device buffers of one launch sequence, and the host copies their uploads read: an
// async H2D copy from pageable memory may still be pending when the caller's
// vector goes away, so upload() stages the bytes in memory this object owns.
// The destructor frees the device buffers first (hipFree waits for the device),
// then the staged host bytes.
struct DevBuf {
  std::vector<void*> p;
  std::vector<std::vector<char>> host;
  template <class T>
  T* get(size_t n) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    p.push_back(q);
    return static_cast<T*>(q);
  }
  ~DevBuf() {
    for (void* q : p) (void)hipFree(q);
  }
};

template <class T>
T* upload(DevBuf& db, const std::vector<T>& v, hipStream_t s) {
  T* d = db.get<T>(v.size());
  if (!v.empty()) {
    const char* src = reinterpret_cast<const char*>(v.data());
    db.host.emplace_back(src, src + v.size() * sizeof(T));
    HIPCHK(hipMemcpyAsync(d, db.host.back().data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
  }
  return d;
}

// The one opt-in for dynamic LDS. A launch may ask for more dynamic LDS than the runtime grants a
// kernel by default (up to the 160 KB of a gfx950 CU) only after the kernel's function attribute
// for the largest dynamic size says so. So every launch with dynamic LDS states its size here
// first, whatever the size. The attribute is per device: the opted-in size is remembered per
// (kernel, device) and raised only when a launch needs more.
inline void lds_opt_in(const void* fn, int lds_bytes, const char* name) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) throw SgError(SG_E_DEVICE, std::string(name) + ": hipGetDevice failed");
  std::lock_guard<std::mutex> lk(mu);
  int& have = done[{fn, dev}];
  if (lds_bytes <= have) return;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess)
    throw SgError(SG_E_DEVICE, std::string(name) + ": dynamic LDS " + std::to_string(lds_bytes) + " B refused");
  have = lds_bytes;
}
template <class K>
void lds_opt_in(K* kernel, int lds_bytes, const char* name) {
  lds_opt_in(reinterpret_cast<const void*>(kernel), lds_bytes, name);
}

// The body of a C entry point with a context: sg::caught, the text left in ctx (when
// there is one) for sg_last_error
template <class F>
int guarded(sg_ctx* ctx, F&& f) {
  return caught(ctx ? &ctx->err : nullptr, f);
}

// What every batch entry point refuses as "`who`: bad arguments": a count that is negative or
// beyond 2^31 - 1, or a null among the pointers a non-empty batch needs
inline void batch_args(const char* who, int64_t n_calls, std::initializer_list<const void*> needed) {
  bool bad = n_calls < 0 || n_calls > 2147483647LL;
  for (const void* q : needed) bad = bad || (n_calls > 0 && !q);
  if (bad) bad_arguments(who);
}

// f(const double*) or f(const float*) on the samples at d_wave: f is a generic lambda
template <class F>
void with_samples(bool is_f64, const void* d_wave, F&& f) {
  if (is_f64)
    f(static_cast<const double*>(d_wave));
  else
    f(static_cast<const float*>(d_wave));
}

// The stage milliseconds of a feature's last profiled launch sequence, which its
// sg_debug_*_kernel_ms reader returns. Process-global because the readers take no context (the
// ABI): two contexts that profile at once overwrite each other.
template <int N>
struct StageTimes {
  double ms[N] = {};
  double* sink(const sg_ctx* ctx) { return ctx->profiling ? ms : nullptr; }
  int read(double* out) const {
    if (!out) return SG_E_ARG;
    std::copy(ms, ms + N, out);
    return SG_OK;
  }
};

// The device time of each stage of a launch sequence, between events on its stream
// (profiling only; ms == nullptr: every call is a no-op). stamp() at each stage
// boundary, in stage order; finish() once the stream is synchronised: ms[k] = the
// time between stamps k and k + 1, 0 for the stages that were not reached.
class StageClock {
 public:
  StageClock(hipStream_t s, double* ms, int nstages) : s_(s), ms_(ms), n_(nstages) {
    if (ms_) e_.reserve((size_t)n_ + 1);
  }
  StageClock(const StageClock&) = delete;
  StageClock& operator=(const StageClock&) = delete;
  ~StageClock() {
    for (hipEvent_t v : e_) (void)hipEventDestroy(v);
  }
  void zero() {
    for (int k = 0; ms_ && k < n_; ++k) ms_[k] = 0;
  }
  void stamp() {
    if (!ms_) return;
    hipEvent_t v;
    HIPCHK(hipEventCreate(&v));
    e_.push_back(v);
    HIPCHK(hipEventRecord(v, s_));
  }
  // A sequence that visits its stages many times and out of order (a sweep): what follows
  // this stamp, up to the next one, is added to ms[stage]; stage < 0: to none. Not to be
  // mixed with stamp() on one clock.
  void stamp(int stage) {
    if (!ms_) return;
    stamp();
    label_.push_back(stage);
  }
  void finish() {
    zero();
    if (!label_.empty()) {
      for (size_t k = 0; k + 1 < e_.size(); ++k) {
        float ms = 0;
        if (label_[k] < 0 || label_[k] >= n_) continue;
        HIPCHK(hipEventElapsedTime(&ms, e_[k], e_[k + 1]));
        ms_[label_[k]] += ms;
      }
      return;
    }
    for (int k = 0; k + 1 < (int)e_.size() && k < n_; ++k) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, e_[k], e_[k + 1]));
      ms_[k] = ms;
    }
  }

 private:
  hipStream_t s_;
  double* ms_;
  int n_;
  std::vector<hipEvent_t> e_;
  std::vector<int> label_;
};

// len doubles of host memory into a buffer of db, complete on return
inline double* upload_sound(DevBuf& db, const double* wave, int64_t len, hipStream_t s) {
  double* d = db.get<double>((size_t)len);
  HIPCHK(hipMemcpyAsync(d, wave, (size_t)len * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return d;
}

// One sound from host memory through a launch sequence that leaves `cells` doubles
// on the device: run(d_wave, d_out), then d_out to out
template <class F>
void single_sound(sg_ctx* ctx, const double* wave, int64_t len, int64_t cells, double* out, F&& run) {
  DevBuf db;
  const double* d = upload_sound(db, wave, len, ctx->stream);
  double* d_o = db.get<double>((size_t)cells);
  run(d, d_o);
  HIPCHK(hipMemcpy(out, d_o, (size_t)cells * sizeof(double), hipMemcpyDeviceToHost));
}

}  // namespace sg
