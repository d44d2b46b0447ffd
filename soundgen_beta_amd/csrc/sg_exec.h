// sg_exec.h — device-side plan (HBM arena) and kernel launch sequence.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "sg_arena.h"
#include "sg_plan.h"

namespace sg {

// per-call 16-bit PCM conversion of a plan's output (sg_wav.hip); built on first use
struct PcmJob {
  char* buf = nullptr;
  SgPcmCall* calls = nullptr;
  SgPcmTile* tiles = nullptr;
  SgPcmStat* stats = nullptr;
  int64_t n = 0, ntiles = 0;
  void prepare(const int64_t* off, const int64_t* len, int64_t n_calls, hipStream_t s);
  void run(const void* in, bool f64, int mode, double nrange, int16_t* out, hipStream_t s) const;
  void free();
};

// What the launch sequence reads beside the arena: the slices, ranges, splits and
// LDS sizes of the plan. device_upload copies it from the Batch; with the section
// counts (DevicePlan::n) it is all that execution needs, so nothing of the host
// plan is read after the upload.
struct ExecInfo {
  std::vector<Slice> slices;
  std::vector<Batch::Copy> copies;  // fl -> fs before the filter phase
  int64_t ptile_hp = 0;             // first crossfade-piece tile of an fp64 syllable
  int64_t fgroup_range[2][3] = {{0, 0, 0}, {0, 0, 0}};
  int fgroup_lds[2][2] = {{0, 0}, {0, 0}};
  int64_t seg_range[2][2] = {{0, 0}, {0, 0}};
  int64_t olatile_split = 0, ola_split = 0;
  int64_t mixtile_hp = 0, mixtile_split = 0;
  int64_t frames64_noise = 0, frames64_w[2] = {0, 0};
  int32_t frames64_maxwl = 0;
  int64_t fe_base = 0;              // the envelope area of fl
};

// The arena pointers (sg_arena.h: one per section, D.segs, D.tasks, ...) and what
// belongs to an uploaded plan beside them
struct DevicePlan : ArenaPtrs {
  bool uploaded = false;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  ArenaCounts n;  // the elements each section was sized for at upload
  ExecInfo x;
  // the sine-bank task classes (sections tall, tlong, tshort, tallp, srun, trun, thp), built at upload
  std::vector<int32_t> tall_host, tlong_host, tshort_host, tallp_host, srun_host, trun_host, thp_host;
  // wavetable path (SgTabJob): tasks of long static-tone spans
  // (a separate allocation made at upload)
  char* tabbuf = nullptr;              // the wavetable spans' jobs (sg_sine_bank_tab)
  size_t tabbuf_bytes = 0;
  SgTabJob* tabjobs = nullptr;         // in task order
  std::vector<SgTabJob> tabjobs_host;
  int64_t tab_samples = 0, tab_terms = 0;  // samples and (sample, row) terms the tables stand in for
  PcmJob pcm;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

int64_t device_bytes(const Batch& B);
void device_upload(const Batch& B, DevicePlan& D, hipStream_t s);
void device_free(DevicePlan& D);
// HIP events bracketing one launch of a profiled kernel (SG_PROF_*), on its stream
struct SgProfEvent {
  int kernel;
  hipEvent_t e0, e1;
};
// One uploaded plan: its harmonic chain (per slice: sine banks, maxima, finalize)
// on s2 while s runs the envelopes and the noise phase; the pre-filter mixes on s
// wait for both (device_execute_many of one plan). prof (optional) receives one
// event pair per slice's sine banks and per sg_stft_ola launch, everything on s.
void device_execute(DevicePlan& D, float* d_out, hipStream_t s, hipStream_t s2, std::vector<SgProfEvent>* prof);
struct PlanRun {
  DevicePlan* D;
  float* out;
};
void device_execute_many(const std::vector<PlanRun>& runs, hipStream_t s, hipStream_t s2,
                         std::vector<SgProfEvent>* prof);
void device_execute_spec(const DevicePlan& D, float* d_out, hipStream_t s, std::vector<SgProfEvent>* prof,
                         bool join = false, hipEvent_t harm_done = nullptr);

// Test hook sg_debug_sine_bank (soundgen_hip.h) on stream s, after sine_bank_args_check
// (sg_sine_check.h); throws SgError
void debug_sine_bank(hipStream_t s, const SgWTask* tasks, int64_t ntasks, const float* amps, int64_t namps, int64_t wlen,
                     const SgTabJob* jobs, int64_t njobs, double env, float* W, double* W64, float* taskmax,
                     int32_t* cls);

// launchers (sg_harm.hip)
void launch_amp_build(const DevicePlan& D, int64_t n_jobs, hipStream_t s);
void launch_ugather(const SgUJob* jobs, int64_t n_jobs, const float* us, float* fl, hipStream_t s);
void launch_sine_bank(const DevicePlan& D, int64_t k0, int64_t n, hipStream_t s);
void launch_sine_bank_pairs(const DevicePlan& D, int64_t k0, int64_t n, hipStream_t s);
void launch_sine_bank_tall(const DevicePlan& D, int64_t k0, int64_t n, hipStream_t s);
void launch_sine_bank_tall_pairs(const DevicePlan& D, int64_t k0, int64_t n, hipStream_t s);
void launch_syl_max(const DevicePlan& D, int64_t s0, int64_t n_syls, hipStream_t s);
void launch_piece_max(const DevicePlan& D, int64_t p0, int64_t n_ptiles, hipStream_t s);
void launch_harm_finalize(const DevicePlan& D, int64_t f0, int64_t n_stiles, float* out, hipStream_t s);
void launch_harm_copy(const DevicePlan& D, int64_t c0, int64_t n_ctiles, float* out, hipStream_t s);
// the fp64 path of ill-conditioned formant-filter calls (SG_TASK_HP, SgSyllable::hp, sg_mix to fh, SgFrame64)
void launch_sine_bank_hp(const DevicePlan& D, int64_t n, hipStream_t s);
void launch_sine_bank_tab(const DevicePlan& D, int logn, int64_t j0, int64_t n, float* out, hipStream_t s);
void launch_piece_max_hp(const DevicePlan& D, int64_t p0, int64_t n_ptiles, hipStream_t s);
void launch_harm_finalize_hp(const DevicePlan& D, int64_t n_stiles, hipStream_t s);
void launch_mix_hp(const DevicePlan& D, int64_t t0, int64_t n_tiles, hipStream_t s);
void launch_fft_frames64(const DevicePlan& D, int ph, hipStream_t s);
// sg_fft.hip
void launch_fft_frames(const DevicePlan& D, int64_t g0, int64_t n_groups, int lds_bytes, hipStream_t s);
void launch_stft_ola(const DevicePlan& D, int phase, int64_t s0, int64_t n_segs, int lds_bytes, hipStream_t s);
void launch_ola(const DevicePlan& D, int64_t t0, int64_t n_tiles, hipStream_t s);
void launch_ola_max(const DevicePlan& D, int64_t o0, int64_t n_olas, hipStream_t s);
void launch_fft_probe(const SgFftGeom* geom, const float* fl, float* data, int M, int nframes, int inverse,
                      hipStream_t s);
void launch_mix(const DevicePlan& D, int64_t t0, int64_t n_tiles, float* out, hipStream_t s);
// sg_env.hip: every spectral-envelope job of the plan (getSpectralEnvelope)
void launch_spec_env(const DevicePlan& D, hipStream_t s);

}  // namespace sg
