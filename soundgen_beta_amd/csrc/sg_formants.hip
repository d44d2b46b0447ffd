// sg_formants.hip — the formant tracks of analyze() on the device (R/analyze.R:486-502;
// phonTools::findformants restated in sg_formants.h, PARITY UNPINNED), fp64 throughout.
// For every frame that passed cond_silence, from the finished table of analyze_frames,
// pitch_candidates or analyze (all three keep cond_silence in column sg::kCondSilence):
//   sg_fmt_lags   one 256-lane workgroup per frame: the windowed frame rebuilt as
//                 sg_anl_acf rebuilds it, pre-emphasis, minus the mean, the Hann window, then
//                 r[0..order] by direct sums. A lag's sum is split into kLagSegs segments of
//                 ceil(n / kLagSegs) terms; a thread sums one segment of four consecutive
//                 lags in index order, and one thread per lag folds its segment sums in index
//                 order: the order depends on n and the lag alone, so a frame's bits are the
//                 same alone and in any batch
//   sg_fmt_roots  one wave per frame, kRootWaves waves per workgroup, lane j holding root j
//                 (sg::fmt_frame): Levinson-Durbin across the lanes, the Aberth-Ehrlich
//                 iteration with the coefficients and the other roots broadcast from LDS,
//                 the conversion, the rank-counting sort and the selection. The waves of a
//                 workgroup never meet: every synchronisation is the wave's own
// A frame that Levinson-Durbin refuses or that hits the iteration cap gets a NaN row.
// findformants on a whole sound (matchPars' initial formants) does not fit that LDS:
// sg_fmt_sound_* below cut the sound into chunks and feed the same sg_fmt_roots.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "sg_analyze.h"
#include "sg_dev64.h"
#include "sg_formants.h"
#include "sg_launch.h"

namespace {

using sg::DevBuf;
using sg::SpgStat;
using sg::upload;

constexpr int kT = 256;
constexpr int kLagSegs = 16;   // segments of a lag's sum
constexpr int kLagPad = 3;     // zeros behind the frame: the later lags of a group of four run into them
constexpr int kRootWaves = 4;  // frames per workgroup of sg_fmt_roots
constexpr int kFmtStages = 2;  // sg_debug_formants_kernel_ms
constexpr int kMaxFrame = 2 * sg::kSpgMaxBins;  // the longest window of spectrogram(); the frame stays in LDS

struct FmtFrame {
  int64_t x0;    // first sample of the frame in the input buffer
  int64_t gate;  // the double that holds the frame's cond_silence in the tables; -1: no gate
  int64_t out;   // first double of its row in the formant buffer
  int32_t snd, pad;
};

// the launch's counters
struct FmtCount {
  unsigned long long capped, analysed, iterations;
};

struct FmtK {
  int n, order, nFormants, windowed;  // windowed: samples are normalised and multiplied by win[]
  double fs, coeff;
};

template <typename T>
__device__ __forceinline__ double fmt_sample(const T* xc, int i, const SpgStat& st, const double* __restrict__ win, int windowed) {
  const double s = (double)xc[i];
  return windowed ? sg::spg_normalise(s, st) * win[i] : s;
}

// LDS: n + kLagPad doubles (the frame), 4 * ceil((order + 1) / 4) * kLagSegs doubles (the segment sums)
template <typename T>
__global__ __launch_bounds__(kT) void sg_fmt_lags(const T* __restrict__ x, const FmtFrame* __restrict__ frames,
                                                  const SpgStat* __restrict__ stat, const double* __restrict__ win,
                                                  const double* __restrict__ tables, FmtK K, double* __restrict__ lags) {
  extern __shared__ double lds_fmt[];
  __shared__ double red[kT];
  const FmtFrame F = frames[blockIdx.x];
  if (F.gate >= 0 && tables[F.gate] != 1.0) return;  // workgroup-uniform
  const int n = K.n, p = K.order;
  double* y = lds_fmt;
  double* part = lds_fmt + n + kLagPad;
  SpgStat st = sg::kSpgStatIdentity;
  if (K.windowed) st = stat[F.snd];
  const T* xc = x + F.x0;  // host: the frame's n samples lie in the buffer
  double acc = 0;
  if (threadIdx.x < kLagPad) y[n + threadIdx.x] = 0.0;
  for (int i = threadIdx.x; i < n; i += kT) {
    const double cur = fmt_sample(xc, i, st, win, K.windowed);
    const double prev = i ? fmt_sample(xc, i - 1, st, win, K.windowed) : 0.0;
    const double v = sg::fmt_preemph(cur, prev, i, K.coeff);
    y[i] = v;
    acc += v;
  }
  const double mean = block_reduce<kT>(acc, 0, red) / (double)n;
  for (int i = threadIdx.x; i < n; i += kT) y[i] = sg::fmt_shape(y[i], mean, i, n);
  __syncthreads();
  const int G = (p + 4) / 4;            // groups of four lags covering 0..p
  const int L = (n + kLagSegs - 1) / kLagSegs;  // terms of a segment
  for (int t = threadIdx.x; t < G * kLagSegs; t += kT) {
    const int g = t / kLagSegs, s = t % kLagSegs;
    const int k = 4 * g;
    const int i0 = s * L, i1 = min(i0 + L, n - k);  // reads up to y[i1 - 1 + k + 3] <= y[n + 2]
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int i = i0; i < i1; ++i) {
      const double a = y[i];
      const double* q = y + i + k;
      s0 += a * q[0];
      s1 += a * q[1];
      s2 += a * q[2];
      s3 += a * q[3];
    }
    double* o = part + (size_t)k * kLagSegs + s;
    o[0] = s0;
    o[kLagSegs] = s1;
    o[2 * kLagSegs] = s2;
    o[3 * kLagSegs] = s3;
  }
  __syncthreads();
  if ((int)threadIdx.x <= p) {
    const double* q = part + (size_t)threadIdx.x * kLagSegs;
    double s = 0;
    for (int j = 0; j < kLagSegs; ++j) s += q[j];
    lags[(int64_t)blockIdx.x * (sg::kFmtMaxOrder + 1) + threadIdx.x] = s;
  }
}

// the wave's own synchronisation, sum and vote
struct WaveOps {
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __device__ __forceinline__ double sum(double v) const { return wsum(v); }
  __device__ __forceinline__ bool all(bool b) const { return __all(b ? 1 : 0) != 0; }
};

__global__ __launch_bounds__(kRootWaves * 64) void sg_fmt_roots(const FmtFrame* __restrict__ frames, int nframes,
                                                                const double* __restrict__ tables,
                                                                const double* __restrict__ lags, FmtK K,
                                                                double* __restrict__ out, FmtCount* __restrict__ count) {
  __shared__ sg::FmtShared shared[kRootWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = blockIdx.x * kRootWaves + wave;
  if (f >= nframes) return;  // wave-uniform, as every branch below
  const FmtFrame F = frames[f];
  double* row = out + F.out;
  const int cols = 2 * K.nFormants;
  if (F.gate >= 0 && tables[F.gate] != 1.0) {
    if (lane < cols) row[lane] = NAN;
    return;
  }
  sg::FmtShared& sh = shared[wave];
  const WaveOps ops;
  const double* r = lags + (int64_t)f * (sg::kFmtMaxOrder + 1);
  for (int k = lane; k <= K.order; k += 64) sh.r[k] = r[k];
  ops.sync();
  const int it = sg::fmt_frame(sh, K.order, K.fs, K.nFormants, lane, 64, ops);
  if (lane < cols) row[lane] = sh.out[lane];
  if (lane == 0) {
    atomicAdd(&count->analysed, 1ull);
    if (it < 0) atomicAdd(&count->capped, 1ull);
    atomicAdd(&count->iterations, (unsigned long long)(it < 0 ? sg::kFmtMaxIter : it));
  }
}

sg::StageTimes<kFmtStages> g_fmt_ms;  // of the last profiled run
int64_t g_fmt_count[3];       // of the last run: capped, analysed, iterations

// The two kernels on the context's stream for the frames in fr; synchronises
template <typename T>
void formants_launch(const T* d_x, const std::vector<FmtFrame>& fr, const SpgStat* d_stat, const double* d_win,
                     const double* d_tables, const FmtK& K, double* d_fmt, hipStream_t s, double* kernel_ms) {
  sg::StageClock clk(s, kernel_ms, kFmtStages);
  clk.zero();
  for (int k = 0; k < 3; ++k) g_fmt_count[k] = 0;
  const int64_t F = (int64_t)fr.size();
  if (F == 0) return;
  if (F > 2147483647LL) throw sg::SgError(SG_E_UNSUPPORTED, "formants: the frames of one launch exceed 2^31");
  if (K.order < 1 || K.order > sg::kFmtMaxOrder || K.n <= K.order || K.nFormants < 1 || K.nFormants > sg::kFmtMaxFormants)
    throw sg::SgError(SG_E_DEVICE, "formants: the setup leaves the wave");  // the entry points refuse these
  if (K.n > kMaxFrame) throw sg::SgError(SG_E_UNSUPPORTED, "formants: a frame may have at most 4096 samples");
  DevBuf db;
  const FmtFrame* d_fr = upload(db, fr, s);
  double* d_lags = db.get<double>((size_t)F * (sg::kFmtMaxOrder + 1));
  FmtCount* d_count = upload(db, std::vector<FmtCount>(1, FmtCount{0, 0, 0}), s);
  const int G = (K.order + 4) / 4;
  const int lds = (K.n + kLagPad + 4 * G * kLagSegs) * (int)sizeof(double);  // under 48 KiB for n <= kMaxFrame
  clk.stamp();  // 0: the lags
  hipLaunchKernelGGL(sg_fmt_lags<T>, dim3((unsigned)F), dim3(kT), (size_t)lds, s, d_x, d_fr, d_stat, d_win, d_tables, K, d_lags);
  HIPCHK(hipGetLastError());
  clk.stamp();  // 1: the predictor, the roots, the formants
  hipLaunchKernelGGL(sg_fmt_roots, dim3((unsigned)((F + kRootWaves - 1) / kRootWaves)), dim3(kRootWaves * 64), 0, s, d_fr,
                     (int)F, d_tables, d_lags, K, d_fmt, d_count);
  HIPCHK(hipGetLastError());
  clk.stamp();
  FmtCount h{0, 0, 0};
  HIPCHK(hipMemcpyAsync(&h, d_count, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
  g_fmt_count[0] = (int64_t)h.capped;
  g_fmt_count[1] = (int64_t)h.analysed;
  g_fmt_count[2] = (int64_t)h.iterations;
}

FmtK make_k(int n, int order, int nFormants, int windowed, double fs) {
  FmtK K;
  K.n = n;
  K.order = order;
  K.nFormants = nFormants;
  K.windowed = windowed;
  K.fs = fs;
  K.coeff = sg::fmt_preemph_coeff(fs);
  return K;
}

// The formant tables of n_calls sounds behind their finished tables (all in device memory)
template <typename T>
void formants_device(const sg::AnlSetup& A, int order, int nFormants, const T* d_x, const int64_t* offsets,
                     const int64_t* lengths, int64_t n_calls, const double* d_tables, const int64_t* out_off, int table_cols,
                     const int32_t* frames, double* d_fmt, const int64_t* fmt_off, hipStream_t s, double* kernel_ms) {
  const int wl = A.spg.wl;
  std::vector<FmtFrame> fr;
  std::vector<int64_t> lens(n_calls);
  for (int64_t c = 0; c < n_calls; ++c) {
    const int nf = sg::anl_frames(A, lengths[c]);
    if (frames[c] != nf && frames[c] != 0)
      throw sg::SgError(SG_E_ARG, "formants: frames[" + std::to_string((long long)c) + "] is not the frame count of the call");
    lens[c] = frames[c] ? lengths[c] : 0;
    for (int f = 0; f < frames[c]; ++f) {
      const int64_t o = sg::spg_frame_start(A.spg, lengths[c], f);
      if (o < 0 || o + wl > lengths[c]) throw sg::SgError(SG_E_DEVICE, "formants: a frame leaves its sound");
      fr.push_back(FmtFrame{offsets[c] + o, out_off[c] + (int64_t)f * table_cols + sg::kCondSilence,
                            fmt_off[c] + (int64_t)f * 2 * nFormants, (int32_t)c, 0});
    }
  }
  if (fr.empty()) {
    formants_launch<T>(d_x, fr, nullptr, nullptr, d_tables, make_k(wl, order, nFormants, 1, A.spg.sr), d_fmt, s, kernel_ms);
    return;
  }
  DevBuf db;
  SpgStat* d_stat = db.get<SpgStat>((size_t)n_calls);
  sg::spg_stats_device<T>(d_x, offsets, lens.data(), n_calls, d_stat, s);
  const double* d_win = upload(db, sg::spg_window(wl, A.spg.wn), s);
  formants_launch<T>(d_x, fr, d_stat, d_win, d_tables, make_k(wl, order, nFormants, 1, A.spg.sr), d_fmt, s, kernel_ms);
}

// ---------------------------------------------------------------- a whole sound
// findformants on all N samples of a sound (matchPars, R/matchPars.R:130). The frame no longer
// fits LDS, so the sound is cut into chunks of kC = sg::kFmtSoundChunk samples:
//   sg_fmt_sound_sums   one workgroup per chunk: the sum of its pre-emphasised samples
//   sg_fmt_sound_mean   one thread per sound: its chunks' sums in chunk order, over N
//   sg_fmt_sound_lags   one workgroup per chunk: the chunk and a halo of order + kSndPad
//                       samples behind it, shaped with the sample's index in the sound (zeros
//                       past the sound's end), into LDS; then the chunk's part of r[0..order]
//   sg_fmt_sound_fold   one workgroup per sound: lag k over its chunks in chunk order, into
//                       the row sg_fmt_roots reads; a sound not longer than the order gets NaN
//   sg_fmt_roots        as for frames, gate -1, nFormants = kFmtMaxFormants
// sg_fmt_sound_lags: the lags go in groups of kSndW = 8, G = ceil((order + 1) / 8) of them, and
// the chunk's samples in S = 256 / G segments of L = ceil(kC / S) | 1 samples (odd: the lanes'
// segment starts then fall on different LDS banks). Thread t < G S sums segment t % S of lag
// group t / S in index order, the eight lags' window sliding through registers (2 LDS reads
// for 8 multiply-adds); thread k <= order then folds lag k's S segment sums in index order.
// Every order depends on (N, order, kC) alone: no atomics, the same bits in any batch.
constexpr int kC = sg::kFmtSoundChunk;
constexpr int kSndW = sg::kFmtSoundLagWidth;  // lags of a group
constexpr int kSndPad = kSndW - 1;        // the last group's later lags run this far behind the halo
constexpr int kSndY = kC + sg::kFmtMaxOrder + kSndPad + 1;  // doubles of the shaped chunk
constexpr int kSndGroupsMax = (sg::kFmtMaxOrder + kSndW) / kSndW;
constexpr int kSndPart = kSndW * kT + kSndW * kSndGroupsMax;  // kSndW G (S | 1) <= this
constexpr int kFmtWholeStages = 4;        // sg_debug_formants_whole_kernel_ms
static_assert(kT == sg::kFmtSoundThreads &&(kSndY + kSndPart + kT) * sizeof(double) <= 65536, "sg_fmt_sound_lags: LDS");

struct FmtChunk {
  int64_t x0;  // first sample of the chunk's sound in the input buffer
  int64_t n;   // samples of that sound
  int64_t i0;  // first sample of the chunk in the sound
  int32_t snd, pad;
};

struct FmtSound {
  int64_t n;       // samples; analysed when n > order
  int64_t chunk0;  // its first chunk in the launch
  int32_t chunks;
  int32_t row;     // its row of lags (the frame index of sg_fmt_roots); -1: not analysed
};

// pre-emphasised sample i of the sound at xs
template <typename T>
__device__ __forceinline__ double snd_preemph(const T* __restrict__ xs, int64_t i, double coeff) {
  const double cur = (double)xs[i];
  return i == 0 ? cur : cur + coeff * (double)xs[i - 1];
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_fmt_sound_sums(const T* __restrict__ x, const FmtChunk* __restrict__ chunks,
                                                        double coeff, double* __restrict__ sums) {
  __shared__ double red[kT];
  const FmtChunk Q = chunks[blockIdx.x];
  const T* xs = x + Q.x0;
  const int nc = (int)min((int64_t)kC, Q.n - Q.i0);
  double acc = 0;
  for (int l = threadIdx.x; l < nc; l += kT) acc += snd_preemph(xs, Q.i0 + l, coeff);
  const double s = block_reduce<kT>(acc, 0, red);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

__global__ __launch_bounds__(kT) void sg_fmt_sound_mean(const FmtSound* __restrict__ sounds, int nsounds,
                                                        const double* __restrict__ sums, double* __restrict__ mean) {
  const int c = blockIdx.x * kT + threadIdx.x;
  if (c >= nsounds) return;
  const FmtSound Sd = sounds[c];
  double s = 0;
  for (int j = 0; j < Sd.chunks; ++j) s += sums[Sd.chunk0 + j];
  mean[c] = Sd.n > 0 ? s / (double)Sd.n : 0.0;
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_fmt_sound_lags(const T* __restrict__ x, const FmtChunk* __restrict__ chunks,
                                                        const double* __restrict__ mean, int p, double coeff,
                                                        double* __restrict__ partial) {
  __shared__ double y[kSndY];
  __shared__ double part[kSndPart];
  const FmtChunk Q = chunks[blockIdx.x];
  const T* xs = x + Q.x0;
  const double mu = mean[Q.snd];
  const int nc = (int)min((int64_t)kC, Q.n - Q.i0);  // samples of the chunk, >= 1
  const int G = sg::fmt_sound_groups(p);             // groups of kSndW lags covering 0..p
  const int S = sg::fmt_sound_segments(p);           // segments of the chunk
  const int L = sg::fmt_sound_seglen(p);             // samples of a segment
  const int PS = S | 1;                              // a lag's row of segment sums
  const int ny = kC + p + kSndPad + 1;               // what the sums below may read: <= kSndY
  for (int l = threadIdx.x; l < ny; l += kT) {
    const int64_t i = Q.i0 + l;
    y[l] = i < Q.n ? sg::fmt_shape(snd_preemph(xs, i, coeff), mu, i, Q.n) : 0.0;  // nothing past the sound's end
  }
  __syncthreads();
  if ((int)threadIdx.x < G * S) {
    const int g = threadIdx.x / S, s = threadIdx.x % S;
    const int i0 = min(s * L, nc), i1 = min(i0 + L, nc);
    const double* q = y + kSndW * g;  // reads up to q[i1 - 1 + kSndPad] = y[<= nc - 1 + p + kSndPad]
    double acc[kSndW], w[kSndW];
#pragma unroll
    for (int j = 0; j < kSndW; ++j) acc[j] = 0;
#pragma unroll
    for (int j = 0; j < kSndPad; ++j) w[j] = q[i0 + j];
#pragma unroll 8
    for (int i = i0; i < i1; ++i) {
      const double a = y[i];
      w[kSndPad] = q[i + kSndPad];
#pragma unroll
      for (int j = 0; j < kSndW; ++j) acc[j] += a * w[j];
#pragma unroll
      for (int j = 0; j < kSndPad; ++j) w[j] = w[j + 1];
    }
    double* o = part + (kSndW * g) * PS + s;
#pragma unroll
    for (int j = 0; j < kSndW; ++j) o[j * PS] = acc[j];
  }
  __syncthreads();
  if ((int)threadIdx.x <= p) {
    const double* o = part + threadIdx.x * PS;
    double s = 0;
    for (int j = 0; j < S; ++j) s += o[j];
    partial[(int64_t)blockIdx.x * (sg::kFmtMaxOrder + 1) + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(128) void sg_fmt_sound_fold(const FmtSound* __restrict__ sounds, const double* __restrict__ partial,
                                                         int p, double* __restrict__ lags, double* __restrict__ out) {
  const FmtSound Sd = sounds[blockIdx.x];
  const int k = threadIdx.x;
  if (Sd.row < 0) {
    if (k < 2 * sg::kFmtMaxFormants) out[(int64_t)blockIdx.x * 2 * sg::kFmtMaxFormants + k] = NAN;
    return;
  }
  if (k > p) return;
  const double* q = partial + Sd.chunk0 * (sg::kFmtMaxOrder + 1) + k;
  double s = 0;
  for (int j = 0; j < Sd.chunks; ++j) s += q[(int64_t)j * (sg::kFmtMaxOrder + 1)];
  lags[(int64_t)Sd.row * (sg::kFmtMaxOrder + 1) + k] = s;
}

sg::StageTimes<kFmtWholeStages> g_fmtw_ms;  // of the last profiled run
int64_t g_fmtw_count[3];            // of the last run: capped, analysed, iterations

// the order of findformants at fs; refuses what the wave cannot hold
int whole_order(double fs) {
  if (!(fs > 0) || !(fs < 1e9)) throw sg::SgError(SG_E_ARG, "formants: fs must be positive");
  const int order = sg::fmt_order(fs);
  if (order > sg::kFmtMaxOrder)
    throw sg::SgError(SG_E_UNSUPPORTED, "formants: the order round(fs / 1000) + 3 = " + std::to_string(order) + " exceeds " +
                                            std::to_string(sg::kFmtMaxOrder) + " (one root per lane of a wave)");
  return order;
}

int64_t whole_chunks(int64_t len) {
  const int64_t nc = sg::fmt_sound_chunks(len);
  if (nc > 2147483647LL) throw sg::SgError(SG_E_UNSUPPORTED, "formants: the chunks of a sound exceed 2^31");
  return nc;
}

// The five kernels on the stream for n_calls sounds of d_x; rows of 16 doubles to d_out; synchronises
template <typename T>
void formants_whole_device(const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls, int order, double fs,
                           double* d_out, hipStream_t s, double* kernel_ms) {
  sg::StageClock clk(s, kernel_ms, kFmtWholeStages);
  clk.zero();
  for (int k = 0; k < 3; ++k) g_fmtw_count[k] = 0;
  if (n_calls == 0) return;
  std::vector<FmtSound> snd((size_t)n_calls);
  std::vector<FmtChunk> ch;
  std::vector<FmtFrame> fr;
  for (int64_t c = 0; c < n_calls; ++c) {
    const int64_t n = lengths[c];
    if (n <= order) {
      snd[c] = FmtSound{n, (int64_t)ch.size(), 0, -1};
      continue;
    }
    const int64_t nc = whole_chunks(n);
    snd[c] = FmtSound{n, (int64_t)ch.size(), (int32_t)nc, (int32_t)fr.size()};
    if ((int64_t)ch.size() + nc > 2147483647LL) throw sg::SgError(SG_E_UNSUPPORTED, "formants: the chunks of one launch exceed 2^31");
    for (int64_t j = 0; j < nc; ++j) ch.push_back(FmtChunk{offsets[c], n, j * kC, (int32_t)c, 0});
    fr.push_back(FmtFrame{offsets[c], -1, c * 2 * sg::kFmtMaxFormants, (int32_t)c, 0});
  }
  const int64_t F = (int64_t)fr.size(), NC = (int64_t)ch.size();
  const FmtK K = make_k(0, order, sg::kFmtMaxFormants, 0, fs);
  DevBuf db;
  const FmtSound* d_snd = upload(db, snd, s);
  const FmtChunk* d_ch = upload(db, ch, s);
  const FmtFrame* d_fr = upload(db, fr, s);
  double* d_sums = db.get<double>((size_t)NC);
  double* d_mean = db.get<double>((size_t)n_calls);
  double* d_part = db.get<double>((size_t)NC * (sg::kFmtMaxOrder + 1));
  double* d_lags = db.get<double>((size_t)F * (sg::kFmtMaxOrder + 1));
  FmtCount* d_count = upload(db, std::vector<FmtCount>(1, FmtCount{0, 0, 0}), s);
  clk.stamp();  // 0: the mean
  if (NC > 0) {
    hipLaunchKernelGGL(sg_fmt_sound_sums<T>, dim3((unsigned)NC), dim3(kT), 0, s, d_x, d_ch, K.coeff, d_sums);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(sg_fmt_sound_mean, dim3((unsigned)((n_calls + kT - 1) / kT)), dim3(kT), 0, s, d_snd, (int)n_calls, d_sums,
                       d_mean);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();  // 1: the chunks' lags
  if (NC > 0) {
    hipLaunchKernelGGL(sg_fmt_sound_lags<T>, dim3((unsigned)NC), dim3(kT), 0, s, d_x, d_ch, d_mean, order, K.coeff, d_part);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();  // 2: their fold, and the NaN rows
  hipLaunchKernelGGL(sg_fmt_sound_fold, dim3((unsigned)n_calls), dim3(128), 0, s, d_snd, d_part, order, d_lags, d_out);
  HIPCHK(hipGetLastError());
  clk.stamp();  // 3: the predictor, the roots, the formants
  if (F > 0) {
    hipLaunchKernelGGL(sg_fmt_roots, dim3((unsigned)((F + kRootWaves - 1) / kRootWaves)), dim3(kRootWaves * 64), 0, s, d_fr, (int)F,
                       (const double*)nullptr, d_lags, K, d_out, d_count);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();
  FmtCount h{0, 0, 0};
  HIPCHK(hipMemcpyAsync(&h, d_count, sizeof h, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
  g_fmtw_count[0] = (int64_t)h.capped;
  g_fmtw_count[1] = (int64_t)h.analysed;
  g_fmtw_count[2] = (int64_t)h.iterations;
}

}  // namespace

extern "C" {

int sg_formants_whole_size(double fs, int64_t len, int32_t* order, int32_t* chunk, int64_t* nchunks) {
  return sg::guarded(nullptr, [&]() {
    if (!order || !chunk || !nchunks) throw sg::SgError(SG_E_ARG, "sg_formants_whole_size: bad arguments");
    *order = whole_order(fs);
    *chunk = kC;
    *nchunks = whole_chunks(len);
    return (int)SG_OK;
  });
}

int sg_formants_whole(sg_ctx* ctx, const double* wave, int64_t len, double fs, double* out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_formants_whole: bad arguments");
    const int order = whole_order(fs);
    if (len <= order)
      throw sg::SgError(SG_E_ARG, "sg_formants_whole: the sound must have more than order = " + std::to_string(order) + " samples");
    whole_chunks(len);
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t off = 0;
    sg::single_sound(ctx, wave, len, 2 * sg::kFmtMaxFormants, out, [&](const double* d, double* d_o) {
      formants_whole_device<double>(d, &off, &len, 1, order, fs, d_o, ctx->stream, g_fmtw_ms.sink(ctx));
    });
    return (int)SG_OK;
  });
}

int sg_formants_whole_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                            double fs, double* d_out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx) sg::bad_arguments("sg_formants_whole_batch");
    sg::batch_args("sg_formants_whole_batch", n_calls, {d_wave, offsets, lengths, d_out});
    const int order = whole_order(fs);
    for (int64_t c = 0; c < n_calls; ++c) whole_chunks(lengths[c]);
    if (n_calls == 0) return (int)SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    formants_whole_device<float>(d_wave, offsets, lengths, n_calls, order, fs, d_out, ctx->stream, g_fmtw_ms.sink(ctx));
    return (int)SG_OK;
  });
}

int sg_debug_formants_whole_kernel_ms(double* out, int64_t* counts) {
  for (int k = 0; out && counts && k < 3; ++k) counts[k] = g_fmtw_count[k];
  return g_fmtw_ms.read(out);
}

int sg_formants_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                      const sg_analyze_params* p, int32_t nFormants, const double* d_tables, const int64_t* out_off,
                      int32_t table_cols, const int32_t* frames, double* d_fmt, const int64_t* fmt_off) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || !p || table_cols <= sg::kCondSilence) sg::bad_arguments("sg_formants_batch");
    sg::batch_args("sg_formants_batch", n_calls, {d_wave, offsets, lengths, d_tables, out_off, frames, d_fmt, fmt_off});
    const int order = sg::formants_order(p->samplingRate, nFormants);
    const sg::AnlSetup S = sg::anl_setup_any(*p);
    sg::formants_window(S.spg.wl, order);
    if (n_calls == 0) return (int)SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    formants_device<float>(S, order, nFormants, d_wave, offsets, lengths, n_calls, d_tables, out_off, table_cols, frames, d_fmt,
                           fmt_off, ctx->stream, g_fmt_ms.sink(ctx));
    return (int)SG_OK;
  });
}

int sg_formants_sound(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params* p, int32_t nFormants, double* out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_formants_sound: bad arguments");
    const int order = sg::formants_order(p->samplingRate, nFormants);
    const sg::AnlSetup S = sg::anl_setup(*p);
    sg::formants_window(S.spg.wl, order);
    if (len <= S.spg.wl)
      throw sg::SgError(SG_E_ARG, "sg_formants_sound: the sound is not longer than the window (the reference's amplitude window "
                                  "sound[a:(a + wl)] leaves it)");
    HIPCHK(hipSetDevice(ctx->device));
    const int32_t nf = sg::anl_frames(S, len);
    const int64_t off = 0;
    DevBuf db;
    const double* d = sg::upload_sound(db, wave, len, ctx->stream);
    double* d_t = db.get<double>((size_t)nf * S.cols);
    double* d_f = db.get<double>((size_t)nf * 2 * nFormants);
    int32_t f = 0;
    sg::analyze_device<double>(S, d, &off, &len, 1, d_t, &off, &f, ctx->stream, nullptr);  // the gate
    formants_device<double>(S, order, nFormants, d, &off, &len, 1, d_t, &off, S.cols, &f, d_f, &off, ctx->stream,
                            g_fmt_ms.sink(ctx));
    HIPCHK(hipMemcpy(out, d_f, (size_t)nf * 2 * nFormants * sizeof(double), hipMemcpyDeviceToHost));
    return (int)SG_OK;
  });
}

int sg_formants_frames(sg_ctx* ctx, const double* frames, int32_t n, int32_t nframes, double fs, int32_t nFormants,
                       double* out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || nframes < 0 || (nframes > 0 && (!frames || !out))) throw sg::SgError(SG_E_ARG, "sg_formants_frames: bad arguments");
    const int order = sg::formants_order(fs, nFormants);
    if (n <= order || n > kMaxFrame)
      throw sg::SgError(SG_E_ARG, "sg_formants_frames: a frame must have more than order = " + std::to_string(order) +
                                      " and at most " + std::to_string(kMaxFrame) + " samples");
    if (nframes == 0) return (int)SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf db;
    const double* d = sg::upload_sound(db, frames, (int64_t)nframes * n, ctx->stream);
    double* d_f = db.get<double>((size_t)nframes * 2 * nFormants);
    std::vector<FmtFrame> fr(nframes);
    for (int32_t f = 0; f < nframes; ++f) fr[f] = FmtFrame{(int64_t)f * n, -1, (int64_t)f * 2 * nFormants, 0, 0};
    formants_launch<double>(d, fr, nullptr, nullptr, nullptr, make_k(n, order, nFormants, 0, fs), d_f, ctx->stream,
                            g_fmt_ms.sink(ctx));
    HIPCHK(hipMemcpy(out, d_f, (size_t)nframes * 2 * nFormants * sizeof(double), hipMemcpyDeviceToHost));
    return (int)SG_OK;
  });
}

int sg_debug_formants_kernel_ms(double* out, int64_t* counts) {
  for (int k = 0; out && counts && k < 3; ++k) counts[k] = g_fmt_count[k];
  return g_fmt_ms.read(out);
}

}  // extern "C"
