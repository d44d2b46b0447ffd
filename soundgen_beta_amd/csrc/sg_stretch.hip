// sg_stretch.hip — time_stretch(), shift_pitch() and resample() on the device: a phase vocoder
// between the analysis operator A and its least-squares inverse A+ (sg_invert.hip, reached
// through sg_invert_ops.h: there is one A and one A+), and a band-limited resampler. fp64
// throughout, no floating-point atomics: a sound's samples have the same bits alone, in any
// batch, at any position and under any workspace cap. The operators are stated in
// soundgen_beta_amd/stretch.py and their integer side in sg_stretch.h.
//
// A spectrum is kept frame after frame, M + 1 bins a frame, so bins across lanes read and write
// coalesced; frames are the serial dimension of the phase sum.
//
//   sg_str_cells     one workgroup per output frame j, a lane per bin k: the magnitude m_j[k]
//                    interpolated between the analysis frames i and i1 of its position, and the
//                    deviation (d / h)_j[k] of its instantaneous frequency from the bin's own
//                    (two hypot, two atan2), left in X'_j[k] as (m, d / h)
//   sg_str_walk      one wave per 64 bins of a sound walks its output frames: psi_j = psi_j-1 +
//                    2 pi (k g_j mod N) / N + g_j (d / h)_j-1, wrapped after every step, and
//                    X'_j[k] = m_j[k] exp(i psi_j[k]) in place of sg_str_cells' (m, d / h). Only the
//                    phase sum is serial: the hypots and atan2s run across (frame, bin) in
//                    sg_str_cells. One kernel that walked and computed its cells itself was
//                    measured slower on a batch of short sounds and on one long recording alike
//                    (DESIGN.md section 5).
//   sg_str_resample  a lane per output sample, 256 a workgroup; the workgroup's contiguous input
//                    span is staged through LDS kStrSpan samples at a time, each lane adding the
//                    taps of its own window that fall inside, in ascending m
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sg_invert.h"
#include "sg_invert_ops.h"
#include "sg_launch.h"
#include "sg_rmath.h"
#include "sg_spectrogram.h"
#include "sg_stretch.h"

namespace {

using sg::DevBuf;
using sg::upload;

constexpr double kPi = 3.141592653589793238462643383279;
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr int kWave = 64;
constexpr int kT = 256;
static_assert(sg::kStrTile == kT, "a lane per output sample of a tile");

struct StrSound {
  int64_t xin0, xout0;  // first complex cell of its X (F_in frames) and of its X' (F_out frames)
  int64_t f0;           // its first record in the frame table
  int32_t nf, pad;      // F_out
};
struct StrFrame {  // output frame j of sound snd
  double a, h, g;  // the position's fraction; s_i1 - s_i; t_j - t_j-1 (0 for j = 0)
  int32_t i, i1;   // the analysis frames on either side of its position
  int32_t hmod, gmod;  // h mod N, g mod N: the index products stay in 32 bits
  int32_t snd, j;
};
static_assert(sizeof(StrFrame) == sg::kStrFrameRecord, "str_workspace_bytes counts the record");
struct StrWalk {
  int32_t snd, k0;  // bins [k0, k0 + 64) of the sound
};

__device__ inline double str_wrap(double v) {
#pragma clang fp contract(off)
  return v - kTwoPi * rint(v / kTwoPi);
}

struct StrCell {
  double m, dh;
};
__device__ inline StrCell str_cell(const double2* __restrict__ Xs, const StrFrame& R, int k, int M1, int N) {
#pragma clang fp contract(off)
  const double2 u = Xs[(int64_t)R.i * M1 + k], v = Xs[(int64_t)R.i1 * M1 + k];
  StrCell c;
  c.m = (1.0 - R.a) * hypot(u.x, u.y) + R.a * hypot(v.x, v.y);
  c.dh = 0.0;
  if (R.h > 0) {
    const double d = (atan2(v.y, v.x) - atan2(u.y, u.x)) - (kTwoPi * (double)((k * R.hmod) % N)) / (double)N;
    c.dh = str_wrap(d) / R.h;
  }
  return c;
}
__device__ inline double str_step(double psi, double dh_prev, const StrFrame& R, int k, int N) {
#pragma clang fp contract(off)
  const double v = (psi + (kTwoPi * (double)((k * R.gmod) % N)) / (double)N) + R.g * dh_prev;
  return str_wrap(v);
}

__global__ __launch_bounds__(kT) void sg_str_cells(const double2* __restrict__ Xin, const StrFrame* __restrict__ frames,
                                                   const StrSound* __restrict__ snds, int M1, int N,
                                                   double2* __restrict__ Xout) {
  const StrFrame R = frames[blockIdx.x];
  const StrSound S = snds[R.snd];
  const double2* Xs = Xin + S.xin0;
  double2* row = Xout + S.xout0 + (int64_t)R.j * M1;
  for (int k = threadIdx.x; k < M1; k += kT) {
    const StrCell c = str_cell(Xs, R, k, M1, N);
    row[k] = make_double2(c.m, c.dh);
  }
}

__global__ __launch_bounds__(kWave) void sg_str_walk(const double2* __restrict__ Xin, const StrFrame* __restrict__ frames,
                                                     const StrSound* __restrict__ snds, const StrWalk* __restrict__ walks,
                                                     int M1, int N, double2* __restrict__ Xout) {
  const StrWalk W = walks[blockIdx.x];
  const StrSound S = snds[W.snd];
  const int k = W.k0 + (int)threadIdx.x;
  if (k >= M1) return;
  const StrFrame* fr = frames + S.f0;
  const double2* Xs = Xin + S.xin0;
  double2* Y = Xout + S.xout0 + k;
  double psi = 0.0, dh = 0.0;
  for (int j = 0; j < S.nf; ++j) {
    const StrFrame R = fr[j];
    const double2 c = Y[(int64_t)j * M1];  // (m, d / h) of sg_str_cells
    if (j == 0) {
      const double2 u = Xs[(int64_t)R.i * M1 + k];
      psi = atan2(u.y, u.x);
    } else {
      psi = str_step(psi, dh, R, k, N);
    }
    dh = c.y;
    double sn, cs;
    sincos(psi, &sn, &cs);
    Y[(int64_t)j * M1] = make_double2(c.x * cs, c.x * sn);
  }
}

struct RsSound {
  int64_t xbase, n, obase, n_out;
  int64_t up, down, D;  // reduced
};
struct RsTile {
  int32_t snd, c;  // outputs [c kStrTile, (c + 1) kStrTile) of the sound
};

// the weight of the tap with numerator num, whose residue mod 2 D is v in [0, 2 D)
__device__ inline double str_weight(int64_t num, int64_t v, int64_t D, double gain) {
#pragma clang fp contract(off)
  if (num == 0) return gain;
  const sg::StrRem q = sg::str_fold2d(v, D);
  const double s = (double)q.sign * sin(kPi * (double)q.rem / (double)D);
  const double sinc = s / (kPi * (double)num / (double)D);
  const double hann = 0.5 * (1.0 + cos(kPi * (double)num / (double)(sg::kStrZ * D)));
  return gain * sinc * hann;
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_str_resample(const T* __restrict__ x, const RsSound* __restrict__ snds,
                                                      const RsTile* __restrict__ tiles, double* __restrict__ out) {
  __shared__ double seg[sg::kStrSpan];
  const RsTile J = tiles[blockIdx.x];
  const RsSound Q = snds[J.snd];
  const sg::StrRatio R{Q.up, Q.down, Q.D};
  const int64_t r0 = (int64_t)J.c * kT, r = r0 + threadIdx.x;
  const bool active = r < Q.n_out;
  const int64_t rl = r0 + kT - 1 < Q.n_out ? r0 + kT - 1 : Q.n_out - 1;  // host: r0 < n_out
  // the taps' ends do not decrease with r: the workgroup reads [lo_b, hi_b], inside [0, n)
  const int64_t lo_b = sg::str_taps(r0, R, Q.n).lo, hi_b = sg::str_taps(rl, R, Q.n).hi;
  sg::StrTaps t{0, -1};
  if (active) t = sg::str_taps(r, R, Q.n);
  const double gain = (double)Q.up / (double)Q.D;
  const int64_t D2 = 2 * Q.D, dv = Q.up % D2;
  double acc = 0.0;
  for (int64_t m0 = lo_b; m0 <= hi_b; m0 += sg::kStrSpan) {
    const int cnt = (int)(hi_b - m0 + 1 < sg::kStrSpan ? hi_b - m0 + 1 : sg::kStrSpan);
    for (int i = threadIdx.x; i < cnt; i += kT) seg[i] = (double)x[Q.xbase + m0 + i];
    __syncthreads();
    const int64_t ma = t.lo > m0 ? t.lo : m0, mb = t.hi < m0 + cnt - 1 ? t.hi : m0 + cnt - 1;
    if (ma <= mb) {
      int64_t num = r * Q.down - ma * Q.up;
      int64_t v = num % D2;
      if (v < 0) v += D2;
      for (int64_t m = ma; m <= mb; ++m) {
#pragma clang fp contract(off)
        acc = acc + seg[m - m0] * str_weight(num, v, Q.D, gain);
        num -= Q.up;
        v -= dv;
        if (v < 0) v += D2;
      }
    }
    __syncthreads();
  }
  if (active) out[Q.obase + r] = acc;
}

sg::StageTimes<sg::kStrStages> g_str_ms;  // of the last profiled launch sequence

struct StrCall {
  int64_t len, out_len;  // as given
  int32_t fin, fout;     // F_in; F_out, 0 for a sound without frames
};

// spectrogram()'s refusals are the caller's; these are the feature's own, all SG_E_ARG
std::vector<StrCall> str_calls(const sg::SpgSetup& S, const int64_t* lengths, const int64_t* out_lengths,
                               const double* positions, const int64_t* pos_off, const int64_t* pos_count, int64_t n_calls) {
  std::vector<StrCall> calls((size_t)n_calls);
  for (int64_t c = 0; c < n_calls; ++c) {
    StrCall& Q = calls[(size_t)c];
    Q.len = lengths[c] > 0 ? lengths[c] : 0;
    Q.out_len = out_lengths[c];
    const std::string who = "time_stretch: call " + std::to_string(c) + ": ";
    if (Q.out_len < 0) throw sg::SgError(SG_E_ARG, who + "a negative output length");
    Q.fin = sg::spg_frames(S, Q.len);
    Q.fout = 0;
    if (Q.fin == 0) continue;  // shorter than the window: no frames, a silent result (as sg_spg_stft_batch has it)
    Q.fout = sg::spg_frames(S, Q.out_len);
    if (Q.fout == 0)
      throw sg::SgError(SG_E_ARG, who + "an output of " + std::to_string(Q.out_len) + " samples is shorter than the window (" +
                                      std::to_string(S.wl) + ")");
    if (pos_count[c] != Q.fout)
      throw sg::SgError(SG_E_ARG, who + "an output of " + std::to_string(Q.out_len) + " samples has " + std::to_string(Q.fout) +
                                      " frames, not " + std::to_string(pos_count[c]) + " positions");
    for (int j = 0; j < Q.fout; ++j)
      if (!sg::str_position_ok(positions[pos_off[c] + j], Q.fin))
        throw sg::SgError(SG_E_ARG, who + "position " + std::to_string(j) + " is not in [0, " + std::to_string(Q.fin - 1) + "]");
  }
  return calls;
}

template <typename T>
void stretch_device(sg_ctx* ctx, const sg::SpgSetup& S, const T* d_x, const int64_t* offsets, const std::vector<StrCall>& calls,
                    const double* positions, const int64_t* pos_off, double* d_out, const int64_t* out_off, int64_t cap,
                    double2* d_spec, const int64_t* spec_off) {
  hipStream_t s = ctx->stream;
  const int64_t n_calls = (int64_t)calls.size();
  const int M1 = S.bins + 1, N = S.N;
  std::vector<int64_t> need((size_t)n_calls), len_in((size_t)n_calls), len_out((size_t)n_calls);
  for (int64_t c = 0; c < n_calls; ++c) {
    const StrCall& Q = calls[(size_t)c];
    need[(size_t)c] = sg::str_workspace_bytes(Q.fin, Q.fout, S.wl, S.bins);
    len_in[(size_t)c] = Q.fin ? Q.len : 0;
    len_out[(size_t)c] = Q.fin ? Q.out_len : 0;
  }
  const std::vector<int64_t> ends = sg::inv_chunk_ends(need, cap > 0 ? cap : sg::kInvWorkspaceCap);
  sg::StageClock clk(s, g_str_ms.sink(ctx), sg::kStrStages);
  clk.zero();
  // X, X' and the windowed frames of the largest chunk, once: every chunk reuses them
  int64_t max_in = 0, max_out = 0, max_ws = 0, c0 = 0;
  for (const int64_t c1 : ends) {
    int64_t fin = 0, fout = 0;
    for (int64_t c = c0; c < c1; ++c) {
      fin += calls[(size_t)c].fin;
      fout += calls[(size_t)c].fout;
    }
    max_in = std::max(max_in, fin * M1);
    max_out = std::max(max_out, fout * M1);
    max_ws = std::max(max_ws, fout * S.wl);
    c0 = c1;
  }
  DevBuf top;
  double2* d_Xin = top.get<double2>((size_t)max_in);
  double2* d_Xout = top.get<double2>((size_t)max_out);
  double* d_ws = top.get<double>((size_t)max_ws);
  c0 = 0;
  for (const int64_t c1 : ends) {
    std::vector<StrSound> snds((size_t)(c1 - c0));
    std::vector<StrFrame> fr;
    std::vector<StrWalk> walks;
    int64_t cells_in = 0, cells_out = 0, ws_cells = 0;
    for (int64_t c = c0; c < c1; ++c) {
      const StrCall& Q = calls[(size_t)c];
      StrSound& U = snds[(size_t)(c - c0)];
      U.xin0 = cells_in;  // sg_invert_ops.h's layout
      U.xout0 = cells_out;
      U.f0 = (int64_t)fr.size();
      U.nf = Q.fout;
      U.pad = 0;
      if ((int64_t)fr.size() + Q.fout > 2147483647LL || (int64_t)walks.size() + M1 / kWave + 1 > 2147483647LL)
        throw sg::SgError(SG_E_UNSUPPORTED, "time_stretch: the frames of one launch exceed 2^31");
      int64_t t_prev = 0;
      for (int j = 0; j < Q.fout; ++j) {
        const sg::StrSplit sp = sg::str_split(positions[pos_off[c] + j], (int64_t)Q.fin,
                                              [&](int64_t i) { return sg::spg_frame_start(S, Q.len, (int)i); });
        const int64_t t = sg::spg_frame_start(S, Q.out_len, j), g = j ? t - t_prev : 0;
        t_prev = t;
        if (sp.h < 0 || g < 0) throw sg::SgError(SG_E_DEVICE, "time_stretch: frame starts decrease");
        fr.push_back(StrFrame{sp.a, (double)sp.h, (double)g, (int32_t)sp.i, (int32_t)sp.i1, (int32_t)(sp.h % N),
                              (int32_t)(g % N), (int32_t)(c - c0), j});
      }
      if (Q.fout)
        for (int k0 = 0; k0 < M1; k0 += kWave) walks.push_back(StrWalk{(int32_t)(c - c0), k0});
      cells_in += (int64_t)Q.fin * M1;
      cells_out += (int64_t)Q.fout * M1;
      ws_cells += (int64_t)Q.fout * S.wl;
    }
    if (cells_in > max_in || cells_out > max_out || ws_cells > max_ws) throw sg::SgError(SG_E_DEVICE, "time_stretch: a chunk outgrows its buffers");
    DevBuf db;  // the chunk's tables
    for (int64_t c = c0; c < c1; ++c)  // a sound without frames: silence
      if (!calls[(size_t)c].fin && calls[(size_t)c].out_len > 0)
        HIPCHK(hipMemsetAsync(d_out + out_off[c], 0, (size_t)calls[(size_t)c].out_len * sizeof(double), s));
    if (!fr.empty()) {
      const StrSound* d_snd = upload(db, snds, s);
      const StrFrame* d_fr = upload(db, fr, s);
      const StrWalk* d_walk = upload(db, walks, s);
      clk.stamp(1);
      sg::inv_forward_launch<T>(S, d_x, offsets, len_in.data(), c0, c1, d_Xin, db, s);
      clk.stamp(2);
      hipLaunchKernelGGL(sg_str_cells, dim3((unsigned)fr.size()), dim3(kT), 0, s, d_Xin, d_fr, d_snd, M1, N, d_Xout);
      SG_LAUNCHED("sg_str_cells");
      hipLaunchKernelGGL(sg_str_walk, dim3((unsigned)walks.size()), dim3(kWave), 0, s, d_Xin, d_fr, d_snd, d_walk, M1, N, d_Xout);
      SG_LAUNCHED("sg_str_walk");
      if (d_spec)
        for (int64_t c = c0; c < c1; ++c)
          if (calls[(size_t)c].fout)
            HIPCHK(hipMemcpyAsync(d_spec + spec_off[c], d_Xout + snds[(size_t)(c - c0)].xout0,
                                  (size_t)calls[(size_t)c].fout * M1 * sizeof(double2), hipMemcpyDeviceToDevice, s));
      sg::inv_synthesis_launch(S, d_Xout, out_off, len_out.data(), c0, c1, d_ws, d_out, db, clk, s);
      clk.stamp(-1);
    }
    HIPCHK(hipStreamSynchronize(s));  // db goes away, and the next chunk writes the same buffers
    c0 = c1;
  }
  clk.finish();
}

struct RsPlan {
  std::vector<RsSound> snds;
  std::vector<RsTile> tiles;
};

RsPlan resample_plan(const int64_t* offsets, const int64_t* lengths, const int64_t* up, const int64_t* down,
                     const int64_t* out_off, int64_t n_calls) {
  RsPlan P;
  P.snds.resize((size_t)n_calls);
  for (int64_t c = 0; c < n_calls; ++c) {
    const std::string who = "resample: call " + std::to_string(c) + ": ";
    sg::StrRatio R;
    const int bad = sg::str_ratio(up[c], down[c], &R);
    if (bad == 1) throw sg::SgError(SG_E_ARG, who + "up and down are positive whole numbers");
    if (bad == 2) throw sg::SgError(SG_E_ARG, who + "up or down is 2^31 or more");
    if (bad == 3)
      throw sg::SgError(SG_E_ARG, who + "a ratio of " + std::to_string(R.up) + " : " + std::to_string(R.down) + " is beyond 1 : " +
                                      std::to_string(sg::kStrMaxRatio) + " (more than 2,048 taps a sample)");
    const int64_t n = lengths[c] > 0 ? lengths[c] : 0;
    const int64_t n_out = sg::str_n_out(n, R);
    if (n_out < 0) throw sg::SgError(SG_E_ARG, who + "the output has 2^31 samples or more");
    P.snds[(size_t)c] = RsSound{offsets ? offsets[c] : 0, n, out_off ? out_off[c] : 0, n_out, R.up, R.down, R.D};
    if ((int64_t)P.tiles.size() + n_out / kT + 1 > 2147483647LL)
      throw sg::SgError(SG_E_UNSUPPORTED, "resample: the tiles of one launch exceed 2^31");
    for (int64_t k = 0; k * kT < n_out; ++k) P.tiles.push_back(RsTile{(int32_t)c, (int32_t)k});
  }
  return P;
}

template <typename T>
void resample_device(sg_ctx* ctx, const RsPlan& P, const T* d_x, double* d_out) {
  hipStream_t s = ctx->stream;
  sg::StageClock clk(s, g_str_ms.sink(ctx), sg::kStrStages);
  clk.zero();
  if (P.tiles.empty()) return;
  DevBuf db;
  const RsSound* d_snd = upload(db, P.snds, s);
  const RsTile* d_tiles = upload(db, P.tiles, s);
  clk.stamp(0);
  hipLaunchKernelGGL(sg_str_resample<T>, dim3((unsigned)P.tiles.size()), dim3(kT), 0, s, d_x, d_snd, d_tiles, d_out);
  SG_LAUNCHED("sg_str_resample");
  clk.stamp(-1);
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
}

}  // namespace

using sg::guarded;

extern "C" {

int sg_time_stretch_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                          int64_t n_calls, const sg_spectrogram_params* p, const int64_t* out_lengths, const double* positions,
                          const int64_t* pos_off, const int64_t* pos_count, double* d_out, const int64_t* out_off,
                          int64_t workspace_cap, double* d_spec, const int64_t* spec_off) {
  return guarded(ctx, [&]() {
    if (!p) throw sg::SgError(SG_E_ARG, "sg_time_stretch_batch: bad arguments");
    const sg::SpgSetup S = sg::spg_setup(*p);  // spectrogram()'s refusals, before anything else
    if (workspace_cap < 0) sg::bad_arguments("sg_time_stretch_batch");
    sg::batch_args("sg_time_stretch_batch", n_calls, {lengths, out_lengths, positions, pos_off, pos_count});
    const std::vector<StrCall> calls = str_calls(S, lengths, out_lengths, positions, pos_off, pos_count, n_calls);
    if (!ctx || (d_spec && !spec_off)) sg::bad_arguments("sg_time_stretch_batch");
    sg::batch_args("sg_time_stretch_batch", n_calls, {d_wave, offsets, d_out, out_off});
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::with_samples(is_f64 != 0, d_wave, [&](auto* d_x) {
      stretch_device(ctx, S, d_x, offsets, calls, positions, pos_off, d_out, out_off, workspace_cap,
                     reinterpret_cast<double2*>(d_spec), spec_off);
    });
    return SG_OK;
  });
}

int sg_resample_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                      int64_t n_calls, const int64_t* up, const int64_t* down, double* d_out, const int64_t* out_off) {
  return guarded(ctx, [&]() {
    sg::batch_args("sg_resample_batch", n_calls, {lengths, up, down});
    const RsPlan P = resample_plan(offsets, lengths, up, down, out_off, n_calls);  // the refusals, before ctx is looked at
    if (!ctx) sg::bad_arguments("sg_resample_batch");
    sg::batch_args("sg_resample_batch", n_calls, {d_wave, offsets, d_out, out_off});
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::with_samples(is_f64 != 0, d_wave, [&](auto* d_x) { resample_device(ctx, P, d_x, d_out); });
    return SG_OK;
  });
}

int sg_stretch_size(int64_t len, const sg_spectrogram_params* p, int64_t out_len, int64_t up, int64_t down, int32_t* frames_in,
                    int32_t* frames_out, int64_t* workspace_bytes, int64_t* n_out, int64_t* taps) {
  return sg::host_guarded([&]() {
    if (len < 0) throw sg::SgError(SG_E_ARG, "sg_stretch_size: bad arguments");
    if (p) {
      if (!frames_in || !frames_out || !workspace_bytes) throw sg::SgError(SG_E_ARG, "sg_stretch_size: bad arguments");
      const sg::SpgSetup S = sg::spg_setup(*p);
      if (out_len < 0) throw sg::SgError(SG_E_ARG, "sg_stretch_size: bad arguments");
      *frames_in = sg::spg_frames(S, len);
      *frames_out = sg::spg_frames(S, out_len);
      *workspace_bytes = sg::str_workspace_bytes(*frames_in, *frames_out, S.wl, S.bins);
      return;
    }
    if (!n_out || !taps) throw sg::SgError(SG_E_ARG, "sg_stretch_size: bad arguments");
    const int64_t off = 0;
    const RsPlan P = resample_plan(&off, &len, &up, &down, &off, 1);
    *n_out = P.snds[0].n_out;
    *taps = sg::str_tap_count(sg::StrRatio{P.snds[0].up, P.snds[0].down, P.snds[0].D});
  });
}

const char* sg_stretch_size_error(void) { return sg::g_host_err.c_str(); }

int sg_debug_stretch_kernel_ms(double* out) { return g_str_ms.read(out); }

}  // extern "C"
