// sg_invert.hip — stft(), istft() and invert_spectrogram() on the device: the analysis
// operator A of spectrogram() with its phases kept, its least-squares inverse A+, and the
// alternating projections between the range of A and a set of prescribed magnitudes
// (Griffin & Lim 1984) on top of the two. fp64 throughout, on the shared transform
// (sg_fft64_dev.h) and bound by SpgSetup (sg_spectrogram.h): the arguments, limits and
// refusals are spectrogram()'s. The operator is stated in sg_invert.h.
//
// A spectrum is kept frame after frame, `rows` bins a frame (rows = M: the reference's
// shape, or M + 1 with the Nyquist bin), complex cells as double2.
//
//   sg_inv_stft     one workgroup per frame: sg_spg_frames' body (spg_forward_frame,
//                   sg_spectrogram_dev.h) storing X_k, k < rows, as double2
//   sg_inv_project  the same transform of the iteration's sound (no normalisation: that
//                   belongs to spectrogram()'s input, not to A) with the projection fused
//                   behind it: X = S Z / |Z| on a constrained bin (X = S where |Z| = 0), X = Z
//                   on the Nyquist bin of an M-row matrix; and the frame's sums of (|Z| - S)^2
//                   and S^2 over its constrained bins, reduced in a fixed order
//   sg_inv_fold     one wave per sound adds its frames' two sums in a fixed order:
//                   e = sqrt(sum (|Z| - S)^2 / sum S^2)
//   sg_inv_start    X_0 = S exp(i phi_0) (phi_0 = 0 without phases; the Nyquist bin of an M-row
//                   matrix starts at 0); flags a negative or NaN magnitude
//   sg_inv_frames   one workgroup per frame: the Hermitian extension folded into the packing
//                   of an M-point complex inverse transform, / N, the pad dropped, x w: wl
//                   doubles per frame to the workspace
//   sg_inv_ola      a gather, one lane per output sample: its covering frames (sg_invert.h)
//                   added in frame order over the window-square sum added the same way; 0
//                   where that sum is 0. No atomics: a sound's samples have the same bits
//                   alone, in any batch, at any position and under any workspace cap.
//
// The iteration keeps x materialised (in the caller's output buffer): sg_inv_project reads it
// as sg_inv_stft reads a sound. One launch sequence per iteration serves a whole chunk of the
// batch; nothing is awaited inside the loop, and the errors stay in HBM until the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "sg_dev64.h"
#include "sg_invert.h"
#include "sg_invert_ops.h"
#include "sg_launch.h"
#include "sg_rmath.h"
#include "sg_spectrogram_dev.h"

namespace {

using sg::DevBuf;
using sg::lds_opt_in;
using sg::SpgFrame;
using sg::SpgStat;
using sg::upload;

struct InvSound {
  int64_t xbase, len;  // its samples [xbase, xbase + len) of the sound buffer (read by A, written by A+)
  int64_t spec0;       // first complex cell of its spectrum
  int64_t mag0;        // first cell of its magnitudes (and initial phases) in the caller's buffer
  int64_t ws0;         // first cell of its windowed frames in the workspace
  int32_t f0, nf;      // frames [f0, f0 + nf) of the launch
};

struct InvTile {
  int32_t snd, c;  // samples [c kInvTile, (c + 1) kInvTile) of the sound
};

constexpr int kT = 256;
static_assert(SG_F64_THREADS == kT && sg::kInvTile == kT, "fft64 strides by SG_F64_THREADS; a lane per sample of a tile");

// A of a frame (spg_forward_frame); stat == nullptr: the samples as they are
template <typename T>
__global__ __launch_bounds__(kT) void sg_inv_stft(const T* __restrict__ x, const SpgFrame* __restrict__ frames,
                                                  const InvSound* __restrict__ snds, const SpgStat* __restrict__ stat,
                                                  const double* __restrict__ win, const double2* __restrict__ TN, int wl,
                                                  int pad, int M, int rows, double2* __restrict__ out) {
  extern __shared__ double2 lds64[];
  const SpgFrame F = frames[blockIdx.x];
  const InvSound S = snds[F.snd];
  double2* row = out + S.spec0 + (int64_t)F.f * rows;
  // host: F.o + wl <= S.len
  spg_forward_frame(lds64, x + S.xbase + F.o, stat ? stat + F.snd : nullptr, win, TN, wl, pad, M, rows,
                    [row](int k, double re, double im) { row[k] = make_double2(re, im); });
}

// A of a frame of the iteration's sound with the projection behind it (see the head of the file):
// mag has mrows rows a frame, X M + 1, and part receives the frame's two sums
__global__ __launch_bounds__(kT) void sg_inv_project(const double* __restrict__ x, const SpgFrame* __restrict__ frames,
                                                     const InvSound* __restrict__ snds, const double* __restrict__ win,
                                                     const double2* __restrict__ TN, int wl, int pad, int M,
                                                     double2* __restrict__ X, const double* __restrict__ mag, int mrows,
                                                     double* __restrict__ part) {
  extern __shared__ double2 lds64[];
  __shared__ double red[kT];
  const SpgFrame F = frames[blockIdx.x];
  const InvSound S = snds[F.snd];
  double2* row = X + S.spec0 + (int64_t)F.f * (M + 1);
  const double* mrow = mag + S.mag0 + (int64_t)F.f * mrows;
  double num = 0, den = 0;
  spg_forward_frame(lds64, x + S.xbase + F.o, nullptr, win, TN, wl, pad, M, M + 1, [&](int k, double re, double im) {
    if (k < mrows) {
      const double s = mrow[k], az = hypot(re, im), d = az - s;
      num += d * d;
      den += s * s;
      if (az > 0) {
        re = (s * re) / az;
        im = (s * im) / az;
      } else {
        re = s;
        im = 0;
      }
    }
    row[k] = make_double2(re, im);
  });
  num = block_reduce<kT>(num, 0, red);
  den = block_reduce<kT>(den, 0, red);
  if (threadIdx.x == 0) {
    part[2 * (int64_t)blockIdx.x] = num;
    part[2 * (int64_t)blockIdx.x + 1] = den;
  }
}

// err[c n_iter + it] of sound c = c0 + its index in the chunk: one wave per sound, lane l adds the
// frames l, l + 64, ... in order and the lanes fold in a butterfly, so the sum depends on the
// sound's frame count alone
__global__ __launch_bounds__(64) void sg_inv_fold(const double* __restrict__ part, const InvSound* __restrict__ snds,
                                                  int64_t c0, int it, int n_iter, double* __restrict__ err) {
  const InvSound S = snds[blockIdx.x];
  double num = 0, den = 0;
  for (int f = threadIdx.x; f < S.nf; f += 64) {
    num += part[2 * (int64_t)(S.f0 + f)];
    den += part[2 * (int64_t)(S.f0 + f) + 1];
  }
  num = wsum(num);
  den = wsum(den);
  if (threadIdx.x == 0) err[(c0 + blockIdx.x) * n_iter + it] = sqrt(num / den);
}

__global__ __launch_bounds__(kT) void sg_inv_start(const SpgFrame* __restrict__ frames, const InvSound* __restrict__ snds,
                                                   const double* __restrict__ mag, const double* __restrict__ phase, int M,
                                                   int mrows, double2* __restrict__ X, int32_t* __restrict__ bad) {
  const SpgFrame F = frames[blockIdx.x];
  const InvSound S = snds[F.snd];
  const double* mrow = mag + S.mag0 + (int64_t)F.f * mrows;
  const double* prow = phase ? phase + S.mag0 + (int64_t)F.f * mrows : nullptr;
  double2* row = X + S.spec0 + (int64_t)F.f * (M + 1);
  int flag = 0;
  for (int k = threadIdx.x; k <= M; k += kT) {
    double2 v = make_double2(0.0, 0.0);
    if (k < mrows) {
      const double s = mrow[k];
      flag |= s >= 0 ? 0 : 1;  // negative or NaN
      v.x = s;
      if (prow) {
        double sn, cs;
        sincos(prow[k], &sn, &cs);
        v = make_double2(s * cs, s * sn);
      }
    }
    row[k] = v;
  }
  if (flag) atomicOr(bad, 1);
}

// A+ up to the overlap-add: frame f of the launch from its `rows` complex bins to wl doubles.
// The N-point Hermitian spectrum goes through the M-point complex inverse of z_n = y_2n + i y_2n+1:
// Z_k = E_k + i O_k with 2 E_k = X_k + conj X_{M-k}, 2 O_k = (X_k - conj X_{M-k}) conj W_N^k; the halves
// are left out and the result divided by N = 2 M. Im X_0 and Im X_M drop out of the real part.
__global__ __launch_bounds__(kT) void sg_inv_frames(const double2* __restrict__ X, const SpgFrame* __restrict__ frames,
                                                    const InvSound* __restrict__ snds, const double* __restrict__ win,
                                                    const double2* __restrict__ TN, int wl, int pad, int M, int rows,
                                                    double* __restrict__ ws) {
  extern __shared__ double2 lds64[];
  const Fft64Lds L = fft64_carve(lds64, M);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  const SpgFrame F = frames[blockIdx.x];
  const InvSound S = snds[F.snd];
  const double2* row = X + S.spec0 + (int64_t)F.f * rows;
  for (int k = threadIdx.x; k < M; k += kT) {
    double2 p = row[k];
    double2 q = M - k < rows ? row[M - k] : make_double2(0.0, 0.0);  // k = 0: the Nyquist bin, 0 when it is not kept
    if (k == 0) p.y = q.y = 0.0;
    const double2 w = TN[k];
    const double2 e = make_double2(p.x + q.x, p.y - q.y), d = make_double2(p.x - q.x, p.y + q.y);
    const double2 o = make_double2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);  // d conj(w)
    a[k] = make_double2(e.x - o.y, e.y + o.x);
  }
  __syncthreads();
  fft64(a, b, M, TN, rt, true);
  double* y = ws + S.ws0 + (int64_t)F.f * wl;
  const double N = (double)(2 * M);
  for (int n = threadIdx.x; n < M; n += kT) {
    const double2 z = a[n];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * n + h - pad;
      if (j >= 0 && j < wl) y[j] = ((h ? z.y : z.x) / N) * win[j];
    }
  }
}

__global__ __launch_bounds__(kT) void sg_inv_ola(const InvTile* __restrict__ tiles, const InvSound* __restrict__ snds,
                                                 const SpgFrame* __restrict__ frames, const double* __restrict__ win,
                                                 const double* __restrict__ ws, int wl, double by,
                                                 double* __restrict__ out) {
  const InvTile J = tiles[blockIdx.x];
  const InvSound S = snds[J.snd];
  const int64_t t = (int64_t)J.c * kT + threadIdx.x;
  if (t >= S.len) return;
  const SpgFrame* fr = frames + S.f0;
  const sg::InvCover c = sg::inv_cover(t, wl, (int64_t)S.nf, by, [fr](int64_t i) { return fr[i].o; });
  const double* y = ws + S.ws0;
  double num = 0, den = 0;
  for (int64_t i = c.first; i <= c.last; ++i) {
    const int64_t j = t - fr[i].o;  // 0 <= j < wl by the cover
    const double w = win[j];
    num += y[i * wl + j];
    den += w * w;
  }
  out[S.xbase + t] = den == 0 ? 0.0 : num / den;
}

sg::StageTimes<sg::kInvStages> g_inv_ms;  // of the last profiled launch sequence

// The tables of sounds [c0, c1) of a batch. Spectra and workspaces are laid out one sound after
// the other from 0 unless spec_off says where each spectrum is.
struct InvTables {
  std::vector<InvSound> snds;
  std::vector<SpgFrame> fr;
  std::vector<InvTile> tiles;
  int64_t spec_cells = 0, ws_cells = 0;
};

InvTables inv_tables(const sg::SpgSetup& S, int64_t c0, int64_t c1, const int64_t* xoff, const int64_t* lengths,
                     const int64_t* spec_off, const int64_t* mag_off, int rows, bool with_tiles) {
  InvTables T;
  T.snds.resize((size_t)(c1 - c0));
  for (int64_t c = c0; c < c1; ++c) {
    const int64_t len = lengths[c] > 0 ? lengths[c] : 0;
    const int nf = sg::spg_frames(S, len);
    InvSound& Q = T.snds[(size_t)(c - c0)];
    Q.xbase = xoff[c];
    Q.len = len;
    Q.spec0 = spec_off ? spec_off[c] : T.spec_cells;
    Q.mag0 = mag_off ? mag_off[c] : 0;
    Q.ws0 = T.ws_cells;
    Q.f0 = (int32_t)T.fr.size();
    Q.nf = nf;
    if ((int64_t)T.tiles.size() + len / kT + 1 > 2147483647LL)
      throw sg::SgError(SG_E_UNSUPPORTED, "invert: the frames of one launch exceed 2^31");
    sg::spg_list_frames(S, len, nf, (int32_t)(c - c0), "invert", T.fr);
    if (with_tiles)
      for (int64_t k = 0; k * kT < len; ++k) T.tiles.push_back(InvTile{(int32_t)(c - c0), (int32_t)k});
    T.spec_cells += (int64_t)nf * rows;
    T.ws_cells += (int64_t)nf * S.wl;
  }
  return T;
}

// what every launch of a sequence shares
struct InvDev {
  const InvSound* snd;
  const SpgFrame* fr;
  const InvTile* tiles;
  const double* win;
  const double2* TN;
  unsigned F, ntiles;
};

// A+: X (rows bins a frame, at the sounds' spec0) to the sounds at d_x; ws: the workspace
void synthesize(const sg::SpgSetup& S, const InvDev& D, const double2* d_X, int rows, double* d_ws, double* d_x,
                sg::StageClock& clk, hipStream_t s) {
  clk.stamp(3);
  if (D.F) {
    hipLaunchKernelGGL(sg_inv_frames, dim3(D.F), dim3(kT), (size_t)fft64_lds_bytes(S.bins), s, d_X, D.fr, D.snd, D.win, D.TN, S.wl,
                       S.pad, S.bins, rows, d_ws);
    SG_LAUNCHED("sg_inv_frames");
  }
  clk.stamp(4);
  if (D.ntiles) {
    hipLaunchKernelGGL(sg_inv_ola, dim3(D.ntiles), dim3(kT), 0, s, D.tiles, D.snd, D.fr, D.win, d_ws, S.wl, S.by, d_x);
    SG_LAUNCHED("sg_inv_ola");
  }
}

InvDev upload_tables(DevBuf& db, const sg::SpgSetup& S, const InvTables& T, hipStream_t s) {
  InvDev D;
  D.snd = upload(db, T.snds, s);
  D.fr = upload(db, T.fr, s);
  D.tiles = upload(db, T.tiles, s);
  D.win = upload(db, sg::spg_window(S.wl, S.wn), s);
  double2* tn = db.get<double2>((size_t)S.N);
  sg::fill_roots64(tn, S.N, s);
  D.TN = tn;
  D.F = (unsigned)T.fr.size();
  D.ntiles = (unsigned)T.tiles.size();
  return D;
}

void check_rows(const sg::SpgSetup& S, int rows, const char* who) {
  if (!sg::inv_rows_ok(rows, S.bins))
    throw sg::SgError(SG_E_ARG, std::string(who) + ": a spectrum of " + std::to_string(S.N) + "-point frames has " +
                                    std::to_string(S.bins) + " rows (the reference's shape) or " +
                                    std::to_string(S.bins + 1) + " (with the Nyquist bin), not " + std::to_string(rows));
}

template <typename T>
void stft_device(sg_ctx* ctx, const sg::SpgSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths,
                 int64_t n_calls, int rows, double2* d_out, const int64_t* out_off) {
  hipStream_t s = ctx->stream;
  const InvTables Tb = inv_tables(S, 0, n_calls, offsets, lengths, out_off, nullptr, rows, false);
  sg::StageClock clk(s, g_inv_ms.sink(ctx), sg::kInvStages);
  clk.zero();
  if (Tb.fr.empty()) return;
  DevBuf db;
  const InvDev D = upload_tables(db, S, Tb, s);
  SpgStat* d_stat = db.get<SpgStat>((size_t)n_calls);
  std::vector<int64_t> lens(lengths, lengths + n_calls);
  for (int64_t c = 0; c < n_calls; ++c)
    if (Tb.snds[(size_t)c].nf == 0) lens[(size_t)c] = 0;  // as spectrogram_device: no statistics of a sound without frames
  clk.stamp(0);
  sg::spg_stats_device<T>(d_x, offsets, lens.data(), n_calls, d_stat, s);
  clk.stamp(1);
  const int lds = fft64_lds_bytes(S.bins);
  lds_opt_in(&sg_inv_stft<T>, lds, "sg_inv_stft");
  hipLaunchKernelGGL(sg_inv_stft<T>, dim3(D.F), dim3(kT), (size_t)lds, s, d_x, D.fr, D.snd, d_stat, D.win, D.TN, S.wl, S.pad,
                     S.bins, rows, d_out);
  SG_LAUNCHED("sg_inv_stft");
  clk.stamp(-1);
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
}

// consecutive sounds whose workspaces fit the cap; at least one sound a chunk
std::vector<int64_t> chunk_ends(const sg::SpgSetup& S, const int64_t* lengths, int64_t n_calls, int64_t cap) {
  std::vector<int64_t> need((size_t)n_calls);
  for (int64_t c = 0; c < n_calls; ++c)
    need[(size_t)c] = sg::inv_workspace_bytes(sg::spg_frames(S, lengths[c] > 0 ? lengths[c] : 0), S.wl, S.bins);
  return sg::inv_chunk_ends(need, cap);
}

}  // namespace

// ---- the pair as launch sequences, for the features between A and A+ (sg_invert_ops.h)
namespace sg {

std::vector<int64_t> inv_chunk_ends(const std::vector<int64_t>& need, int64_t cap) {
  std::vector<int64_t> ends;
  int64_t used = 0;
  for (size_t c = 0; c < need.size(); ++c) {
    if (used > 0 && used + need[c] > cap) {
      ends.push_back((int64_t)c);
      used = 0;
    }
    used += need[c];
  }
  ends.push_back((int64_t)need.size());
  return ends;
}

template <typename T>
void inv_forward_launch(const SpgSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t c0,
                        int64_t c1, double2* d_X, DevBuf& db, hipStream_t s) {
  const InvTables Tb = inv_tables(S, c0, c1, offsets, lengths, nullptr, nullptr, S.bins + 1, false);
  if (Tb.fr.empty()) return;
  const InvDev D = upload_tables(db, S, Tb, s);
  const int lds = fft64_lds_bytes(S.bins);
  lds_opt_in(&sg_inv_stft<T>, lds, "sg_inv_stft");
  hipLaunchKernelGGL(sg_inv_stft<T>, dim3(D.F), dim3(kT), (size_t)lds, s, d_x, D.fr, D.snd, (const SpgStat*)nullptr, D.win, D.TN,
                     S.wl, S.pad, S.bins, S.bins + 1, d_X);
  SG_LAUNCHED("sg_inv_stft");
}
template void inv_forward_launch<float>(const SpgSetup&, const float*, const int64_t*, const int64_t*, int64_t, int64_t,
                                        double2*, DevBuf&, hipStream_t);
template void inv_forward_launch<double>(const SpgSetup&, const double*, const int64_t*, const int64_t*, int64_t, int64_t,
                                         double2*, DevBuf&, hipStream_t);

void inv_synthesis_launch(const SpgSetup& S, const double2* d_X, const int64_t* out_off, const int64_t* lengths,
                          int64_t c0, int64_t c1, double* d_ws, double* d_out, DevBuf& db, StageClock& clk, hipStream_t s) {
  const InvTables Tb = inv_tables(S, c0, c1, out_off, lengths, nullptr, nullptr, S.bins + 1, true);
  const InvDev D = upload_tables(db, S, Tb, s);
  lds_opt_in(&sg_inv_frames, fft64_lds_bytes(S.bins), "sg_inv_frames");
  synthesize(S, D, d_X, S.bins + 1, d_ws, d_out, clk, s);
}

}  // namespace sg

using sg::guarded;

extern "C" {

int sg_spg_stft_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                      int64_t n_calls, const sg_spectrogram_params* p, int32_t rows, double* d_out,
                      const int64_t* out_off) {
  return guarded(ctx, [&]() {
    if (!p) throw sg::SgError(SG_E_ARG, "sg_spg_stft_batch: bad arguments");
    const sg::SpgSetup S = sg::spg_setup(*p);  // spectrogram()'s refusals, before anything else
    check_rows(S, rows, "sg_spg_stft_batch");
    if (!ctx) sg::bad_arguments("sg_spg_stft_batch");
    sg::batch_args("sg_spg_stft_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off});
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::with_samples(is_f64 != 0, d_wave, [&](auto* d_x) {
      stft_device(ctx, S, d_x, offsets, lengths, n_calls, rows, reinterpret_cast<double2*>(d_out), out_off);
    });
    return SG_OK;
  });
}

int sg_spg_istft_batch(sg_ctx* ctx, const double* d_spec, const int64_t* spec_off, const int64_t* lengths, int64_t n_calls,
                       const sg_spectrogram_params* p, int32_t rows, double* d_out, const int64_t* out_off) {
  return guarded(ctx, [&]() {
    if (!p) throw sg::SgError(SG_E_ARG, "sg_spg_istft_batch: bad arguments");
    const sg::SpgSetup S = sg::spg_setup(*p);
    check_rows(S, rows, "sg_spg_istft_batch");
    if (!ctx) sg::bad_arguments("sg_spg_istft_batch");
    sg::batch_args("sg_spg_istft_batch", n_calls, {d_spec, spec_off, lengths, d_out, out_off});
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const InvTables Tb = inv_tables(S, 0, n_calls, out_off, lengths, spec_off, nullptr, rows, true);
    sg::StageClock clk(s, g_inv_ms.sink(ctx), sg::kInvStages);
    clk.zero();
    DevBuf db;
    const InvDev D = upload_tables(db, S, Tb, s);
    double* d_ws = db.get<double>((size_t)Tb.ws_cells);
    lds_opt_in(&sg_inv_frames, fft64_lds_bytes(S.bins), "sg_inv_frames");
    synthesize(S, D, reinterpret_cast<const double2*>(d_spec), rows, d_ws, d_out, clk, s);
    clk.stamp(-1);
    HIPCHK(hipStreamSynchronize(s));
    clk.finish();
    return SG_OK;
  });
}

int sg_invert_spectrogram_batch(sg_ctx* ctx, const double* d_mag, const int64_t* mag_off, const double* d_phase,
                                const int64_t* lengths, int64_t n_calls, const sg_spectrogram_params* p, int32_t rows,
                                int32_t n_iter, int64_t workspace_cap, double* d_out, const int64_t* out_off,
                                double* err_out) {
  return guarded(ctx, [&]() {
    if (!p) throw sg::SgError(SG_E_ARG, "sg_invert_spectrogram_batch: bad arguments");
    const sg::SpgSetup S = sg::spg_setup(*p);
    check_rows(S, rows, "sg_invert_spectrogram_batch");
    if (!ctx || n_iter < 0 || workspace_cap < 0) sg::bad_arguments("sg_invert_spectrogram_batch");
    sg::batch_args("sg_invert_spectrogram_batch", n_calls, {d_mag, mag_off, lengths, d_out, out_off});
    if (n_calls == 0) return SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int M = S.bins, lds = fft64_lds_bytes(M);
    lds_opt_in(&sg_inv_frames, lds, "sg_inv_frames");
    lds_opt_in(&sg_inv_project, lds, "sg_inv_project");
    const std::vector<int64_t> ends = chunk_ends(S, lengths, n_calls, workspace_cap > 0 ? workspace_cap : sg::kInvWorkspaceCap);
    sg::StageClock clk(s, g_inv_ms.sink(ctx), sg::kInvStages);
    clk.zero();
    DevBuf top;
    double* d_err = top.get<double>((size_t)n_calls * (size_t)std::max(n_iter, 1));
    int32_t* d_bad = top.get<int32_t>(1);
    HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), s));
    int64_t c0 = 0;
    for (const int64_t c1 : ends) {
      const InvTables Tb = inv_tables(S, c0, c1, out_off, lengths, nullptr, mag_off, M + 1, true);
      DevBuf db;
      const InvDev D = upload_tables(db, S, Tb, s);
      double2* d_X = db.get<double2>((size_t)Tb.spec_cells);
      double* d_ws = db.get<double>((size_t)Tb.ws_cells);
      double* d_part = db.get<double>(2 * (size_t)D.F);
      const unsigned NS = (unsigned)(c1 - c0);
      clk.stamp(2);
      if (D.F) {
        hipLaunchKernelGGL(sg_inv_start, dim3(D.F), dim3(kT), 0, s, D.fr, D.snd, d_mag, d_phase, M, (int)rows, d_X, d_bad);
        SG_LAUNCHED("sg_inv_start");
      }
      clk.stamp(-1);
      int32_t bad = 0;  // before the loop: the only wait of a chunk but the last
      HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (bad) throw sg::SgError(SG_E_ARG, "invert_spectrogram: a magnitude is negative or NaN");
      for (int it = 0; it < n_iter; ++it) {
        synthesize(S, D, d_X, M + 1, d_ws, d_out, clk, s);
        clk.stamp(1);
        if (D.F) {
          hipLaunchKernelGGL(sg_inv_project, dim3(D.F), dim3(kT), (size_t)lds, s, d_out, D.fr, D.snd, D.win, D.TN, S.wl, S.pad,
                             M, d_X, d_mag, (int)rows, d_part);
          SG_LAUNCHED("sg_inv_project");
        }
        clk.stamp(5);
        hipLaunchKernelGGL(sg_inv_fold, dim3(NS), dim3(64), 0, s, d_part, D.snd, c0, it, (int)n_iter, d_err);
        SG_LAUNCHED("sg_inv_fold");
      }
      synthesize(S, D, d_X, M + 1, d_ws, d_out, clk, s);
      clk.stamp(-1);
      HIPCHK(hipStreamSynchronize(s));  // db goes away
      c0 = c1;
    }
    clk.finish();
    if (err_out && n_iter > 0)
      HIPCHK(hipMemcpy(err_out, d_err, (size_t)n_calls * (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost));
    return SG_OK;
  });
}

int sg_invert_size(int64_t len, const sg_spectrogram_params* p, int32_t rows, int32_t* wl, int32_t* n_fft, int32_t* bins,
                   int32_t* frames, int64_t* samples, int64_t* workspace_bytes) {
  return sg::host_guarded([&]() {
    if (!p || !wl || !n_fft || !bins || !frames || !samples || !workspace_bytes) sg::bad_arguments("sg_invert_size");
    const sg::SpgSetup S = sg::spg_setup(*p);
    if (rows != 0) check_rows(S, rows, "sg_invert_size");
    if (len < 0) sg::bad_arguments("sg_invert_size");
    *wl = S.wl;
    *n_fft = S.N;
    *bins = S.bins;
    *frames = sg::spg_frames(S, len);
    *samples = len;
    *workspace_bytes = sg::inv_workspace_bytes(*frames, S.wl, S.bins);
  });
}

const char* sg_invert_size_error(void) { return sg::g_host_err.c_str(); }

int sg_debug_invert_kernel_ms(double* out) { return g_inv_ms.read(out); }

}  // extern "C"
