// sg_segment.hip — segment() on the device (R/segment.R:79-219), fp64 throughout; the host
// decisions are sg_segment.cpp's, what runs behind the envelope is sg_segment.h's.
//
// The Hilbert envelope needs the transform of the WHOLE sound padded to N = 2^p points
// (seewave::hilbert), p <= 22: far more than the 2048-point frame fft64 (sg_fft64_dev.h)
// holds in LDS. For p >= 12 the transform is the four-step scheme over N = N1 N2 (N1 =
// 2^(p / 2) <= N2 <= 2048), with fft64 as the building block, in place in a workspace of N
// complex doubles, cell k1 N2 + n2:
//   sg_seg_cols_fwd   one workgroup per column n2: the N1-point transform over n1 of the
//                     normalized, padded sound x[N2 n1 + n2] (read from the sound itself:
//                     the padded signal is never stored), times the twiddle W_N^(n2 k1)
//   sg_seg_rows       one workgroup per row k1: the N2-point transform over n2 leaves
//                     X[k1 + N1 k2] for every k2 -- exactly one column of the inverse
//                     transform's first pass -- so, in the same LDS buffers: times
//                     hilbert's h, the inverse N2-point transform over k2, times the
//                     twiddle W_N^(-b k1), back to the row
//   sg_seg_cols_inv   one workgroup per column b: the inverse N1-point transform over k1
//                     gives N x[N2 a + b] for every a; / N, Mod (hypot), and the store
//                     shifted by the un-padding rule
// Three passes over the workspace per sound instead of the four of two separate
// transforms. The column passes touch the workspace with a stride of N2 cells; the
// workgroups of neighbouring columns run together and share the cache lines.
// p <= 11: sg_seg_fft_one, the whole chain in one workgroup's LDS.
//
// Normalization (segment.R:119-123) needs min, max, mean and sd first: sg_seg_part reduces
// tiles of kTile samples (block_reduce: a fixed tree), sg_seg_stat folds a sound's tiles
// (thread t adds tiles t, t + 256, ... in order, then the same tree); pass 0 gives the sum
// and the extremes, pass 1 (only for min > 0, the scale() branch) the sum of squares about
// the mean. A sound's tiles depend on its length alone, so its statistics do not depend on
// the batch around it.
//
// sg_seg_smooth: one wavefront per envelope value: lane l adds its window's points l, l +
// 64, ... in order, the 64 partial sums fold in wsum's butterfly, / points. The first index,
// the points and the skipped value (if any) of every window come from the host (sg_segment.cpp).
// sg_seg_tail: one 64-lane workgroup per sound runs sg::seg_sound (sg_segment.h).
//
// A batch runs in chunks of consecutive sounds whose workspaces fit the cap
// (sg_segment_params.workspace_cap, default sg::kSegWorkspaceCap); every kernel's work on a
// sound is the same in any chunking.
//
// A parameter sweep (sg_segment_sweep: what optimizePars() evaluates) runs the same kernels
// up to the raw envelope once per sound, sg_seg_smooth once per group of rows with equal
// (windowLength, overlap), and sg_seg_sweep_tail, one workgroup per (row, sound), over chunks
// of rows; sg_sweep_fit turns a column of the summaries into the fitness of every row.
#include <hip/hip_runtime.h>

#include <array>
#include <memory>
#include <string>
#include <utility>

#include "sg_dev64.h"
#include "sg_fft64_dev.h"
#include "sg_launch.h"
#include "sg_segment_plan.h"
#include "sg_spectrogram.h"

namespace {

constexpr int kT = SG_F64_THREADS;
constexpr int kTile = 8192;  // samples of a statistics tile
constexpr int kTailT = 64;

struct SegSound {
  int64_t x0, n1;    // the sound in the input; n1 == 0: a sound the reference stops on
  int64_t w0;        // first cell of its workspace (p >= 12)
  int64_t e0;        // first cell of its un-padded envelope
  int64_t o0;        // first cell of its output
  int64_t minCount;  // ceiling(shortestSyl / timestep)
  double timestep;
  int32_t p, lg1;    // N = 2^p; N1 = 2^lg1 (p >= 12)
  int32_t left, shift, n_env, m;
  int32_t t1, t2;    // first root of the tables of N1 (p <= 11: N) and N2
  int32_t tile0, ntiles;
};
struct SegStat {
  double mean, sd, div, mn, mx;
  int32_t scale, pad;
};
struct SegItem {
  int32_t snd, idx;
};
struct SegWin {
  int32_t snd, idx, first, count;
  int32_t jump, pad;  // point j is value first + j, first + j + 1 from j = jump on
};
// A sweep (sg_segment_sweep). Slot (group, sound): the smoothed envelope of the sound under
// the group's (windowLength, overlap), kept once for all rows of the group
struct SweepSlot {
  int64_t e0;  // its cells among the envelopes: seg_env0() unused ones (sg_seg_smooth writes as into a sound's cells), then m values
  int64_t w0;  // first cell of the sound's pair within a row's workspace
  double timestep;
  int32_t m, pad;
};
struct SweepRow {
  sg::SegPars P;
  int64_t w0;  // first cell of the row's workspace within its chunk
  int32_t group, pad;
};

__device__ __forceinline__ double seg_norm(double v, const SegStat& q) {
  if (q.scale) v = (v - q.mean) / q.sd;  // scale(): centre, then / sqrt(sum(x^2) / (n - 1))
  return v / q.div;
}
// sample j of the normalized sound between hilbert()'s zeros
template <typename T>
__device__ __forceinline__ double seg_padded(const T* __restrict__ px, const SegSound& S, const SegStat& q, int64_t j) {
  const int64_t i = j - S.left;
  return i >= 0 && i < S.n1 ? seg_norm((double)px[i], q) : 0.0;
}
// hilbert()'s h, 0-based k: 1 at 0 and N / 2, 2 between, 0 above (N == 2: h[2:1] <- 2 hits both)
__device__ __forceinline__ double seg_h(int64_t k, int64_t N) {
  if (N == 2) return 2.0;
  if (k == 0 || k == N / 2) return 1.0;
  return k < N / 2 ? 2.0 : 0.0;
}
// |ht[j]| to the envelope, through the un-padding rule
__device__ __forceinline__ void seg_store(double* __restrict__ env, const SegSound& S, int64_t j, double2 v, double N) {
  const int64_t k = j - S.shift;
  if (k >= 0 && k < S.n_env) env[S.e0 + k] = hypot(v.x / N, v.y / N);
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_seg_part(const T* __restrict__ x, const SegSound* __restrict__ snds,
                                                  const SegItem* __restrict__ tiles, const SegStat* __restrict__ st,
                                                  int pass, double* __restrict__ part) {
  __shared__ double red[kT];
  const SegItem I = tiles[blockIdx.x];
  const SegSound S = snds[I.snd];
  const int64_t a = (int64_t)I.idx * kTile, b = min(a + (int64_t)kTile, S.n1);
  const T* px = x + S.x0;
  double* q = part + 3 * ((int64_t)S.tile0 + I.idx);
  if (pass == 0) {
    double s = 0, mn = INFINITY, mx = -INFINITY;
    for (int64_t i = a + threadIdx.x; i < b; i += kT) {
      const double v = (double)px[i];
      s += v;
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    }
    s = block_reduce<kT>(s, 0, red);
    mn = block_reduce<kT>(mn, 1, red);
    mx = block_reduce<kT>(mx, 2, red);
    if (threadIdx.x == 0) {
      q[0] = s;
      q[1] = mn;
      q[2] = mx;
    }
  } else {
    const SegStat Q = st[I.snd];
    if (!(Q.mn > 0)) return;  // workgroup-uniform: no scale(), no sd
    double s = 0;
    for (int64_t i = a + threadIdx.x; i < b; i += kT) {
      const double d = (double)px[i] - Q.mean;
      s += d * d;
    }
    s = block_reduce<kT>(s, 0, red);
    if (threadIdx.x == 0) q[0] = s;
  }
}

__global__ __launch_bounds__(kT) void sg_seg_stat(const SegSound* __restrict__ snds, const double* __restrict__ part,
                                                  int pass, SegStat* __restrict__ st) {
  __shared__ double red[kT];
  const SegSound S = snds[blockIdx.x];
  if (S.n1 <= 0) return;  // workgroup-uniform
  SegStat* Q = st + blockIdx.x;
  const double* q = part + 3 * (int64_t)S.tile0;
  if (pass == 0) {
    double s = 0, mn = INFINITY, mx = -INFINITY;
    for (int t = threadIdx.x; t < S.ntiles; t += kT) {
      s += q[3 * t];
      mn = fmin(mn, q[3 * t + 1]);
      mx = fmax(mx, q[3 * t + 2]);
    }
    s = block_reduce<kT>(s, 0, red);
    mn = block_reduce<kT>(mn, 1, red);
    mx = block_reduce<kT>(mx, 2, red);
    if (threadIdx.x == 0) {
      Q->mean = s / (double)S.n1;
      Q->mn = mn;
      Q->mx = mx;
      Q->sd = 1.0;
      Q->scale = 0;
      Q->div = fmax(fabs(mx), fabs(mn));  // max(abs(max(sound)), abs(min(sound)))
    }
  } else {
    if (!(Q->mn > 0)) return;  // workgroup-uniform
    double s = 0;
    for (int t = threadIdx.x; t < S.ntiles; t += kT) s += q[3 * t];
    s = block_reduce<kT>(s, 0, red);
    if (threadIdx.x == 0) {
      const double sd = sqrt(s / (double)max((int64_t)1, S.n1 - 1));
      Q->sd = sd;
      Q->scale = 1;
      Q->div = fmax(fabs((Q->mx - Q->mean) / sd), fabs((Q->mn - Q->mean) / sd));
    }
  }
}

extern __shared__ double2 seg_lds[];

// p <= 11: the whole chain for one sound per workgroup
template <typename T>
__global__ __launch_bounds__(kT) void sg_seg_fft_one(const T* __restrict__ x, const SegSound* __restrict__ snds,
                                                     const int32_t* __restrict__ list, const SegStat* __restrict__ st,
                                                     const double2* __restrict__ TN, double* __restrict__ env) {
  const int c = list[blockIdx.x];
  const SegSound S = snds[c];
  const SegStat Q = st[c];
  const int N = 1 << S.p;
  const Fft64Lds L = fft64_carve(seg_lds, N);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  const T* px = x + S.x0;
  for (int j = threadIdx.x; j < N; j += kT) a[j] = make_double2(seg_padded(px, S, Q, j), 0.0);
  __syncthreads();
  fft64(a, b, N, TN + S.t1, rt, false);
  for (int k = threadIdx.x; k < N; k += kT) {
    const double h = seg_h(k, N);
    a[k] = make_double2(a[k].x * h, a[k].y * h);
  }
  __syncthreads();
  fft64(a, b, N, TN + S.t1, rt, true);
  for (int j = threadIdx.x; j < N; j += kT) seg_store(env, S, j, a[j], (double)N);
}

template <typename T>
__global__ __launch_bounds__(kT) void sg_seg_cols_fwd(const T* __restrict__ x, const SegSound* __restrict__ snds,
                                                      const SegItem* __restrict__ cols, const SegStat* __restrict__ st,
                                                      const double2* __restrict__ TN, double2* __restrict__ W) {
  const SegItem I = cols[blockIdx.x];
  const SegSound S = snds[I.snd];
  const SegStat Q = st[I.snd];
  const int N1 = 1 << S.lg1, N2 = 1 << (S.p - S.lg1), N = 1 << S.p, n2 = I.idx;
  const Fft64Lds L = fft64_carve(seg_lds, N1);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  const T* px = x + S.x0;
  for (int n1 = threadIdx.x; n1 < N1; n1 += kT) a[n1] = make_double2(seg_padded(px, S, Q, (int64_t)N2 * n1 + n2), 0.0);
  __syncthreads();
  fft64(a, b, N1, TN + S.t1, rt, false);
  double2* w = W + S.w0 + n2;
  for (int k1 = threadIdx.x; k1 < N1; k1 += kT) w[(int64_t)k1 * N2] = cmul64(a[k1], root64(n2 * k1, N));
}

__global__ __launch_bounds__(kT) void sg_seg_rows(const SegSound* __restrict__ snds, const SegItem* __restrict__ rows,
                                                  const double2* __restrict__ TN, double2* __restrict__ W) {
  const SegItem I = rows[blockIdx.x];
  const SegSound S = snds[I.snd];
  const int N1 = 1 << S.lg1, N2 = 1 << (S.p - S.lg1), N = 1 << S.p, k1 = I.idx;
  const Fft64Lds L = fft64_carve(seg_lds, N2);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  double2* w = W + S.w0 + (int64_t)k1 * N2;
  for (int n2 = threadIdx.x; n2 < N2; n2 += kT) a[n2] = w[n2];
  __syncthreads();
  fft64(a, b, N2, TN + S.t2, rt, false);
  for (int k2 = threadIdx.x; k2 < N2; k2 += kT) {  // a[k2] = X[k1 + N1 k2]
    const double h = seg_h((int64_t)k1 + (int64_t)N1 * k2, N);
    a[k2] = make_double2(a[k2].x * h, a[k2].y * h);
  }
  __syncthreads();
  fft64(a, b, N2, TN + S.t2, rt, true);
  for (int q = threadIdx.x; q < N2; q += kT) w[q] = cmul64(a[q], conj_if(root64(q * k1, N), true));
}

__global__ __launch_bounds__(kT) void sg_seg_cols_inv(const SegSound* __restrict__ snds, const SegItem* __restrict__ cols,
                                                      const double2* __restrict__ TN, const double2* __restrict__ W,
                                                      double* __restrict__ env) {
  const SegItem I = cols[blockIdx.x];
  const SegSound S = snds[I.snd];
  const int N1 = 1 << S.lg1, N2 = 1 << (S.p - S.lg1), q = I.idx;
  const Fft64Lds L = fft64_carve(seg_lds, N1);
  double2 *a = L.a, *b = L.b, *rt = L.rt;
  const double2* w = W + S.w0 + q;
  for (int k1 = threadIdx.x; k1 < N1; k1 += kT) a[k1] = w[(int64_t)k1 * N2];
  __syncthreads();
  fft64(a, b, N1, TN + S.t1, rt, true);
  const double N = (double)((int64_t)1 << S.p);
  for (int j = threadIdx.x; j < N1; j += kT) seg_store(env, S, (int64_t)N2 * j + q, a[j], N);
}

__global__ __launch_bounds__(kT) void sg_seg_smooth(const SegSound* __restrict__ snds, const SegWin* __restrict__ wins,
                                                    int64_t nwin, const double* __restrict__ raw, double* __restrict__ out) {
  const int64_t w = (int64_t)blockIdx.x * (kT / 64) + threadIdx.x / 64;
  if (w >= nwin) return;  // wavefront-uniform
  const int lane = threadIdx.x & 63;
  const SegWin Q = wins[w];
  const SegSound S = snds[Q.snd];
  const double* e = raw + S.e0 + Q.first;
  double s = 0;
  for (int i = lane; i < Q.count; i += 64) s += e[i + (i >= Q.jump)];
  s = wsum(s);
  if (lane == 0) out[S.o0 + sg::seg_env0() + Q.idx] = s / (double)Q.count;
}

struct WgSync {
  __device__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(kTailT) void sg_seg_tail(const SegSound* __restrict__ snds, sg::SegPars P,
                                                      double* __restrict__ out) {
  __shared__ double red[kTailT];
  const SegSound S = snds[blockIdx.x];
  sg::seg_sound(P, S.timestep, S.minCount, (int64_t)S.m, out + S.o0, (int)threadIdx.x, kTailT, red, WgSync());
}

// The sweep's tail: workgroup b of a chunk of rows is (row row0 + b / n_calls, sound b %
// n_calls). The envelope is the one its row's group smoothed for the sound; the pair's head,
// tables and scratch are cells of the chunk's workspace; the summary row goes to the output.
// An envelope of at most lds_values values is first copied to LDS (the lanes then read it
// there; the same values, so the same results); a longer one is read where it lies.
__global__ __launch_bounds__(kTailT) void sg_seg_sweep_tail(const SweepSlot* __restrict__ slots,
                                                            const SweepRow* __restrict__ rows, int64_t row0,
                                                            int32_t n_calls, int32_t lds_values,
                                                            const double* __restrict__ envs, double* __restrict__ work,
                                                            double* __restrict__ out) {
  __shared__ double red[kTailT];
  const int64_t r = row0 + (int64_t)(blockIdx.x / (unsigned)n_calls);
  const int c = (int)(blockIdx.x % (unsigned)n_calls);
  const SweepRow R = rows[r];
  const SweepSlot S = slots[(int64_t)R.group * n_calls + c];
  const int64_t m = S.m;
  const double* env = envs + S.e0 + sg::seg_env0();
  if (m > 0 && m <= (int64_t)lds_values) {  // workgroup-uniform
    double* stage = reinterpret_cast<double*>(seg_lds);
    for (int64_t i = threadIdx.x; i < m; i += kTailT) stage[i] = env[i];
    __syncthreads();
    env = stage;
  }
  double* w = work + R.w0 + S.w0;
  const int64_t minCount = m > 0 ? sg::seg_min_count(R.P.shortestSyl, S.timestep) : 0;
  sg::seg_sound_at(R.P, S.timestep, minCount, m, env, w, out + (r * n_calls + c) * sg::kSegSummary,
                   w + sg::seg_pair_syl0(), w + sg::seg_pair_bur0(m), w + sg::seg_pair_scr0(m), (int)threadIdx.x, kTailT,
                   red, WgSync());
}

// 1 - cor(column `col` of row r, key, use = 'pairwise.complete.obs'): one wavefront per row
// of a matrix of n_rows x n_calls x width doubles. Lane l takes the sounds l, l + 64, ...
// in order and skips a pair with a NaN on either side; the 64 partial sums fold in wsum's
// butterfly. Two passes: the count and the two means, then the sums of squares and of
// products about them. The order depends on n_calls alone. NaN for fewer than two complete
// pairs or a side without variance (all its values equal; R: NA); the correlation is
// clamped to [-1, 1] as cov.c does.
__global__ __launch_bounds__(kT) void sg_sweep_fit(const double* __restrict__ mat, int64_t n_rows, int64_t n_calls,
                                                   int32_t width, int32_t col, const double* __restrict__ key,
                                                   double* __restrict__ fit) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * (kT / 64) + threadIdx.x / 64;
  if (r >= n_rows) return;  // wavefront-uniform
  const int lane = threadIdx.x & 63;
  const double* x = mat + r * n_calls * width + col;
  double n = 0, sx = 0, sk = 0, lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
  for (int64_t c = lane; c < n_calls; c += 64) {
    const double a = x[c * width], b = key[c];
    if (a != a || b != b) continue;
    n += 1;
    sx += a;
    sk += b;
    lo[0] = fmin(lo[0], a);
    hi[0] = fmax(hi[0], a);
    lo[1] = fmin(lo[1], b);
    hi[1] = fmax(hi[1], b);
  }
  n = wsum(n);
  sx = wsum(sx);
  sk = wsum(sk);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], o));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], o));
    }
  const bool flat = !(lo[0] < hi[0]) || !(lo[1] < hi[1]);  // a constant side: no variance, whatever the mean rounds to
  const double mx = sx / n, mk = sk / n;
  double sxx = 0, skk = 0, sxk = 0;
  for (int64_t c = lane; c < n_calls; c += 64) {
    const double a = x[c * width], b = key[c];
    if (a != a || b != b) continue;
    const double da = a - mx, db = b - mk;
    sxx += da * da;
    skk += db * db;
    sxk += da * db;
  }
  sxx = wsum(sxx);
  skk = wsum(skk);
  sxk = wsum(sxk);
  if (lane != 0) return;
  double v = NAN;
  if (n >= 2 && !flat && sxx > 0 && skk > 0) {
    v = sxk / (sqrt(sxx) * sqrt(skk));
    v = v > 1 ? 1 : v < -1 ? -1 : v;
  }
  fit[r] = 1 - v;
}

sg::StageTimes<sg::kSegStages> g_seg_ms;  // of the last profiled launch sequence

// first root of the table of an M = 2^lg-point frame (2 M roots) among the tables of 2^1 .. 2^11
int root_table(int lg) { return (1 << (lg + 1)) - 4; }

// What a sweep launches behind the raw envelopes in place of the one smoothing and the one
// tail: launch() on the stream, finish() once it is synchronised (ms: the device time of the
// smoothing and of the tail, as kernel_ms[4] and [5])
struct SegBehind {
  virtual void launch(const std::vector<SegSound>& snds, const double* d_raw, sg::DevBuf& db, hipStream_t s,
                      bool timed) = 0;
  virtual void finish(double* ms) = 0;
  virtual ~SegBehind() {}
};

// the smoothing windows of sound c behind those of the sounds in front of it
void push_windows(std::vector<SegWin>& wins, int64_t c, const sg::SegPlan& S) {
  if ((int64_t)wins.size() + S.m > 2147483647LL)
    throw sg::SgError(SG_E_UNSUPPORTED, "segment: the tiles or windows of one launch exceed 2^31");
  if ((int64_t)S.first.size() != S.m || (int64_t)S.count.size() != S.m || (int64_t)S.jump.size() != S.m)
    throw sg::SgError(SG_E_DEVICE, "segment: a sound's plan has no windows");
  for (int64_t i = 0; i < S.m; ++i) {
    if (S.first[i] < 0 || S.count[i] < 1 || S.jump[i] < 0 || S.jump[i] > S.count[i] ||
        (int64_t)S.first[i] + S.count[i] + (S.jump[i] < S.count[i]) > S.n_env)
      throw sg::SgError(SG_E_DEVICE, "segment: a smoothing window leaves the envelope");
    wins.push_back(SegWin{(int32_t)c, (int32_t)i, S.first[i], S.count[i], S.jump[i], 0});
  }
}

void launch_smooth(const SegSound* d_snd, const std::vector<SegWin>& wins, const double* d_raw, double* d_out,
                   sg::DevBuf& db, hipStream_t s) {
  if (wins.empty()) return;
  const SegWin* d_wins = sg::upload(db, wins, s);
  const int64_t nwin = (int64_t)wins.size(), per = kT / 64;
  hipLaunchKernelGGL(sg_seg_smooth, dim3((unsigned)((nwin + per - 1) / per)), dim3(kT), 0, s, d_snd, d_wins, nwin, d_raw,
                     d_out);
  HIPCHK(hipGetLastError());
}

}  // namespace

namespace sg {

// segment_device(), or with `behind` a sweep's front: the raw envelopes of the sounds (only
// the hilbert fields of the plans are read; d_out and out_off are not), then behind->launch()
template <typename T>
void segment_run(const sg_segment_params& p, const std::vector<SegPlan>& plans, const T* d_x, const int64_t* offsets,
                 int64_t n_calls, double* d_out, const int64_t* out_off, hipStream_t s, double* kernel_ms,
                 SegBehind* behind) {
  const bool env_only = p.mode == 1;
  const SegPars P = env_only ? SegPars{} : seg_pars(p);
  const int64_t cap_cells = std::max<int64_t>(1, (p.workspace_cap > 0 ? p.workspace_cap : kSegWorkspaceCap) / (int64_t)sizeof(double2));
  std::vector<SegSound> snds(n_calls);
  std::vector<SegItem> tiles;
  std::vector<SegWin> wins;
  std::vector<int64_t> chunk_end;  // one past the last sound of each chunk
  int64_t raw = 0, work = 0, work_max = 0;
  bool lg_used[12] = {};
  for (int64_t c = 0; c < n_calls; ++c) {
    const SegPlan& S = plans[c];
    SegSound& Q = snds[c];
    Q = SegSound{};
    Q.x0 = offsets[c];
    Q.o0 = behind ? 0 : out_off[c];
    const int64_t room = behind ? INT64_MAX : out_off[c + 1] - out_off[c];
    if (S.n1 == 0) {
      if (room < seg_cells(0)) throw SgError(SG_E_CAPACITY, "segment: a sound's cells do not fit");
      continue;
    }
    if (S.p < 1 || S.p > kSegMaxLog2 || S.n_env > S.N || S.shift < 0 || S.shift + S.n_env > S.N || S.left + S.n1 > S.N ||
        room < seg_out_cells(p, S))
      throw SgError(room < seg_out_cells(p, S) ? SG_E_CAPACITY : SG_E_DEVICE, "segment: a sound's plan leaves its buffers");
    Q.n1 = S.n1;
    Q.p = S.p;
    Q.left = (int32_t)S.left;
    Q.shift = (int32_t)S.shift;
    Q.n_env = (int32_t)S.n_env;
    Q.m = (int32_t)S.m;
    Q.timestep = S.timestep;
    Q.minCount = S.minCount;
    Q.e0 = env_only ? out_off[c] : raw;
    raw += S.n_env;
    if (S.p <= 11) {
      Q.t1 = root_table(S.p);
      lg_used[S.p] = true;
    } else {
      Q.lg1 = S.p / 2;
      Q.t1 = root_table(Q.lg1);
      Q.t2 = root_table(S.p - Q.lg1);
      lg_used[Q.lg1] = lg_used[S.p - Q.lg1] = true;
      if (work > 0 && work + S.N > cap_cells) {  // the cap is reached: this sound opens the next chunk
        chunk_end.push_back(c);
        work = 0;
      }
      Q.w0 = work;
      work += S.N;
      work_max = std::max(work_max, work);
    }
    if (!env_only) {
      Q.tile0 = (int32_t)tiles.size();
      Q.ntiles = (int32_t)((S.n1 + kTile - 1) / kTile);
      if ((int64_t)tiles.size() + Q.ntiles > 2147483647LL)
        throw SgError(SG_E_UNSUPPORTED, "segment: the tiles or windows of one launch exceed 2^31");
      for (int32_t t = 0; t < Q.ntiles; ++t) tiles.push_back(SegItem{(int32_t)c, t});
      if (!behind) push_windows(wins, c, S);
    }
  }
  chunk_end.push_back(n_calls);
  double msA[1] = {0}, msB[2] = {0, 0};
  std::vector<std::array<double, 3>> msC(chunk_end.size());
  std::vector<std::unique_ptr<StageClock>> clkC;
  StageClock clkA(s, kernel_ms ? msA : nullptr, 1), clkB(s, kernel_ms ? msB : nullptr, 2);
  for (int k = 0; kernel_ms && k < kSegStages; ++k) kernel_ms[k] = 0;
  if (n_calls == 0) return;

  DevBuf db;
  SegSound* d_snd = upload(db, snds, s);
  double2* d_TN = db.get<double2>((size_t)root_table(12));
  for (int lg = 1; lg <= 11; ++lg)
    if (lg_used[lg]) fill_roots64(d_TN + root_table(lg), 2 << lg, s);
  double2* d_W = db.get<double2>((size_t)work_max);
  double* d_raw = env_only ? d_out : db.get<double>((size_t)raw);
  SegStat* d_st;
  const dim3 bT(kT);
  clkA.stamp();
  if (env_only) {
    d_st = upload(db, std::vector<SegStat>(n_calls, SegStat{0.0, 1.0, 1.0, 0.0, 0.0, 0, 0}), s);
  } else {
    d_st = db.get<SegStat>((size_t)n_calls);
    const SegItem* d_tiles = upload(db, tiles, s);
    double* d_part = db.get<double>(3 * tiles.size());
    for (int pass = 0; pass < 2 && !tiles.empty(); ++pass) {
      hipLaunchKernelGGL(sg_seg_part<T>, dim3((unsigned)tiles.size()), bT, 0, s, d_x, d_snd, d_tiles, d_st, pass, d_part);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(sg_seg_stat, dim3((unsigned)n_calls), bT, 0, s, d_snd, d_part, pass, d_st);
      HIPCHK(hipGetLastError());
    }
  }
  clkA.stamp();
  int64_t c0 = 0;
  for (size_t ch = 0; ch < chunk_end.size(); ++ch) {
    const int64_t c1 = chunk_end[ch];
    std::vector<int32_t> ones;
    std::vector<SegItem> cols, rows;
    int M1 = 0, Mc = 0, Mr = 0;  // the largest frame of each kernel
    for (int64_t c = c0; c < c1; ++c) {
      const SegSound& Q = snds[c];
      if (Q.n1 == 0) continue;
      if (Q.p <= 11) {
        ones.push_back((int32_t)c);
        M1 = std::max(M1, 1 << Q.p);
      } else {
        const int N1 = 1 << Q.lg1, N2 = 1 << (Q.p - Q.lg1);
        if (N1 > kSpgMaxBins || N2 > kSpgMaxBins || Q.w0 + ((int64_t)1 << Q.p) > work_max)
          throw SgError(SG_E_DEVICE, "segment: a transform leaves its workspace");
        for (int i = 0; i < N2; ++i) cols.push_back(SegItem{(int32_t)c, i});
        for (int i = 0; i < N1; ++i) rows.push_back(SegItem{(int32_t)c, i});
        Mc = std::max(Mc, N1);
        Mr = std::max(Mr, N2);
      }
    }
    clkC.emplace_back(new StageClock(s, kernel_ms ? msC[ch].data() : nullptr, 3));
    StageClock& clk = *clkC.back();
    clk.stamp();  // forward columns; the short sounds' whole chain
    const SegItem* d_cols = upload(db, cols, s);
    const SegItem* d_rows = upload(db, rows, s);
    if (!ones.empty()) {
      const int32_t* d_ones = upload(db, ones, s);
      sg::lds_opt_in(&sg_seg_fft_one<T>, fft64_lds_bytes(M1), "sg_seg_fft_one");
      hipLaunchKernelGGL(sg_seg_fft_one<T>, dim3((unsigned)ones.size()), bT, (size_t)fft64_lds_bytes(M1), s, d_x, d_snd, d_ones,
                         d_st, d_TN, d_raw);
      HIPCHK(hipGetLastError());
    }
    if (!cols.empty()) {
      sg::lds_opt_in(&sg_seg_cols_fwd<T>, fft64_lds_bytes(Mc), "sg_seg_cols_fwd");
      hipLaunchKernelGGL(sg_seg_cols_fwd<T>, dim3((unsigned)cols.size()), bT, (size_t)fft64_lds_bytes(Mc), s, d_x, d_snd, d_cols,
                         d_st, d_TN, d_W);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // rows
    if (!rows.empty()) {
      sg::lds_opt_in(&sg_seg_rows, fft64_lds_bytes(Mr), "sg_seg_rows");
      hipLaunchKernelGGL(sg_seg_rows, dim3((unsigned)rows.size()), bT, (size_t)fft64_lds_bytes(Mr), s, d_snd, d_rows, d_TN, d_W);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();  // inverse columns
    if (!cols.empty()) {
      sg::lds_opt_in(&sg_seg_cols_inv, fft64_lds_bytes(Mc), "sg_seg_cols_inv");
      hipLaunchKernelGGL(sg_seg_cols_inv, dim3((unsigned)cols.size()), bT, (size_t)fft64_lds_bytes(Mc), s, d_snd, d_cols, d_TN,
                         d_W, d_raw);
      HIPCHK(hipGetLastError());
    }
    clk.stamp();
    c0 = c1;
  }
  clkB.stamp();  // smoothing
  if (behind) {
    behind->launch(snds, d_raw, db, s, kernel_ms != nullptr);
  } else if (!env_only) {
    launch_smooth(d_snd, wins, d_raw, d_out, db, s);
    clkB.stamp();  // tail
    hipLaunchKernelGGL(sg_seg_tail, dim3((unsigned)n_calls), dim3(kTailT), 0, s, d_snd, P, d_out);
    HIPCHK(hipGetLastError());
    clkB.stamp();
  }
  HIPCHK(hipStreamSynchronize(s));
  if (kernel_ms) {
    clkA.finish();
    clkB.finish();
    kernel_ms[0] = msA[0];
    for (size_t ch = 0; ch < clkC.size(); ++ch) {
      clkC[ch]->finish();
      for (int k = 0; k < 3; ++k) kernel_ms[1 + k] += msC[ch][k];
    }
    kernel_ms[4] = msB[0];
    kernel_ms[5] = msB[1];
    if (behind) behind->finish(kernel_ms + 4);
  }
}

template <typename T>
void segment_device(const sg_segment_params& p, const std::vector<SegPlan>& plans, const T* d_x, const int64_t* offsets,
                    int64_t n_calls, double* d_out, const int64_t* out_off, hipStream_t s, double* kernel_ms) {
  segment_run<T>(p, plans, d_x, offsets, n_calls, d_out, out_off, s, kernel_ms, nullptr);
}

template void segment_device<float>(const sg_segment_params&, const std::vector<SegPlan>&, const float*, const int64_t*,
                                    int64_t, double*, const int64_t*, hipStream_t, double*);
template void segment_device<double>(const sg_segment_params&, const std::vector<SegPlan>&, const double*, const int64_t*,
                                     int64_t, double*, const int64_t*, hipStream_t, double*);

}  // namespace sg

namespace {

// sg_segment_sweep: n_rows parameter rows over n_calls sounds. The raw envelopes come from
// segment_run (once per sound); per envelope group one sg_seg_smooth launch over all sounds
// into the group's slots; then sg_seg_sweep_tail over chunks of consecutive rows whose pair
// workspaces fit the cap. Every kernel's work on a (sound, row) pair is the same whatever
// other rows and sounds share the launch and however the rows are chunked.
constexpr int kSweepLdsValues = 8192;  // 64 KiB of a CU's 160: two workgroups' envelopes
int g_sweep_staging = 1;               // sg_set_sweep_staging
sg::StageTimes<sg::kSegStages> g_sweep_ms;  // of the last profiled sweep

struct Sweep : SegBehind {
  int64_t n_calls = 0;
  std::vector<std::vector<sg::SegPlan>> plans;  // [group][sound]
  std::vector<SweepSlot> slots;                 // [group * n_calls + sound]
  std::vector<SweepRow> rows;
  std::vector<int64_t> chunk_end;               // one past the last row of each chunk
  int64_t env_cells = 0, work_cells = 0;
  int32_t max_m = 0;
  double* d_out = nullptr;
  double ms[2] = {0, 0};
  std::unique_ptr<sg::StageClock> clk;

  void launch(const std::vector<SegSound>& snds, const double* d_raw, sg::DevBuf& db, hipStream_t s,
              bool timed) override {
    clk.reset(new sg::StageClock(s, timed ? ms : nullptr, 2));
    double* d_env = db.get<double>((size_t)env_cells);
    clk->stamp();  // smoothing, group by group
    for (size_t g = 0; g < plans.size(); ++g) {
      std::vector<SegSound> gs = snds;  // the group's view of the sounds: where sg_seg_smooth writes
      std::vector<SegWin> wins;
      for (int64_t c = 0; c < n_calls; ++c) {
        gs[c].o0 = slots[g * n_calls + c].e0;
        if (plans[g][c].n1 > 0) push_windows(wins, c, plans[g][c]);
      }
      launch_smooth(sg::upload(db, gs, s), wins, d_raw, d_env, db, s);
    }
    clk->stamp();  // tails, chunk by chunk
    const SweepSlot* d_slots = sg::upload(db, slots, s);
    const SweepRow* d_rows = sg::upload(db, rows, s);
    double* d_work = db.get<double>((size_t)work_cells);
    const int32_t lds_values = g_sweep_staging ? std::min(max_m, (int32_t)kSweepLdsValues) : 0;
    const size_t lds = (size_t)lds_values * sizeof(double);
    sg::lds_opt_in(&sg_seg_sweep_tail, (int)lds, "sg_seg_sweep_tail");
    int64_t r0 = 0;
    for (int64_t r1 : chunk_end) {
      hipLaunchKernelGGL(sg_seg_sweep_tail, dim3((unsigned)((r1 - r0) * n_calls)), dim3(kTailT), lds, s, d_slots, d_rows,
                         r0, (int32_t)n_calls, lds_values, d_env, d_work, d_out);
      HIPCHK(hipGetLastError());
      r0 = r1;
    }
    clk->stamp();
  }
  void finish(double* out) override {
    clk->finish();
    out[0] = ms[0];
    out[1] = ms[1];
  }
};

std::string sweep_where(int64_t r, int64_t c) {
  return "sg_segment_sweep: row " + std::to_string(r) + (c >= 0 ? ", sound " + std::to_string(c) : std::string()) + ": ";
}

void segment_sweep(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                   const sg_segment_params* prow, int64_t n_rows, double* d_out) {
  const sg_segment_params& p0 = prow[0];
  Sweep W;
  W.n_calls = n_calls;
  W.d_out = d_out;
  W.rows.resize((size_t)n_rows);
  std::vector<std::pair<double, double>> keys;  // a group's (windowLength, clamped overlap)
  for (int64_t r = 0; r < n_rows; ++r) {  // every refusal comes before the first launch
    const sg_segment_params& p = prow[r];
    try {
      W.rows[r].P = sg::seg_pars(p);
    } catch (const sg::SgError& e) {
      throw sg::SgError(e.code, sweep_where(r, -1) + e.what());
    }
    if (p.samplingRate != p0.samplingRate || p.mode != 0 || p.workspace_cap != p0.workspace_cap)
      throw sg::SgError(SG_E_ARG, sweep_where(r, -1) + "samplingRate, mode = 0 and workspace_cap are those of row 0");
    const std::pair<double, double> key(p.windowLength, std::fmin(std::fmax(p.overlap, 0.0), 99.0));
    size_t g = 0;
    while (g < keys.size() && keys[g] != key) ++g;
    if (g == keys.size()) {
      keys.push_back(key);
      W.plans.emplace_back((size_t)n_calls);
      for (int64_t c = 0; c < n_calls; ++c) {
        if (lengths[c] < 3) continue;
        try {
          W.plans[g][c] = sg::seg_plan(p, lengths[c], true);
        } catch (const sg::SgError& e) {
          throw sg::SgError(e.code, sweep_where(r, c) + e.what());
        }
      }
    }
    W.rows[r].group = (int32_t)g;
  }
  const int64_t cap_cells =
      std::max<int64_t>(1, (p0.workspace_cap > 0 ? p0.workspace_cap : sg::kSegWorkspaceCap) / (int64_t)sizeof(double));
  std::vector<int64_t> row_cells(keys.size(), 0);
  W.slots.resize(keys.size() * (size_t)n_calls);
  for (size_t g = 0; g < keys.size(); ++g)
    for (int64_t c = 0; c < n_calls; ++c) {
      const sg::SegPlan& S = W.plans[g][c];
      SweepSlot& Q = W.slots[g * n_calls + c];
      Q = SweepSlot{W.env_cells, row_cells[g], S.timestep, (int32_t)S.m, 0};
      W.env_cells += sg::seg_env0() + S.m;
      row_cells[g] += sg::seg_pair_cells(S.m);
      W.max_m = std::max(W.max_m, Q.m);
    }
  int64_t work = 0, first = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    const int64_t need = row_cells[W.rows[r].group];
    if (r > first && (work + need > cap_cells || (r - first + 1) * n_calls > 2147483647LL)) {
      W.chunk_end.push_back(r);  // the cap is reached: this row opens the next chunk
      first = r;
      work = 0;
    }
    W.rows[r].w0 = work;
    work += need;
    W.work_cells = std::max(W.work_cells, work);
  }
  W.chunk_end.push_back(n_rows);
  HIPCHK(hipSetDevice(ctx->device));
  sg::segment_run<float>(p0, W.plans[0], d_wave, offsets, n_calls, nullptr, nullptr, ctx->stream, g_sweep_ms.sink(ctx), &W);
}

void sweep_fitness(sg_ctx* ctx, const double* d_matrix, int64_t n_rows, int64_t n_calls, int32_t width, int32_t column,
                   const double* key, double* fit) {
  HIPCHK(hipSetDevice(ctx->device));
  sg::DevBuf db;
  const double* d_key = sg::upload(db, std::vector<double>(key, key + n_calls), ctx->stream);
  double* d_fit = db.get<double>((size_t)n_rows);
  const int64_t per = kT / 64;
  hipLaunchKernelGGL(sg_sweep_fit, dim3((unsigned)((n_rows + per - 1) / per)), dim3(kT), 0, ctx->stream, d_matrix, n_rows,
                     n_calls, width, column, d_key, d_fit);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(fit, d_fit, (size_t)n_rows * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
}

}  // namespace

extern "C" {

int sg_segment_sweep(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_segment_params* rows, int64_t n_rows, double* d_out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || n_rows < 0 || (n_rows > 0 && !rows) || (n_calls > 0 && n_rows > 0 && !d_out)) sg::bad_arguments("sg_segment_sweep");
    sg::batch_args("sg_segment_sweep", n_calls, {d_wave, offsets, lengths});
    if (n_calls == 0 || n_rows == 0) return (int)SG_OK;
    segment_sweep(ctx, d_wave, offsets, lengths, n_calls, rows, n_rows, d_out);
    return (int)SG_OK;
  });
}

int sg_sweep_fitness(sg_ctx* ctx, const double* d_matrix, int64_t n_rows, int64_t n_calls, int32_t width, int32_t column,
                     const double* key, double* fit) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || n_rows < 0 || n_calls < 0 || width < 1 || column < 0 || column >= width ||
        (n_rows + 3) / 4 > 2147483647LL || (n_rows > 0 && (!fit || (n_calls > 0 && (!d_matrix || !key)))))
      throw sg::SgError(SG_E_ARG, "sg_sweep_fitness: bad arguments");
    if (n_rows == 0) return (int)SG_OK;
    sweep_fitness(ctx, d_matrix, n_rows, n_calls, width, column, key, fit);
    return (int)SG_OK;
  });
}

int sg_set_sweep_staging(int32_t mode) {
  if (mode != 0 && mode != 1) return SG_E_ARG;
  g_sweep_staging = mode;
  return SG_OK;
}

int sg_debug_sweep_kernel_ms(double* out) { return g_sweep_ms.read(out); }

int sg_segment(sg_ctx* ctx, const double* wave, int64_t len, const sg_segment_params* p, double* out) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !out) throw sg::SgError(SG_E_ARG, "sg_segment: bad arguments");
    const std::vector<sg::SegPlan> plans(1, sg::seg_plan(*p, len, p->mode == 0));
    const int64_t cells = sg::seg_out_cells(*p, plans[0]);
    HIPCHK(hipSetDevice(ctx->device));
    sg::single_sound(ctx, wave, len, cells, out, [&](const double* d, double* d_o) {
      const int64_t off[2] = {0, cells}, zero = 0;
      sg::segment_device<double>(*p, plans, d, &zero, 1, d_o, off, ctx->stream, g_seg_ms.sink(ctx));
    });
    return (int)SG_OK;
  });
}

int sg_segment_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_segment_params* p, double* d_out, const int64_t* out_off) {
  return sg::guarded(ctx, [&]() {
    if (!ctx || !p || p->mode != 0) sg::bad_arguments("sg_segment_batch");
    sg::batch_args("sg_segment_batch", n_calls, {d_wave, offsets, lengths, d_out, out_off});
    (void)sg::seg_pars(*p);
    std::vector<sg::SegPlan> plans(n_calls);  // every refusal comes before the first launch
    for (int64_t c = 0; c < n_calls; ++c)
      if (lengths[c] >= 3) plans[c] = sg::seg_plan(*p, lengths[c], true);
    if (n_calls == 0) return (int)SG_OK;
    HIPCHK(hipSetDevice(ctx->device));
    sg::segment_device<float>(*p, plans, d_wave, offsets, n_calls, d_out, out_off, ctx->stream, g_seg_ms.sink(ctx));
    return (int)SG_OK;
  });
}

int sg_debug_segment_kernel_ms(double* out) { return g_seg_ms.read(out); }

}  // extern "C"
