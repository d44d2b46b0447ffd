// sg_ssm.hip — ssm() on the device (R/SSM.R:63-360): tuneR melfcc(spec_out =
// TRUE) of a batch of sounds (the front end of sg_mel.hip, sg_mel_dev.h), then
// selfsim() and getNovelty().
//
//   sg_ssm_stats    tuneR::normalize's mean and max|x - mean| per sound (the
//                   numeric-vector path), one workgroup per 64 Ki samples and a
//                   fold per sound (sg_ssm_stats_fold); integer-valued samples sum
//                   exactly, so a wave with a zero sum centres to exact zeros
//   sg_ssm_frames   one workgroup per frame: centring and scaling on the fly,
//                   pre-emphasis, hamming, the real FFT's nfft / 2 powers (pspectrum)
//                   or their mel bands (aspectrum), no frame stripping
//   sg_ssm_feat     one workgroup per frame: the rows selfsim() sees -- for mfcc
//                   log, the requested DCT-II rows and the lifter weight -- and the
//                   optional zeroOne per frame; D x n_frames column-major, so a
//                   window's stacked vector as.vector(m[, a:(a + win - 1)]) is the
//                   contiguous run of D win doubles from frame a
//   sg_ssm_winstat  one wavefront per window: its mean (cor) and squared norm
//   sg_ssm_gram     the hot path: one wavefront per 16 x 16 tile of window pairs
//                   on or above the diagonal, accumulated over D win in steps of 4
//                   with v_mfma_f64_16x16x4_f64, divided by the norms, mirrored,
//                   and each sound's min / max / NaN flag (zeroOne has no na.rm)
//   sg_ssm_novelty  one wavefront per diagonal point: Pearson correlation of the
//                   zero-padded K x K patch (zeroOne applied on read) with the
//                   checkerboard kernel, two passes; 0 for a constant patch or a
//                   NaN matrix
//   sg_ssm_out      zeroOne of the matrices, when the caller asks for them
// fp64 throughout, for sg_mel.hip's reason: log of weak mel bands, zeroOne of a
// narrow similarity range and a correlation all amplify fp32 round-off past
// the 1e-6 parity bar.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sg_dev64.h"
#include "sg_launch.h"
#include "sg_mel.h"
#include "sg_mel_dev.h"
#include "sg_rmath.h"
#include "sg_ssm.h"

namespace {

using sg::DevBuf;
using sg::MelBand;
using sg::upload;

struct SsmSound {
  int64_t base, len;  // samples [base, base + len) of the input buffer
  int64_t cell0;      // first cell of its n x n matrix
  int32_t w0, n;      // windows [w0, w0 + n)
  int32_t L;          // doubles of a window's stacked vector (D win)
  int32_t ch0;        // first of its ceil(len / kStatChunk) chunks (sg_ssm_stats)
};

struct SsmFrame {
  int64_t base;
  int32_t o;    // frame start within the sound
  int32_t seg;  // samples of the frame inside the sound (<= winpts)
  int32_t snd;
  int32_t pad;
};

struct SsmTile {
  int32_t snd, ti, tj, pad;
};

struct SsmPoint {
  int32_t snd, i;
};

// per sound: min and max as order-preserving keys, and the NaN flag
struct SsmRange {
  unsigned long long lo, hi;
  int32_t nan, pad;
};

__device__ __forceinline__ double wmin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wor(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

// tuneR::normalize(unit = "32") as ssm() uses it: stat[2 c] = mean(x), stat[2 c + 1] =
// max|x - mean| (1 when all.equal(m, 0): no division). Two passes, each a kernel
// over chunks of kStatChunk samples (a long recording spreads over the CUs) and a
// fold per sound; every sum runs in a fixed order.
constexpr int kStatChunk = 1 << 16;

struct SsmChunk {
  int32_t snd, c;
};

template <typename T>
__global__ __launch_bounds__(256) void sg_ssm_stats(const T* __restrict__ x, const SsmChunk* __restrict__ chunks,
                                                    const SsmSound* __restrict__ snds, const double* __restrict__ stat,
                                                    int pass, double* __restrict__ part) {
  __shared__ double red[256];
  const SsmChunk J = chunks[blockIdx.x];
  const SsmSound S = snds[J.snd];
  const T* xc = x + S.base;
  const int64_t i0 = (int64_t)J.c * kStatChunk, i1 = S.len < i0 + kStatChunk ? S.len : i0 + kStatChunk;
  double acc = 0;
  if (pass == 0) {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc += (double)xc[i];
  } else {
    const double mean = stat[2 * J.snd];
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) acc = fmax(acc, fabs((double)xc[i] - mean));
  }
  acc = block_reduce<256>(acc, pass ? 2 : 0, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// one wavefront per sound: its chunks' partial sums into the mean (pass 0), their
// maxima into max|x - mean| (pass 1)
__global__ __launch_bounds__(64) void sg_ssm_stats_fold(const double* __restrict__ part,
                                                        const SsmSound* __restrict__ snds, int pass,
                                                        double* __restrict__ stat) {
  const SsmSound S = snds[blockIdx.x];
  const int nch = (int)((S.len + kStatChunk - 1) / kStatChunk);
  double acc = 0;
  for (int k = threadIdx.x; k < nch; k += 64) {
    const double v = part[S.ch0 + k];
    acc = pass ? fmax(acc, v) : acc + v;
  }
  acc = pass ? wmax(acc) : wsum(acc);
  if (threadIdx.x == 0) {
    if (pass == 0)
      stat[2 * blockIdx.x] = S.len > 0 ? acc / (double)S.len : 0.0;
    else
      stat[2 * blockIdx.x + 1] = acc > 1.5e-8 ? acc : 1.0;  // !isTRUE(all.equal(m, 0))
  }
}

// melfcc's pspectrum (bands == nullptr: R = M rows) or aspectrum (R = nb rows) of
// every frame, R x frames column-major
template <typename T>
__global__ __launch_bounds__(256) void sg_ssm_frames(const T* __restrict__ x, const SsmFrame* __restrict__ frames,
                                                     const double* __restrict__ stat, const double* __restrict__ ham,
                                                     const double2* __restrict__ tw, const double2* __restrict__ twN,
                                                     const MelBand* __restrict__ bands,
                                                     const double* __restrict__ wts, int winpts, int M, int logM,
                                                     int nb, double* __restrict__ raw) {
  extern __shared__ double2 lds[];
  double2* A = lds;
  double2* B = lds + M;
  const SsmFrame F = frames[blockIdx.x];
  const T* xc = x + F.base;
  double mean = 0, m = 1;
  if (stat) {
    mean = stat[2 * F.snd];
    m = stat[2 * F.snd + 1];
  }
  for (int n = threadIdx.x; n < M; n += blockDim.x) {
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * n + h;
      double s = 0;
      if (i < F.seg && i < winpts) {
        const int q = F.o + i;  // filter(x, c(1, -0.97), sides = 1): y[1] = x[1]
        s = ((double)xc[q] - mean) / m;
        if (q > 0) s -= 0.97 * (((double)xc[q - 1] - mean) / m);
        s *= ham[i];
      }
      v[h] = s;
    }
    A[n] = make_double2(v[0], v[1]);
  }
  __syncthreads();
  const double* P = sg::mel_frame_power(A, B, tw, twN, M, logM);
  if (bands) {
    for (int b = threadIdx.x; b < nb; b += blockDim.x) raw[(int64_t)blockIdx.x * nb + b] = sg::mel_band(bands[b], wts, P);
  } else {
    for (int k = threadIdx.x; k < M; k += blockDim.x) raw[(int64_t)blockIdx.x * M + k] = P[k];
  }
}

// The rows of one frame that selfsim() sees: dct != nullptr: lift[d] sum_b dct[d][b]
// log(raw[b]) (tuneR spec2cep + lifter), else a copy of the R rows; then the
// optional zeroOne of the frame (apply(m, 2, zeroOne); a NaN makes the frame NaN)
__global__ __launch_bounds__(256) void sg_ssm_feat(const double* __restrict__ raw, int R, const double* __restrict__ dct,
                                                   const double* __restrict__ lift, int D, int norm,
                                                   double* __restrict__ feat) {
  extern __shared__ double sh[];  // R logs, then D values
  __shared__ double rlo[256], rhi[256];
  __shared__ int rnan[256];
  double* lg = sh;
  double* v = sh + R;
  const double* rc = raw + (int64_t)blockIdx.x * R;
  if (dct) {
    for (int b = threadIdx.x; b < R; b += 256) lg[b] = log(rc[b]);
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
      const double* row = dct + (int64_t)d * R;
      double acc = 0;
      for (int b = 0; b < R; ++b) acc += row[b] * lg[b];
      v[d] = lift[d] * acc;
    }
  } else {
    for (int d = threadIdx.x; d < D; d += 256) v[d] = rc[d];
  }
  __syncthreads();
  double lo = 0, den = 1;
  int bad = 0;
  if (norm) {
    double l = INFINITY, h = -INFINITY;
    int nn = 0;
    for (int d = threadIdx.x; d < D; d += 256) {
      l = fmin(l, v[d]);
      h = fmax(h, v[d]);
      nn |= isnan(v[d]) ? 1 : 0;
    }
    rlo[threadIdx.x] = l;
    rhi[threadIdx.x] = h;
    rnan[threadIdx.x] = nn;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (threadIdx.x < o) {
        rlo[threadIdx.x] = fmin(rlo[threadIdx.x], rlo[threadIdx.x + o]);
        rhi[threadIdx.x] = fmax(rhi[threadIdx.x], rhi[threadIdx.x + o]);
        rnan[threadIdx.x] |= rnan[threadIdx.x + o];
      }
      __syncthreads();
    }
    lo = rlo[0];
    den = rhi[0] - rlo[0];
    bad = rnan[0];
  }
  double* out = feat + (int64_t)blockIdx.x * D;
  for (int d = threadIdx.x; d < D; d += 256) out[d] = norm ? (bad ? NAN : (v[d] - lo) / den) : v[d];
}

// per window: its mean (cor; 0 for cosine) and the squared norm of what the Gram sees
__global__ __launch_bounds__(64) void sg_ssm_winstat(const double* __restrict__ feat,
                                                     const int64_t* __restrict__ wstart,
                                                     const int32_t* __restrict__ wsnd,
                                                     const SsmSound* __restrict__ snds, int cor,
                                                     double* __restrict__ wmean, double* __restrict__ wnn) {
  const int w = blockIdx.x;
  const int L = snds[wsnd[w]].L;
  const double* p = feat + wstart[w];
  double mean = 0;
  if (cor) {
    double s = 0;
    for (int k = threadIdx.x; k < L; k += 64) s += p[k];
    mean = wsum(s) / L;
  }
  double q = 0;
  for (int k = threadIdx.x; k < L; k += 64) {
    const double a = p[k] - mean;
    q += a * a;
  }
  q = wsum(q);
  if (threadIdx.x == 0) {
    wmean[w] = mean;
    wnn[w] = q;
  }
}

typedef double v4f64 __attribute__((ext_vector_type(4)));

// One wavefront per 16 x 16 tile (ti <= tj) of one sound's window pairs.
// v_mfma_f64_16x16x4_f64 operands: lane t holds A[row t & 15][k = t >> 4] and
// B[k = t >> 4][col t & 15]; its 4 results are D[row (t >> 4) + 4 r][col t & 15],
// r = 0..3 (the f64 map, not the f32 one). A's rows are the windows of tile ti, B's
// columns those of tile tj; rows / columns past n and k past L contribute zeros
// and are neither written nor reduced. raw != 0: the unnormalised Gram (test hook).
__global__ __launch_bounds__(64) void sg_ssm_gram(const SsmTile* __restrict__ tiles, const SsmSound* __restrict__ snds,
                                                  const double* __restrict__ feat, const int64_t* __restrict__ wstart,
                                                  const double* __restrict__ wmean, const double* __restrict__ wnn,
                                                  int raw, double* __restrict__ ssm, SsmRange* __restrict__ range) {
  const SsmTile T = tiles[blockIdx.x];
  const SsmSound S = snds[T.snd];
  const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
  const int ia = T.ti * 16 + r16, jb = T.tj * 16 + r16;
  const bool va = ia < S.n, vb = jb < S.n;
  const double* pa = feat + (va ? wstart[S.w0 + ia] : 0);
  const double* pb = feat + (vb ? wstart[S.w0 + jb] : 0);
  const double ma = va ? wmean[S.w0 + ia] : 0.0, mb = vb ? wmean[S.w0 + jb] : 0.0;
  v4f64 acc = {0, 0, 0, 0};
  for (int k0 = 0; k0 < S.L; k0 += 4) {
    const int k = k0 + kq;
    const bool vk = k < S.L;
    const double a = (va && vk) ? pa[k] - ma : 0.0;
    const double b = (vb && vk) ? pb[k] - mb : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  const int j = T.tj * 16 + r16;
  const double nj = j < S.n ? wnn[S.w0 + j] : 0.0;
  double lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  double* out = ssm + S.cell0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = T.ti * 16 + kq + 4 * r;
    if (i < S.n && j < S.n) {
      const double v = raw ? acc[r] : acc[r] / sqrt(wnn[S.w0 + i] * nj);
      out[(int64_t)i + (int64_t)j * S.n] = v;
      if (T.ti != T.tj) out[(int64_t)j + (int64_t)i * S.n] = v;
      lo = fmin(lo, v);
      hi = fmax(hi, v);
      bad |= isnan(v) ? 1 : 0;
    }
  }
  lo = wmin(lo);
  hi = wmax(hi);
  bad = wor(bad);
  if (lane == 0) {
    SsmRange* R = range + T.snd;
    if (lo <= hi) {
      atomicMin(&R->lo, dkey(lo));
      atomicMax(&R->hi, dkey(hi));
    }
    if (bad) atomicOr(&R->nan, 1);
  }
}

// One wavefront per diagonal point i of one sound: cor(as.vector(ssm_padded[n, n]),
// as.vector(kernel)), n = (i - K / 2):(i + K / 2 - 1), zeros outside the matrix;
// kc is the kernel minus its mean, kss its sum of squares. NA becomes 0.
__global__ __launch_bounds__(64) void sg_ssm_novelty(const SsmPoint* __restrict__ pts, const SsmSound* __restrict__ snds,
                                                     const double* __restrict__ ssm, const SsmRange* __restrict__ range,
                                                     const double* __restrict__ kc, double kss, int K,
                                                     const int64_t* __restrict__ nov0, double* __restrict__ nov) {
  const SsmPoint Pt = pts[blockIdx.x];
  const SsmSound S = snds[Pt.snd];
  const SsmRange R = range[Pt.snd];
  double* out = nov + nov0[Pt.snd] + Pt.i;
  const double mn = dunkey(R.lo), den = dunkey(R.hi) - mn;
  if (R.nan || !(den > 0)) {  // zeroOne without na.rm (or 0 / 0): the whole matrix is NaN
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  const double* m = ssm + S.cell0;
  const int h = K / 2, KK = K * K, n = S.n;
  double s = 0, lo = INFINITY, hi = -INFINITY;
  for (int e = threadIdx.x; e < KK; e += 64) {
    const int gi = Pt.i - h + e / K, gj = Pt.i - h + e % K;
    const double v = (gi >= 0 && gi < n && gj >= 0 && gj < n) ? (m[(int64_t)gi + (int64_t)gj * n] - mn) / den : 0.0;
    s += v;
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  const double mp = wsum(s) / KK;
  lo = wmin(lo);
  hi = wmax(hi);
  double pk = 0, pp = 0;
  for (int e = threadIdx.x; e < KK; e += 64) {
    const int gi = Pt.i - h + e / K, gj = Pt.i - h + e % K;
    const double v = (gi >= 0 && gi < n && gj >= 0 && gj < n) ? (m[(int64_t)gi + (int64_t)gj * n] - mn) / den : 0.0;
    const double a = v - mp;
    pk += a * kc[e];
    pp += a * a;
  }
  pk = wsum(pk);
  pp = wsum(pp);
  if (threadIdx.x == 0) {
    const double d = sqrt(pp * kss);
    *out = (hi > lo && d > 0) ? pk / d : 0.0;
  }
}

// zeroOne of each sound's matrix in place (blockIdx.x = sound, blockIdx.y = its share)
__global__ __launch_bounds__(256) void sg_ssm_out(const SsmSound* __restrict__ snds, const SsmRange* __restrict__ range,
                                                  double* __restrict__ ssm) {
  const SsmSound S = snds[blockIdx.x];
  const SsmRange R = range[blockIdx.x];
  const int64_t cells = (int64_t)S.n * S.n;
  const double mn = dunkey(R.lo), den = dunkey(R.hi) - mn;
  double* m = ssm + S.cell0;
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < cells; e += (int64_t)gridDim.y * 256)
    m[e] = R.nan ? NAN : (m[e] - mn) / den;
}

constexpr int kSsmStages = 7;  // stats, frames, feat, winstat, gram, novelty, out
sg::StageTimes<kSsmStages> g_ssm_ms;  // of the last profiled launch sequence (sg_debug_ssm_kernel_ms)
constexpr int64_t kMaxCells = (int64_t)1 << 28;  // 2 GiB of fp64 cells per launch sequence

}  // namespace

namespace sg {

template <typename T>
void ssm_device(const SsmSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                int32_t* n_out, double* novelty_out, const int64_t* novelty_off, double* ssm_out,
                const int64_t* ssm_off, hipStream_t s, double* kernel_ms) {
  const MelGeom g = mel_geom(S.sr, S.windowLength, S.step, S.maxFreq, S.nb, 0.0);
  const std::vector<double> kern = ssm_checkerboard(S.K, S.kernelSD);
  const int M = g.nfreqs;
  const int R = S.input == 2 ? M : g.nb;                     // rows the frame kernel writes
  const int D = S.input == 0 ? (int)S.mfcc.size() : R;       // rows selfsim() sees
  // host: frames, windows, tiles and diagonal points of every sound
  std::vector<SsmSound> snds(n_calls);
  std::vector<SsmFrame> fr;
  std::vector<int64_t> wstart, nov0(n_calls);
  std::vector<int32_t> wsnd;
  std::vector<SsmTile> tiles;
  std::vector<SsmPoint> pts;
  std::vector<SsmChunk> chunks;
  int64_t cells = 0, npts = 0;
  int nmax = 0;
  for (int64_t c = 0; c < n_calls; ++c) {
    const SsmDims d = ssm_dims(S, lengths[c]);
    SsmSound& Q = snds[c];
    Q.base = offsets[c];
    Q.len = std::max<int64_t>(lengths[c], 0);
    Q.cell0 = cells;
    Q.w0 = (int32_t)wstart.size();
    Q.n = (int32_t)d.idx.size();
    Q.L = D * d.win;
    Q.ch0 = (int32_t)chunks.size();
    nov0[c] = npts;
    n_out[c] = Q.n;
    if (Q.n == 0) {
      Q.len = 0;
      continue;
    }
    for (int64_t k = 0; k * kStatChunk < Q.len; ++k) chunks.push_back(SsmChunk{(int32_t)c, (int32_t)k});
    const int64_t f0 = (int64_t)fr.size();
    for (int f = 0; f < d.nf; ++f) {
      const int64_t o = (int64_t)f * g.steppts;
      fr.push_back(SsmFrame{offsets[c], (int32_t)o, (int32_t)std::min<int64_t>(g.winpts, lengths[c] - o), (int32_t)c, 0});
    }
    for (int32_t a : d.idx) {
      wstart.push_back((f0 + a) * D);
      wsnd.push_back((int32_t)c);
    }
    const int nt = (Q.n + 15) / 16;
    for (int ti = 0; ti < nt; ++ti)
      for (int tj = ti; tj < nt; ++tj) tiles.push_back(SsmTile{(int32_t)c, ti, tj, 0});
    for (int i = 0; i < Q.n; ++i) pts.push_back(SsmPoint{(int32_t)c, i});
    cells += (int64_t)Q.n * Q.n;
    npts += Q.n;
    nmax = std::max(nmax, (int)Q.n);
    if (cells > kMaxCells)
      throw SgError(SG_E_UNSUPPORTED, "ssm: the self-similarity matrices of one launch exceed 2^28 cells");
  }
  if (npts == 0) return;
  if ((int64_t)fr.size() * std::max(R, D) > ((int64_t)1 << 31))
    throw SgError(SG_E_UNSUPPORTED, "ssm: the frames of one launch exceed 2^31 spectrum cells");
  const int64_t F = (int64_t)fr.size(), W = (int64_t)wstart.size();
  DevBuf db;
  const SsmSound* d_snd = upload(db, snds, s);
  const SsmFrame* d_fr = upload(db, fr, s);
  const int64_t* d_ws = upload(db, wstart, s);
  const int32_t* d_wsnd = upload(db, wsnd, s);
  const SsmTile* d_tiles = upload(db, tiles, s);
  const SsmPoint* d_pts = upload(db, pts, s);
  const int64_t* d_nov0 = upload(db, nov0, s);
  const double* d_ham = upload(db, g.ham, s);
  const double2* d_tw = reinterpret_cast<const double2*>(upload(db, g.tw, s));
  const double2* d_twN = reinterpret_cast<const double2*>(upload(db, g.twN, s));
  std::vector<MelBand> bands(g.nb);
  for (int b = 0; b < g.nb; ++b) bands[b] = MelBand{g.band_k0[b], g.band_n[b], g.band_w0[b], 0};
  const MelBand* d_bands = upload(db, bands, s);
  const double* d_w = upload(db, g.w, s);
  // the kernel minus its mean, and its sum of squares
  std::vector<double> kc(kern);
  double km = 0, kss = 0;
  for (double v : kc) km += v;
  km /= (double)kc.size();
  for (double& v : kc) {
    v -= km;
    kss += v * v;
  }
  const double* d_kc = upload(db, kc, s);
  std::vector<SsmRange> r0(n_calls, SsmRange{~0ull, 0ull, 0, 0});
  SsmRange* d_range = upload(db, r0, s);
  StageClock clk(s, kernel_ms, kSsmStages);
  clk.stamp();
  double* d_stat = nullptr;
  if (S.normalize) {
    d_stat = db.get<double>((size_t)2 * n_calls);
    const SsmChunk* d_ch = upload(db, chunks, s);
    double* d_part = db.get<double>(chunks.size());
    for (int pass = 0; pass < 2; ++pass) {
      hipLaunchKernelGGL(sg_ssm_stats<T>, dim3((unsigned)chunks.size()), dim3(256), 0, s, d_x, d_ch, d_snd, d_stat, pass,
                         d_part);
      HIPCHK(hipGetLastError());
      hipLaunchKernelGGL(sg_ssm_stats_fold, dim3((unsigned)n_calls), dim3(64), 0, s, d_part, d_snd, pass, d_stat);
      HIPCHK(hipGetLastError());
    }
  }
  clk.stamp();
  double* d_raw = db.get<double>((size_t)F * R);
  int logM = 0;
  while ((1 << logM) < M) ++logM;
  hipLaunchKernelGGL(sg_ssm_frames<T>, dim3((unsigned)F), dim3(256), (size_t)2 * M * sizeof(double2), s, d_x, d_fr,
                     d_stat, d_ham, d_tw, d_twN, S.input == 2 ? nullptr : d_bands, d_w, g.winpts, M, logM, g.nb, d_raw);
  HIPCHK(hipGetLastError());
  clk.stamp();
  double* d_feat = d_raw;  // audiogram / spectrum without norm: the rows as they are
  if (S.input == 0 || S.norm) {
    const double *d_dct = nullptr, *d_lift = nullptr;
    if (S.input == 0) {
      std::vector<double> dct, lift;
      ssm_dct(S, dct, lift);
      d_dct = upload(db, dct, s);
      d_lift = upload(db, lift, s);
    }
    d_feat = db.get<double>((size_t)F * D);
    hipLaunchKernelGGL(sg_ssm_feat, dim3((unsigned)F), dim3(256), (size_t)(R + D) * sizeof(double), s, d_raw, R, d_dct,
                       d_lift, D, S.norm, d_feat);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();
  double* d_wmean = db.get<double>((size_t)W);
  double* d_wnn = db.get<double>((size_t)W);
  hipLaunchKernelGGL(sg_ssm_winstat, dim3((unsigned)W), dim3(64), 0, s, d_feat, d_ws, d_wsnd, d_snd, S.simil == 1,
                     d_wmean, d_wnn);
  HIPCHK(hipGetLastError());
  double* d_ssm = db.get<double>((size_t)cells);
  clk.stamp();
  hipLaunchKernelGGL(sg_ssm_gram, dim3((unsigned)tiles.size()), dim3(64), 0, s, d_tiles, d_snd, d_feat, d_ws, d_wmean,
                     d_wnn, 0, d_ssm, d_range);
  HIPCHK(hipGetLastError());
  double* d_nov = db.get<double>((size_t)npts);
  clk.stamp();
  hipLaunchKernelGGL(sg_ssm_novelty, dim3((unsigned)npts), dim3(64), 0, s, d_pts, d_snd, d_ssm, d_range, d_kc, kss, S.K,
                     d_nov0, d_nov);
  HIPCHK(hipGetLastError());
  clk.stamp();
  std::vector<double> hn((size_t)npts), hs;
  HIPCHK(hipMemcpyAsync(hn.data(), d_nov, hn.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  if (ssm_out) {
    const int64_t per = (int64_t)nmax * nmax;
    hipLaunchKernelGGL(sg_ssm_out, dim3((unsigned)n_calls, (unsigned)std::min<int64_t>((per + 255) / 256, 1024)),
                       dim3(256), 0, s, d_snd, d_range, d_ssm);
    HIPCHK(hipGetLastError());
    clk.stamp();
    hs.resize((size_t)cells);
    HIPCHK(hipMemcpyAsync(hs.data(), d_ssm, hs.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
  for (int64_t c = 0; c < n_calls; ++c) {
    const int64_t n = snds[c].n;
    if (n == 0) continue;
    std::memcpy(novelty_out + novelty_off[c], hn.data() + nov0[c], (size_t)n * sizeof(double));
    if (ssm_out) std::memcpy(ssm_out + ssm_off[c], hs.data() + snds[c].cell0, (size_t)(n * n) * sizeof(double));
  }
}

template void ssm_device<float>(const SsmSetup&, const float*, const int64_t*, const int64_t*, int64_t, int32_t*, double*,
                                const int64_t*, double*, const int64_t*, hipStream_t, double*);
template void ssm_device<double>(const SsmSetup&, const double*, const int64_t*, const int64_t*, int64_t, int32_t*,
                                 double*, const int64_t*, double*, const int64_t*, hipStream_t, double*);

void ssm_debug_gram(const double* feat, int L, int n, double* out, hipStream_t s) {
  DevBuf db;
  std::vector<SsmSound> snds(1, SsmSound{0, 0, 0, 0, n, L, 0});
  std::vector<int64_t> wstart(n);
  for (int i = 0; i < n; ++i) wstart[i] = (int64_t)i * L;
  std::vector<SsmTile> tiles;
  const int nt = (n + 15) / 16;
  for (int ti = 0; ti < nt; ++ti)
    for (int tj = ti; tj < nt; ++tj) tiles.push_back(SsmTile{0, ti, tj, 0});
  const SsmSound* d_snd = upload(db, snds, s);
  const int64_t* d_ws = upload(db, wstart, s);
  const SsmTile* d_tiles = upload(db, tiles, s);
  const double* d_feat = upload(db, std::vector<double>(feat, feat + (size_t)n * L), s);
  const double* d_zero = upload(db, std::vector<double>((size_t)n, 0.0), s);
  SsmRange* d_range = upload(db, std::vector<SsmRange>(1, SsmRange{~0ull, 0ull, 0, 0}), s);
  double* d_ssm = db.get<double>((size_t)n * n);
  hipLaunchKernelGGL(sg_ssm_gram, dim3((unsigned)tiles.size()), dim3(64), 0, s, d_tiles, d_snd, d_feat, d_ws, d_zero,
                     d_zero, 1, d_ssm, d_range);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_ssm, (size_t)n * n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
}

}  // namespace sg

// The C entry points live here, not in sg_api.cpp: the host-only sanitizer build
// links sg_api.cpp without this file's device code.
using sg::guarded;

extern "C" {

int sg_ssm(sg_ctx* ctx, const double* wave, int64_t len, const sg_ssm_params* p, double* ssm_out,
           double* novelty_out) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || !wave || !novelty_out) throw sg::SgError(SG_E_ARG, "sg_ssm: bad arguments");
    if (len < 2) throw sg::SgError(SG_E_ARG, "sg_ssm: the sound must be longer than 1 sample");
    HIPCHK(hipSetDevice(ctx->device));
    const sg::SsmSetup S = sg::ssm_setup(*p);
    DevBuf db;
    const double* d = sg::upload_sound(db, wave, len, ctx->stream);
    const int64_t off = 0;
    int32_t n = 0;
    sg::ssm_device<double>(S, d, &off, &len, 1, &n, novelty_out, &off, ssm_out, &off, ctx->stream,
                           g_ssm_ms.sink(ctx));
    return SG_OK;
  });
}

int sg_ssm_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                 const sg_ssm_params* p, int32_t* n_out, double* novelty_out, const int64_t* novelty_off,
                 double* ssm_out, const int64_t* ssm_off) {
  return guarded(ctx, [&]() {
    if (!ctx || !p || n_calls < 0 ||
        (n_calls > 0 && (!d_wave || !offsets || !lengths || !n_out || !novelty_out || !novelty_off)) ||
        (ssm_out && !ssm_off))
      throw sg::SgError(SG_E_ARG, "sg_ssm_batch: bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    const sg::SsmSetup S = sg::ssm_setup(*p);
    if (n_calls == 0) return SG_OK;
    sg::ssm_device<float>(S, d_wave, offsets, lengths, n_calls, n_out, novelty_out, novelty_off, ssm_out, ssm_off,
                          ctx->stream, g_ssm_ms.sink(ctx));
    return SG_OK;
  });
}

int sg_debug_ssm_gram(sg_ctx* ctx, const double* feat, int32_t L, int32_t n, double* out) {
  return guarded(ctx, [&]() {
    if (!ctx || !feat || !out || L < 1 || n < 1 || n > 4096) throw sg::SgError(SG_E_ARG, "sg_debug_ssm_gram: bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    sg::ssm_debug_gram(feat, L, n, out, ctx->stream);
    return SG_OK;
  });
}

int sg_debug_ssm_kernel_ms(double* out) { return g_ssm_ms.read(out); }

}  // extern "C"
