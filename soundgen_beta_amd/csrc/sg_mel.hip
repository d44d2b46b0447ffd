// sg_mel.hip — compareSounds() on the device (R/matchPars.R:313-416), the
// similarity metric of matchPars(): getMelSpec()
// (R/matchPars.R:510-560 = tuneR 1.3.2 melfcc(spec_out = TRUE)$aspectrum:
// tuneR/R/melfcc.R, powspec.R, audspec.R, fft2melmx.R, hz2mel.R, mel2hz.R;
// signal 0.7-6 specgram.R, hamming.R) of a batch of sounds and the per-column
// cor / cosine / pixel / dtw of (target, candidate) pairs of them.
//
//   sg_mel_frames   one workgroup per frame: pre-emphasis 0.97 on the fly,
//                   hamming(winpts), zero-padded real nfft-point FFT (complex
//                   nfft/2 radix-2 Stockham in LDS + untangling; nfft <= 4096), |X|^2 of the
//                   first nfft/2 bins, the Slaney mel bands (sparse triangles),
//                   and the column's mean (soundgen's frame stripping)
//   sg_mel_cand     one workgroup per candidate: kept columns (colMeans >
//                   2^(throwaway/10)) compacted in order, their min and max (log01)
//   sg_mel_out      the normalised kept columns of one spectrum (getMelSpec's value)
// and, over what the first two kernels leave in HBM (a MelRun; sg::MelSet keeps one), the one
// comparison path of sg_compare_sounds_pairs and sg_compare_sounds_batch (whose target is a
// run made from getMelSpec's value: one sound, already normalised):
//   sg_mel_pair     one wavefront per (pair, output column) of a list of (target,
//                   candidate) pairs of two runs: matchColumns' central NA padding of
//                   the shorter spectrum, both columns log01-normalised on the fly (a
//                   ready-made target's is read as it stands), then cor, cosine, pixel
//                   and the dtw package's symmetric2 distance (anti-diagonal wavefront
//                   in LDS; mel_column_sims)
//   sg_mel_pair_reduce  compareSounds' reduction of each pair's columns in index order
//                   and the summary over the methods: 4 + 1 doubles per pair
// Everything is fp64: R computes in doubles, and the log01 spectra of weak
// bins amplify an fp32 FFT's absolute error past the 1e-6 parity bar.
// HBM-light: each candidate sample is read ~2x (50 % overlap), the work is the
// nfft log nfft FFT per frame and 200^2 DTW cells per column.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sg_dev64.h"
#include "sg_launch.h"
#include "sg_mel.h"
#include "sg_mel_dev.h"
#include "sg_rmath.h"

namespace {

struct MelFrame {
  int64_t base;  // candidate sample 0 in the input buffer
  int32_t o;     // frame start within the candidate
  int32_t seg;   // samples of the frame inside the candidate (<= winpts)
};

using sg::MelBand;

struct MelCand {
  int32_t f0, nf;  // frames [f0, f0 + nf)
  int32_t job0;    // first column job
  int32_t pad;
};

template <typename T>
__global__ __launch_bounds__(256) void sg_mel_frames(const T* __restrict__ x, const MelFrame* __restrict__ frames,
                                                     const double* __restrict__ ham, const double2* __restrict__ tw,
                                                     const double2* __restrict__ twN, const MelBand* __restrict__ bands,
                                                     const double* __restrict__ wts, int winpts, int M, int logM,
                                                     int nb, double* __restrict__ spec,
                                                     double* __restrict__ colmean) {
  extern __shared__ double2 lds[];
  double2* A = lds;
  double2* B = lds + M;
  __shared__ double red[256];
  const MelFrame F = frames[blockIdx.x];
  const T* xc = x + F.base;
  // windowed, pre-emphasised frame packed as z[n] = xw[2n] + i xw[2n+1]
  for (int n = threadIdx.x; n < M; n += blockDim.x) {
    double v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = 2 * n + h;
      double s = 0;
      if (i < F.seg && i < winpts) {
        const int q = F.o + i;  // filter(x, c(1, -0.97), sides = 1): y[1] = x[1]
        s = (double)xc[q];
        if (q > 0) s -= 0.97 * (double)xc[q - 1];
        s *= ham[i];
      }
      v[h] = s;
    }
    A[n] = make_double2(v[0], v[1]);
  }
  __syncthreads();
  const double* P = sg::mel_frame_power(A, B, tw, twN, M, logM);
  double part = 0;
  for (int b = threadIdx.x; b < nb; b += blockDim.x) {
    const double acc = sg::mel_band(bands[b], wts, P);
    spec[(int64_t)blockIdx.x * nb + b] = acc;
    part += acc;
  }
  red[threadIdx.x] = part;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) colmean[blockIdx.x] = red[0] / nb;
}

// kept columns in frame order (colMeans(spec) > thr) and their min / max
__global__ __launch_bounds__(256) void sg_mel_cand(const MelCand* __restrict__ cands, const double* __restrict__ spec,
                                                   const double* __restrict__ colmean, double thr, int nb,
                                                   int32_t* __restrict__ kept, int32_t* __restrict__ nkept,
                                                   double* __restrict__ mn, double* __restrict__ mx) {
  __shared__ int32_t sc[256];
  __shared__ double rmn[256], rmx[256];
  const MelCand C = cands[blockIdx.x];
  int32_t run = 0;
  for (int c0 = 0; c0 < C.nf; c0 += 256) {
    const int f = c0 + threadIdx.x;
    const int flag = f < C.nf && colmean[C.f0 + f] > thr;
    sc[threadIdx.x] = flag;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const int v = threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
      __syncthreads();
      sc[threadIdx.x] += v;
      __syncthreads();
    }
    if (flag) kept[C.f0 + run + sc[threadIdx.x] - 1] = C.f0 + f;
    run += sc[255];
    __syncthreads();
  }
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t e = threadIdx.x; e < (int64_t)run * nb; e += 256) {
    const double v = spec[(int64_t)kept[C.f0 + e / nb] * nb + e % nb];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  rmn[threadIdx.x] = lo;
  rmx[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      rmn[threadIdx.x] = fmin(rmn[threadIdx.x], rmn[threadIdx.x + o]);
      rmx[threadIdx.x] = fmax(rmx[threadIdx.x], rmx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    nkept[blockIdx.x] = run;
    mn[blockIdx.x] = rmn[0];
    mx[blockIdx.x] = rmx[0];
  }
}

// log01 of one kept column (melfcc + soundgen's log01: log(v - min + 1) / log(max - min + 1))
__device__ __forceinline__ double log01(double v, double lo, double den) { return log(v - lo + 1.0) / den; }

// central NA padding of matchColumns(m, ncol) (matchLengths 'central'): output
// column j shows column j + off of the short matrix, NA outside [0, mcols)
__device__ __forceinline__ int pad_off(int ncol, int mcols) { return (ncol + mcols + 2) / 2 - 1 - ncol; }

// cor, cosine, pixel and the dtw package's symmetric2 similarity of one pair of columns in
// LDS, by one wavefront: t and d hold the nb values of the two columns, lane l having written
// (and read back here) entries l, l + 64, ...; st and sd are the lane's partial sums of them;
// D0 is 3 nb doubles of scratch. Lane 0 writes out[0..3]. sg_mel_pair is its only caller, so
// a column pair has one value whichever entry scores it.
__device__ __forceinline__ void mel_column_sims(const double* t, const double* d, double* D0, int nb, double st,
                                                double sd, int do_dtw, double* __restrict__ out) {
  double* D1 = D0 + nb;
  double* D2 = D1 + nb;
  st = wsum(st);
  sd = wsum(sd);
  const double mt = st / nb, md = sd / nb;
  double ab = 0, aa = 0, bb = 0, td = 0, tt = 0, dd = 0, ad = 0;
  for (int b = threadIdx.x; b < nb; b += 64) {
    const double a = t[b] - mt, e = d[b] - md;
    ab += a * e;
    aa += a * a;
    bb += e * e;
    td += t[b] * d[b];
    tt += t[b] * t[b];
    dd += d[b] * d[b];
    ad += fabs(t[b] - d[b]);
  }
  ab = wsum(ab);
  aa = wsum(aa);
  bb = wsum(bb);
  td = wsum(td);
  tt = wsum(tt);
  dd = wsum(dd);
  ad = wsum(ad);
  double dtw = NAN;
  if (do_dtw) {
    // symmetric2 DP (dtw package default; the host restatement is sg_dtw_symmetric2):
    // g(i, j) = min(g(i-1, j-1) + 2 d, g(i-1, j) + d, g(i, j-1) + d), d = |t_i - d_j|;
    // anti-diagonal a = i + j, entries indexed by i (D1: a - 1, D2: a - 2)
    __syncthreads();
    for (int a = 0; a <= 2 * nb - 2; ++a) {
      const int i0 = a - (nb - 1) > 0 ? a - (nb - 1) : 0, i1 = a < nb - 1 ? a : nb - 1;
      for (int i = i0 + threadIdx.x; i <= i1; i += 64) {
        const int jj = a - i;
        const double dist = fabs(t[i] - d[jj]);
        double g;
        if (a == 0) {
          g = dist;
        } else {
          g = INFINITY;
          if (i > 0 && jj > 0) g = fmin(g, D2[i - 1] + 2 * dist);
          if (i > 0) g = fmin(g, D1[i - 1] + dist);
          if (jj > 0) g = fmin(g, D1[i] + dist);
        }
        D0[i] = g;
      }
      __syncthreads();
      double* r = D2;
      D2 = D1;
      D1 = D0;
      D0 = r;
    }
    dtw = 1.0 - D1[nb - 1] / (double)(2 * nb);
  }
  if (threadIdx.x == 0) {
    const double cden = sqrt(aa * bb);
    out[0] = cden > 0 ? ab / cden : NAN;
    out[1] = td / sqrt(tt * dd);
    out[2] = 1.0 - ad / nb;
    out[3] = dtw;
  }
}

// One job of sg_mel_pair: jobs [job0[p], job0[p + 1]) are the output columns of pair p
// (a bound from the frame counts before dropping; the columns past the pair's own count leave at once)
__device__ __forceinline__ int64_t mel_pair_of_job(const int64_t* __restrict__ job0, int64_t n_pairs, int64_t job) {
  int64_t lo = 0, hi = n_pairs;  // job0[lo] <= job < job0[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (job0[mid] <= job) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One wavefront per (pair, output column): column j of compareSounds(target = sound pairs[2 p]
// of the run T, cand = sound pairs[2 p + 1] of the run C), both read from the runs' raw band
// spectra and log01-normalised here with the sound's own min and max (readyT: specT holds
// normalised values already, read as they stand; mnT and mxT are not read); the shorter side
// gets matchColumns' central NA padding. sims[4 job + m], m = cor, cosine, pixel, dtw.
__global__ __launch_bounds__(64) void sg_mel_pair(
    const int32_t* __restrict__ pairs, const int64_t* __restrict__ job0, int64_t n_pairs, int nb,
    const double* __restrict__ specT, const int32_t* __restrict__ keptT, const MelCand* __restrict__ sndT,
    const int32_t* __restrict__ nkeptT, const double* __restrict__ mnT, const double* __restrict__ mxT, int readyT,
    const double* __restrict__ specC, const int32_t* __restrict__ keptC, const MelCand* __restrict__ sndC,
    const int32_t* __restrict__ nkeptC, const double* __restrict__ mnC, const double* __restrict__ mxC, int do_dtw,
    double* __restrict__ sims) {
  extern __shared__ double sh[];
  double* t = sh;
  double* d = sh + nb;
  const int64_t p = mel_pair_of_job(job0, n_pairs, (int64_t)blockIdx.x);
  const int j = (int)((int64_t)blockIdx.x - job0[p]);
  const int ti = pairs[2 * p], ci = pairs[2 * p + 1];
  const int ncT = nkeptT[ti], nk = nkeptC[ci];
  const int ncol = nk > ncT ? nk : ncT;
  if (j >= ncol) return;
  double* out = sims + (int64_t)blockIdx.x * 4;
  int tj = j, cj = j;
  if (ncT < ncol) tj = j + pad_off(ncol, ncT);
  if (nk < ncol) cj = j + pad_off(ncol, nk);
  const double lo = mnC[ci], den = log(mxC[ci] - lo + 1.0);
  if (tj < 0 || tj >= ncT || cj < 0 || cj >= nk || !(den > 0)) {
    if (threadIdx.x < 4) out[threadIdx.x] = NAN;
    return;
  }
  double loT = 0, denT = 1;
  if (!readyT) {
    loT = mnT[ti];
    denT = log(mxT[ti] - loT + 1.0);
  }
  const double* tc = specT + (int64_t)keptT[sndT[ti].f0 + tj] * nb;
  const double* sc = specC + (int64_t)keptC[sndC[ci].f0 + cj] * nb;
  double st = 0, sd = 0;
  for (int b = threadIdx.x; b < nb; b += 64) {
    const double tv = readyT ? tc[b] : log01(tc[b], loT, denT), dv = log01(sc[b], lo, den);
    t[b] = tv;
    d[b] = dv;
    st += tv;
    sd += dv;
  }
  mel_column_sims(t, d, sh + 2 * nb, nb, st, sd, do_dtw, out);
}

// compareSounds' reduction (R/matchPars.R:378-416) of each pair's columns: thread (pair, m)
// adds the pair's values of method m in column order with the NAs dropped and divides by the
// column count (penalize) or by the number added; then the pair's first thread takes the mean
// of the computed methods that are not NA. A sound without a frame is absent (a failed slot):
// NaN throughout; a ready-made target (readyT) is present even with no column, and then every
// column value is NA: 0 / ncol (penalize) or NaN, as R gives. out[4 p + m], summary[p].
__global__ __launch_bounds__(256) void sg_mel_pair_reduce(
    const int32_t* __restrict__ pairs, const int64_t* __restrict__ job0, int64_t n_pairs,
    const MelCand* __restrict__ sndT, const int32_t* __restrict__ nkeptT, int readyT, const MelCand* __restrict__ sndC,
    const int32_t* __restrict__ nkeptC, const double* __restrict__ sims, int methods, int penalize,
    double* __restrict__ out, double* __restrict__ summary) {
  __shared__ double so[256];
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x / 4;
  const int m = threadIdx.x & 3;
  double o = NAN;
  if (p < n_pairs) {
    const int ti = pairs[2 * p], ci = pairs[2 * p + 1];
    if ((readyT || sndT[ti].nf > 0) && sndC[ci].nf > 0 && (methods & (1 << m))) {
      const int ncT = nkeptT[ti], nk = nkeptC[ci];
      const int ncol = nk > ncT ? nk : ncT;
      const double* v = sims + job0[p] * 4 + m;
      double sm = 0;
      int cnt = 0;
      for (int j = 0; j < ncol; ++j) {
        const double x = v[(int64_t)j * 4];
        if (!isnan(x)) {
          sm += x;
          ++cnt;
        }
      }
      o = penalize ? sm / ncol : (cnt ? sm / cnt : NAN);
    }
    out[4 * p + m] = o;
  }
  so[threadIdx.x] = o;
  __syncthreads();
  if (p < n_pairs && m == 0) {
    double sm = 0;
    int cnt = 0;
    for (int k = 0; k < 4; ++k) {
      const double x = so[threadIdx.x + k];
      if (!isnan(x)) {
        sm += x;
        ++cnt;
      }
    }
    summary[p] = cnt ? sm / cnt : NAN;
  }
}

// getMelSpec's value: the kept columns, log01-normalised, nb x nk column-major
__global__ __launch_bounds__(256) void sg_mel_out(const double* __restrict__ spec, const int32_t* __restrict__ kept,
                                                  int nk, int nb, const double* __restrict__ mn,
                                                  const double* __restrict__ mx, double* __restrict__ out) {
  const double lo = mn[0], den = log(mx[0] - lo + 1.0);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)nk * nb; e += (int64_t)gridDim.x * 256)
    out[e] = log01(spec[(int64_t)kept[e / nb] * nb + e % nb], lo, den);
}

// Slaney mel scale (tuneR hz2mel / mel2hz, htk = FALSE)
double hz2mel(double f) {
  const double f_sp = 200.0 / 3, brkfrq = 1000.0, brkpt = brkfrq / f_sp, logstep = std::exp(std::log(6.4) / 27);
  return f < brkfrq ? f / f_sp : brkpt + std::log(std::max(f, 1e-300) / brkfrq) / std::log(logstep);
}
double mel2hz(double z) {
  const double f_sp = 200.0 / 3, brkfrq = 1000.0, brkpt = brkfrq / f_sp, logstep = std::exp(std::log(6.4) / 27);
  return z < brkpt ? f_sp * z : brkfrq * std::exp(std::log(logstep) * (z - brkpt));
}

using sg::DevBuf;
using sg::upload;

}  // namespace

namespace sg {

MelGeom mel_geom(const sg_mel_params& p) {
  if (!(p.samplingRate > 0) || !(p.windowLength > 0))
    throw SgError(SG_E_ARG, "getMelSpec: samplingRate and windowLength must be > 0");
  const double step = std::isnan(p.step) ? p.windowLength * (1 - p.overlap / 100) : p.step;
  // melfcc(nbands = 100 * windowLength / 20, maxfreq = samplingRate / 2)
  return mel_geom(p.samplingRate, p.windowLength, step, std::isnan(p.maxFreq) ? p.samplingRate / 2 : p.maxFreq,
                  (int)(100 * p.windowLength / 20), p.throwaway);
}

MelGeom mel_geom(double sr, double windowLength, double step, double maxf, int nb, double throwaway) {
  MelGeom g;
  if (!(sr > 0) || !(windowLength > 0)) throw SgError(SG_E_ARG, "getMelSpec: samplingRate and windowLength must be > 0");
  if (!(step > 0)) throw SgError(SG_E_ARG, "getMelSpec: step must be > 0");
  // tuneR powspec: winpts = round(wintime sr), steppts = round(steptime sr), nfft = 2^ceil(log2(winpts))
  g.winpts = (int)r_round(windowLength / 1000 * sr);
  g.steppts = (int)r_round(step / 1000 * sr);
  if (g.winpts < 2 || g.steppts < 1) throw SgError(SG_E_ARG, "getMelSpec: window shorter than 2 samples");
  g.nfft = (int)std::pow(2.0, std::ceil(std::log((double)g.winpts) / std::log(2.0)));
  if (g.nfft > 4096) throw SgError(SG_E_UNSUPPORTED, "getMelSpec: windows above 4096 points are not supported");
  g.nfreqs = g.nfft / 2;
  g.nb = nb;
  if (g.nb < 1) throw SgError(SG_E_ARG, "getMelSpec: no mel bands");
  g.thr = std::pow(2.0, throwaway / 10);
  g.ham.resize(g.winpts);
  for (int i = 0; i < g.winpts; ++i) g.ham[i] = 0.54 - 0.46 * std::cos(2 * M_PI * i / (g.winpts - 1));
  // fft2melmx((nfreqs - 1) * 2, sr, nbands, 1, 0, maxFreq)[, 1:nfreqs] (audspec's nfft quirk)
  const int nfft2 = (g.nfreqs - 1) * 2;
  const double minmel = hz2mel(0.0), maxmel = hz2mel(maxf);
  std::vector<double> binf(g.nb + 2);
  for (int i = 0; i < g.nb + 2; ++i) binf[i] = mel2hz(minmel + (double)i / (g.nb + 1) * (maxmel - minmel));
  for (int b = 0; b < g.nb; ++b) {
    // fs = fs[2] + width (fs - fs[2]) with width = 1, in R's (and numpy's) rounding
    const double f1 = binf[b + 1], f0 = f1 + 1.0 * (binf[b] - f1), f2 = f1 + 1.0 * (binf[b + 2] - f1);
    const double sc = 2 / (binf[b + 2] - binf[b]);
    int k0 = -1, n = 0;
    const int w0 = (int)g.w.size();
    for (int k = 0; k < g.nfreqs; ++k) {
      const double f = (double)k / nfft2 * sr;
      const double lo = (f - f0) / (f1 - f0), hi = (f2 - f) / (f2 - f1);
      const double w = sc * std::max(0.0, std::min(lo, hi));
      if (w > 0) {
        if (k0 < 0) k0 = k;
        // weights are contiguous in k (a triangle); zeros between would break the band
        while (k0 + n < k) { g.w.push_back(0.0); ++n; }
        g.w.push_back(w);
        ++n;
      }
    }
    g.band_k0.push_back(k0 < 0 ? 0 : k0);
    g.band_n.push_back(n);
    g.band_w0.push_back(w0);
  }
  const int M = g.nfreqs;  // complex points of the real nfft transform
  g.tw.resize(std::max(1, M / 2) * 2);
  for (int t = 0; t < M / 2; ++t) {
    g.tw[2 * t] = std::cos(2 * M_PI * t / M);
    g.tw[2 * t + 1] = -std::sin(2 * M_PI * t / M);
  }
  g.twN.resize(2 * M);
  for (int k = 0; k < M; ++k) {
    g.twN[2 * k] = std::cos(2 * M_PI * k / g.nfft);
    g.twN[2 * k + 1] = -std::sin(2 * M_PI * k / g.nfft);
  }
  return g;
}

// frames of a candidate of `len` samples (tuneR powspec via signal::specgram):
// starts 0, steppts, ..., nn steppts with nn = (len - winpts - 1) %/% steppts
int mel_frames(const MelGeom& g, int64_t len) {
  if (len > g.winpts) return (int)((double)(len - g.winpts - 1) / g.steppts + 1e-10) + 1;
  return 1;
}

// what sg_mel_frames and sg_mel_cand leave on the device for a batch of sounds (mel_run), or
// one sound given as getMelSpec's value (mel_run_ready): ready, spec holds the normalised
// columns as they stand, every one kept, and mn and mx stay unset
struct MelRun {
  bool ready = false;
  int F = 0;
  DevBuf db;
  double* spec = nullptr;
  int32_t* kept = nullptr;
  int32_t* nkept = nullptr;
  double *mn = nullptr, *mx = nullptr;
  MelCand* cands = nullptr;
  std::vector<MelCand> hc;
};

namespace {

template <typename T>
void mel_run(MelRun& r, const MelGeom& g, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n,
             hipStream_t s) {
  std::vector<MelFrame> fr;
  r.hc.resize(n);
  for (int64_t c = 0; c < n; ++c) {
    MelCand& C = r.hc[c];
    C.f0 = (int32_t)fr.size();
    C.nf = 0;
    if (lengths[c] <= 0) continue;
    const int nf = mel_frames(g, lengths[c]);
    for (int f = 0; f < nf; ++f) {
      const int64_t o = (int64_t)f * g.steppts;
      fr.push_back(MelFrame{offsets[c], (int32_t)o, (int32_t)std::min<int64_t>(g.winpts, lengths[c] - o)});
    }
    C.nf = nf;
  }
  r.F = (int)fr.size();
  std::vector<MelBand> bands(g.nb);
  for (int b = 0; b < g.nb; ++b) bands[b] = MelBand{g.band_k0[b], g.band_n[b], g.band_w0[b], 0};
  const MelFrame* d_fr = upload(r.db, fr, s);
  const double* d_ham = upload(r.db, g.ham, s);
  const double2* d_tw = reinterpret_cast<const double2*>(upload(r.db, g.tw, s));
  const double2* d_twN = reinterpret_cast<const double2*>(upload(r.db, g.twN, s));
  const MelBand* d_bands = upload(r.db, bands, s);
  const double* d_w = upload(r.db, g.w, s);
  r.cands = upload(r.db, r.hc, s);
  r.spec = r.db.get<double>((size_t)std::max(r.F, 1) * g.nb);
  double* colmean = r.db.get<double>(std::max(r.F, 1));
  r.kept = r.db.get<int32_t>(std::max(r.F, 1));
  r.nkept = r.db.get<int32_t>(n);
  r.mn = r.db.get<double>(n);
  r.mx = r.db.get<double>(n);
  const int M = g.nfreqs;
  int logM = 0;
  while ((1 << logM) < M) ++logM;
  if (r.F > 0) {
    hipLaunchKernelGGL(sg_mel_frames<T>, dim3((unsigned)r.F), dim3(256), (size_t)2 * M * sizeof(double2), s, d_x, d_fr,
                       d_ham, d_tw, d_twN, d_bands, d_w, g.winpts, M, logM, g.nb, r.spec, colmean);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(sg_mel_cand, dim3((unsigned)n), dim3(256), 0, s, r.cands, r.spec, colmean, g.thr, g.nb, r.kept,
                     r.nkept, r.mn, r.mx);
  HIPCHK(hipGetLastError());
}

// One sound given as getMelSpec's value (host, nb x nc, already through log01). nf = nc, so
// a pair's column-job bound max(nfT, nfC) covers its columns as it does for frames.
void mel_run_ready(MelRun& r, const double* tspec, int nc, int nb, hipStream_t s) {
  r.ready = true;
  r.F = nc;
  r.hc.assign(1, MelCand{0, nc, 0, 0});
  // one upload (this runs once per scoring call): the columns, then as int32 the sound table (a
  // MelCand is four), nkept and the identity kept list
  std::vector<int32_t> t{0, nc, 0, 0, nc};
  for (int j = 0; j < nc; ++j) t.push_back(j);
  const size_t ns = (size_t)nc * nb;
  std::vector<double> h(ns + (t.size() + 1) / 2);
  std::copy(tspec, tspec + ns, h.begin());
  std::memcpy(h.data() + ns, t.data(), t.size() * sizeof(int32_t));
  r.spec = upload(r.db, h, s);
  int32_t* d = reinterpret_cast<int32_t*>(r.spec + ns);
  r.cands = reinterpret_cast<MelCand*>(d);
  r.nkept = d + 4;
  r.kept = d + 5;
}

// getMelSpec's value of sound i of a run, which kept nk columns: nb x nk column-major
void mel_run_spec(const MelRun& r, int64_t i, int nk, int nb, std::vector<double>& out, hipStream_t s) {
  out.assign((size_t)nk * nb, 0.0);
  if (nk == 0) return;
  DevBuf db;
  const int64_t tot = (int64_t)nk * nb;
  double* d_out = db.get<double>((size_t)tot);
  hipLaunchKernelGGL(sg_mel_out, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 4096)), dim3(256), 0, s, r.spec,
                     r.kept + r.hc[(size_t)i].f0, nk, nb, r.mn + i, r.mx + i, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out.data(), d_out, (size_t)tot * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
}

StageTimes<2> g_mel_pair_ms;  // of the last profiled compare_pairs (sg_debug_mel_pair_kernel_ms)

// compareSounds(target = sound pairs[2 p] of T, cand = sound pairs[2 p + 1] of C), two runs of
// nb bands: sg_mel_pair, sg_mel_pair_reduce, then out[4 p + m] and summary[p] (may be null)
void compare_pairs(const MelRun& T, const MelRun& C, int nb, const int32_t* pairs, int64_t n_pairs, int methods,
                   int penalize, double* out, double* summary, hipStream_t s, bool profile) {
  // column jobs: a pair may need up to max(frames of its two sounds) output columns, known
  // here without asking the device for the kept counts
  if (n_pairs > INT32_MAX) throw SgError(SG_E_UNSUPPORTED, "compareSounds: more than 2^31 - 1 pairs");
  // job0 and, behind it in the same upload, the pairs (two int32 per entry)
  std::vector<int64_t> job0((size_t)n_pairs + 1 + (size_t)n_pairs);
  int64_t J = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    job0[(size_t)p] = J;
    const int nfT = T.hc[(size_t)pairs[2 * p]].nf, nfC = C.hc[(size_t)pairs[2 * p + 1]].nf;
    if ((T.ready || nfT > 0) && nfC > 0) J += std::max(nfT, nfC);
    if (J > INT32_MAX) throw SgError(SG_E_UNSUPPORTED, "compareSounds: more than 2^31 - 1 column jobs");
  }
  job0[(size_t)n_pairs] = J;
  std::memcpy(job0.data() + n_pairs + 1, pairs, (size_t)n_pairs * 2 * sizeof(int32_t));
  DevBuf db;
  const int64_t* d_job0 = upload(db, job0, s);
  const int32_t* d_pairs = reinterpret_cast<const int32_t*>(d_job0 + n_pairs + 1);
  // one allocation: the column values, then the pairs' 4 + 1 results
  double* d_sims = db.get<double>((size_t)J * 4 + (size_t)n_pairs * 5);
  double* d_out = d_sims + J * 4;
  double* d_sum = d_out + n_pairs * 4;
  StageClock clk(s, profile ? g_mel_pair_ms.ms : nullptr, 2);
  clk.stamp();
  if (J > 0) {
    hipLaunchKernelGGL(sg_mel_pair, dim3((unsigned)J), dim3(64), (size_t)5 * nb * sizeof(double), s, d_pairs, d_job0,
                       n_pairs, nb, T.spec, T.kept, T.cands, T.nkept, T.mn, T.mx, T.ready ? 1 : 0, C.spec, C.kept,
                       C.cands, C.nkept, C.mn, C.mx, (methods & 8) ? 1 : 0, d_sims);
    HIPCHK(hipGetLastError());
  }
  clk.stamp();
  hipLaunchKernelGGL(sg_mel_pair_reduce, dim3((unsigned)((n_pairs + 63) / 64)), dim3(256), 0, s, d_pairs, d_job0,
                     n_pairs, T.cands, T.nkept, T.ready ? 1 : 0, C.cands, C.nkept, d_sims, methods, penalize ? 1 : 0,
                     d_out, d_sum);
  HIPCHK(hipGetLastError());
  clk.stamp();
  HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n_pairs * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (summary) HIPCHK(hipMemcpyAsync(summary, d_sum, (size_t)n_pairs * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  clk.finish();
}

}  // namespace

void mel_spec_device(const MelGeom& g, const double* d_x, int64_t len, std::vector<double>& out, int* nk_out,
                     hipStream_t s) {
  MelRun r;
  const int64_t off = 0;
  mel_run<double>(r, g, d_x, &off, &len, 1, s);
  int32_t nk = 0;
  HIPCHK(hipMemcpyAsync(&nk, r.nkept, sizeof nk, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *nk_out = nk;
  mel_run_spec(r, 0, nk, g.nb, out, s);
}

void compare_sounds_device(const MelGeom& g, const double* tspec, int ncT, const float* d_x, const int64_t* offsets,
                           const int64_t* lengths, int64_t n, int methods, int penalize, double* out, double* summary,
                           hipStream_t s) {
  MelRun T, C;
  mel_run<float>(C, g, d_x, offsets, lengths, n, s);
  mel_run_ready(T, tspec, ncT, g.nb, s);
  std::vector<int32_t> pairs((size_t)2 * n, 0);  // (0, c)
  for (int64_t c = 0; c < n; ++c) pairs[(size_t)2 * c + 1] = (int32_t)c;
  compare_pairs(T, C, g.nb, pairs.data(), n, methods, penalize, out, summary, s, false);
}

MelSet::MelSet(sg_ctx* c, const sg_mel_params& p, const void* d_x, bool f64, const int64_t* offsets,
               const int64_t* lengths, int64_t n_)
    : ctx(c), g(mel_geom(p)), maxFreq(std::isnan(p.maxFreq) ? p.samplingRate / 2 : p.maxFreq),
      throwaway(p.throwaway), n(n_), ncols((size_t)n_, 0), r(nullptr) {
  if (n == 0) return;
  std::unique_ptr<MelRun> run(new MelRun);
  hipStream_t s = ctx->stream;
  if (f64) mel_run<double>(*run, g, static_cast<const double*>(d_x), offsets, lengths, n, s);
  else mel_run<float>(*run, g, static_cast<const float*>(d_x), offsets, lengths, n, s);
  HIPCHK(hipMemcpyAsync(ncols.data(), run->nkept, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  // the caller's waveform is free to go once this returns, and so are the staged uploads
  HIPCHK(hipStreamSynchronize(s));
  run->db.host.clear();
  r = run.release();
}

MelSet::~MelSet() { delete r; }

void MelSet::spec(int64_t i, std::vector<double>& out, int* nk_out) const {
  *nk_out = ncols[(size_t)i];
  mel_run_spec(*r, i, *nk_out, g.nb, out, ctx->stream);
}

bool MelSet::same_geometry(const MelSet& o) const {
  return g.winpts == o.g.winpts && g.steppts == o.g.steppts && g.nfft == o.g.nfft && g.nb == o.g.nb &&
         maxFreq == o.maxFreq && throwaway == o.throwaway;
}

void compare_sounds_pairs_device(const MelSet& T, const MelSet& C, const int32_t* pairs, int64_t n_pairs, int methods,
                                 int penalize, double* out, double* summary, hipStream_t s, bool profile) {
  compare_pairs(*T.r, *C.r, T.g.nb, pairs, n_pairs, methods, penalize, out, summary, s, profile);
}

}  // namespace sg

extern "C" int sg_debug_mel_pair_kernel_ms(double* out) { return sg::g_mel_pair_ms.read(out); }
