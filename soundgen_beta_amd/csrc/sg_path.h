// sg_path.h — analyze()'s tail once every frame has its pitch candidates
// (R/analyze.R:576-707, R/utilities_pitch_postprocessing.R): the prior, findVoicedSegments,
// pathfinder (interpolate, pathfinding 'none' / 'fast', costJumps, snake, forcePerPath,
// findGrad), medianSmoother and the final columns; and pathfinding 'exact', which the
// reference does not have: the minimum of its own costPerPath() (:347-372, what 'slow'
// anneals towards) by dynamic programming, path_exact() below. The scalar routines are plain
// functions; path_sound() drives them for one sound with `nl` cooperating lanes: the 64
// lanes of sg_anl_path's workgroup on the device, one lane (and a sync that does nothing)
// on the host (tests/cpp/path_pins.cpp, tests/cpp/path_exact_pins.cpp). path_sound_at() is the same with the candidates in a
// table apart that it leaves untouched (a sweep's pairs, sg_anl_sweep_path;
// tests/cpp/path_at_pins.cpp). No HIP header is needed on the host side, no dynamic memory
// anywhere.
//
// A frame's candidates live in global scratch, path_stride() doubles per frame: W = 2 +
// 3 nCands log2 pitches (dom, autocor[.], cep[.], spec[.] as pitch_matrices packs them,
// then room for the one interpolate() adds), W certainties, and kPathSlots per-frame
// values. What R keeps as matrices with NA-padded columns is here a packed list per
// frame: order() puts NA last and the all-NA rows are dropped (:67-83), so nrow is the
// largest count of a frame and which.min / which.max index the packed values.
//
// Sums over frames (the two path costs, mean(|force|)) are made by a scheme that depends
// on nl alone: lane l adds its frames l, l + nl, ... in order, then every lane folds the
// nl partial sums in lane order. A sound's result therefore does not depend on the launch.
//
// 'exact' needs path_width() more cells per frame, behind the nf * path_stride() cells of
// the other modes (path_scratch() doubles per frame in all): the back-pointers of its
// recursion. The only operation it makes across candidates is a minimum with a
// lowest-index tie rule, which is associative, unlike the sums above: however the lanes
// share the (i, k) pairs of a frame, the picks equal those of the one-lane host run.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_PATH_HD __host__ __device__
#define SG_PATH_CALL __attribute__((noinline))  // a call of its own: keeps the caller's registers what they were
#else
#define SG_PATH_HD
#define SG_PATH_CALL
#endif

namespace sg {

// columns of a frame's row read or rewritten here (sg::AnlCol; sg_analyze.hip asserts they agree)
constexpr int kPathAmpl = 0, kPathHNR = 2, kPathDom = 3, kPathQ25 = 7, kPathQ75 = 9, kPathDomCand = 11, kPathDomCert = 12,
              kPathFixed = 15;
// the four columns behind the candidates
constexpr int kPathPitch = 0, kPathAmplVoiced = 1, kPathVoiced = 2, kPathHarmonics = 3, kPathCols = 4;
// per-frame scratch slots behind the 2 W candidate cells
constexpr int kSlotCog = 0,     // pitchCenterGravity
              kSlotPath = 1,    // the path (log2), forward while both are alive
              kSlotAux = 2,     // the backward path, then the snake's force
              kSlotCnt = 3,     // candidates in the frame
              kSlotHz = 4,      // pitchFinal (Hz) before the smoother
              kSlotDom = 5,     // dom before the smoother
              kSlotVoiced = 6,  // putativelyVoiced
              kPathSlots = 7;
// interpolWin and the smoother's half width: a median costs its width squared, and interpolate()'s run in one lane
constexpr int kPathMaxWin = 64;

struct PathPars {
  int nCands;       // per method
  int cols;         // doubles of a row: kPathFixed + 6 nCands + kPathCols
  int minVoiced;    // minVoicedCands, resolved
  int noRequired;   // max(1, ceiling(shortestSyl / step))
  int nTolerated;   // floor(shortestPause / step)
  int interpolWin;  // 0: interpolate() is not called
  int pathfinding;  // 0 'none', 1 'fast', 3 'exact' (2, 'slow', is refused by the setup)
  int do_prior, smooth_pitch, smooth_dom;
  double shape, rate, lconst, prior_norm;  // lconst = shape log(rate) - lgamma(shape); prior_norm = max(dgamma(seq))
  double interpolTol, interpolCert, certWeight;
  double snakeStep;    // <= 0: no snake
  double smoothThres;  // 4 / smooth
};

SG_PATH_HD inline int path_width(int nCands) { return 2 + 3 * nCands; }
SG_PATH_HD inline int path_stride(int nCands) { return 2 * path_width(nCands) + kPathSlots; }
// doubles of scratch per frame of a sound: 'exact' keeps path_width() back-pointers per frame behind the rest
SG_PATH_HD inline int path_scratch(int nCands, int pathfinding) {
  return path_stride(nCands) + (pathfinding == 3 ? path_width(nCands) : 0);
}
// doubles of a sound's optional segment list: the count, then kPathSegCells per voiced segment (first frame, last
// frame (1-based), nrow after the dropped rows, costPerPath() of the path handed to the snake)
constexpr int kPathSegCells = 4;
SG_PATH_HD inline int64_t path_seg_cells(int64_t nf) { return 1 + kPathSegCells * nf; }

// to_dB(), R/utilities_math.R:37-39; a ratio <= 0 gives NaN as log10 does
SG_PATH_HD inline double path_to_dB(double x) { return 10 * log10(x / (1 - x)); }

// dgamma(x, shape, rate) = exp((shape - 1) ln x - rate x + shape ln(rate) - lgamma(shape)); 0 for x < 0
SG_PATH_HD inline double path_dgamma(double x, double shape, double rate, double lconst) {
  if (x < 0) return 0.0;
  if (x == 0) return shape > 1 ? 0.0 : (shape == 1 ? rate : INFINITY);
  return exp((shape - 1) * log(x) - rate * x + lconst);
}

// pitchCert_multiplier (R/analyze.R:606-610) of a candidate in Hz
SG_PATH_HD inline double path_prior(double hz, const PathPars& P) {
  const double semitones = log2(hz / 16.3516) * 12;  // HzToSemitones
  return path_dgamma(semitones, P.shape, P.rate, P.lconst) / P.prior_norm;
}

// findVoicedSegments (:622-669), resumable: v[(k - 1) * stride] != 0 says frame k (1-based)
// is putatively voiced; *ip is the loop's i (1 before the first call). Returns 1 with the
// next segment [*s, *e] (1-based, inclusive), 0 when the outer loop has ended.
SG_PATH_HD inline int path_next_segment(const double* v, int stride, int64_t n, int64_t noRequired, int64_t nTolerated,
                                        int64_t* ip, int64_t* s, int64_t* e) {
  int64_t i = *ip;
  while (i < n - noRequired + 1) {
    bool found = false;
    while (i < n - noRequired + 1) {  // find beginning
      bool all = true;
      for (int64_t k = i; k <= i + noRequired - 1 && all; ++k) all = v[(k - 1) * stride] != 0;
      if (all) {
        found = true;
        break;
      }
      ++i;
    }
    if (found) {
      *s = i;
      while (i < n - nTolerated + 1) {  // find end
        bool any = false;
        for (int64_t k = i; k <= i + nTolerated && !any; ++k) any = v[(k - 1) * stride] != 0;
        if (!any) {
          *e = i - 1;
          *ip = i;  // i = i - 1, then i = i + 1
          return 1;
        }
        ++i;
      }
      int64_t last = *s;  // the end is not found: the last non-NA value, and the outer loop breaks
      for (int64_t k = n; k > *s; --k)
        if (v[(k - 1) * stride] != 0) {
          last = k;
          break;
        }
      *e = last;
      *ip = n + 1;
      return 1;
    }
    ++i;
  }
  *ip = i;
  return 0;
}

// median(x, na.rm = TRUE) of the n values p[j * stride], by ranks (no storage); NaN if none
SG_PATH_HD inline double path_median(const double* p, int stride, int n) {
  int m = 0;
  for (int j = 0; j < n; ++j) m += p[(int64_t)j * stride] == p[(int64_t)j * stride];
  if (!m) return NAN;
  const int k1 = (m - 1) / 2, k2 = m / 2;
  double a = NAN, b = NAN;
  for (int j = 0; j < n; ++j) {
    const double v = p[(int64_t)j * stride];
    if (v != v) continue;
    int lt = 0, le = 0;
    for (int i = 0; i < n; ++i) {
      const double w = p[(int64_t)i * stride];
      lt += w < v;
      le += w <= v;
    }
    if (lt <= k1 && k1 < le) a = v;
    if (lt <= k2 && k2 < le) b = v;
  }
  return k1 == k2 ? a : (a + b) / 2;
}

// mean(x): the weights argument of the reference's mean(x, weights = ...) is ignored
SG_PATH_HD inline double path_mean(const double* c, int cnt) {
  if (cnt <= 0) return NAN;
  double s = 0;
  for (int k = 0; k < cnt; ++k) s += c[k];
  return s / cnt;
}

// interpolate() (:149-184) at frame f of the n frames of a segment whose scratch starts
// at seg: 1 if a candidate was added. Sequential in f: the updated centre of gravity
// enters the medians of the next interpolWin frames.
SG_PATH_HD inline int path_interpolate_frame(double* seg, int S, int W, int n, int f, const PathPars& P) {
  const int left = f - P.interpolWin < 0 ? 0 : f - P.interpolWin;
  const int right = f + P.interpolWin > n - 1 ? n - 1 : f + P.interpolWin;
  const double med = path_median(seg + (int64_t)left * S + 2 * W + kSlotCog, S, right - left + 1);
  if (med != med) return 0;
  double* c = seg + (int64_t)f * S;
  const int cnt = (int)c[2 * W + kSlotCnt];
  const double lo = (1 - P.interpolTol) * med, hi = (1 + P.interpolTol) * med;
  for (int k = 0; k < cnt; ++k)
    if (c[k] > lo && c[k] < hi) return 0;
  if (cnt >= W) return 0;  // cannot happen: W has room for one more than a row holds
  c[cnt] = med;
  c[W + cnt] = P.interpolCert;
  c[2 * W + kSlotCnt] = cnt + 1;
  c[2 * W + kSlotCog] = path_mean(c, cnt + 1);
  return 1;
}

// order(pitchCands[, x]) (:69-79): ascending, stable, the certainties carried along
SG_PATH_HD inline void path_sort_frame(double* c, double* a, int cnt) {
  for (int i = 1; i < cnt; ++i) {
    const double v = c[i], w = a[i];
    int k = i;
    for (; k > 0 && c[k - 1] > v; --k) {
      c[k] = c[k - 1];
      a[k] = a[k - 1];
    }
    c[k] = v;
    a[k] = w;
  }
}

// costJumps() (:283-285)
SG_PATH_HD inline double path_cost_jump(double a, double b) { return 1 / (1 + 10 * exp(3 - 7 * fabs(a - b))); }

// The start of pathfinding_fast (:209-213, :240-243): which.max(cert / |cand - p|), NA
// skipped. p NaN (the backward median has no na.rm) leaves no start: NaN.
SG_PATH_HD inline double path_start(const double* c, const double* a, int cnt, double p) {
  if (p != p) return NAN;
  int best = -1;
  double bv = 0;
  for (int k = 0; k < cnt; ++k) {
    const double v = a[k] / fabs(c[k] - p);
    if (v != v) continue;
    if (best < 0 || v > bv) {
      best = k;
      bv = v;
    }
  }
  return best < 0 ? NAN : c[best];
}

// which.min(costs) over a frame's candidates and min(costs). fast == 0 ('none', :110-113):
// |cand - cog|. fast == 1 (:220-231): certWeight |cand - cog| + (1 - certWeight)
// costJumps(start, cand); start is the segment's start point for every frame
// (point_current is never updated) and the jump cost is 0 where there is no start.
SG_PATH_HD inline int path_choose(const double* c, int cnt, double cog, double start, int fast, double certWeight,
                                  double* cost) {
  int best = -1;
  double bv = 0;
  for (int k = 0; k < cnt; ++k) {
    double v = fabs(c[k] - cog);
    if (fast) v = certWeight * v + (1 - certWeight) * (start == start ? path_cost_jump(start, c[k]) : 0.0);
    if (v != v) continue;
    if (best < 0 || v < bv) {
      best = k;
      bv = v;
    }
  }
  *cost = best < 0 ? 0.0 : bv;
  return best;
}

// findGrad() (:534-562): the slopes lm() fits to the first and the last min(3, n) points
// (closed forms), the two extrapolated points at either end, the fourth difference
SG_PATH_HD inline void path_end_slopes(const double* p, int S, int n, double* sl, double* sr) {
  if (n < 2) {
    *sl = *sr = 0;  // interpol == 1: the end values are repeated
  } else if (n == 2) {
    *sl = *sr = p[S] - p[0];
  } else {
    *sl = (p[2 * (int64_t)S] - p[0]) / 2;
    *sr = (p[(int64_t)(n - 1) * S] - p[(int64_t)(n - 3) * S]) / 2;
  }
}
SG_PATH_HD inline double path_ext(const double* p, int S, int n, int j, double sl, double sr) {
  if (j < 0) return p[0] - (double)(-j) * sl;
  if (j >= n) return p[(int64_t)(n - 1) * S] + (double)(j - n + 1) * sr;
  return p[(int64_t)j * S];
}
SG_PATH_HD inline double path_grad(const double* p, int S, int n, int f, double sl, double sr) {
  return path_ext(p, S, n, f - 2, sl, sr) - 4 * path_ext(p, S, n, f - 1, sl, sr) + 6 * path_ext(p, S, n, f, sl, sr) -
         4 * path_ext(p, S, n, f + 1, sl, sr) + path_ext(p, S, n, f + 2, sl, sr);
}

// forcePerPath() (:495-521) at one frame: a candidate pulls with cert / exp((cand - pitch)^2),
// towards itself only where cand > pitch (one equal to pitch pushes with -cert)
SG_PATH_HD inline double path_force(const double* c, const double* a, int cnt, double pitch, double grad, double certWeight) {
  double external = 0;
  for (int k = 0; k < cnt; ++k) {
    const double d = c[k] - pitch;
    const double f = a[k] * (1 / exp(d * d));
    external += c[k] > pitch ? f : -f;
  }
  return certWeight * external + (1 - certWeight) * (-grad);
}

// medianSmoother()'s decision (:595-597): abs(deviance - 1), not abs(deviance); NA keeps v
SG_PATH_HD inline double path_smooth(double v, double med, double thres) {
  const double deviance = 12 * log2(v / med);
  return fabs(deviance - 1) > thres ? med : v;
}

// op 0 sum, 1 min, 2 max of v over the lanes, folded in lane order; every lane gets it
template <class Sync>
SG_PATH_HD inline double path_reduce(double v, int op, int lane, int nl, double* red, Sync& sync) {
  sync();
  red[lane] = v;
  sync();
  double r = red[0];
  for (int t = 1; t < nl; ++t) r = op == 0 ? r + red[t] : (op == 1 ? fmin(r, red[t]) : fmax(r, red[t]));
  return r;
}

// The inner minimum of 'exact' for one candidate v of a frame: the k (lowest on ties) of the pc candidates c0[.] of
// the frame before that minimises D0[k] + wj costJumps(c0[k], v), and that minimum
SG_PATH_HD inline int path_exact_arg(const double* c0, const double* D0, int pc, double v, double wj, double* best) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int bk = 0;
  double bv = 0;
  for (int k = 0; k < pc; ++k) {
    const double t = D0[k] + wj * path_cost_jump(c0[k], v);
    if (k == 0 || t < bv) {
      bk = k;
      bv = t;
    }
  }
  *best = bv;
  return bk;
}

// the lowest index of the least of D[0 .. cnt)
SG_PATH_HD inline int path_exact_end(const double* D, int cnt) {
  int b = 0;
  for (int i = 1; i < cnt; ++i)
    if (D[i] < D[b]) b = i;
  return b;
}

// pathfinding 'exact' (not in the reference): the path that minimises costPerPath() (:347-372) over the n >= 2
// frames of a segment at seg, sorted. With n_c frames that have a candidate and n_j neighbouring pairs of them (the
// denominators of the reference's two mean(..., na.rm = TRUE)), wc = certWeight / n_c, wj = (1 - certWeight) / n_j:
//   D(f, i) = wc |c[f][i] - cog[f]|                                                  in the first frame of a run
//   D(f, i) = wc |c[f][i] - cog[f]| + min_k (D(f - 1, k) + wj costJumps(c[f-1][k], c[f][i]))   otherwise
// the lowest k winning ties; at the last frame of every maximal run of non-empty frames the lowest i with the least D
// is taken and the chosen k are followed back. Frames are sequential, one sync each; lane i of a frame has candidate
// i. dd: 2 W doubles shared by the lanes (D of the frame before and of this one); bp: W cells per frame, the chosen
// k. Returns false, with nothing written to the path, when n_j = 0 (every path costs NaN in the reference): the
// caller then takes 'none'. Otherwise the path is in kSlotPath (NaN for a frame without candidates); the caller syncs.
template <class Sync>
SG_PATH_HD SG_PATH_CALL inline bool path_exact(double* seg, int S, int W, int n, double certWeight, double* bp, double* dd, int lane,
                                  int nl, double* red, Sync& sync) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int X = 2 * W;
  double nc = 0, nj = 0;  // whole numbers: their sums do not depend on the order
  for (int f = lane; f < n; f += nl)
    if (seg[(int64_t)f * S + X + kSlotCnt] > 0) {
      nc += 1;
      if (f + 1 < n && seg[(int64_t)(f + 1) * S + X + kSlotCnt] > 0) nj += 1;
    }
  nc = path_reduce(nc, 0, lane, nl, red, sync);
  nj = path_reduce(nj, 0, lane, nl, red, sync);
  if (nj == 0) return false;
  const double wc = certWeight / nc, wj = (1 - certWeight) / nj;
  int prev = 0;  // candidates of the frame before
  for (int f = 0; f < n; ++f) {
    double* c = seg + (int64_t)f * S;
    const int cnt = (int)c[X + kSlotCnt];
    double* cur = dd + (f & 1) * W;
    const double* old = dd + ((f & 1) ^ 1) * W;
    if (lane == 0 && prev > 0 && cnt == 0) (c - S)[X + kSlotAux] = path_exact_end(old, prev);  // a run ends before f
    for (int i = lane; i < cnt; i += nl) {
      const double node = wc * fabs(c[i] - c[X + kSlotCog]);
      double best = 0;
      const int k = prev > 0 ? path_exact_arg(c - S, old, prev, c[i], wj, &best) : -1;
      cur[i] = prev > 0 ? node + best : node;
      bp[(int64_t)f * W + i] = k;
    }
    prev = cnt;
    sync();
  }
  if (lane == 0) {
    if (prev > 0) seg[(int64_t)(n - 1) * S + X + kSlotAux] = path_exact_end(dd + ((n - 1) & 1) * W, prev);
    int at = -1;  // the candidate taken in the frame behind, if the run goes on
    for (int f = n - 1; f >= 0; --f) {
      double* c = seg + (int64_t)f * S;
      if (!(c[X + kSlotCnt] > 0)) {
        c[X + kSlotPath] = NAN;
        at = -1;
        continue;
      }
      if (at < 0) at = (int)c[X + kSlotAux];
      c[X + kSlotPath] = c[at];
      at = (int)bp[(int64_t)f * W + at];
    }
  }
  return true;
}

// costPerPath() (:347-372) of the path in kSlotPath over the n frames of the segment at seg: certWeight mean(|path -
// cog|) + (1 - certWeight) mean(costJumps(path[f], path[f + 1])), both means with na.rm = TRUE (a frame without a
// path value, and a pair with one, are left out); NaN where a mean has no term, as in the reference. Every lane
// gets it; the sums as the header's other sums over frames.
template <class Sync>
SG_PATH_HD SG_PATH_CALL inline double path_cost(const double* seg, int S, int W, int n, double certWeight, int lane, int nl, double* red,
                                   Sync& sync) {
  const int X = 2 * W;
  double sc = 0, sj = 0, kc = 0, kj = 0;
  for (int f = lane; f < n; f += nl) {
    const double* c = seg + (int64_t)f * S;
    const double p = c[X + kSlotPath];
    if (p != p) continue;
    sc += fabs(p - c[X + kSlotCog]);
    kc += 1;
    if (f + 1 >= n) continue;
    const double q = (c + S)[X + kSlotPath];
    if (q != q) continue;
    sj += path_cost_jump(p, q);
    kj += 1;
  }
  sc = path_reduce(sc, 0, lane, nl, red, sync);
  kc = path_reduce(kc, 0, lane, nl, red, sync);
  sj = path_reduce(sj, 0, lane, nl, red, sync);
  kj = path_reduce(kj, 0, lane, nl, red, sync);
  const double cost_cert = sc / kc, cost_jump = sj / kj;  // 0 / 0: NaN
  return certWeight * cost_cert + (1 - certWeight) * cost_jump;
}

// One sound: nf rows of src_cols doubles at src_rows (the candidates as pitch_candidates
// leaves them, in their first P.cols - kPathCols columns) -> nf rows of P.cols doubles at
// rows: those columns, then pitch, amplVoiced, voiced (harmonics NaN: sg_anl_harm fills it),
// with the smoothed dom, the blanked quartiles and HNR in dB. src_rows may be rows itself
// (src_cols == P.cols: the table is rewritten in place, path_sound) or a table apart that
// stays untouched (a sweep's shared candidates, sg_anl_sweep_path). scr: nf * path_scratch()
// doubles; red: nl doubles and sh: 3 int64 shared by the lanes; hw: floor(smoothing_ww / 2).
// kMode says what else is compiled in, so that the modes of the reference do not pay for code they do not run (the
// default, 0, is the tail as it was): bit 0 (kPathExact) 'exact', P.pathfinding == 3, which needs dd, 2 path_width()
// doubles shared by the lanes (without the bit, 3 takes 'none': the callers choose the instantiation by P); bit 1
// (kPathSegs) the segment list: segs, nullptr or path_seg_cells(nf) doubles that receive the sound's voiced
// segments (kPathSegCells). Every lane must call it.
constexpr int kPathExact = 1, kPathSegs = 2;
template <class Sync, int kMode = 0>
SG_PATH_HD inline void path_sound_at(const PathPars& P, int nf, int hw, const double* src_rows, int src_cols, double* rows,
                                     double* scr, int lane, int nl, double* red, int64_t* sh, Sync sync, double* dd = nullptr,
                                     double* segs = nullptr) {
  const int W = path_width(P.nCands), S = path_stride(P.nCands), X = 2 * W;
  const int c0 = P.cols - kPathCols;
  int nseg = 0;
  // pitch_matrices (:578-591), log2 (pathfinder :39), the prior (:598-612), the centre of gravity (:43-49)
  for (int f = lane; f < nf; f += nl) {
    const double* row = src_rows + (int64_t)f * src_cols;
    double* c = scr + (int64_t)f * S;
    int cnt = 0;
    for (int j = 0; j < 1 + 3 * P.nCands; ++j) {
      const int m = (j - 1) / P.nCands, k = (j - 1) % P.nCands;
      const double cand = j == 0 ? row[kPathDomCand] : row[kPathFixed + 2 * m * P.nCands + k];
      const double cert = j == 0 ? row[kPathDomCert] : row[kPathFixed + (2 * m + 1) * P.nCands + k];
      if (cand != cand) continue;
      c[cnt] = log2(cand);
      c[W + cnt] = P.do_prior ? cert * path_prior(cand, P) : cert;
      ++cnt;
    }
    for (int k = cnt; k < W; ++k) c[k] = c[W + k] = NAN;
    c[X + kSlotCog] = path_mean(c, cnt);
    c[X + kSlotPath] = c[X + kSlotAux] = c[X + kSlotHz] = NAN;
    c[X + kSlotCnt] = cnt;
    c[X + kSlotDom] = row[kPathDom];
    c[X + kSlotVoiced] = cnt >= P.minVoiced ? 1.0 : 0.0;
  }
  if (lane == 0) sh[0] = 1;
  for (;;) {
    sync();
    if (lane == 0) {
      int64_t i = sh[0], s = 0, e = 0;
      if (!path_next_segment(scr + X + kSlotVoiced, S, nf, P.noRequired, P.nTolerated, &i, &s, &e)) s = 0;
      sh[0] = i;
      sh[1] = s;
      sh[2] = e;
    }
    sync();
    if (sh[1] == 0) break;
    double* seg = scr + (sh[1] - 1) * S;
    const int n = (int)(sh[2] - sh[1] + 1);
    if (P.interpolWin > 0) {
      if (lane == 0)
        for (int f = 0; f < n; ++f) path_interpolate_frame(seg, S, W, n, f, P);
      sync();
    }
    double lo = INFINITY, hi = -INFINITY, most = 0, least = INFINITY;
    for (int f = lane; f < n; f += nl) {
      double* c = seg + (int64_t)f * S;
      const int cnt = (int)c[X + kSlotCnt];
      path_sort_frame(c, c + W, cnt);
      if (cnt) {
        lo = fmin(lo, c[0]);
        hi = fmax(hi, c[cnt - 1]);
      }
      most = fmax(most, (double)cnt);
      least = fmin(least, (double)cnt);
    }
    most = path_reduce(most, 2, lane, nl, red, sync);
    least = path_reduce(least, 1, lane, nl, red, sync);
    if (most <= 1) {  // a single row: no paths to choose among (:87-89)
      for (int f = lane; f < n; f += nl) {
        double* c = seg + (int64_t)f * S;
        c[X + kSlotHz] = c[X + kSlotCnt] > 0 ? exp2(c[0]) : NAN;
        if ((kMode & kPathSegs) && segs) c[X + kSlotPath] = c[X + kSlotCnt] > 0 ? c[0] : NAN;
      }
      if ((kMode & kPathSegs) && segs) {  // the cost of the only path there is
        sync();
        const double cost = path_cost(seg, S, W, n, P.certWeight, lane, nl, red, sync);
        if (lane == 0) {
          double* o = segs + 1 + (int64_t)kPathSegCells * nseg;
          o[0] = (double)sh[1], o[1] = (double)sh[2], o[2] = most, o[3] = cost;
        }
        ++nseg;
      }
      continue;
    }
    if (n >= 2 && P.pathfinding == 1) {  // pathfinding_fast (:203-267)
      const int nh = n < 5 ? n : 5;
      const double pF = path_median(seg + X + kSlotCog, S, nh);
      bool na = false;  // the backward median has no na.rm
      for (int f = n - nh; f < n; ++f) na = na || seg[(int64_t)f * S + X + kSlotCog] != seg[(int64_t)f * S + X + kSlotCog];
      const double pB = na ? NAN : path_median(seg + (int64_t)(n - nh) * S + X + kSlotCog, S, nh);
      const double* c1 = seg + (int64_t)(n - 1) * S;
      const double startF = path_start(seg, seg + W, (int)seg[X + kSlotCnt], pF);
      const double startB = path_start(c1, c1 + W, (int)c1[X + kSlotCnt], pB);
      double costF = 0, costB = 0;
      for (int f = lane; f < n; f += nl) {
        double* c = seg + (int64_t)f * S;
        const int cnt = (int)c[X + kSlotCnt];
        double cost = 0;
        int k = f == 0 ? -1 : path_choose(c, cnt, c[X + kSlotCog], startF, 1, P.certWeight, &cost);
        c[X + kSlotPath] = f == 0 ? startF : (k < 0 ? NAN : c[k]);
        if (f != 0) costF += cost;
        k = f == n - 1 ? -1 : path_choose(c, cnt, c[X + kSlotCog], startB, 1, P.certWeight, &cost);
        c[X + kSlotAux] = f == n - 1 ? startB : (k < 0 ? NAN : c[k]);
        if (f != n - 1) costB += cost;
      }
      costF = path_reduce(costF, 0, lane, nl, red, sync);
      costB = path_reduce(costB, 0, lane, nl, red, sync);
      if (!(costF < costB))
        for (int f = lane; f < n; f += nl) seg[(int64_t)f * S + X + kSlotPath] = seg[(int64_t)f * S + X + kSlotAux];
    } else if (!((kMode & kPathExact) && n >= 2 && P.pathfinding == 3 && dd &&  // 'exact'; false: no neighbouring frames
                 path_exact(seg, S, W, n, P.certWeight, scr + (int64_t)nf * S + (sh[1] - 1) * W, dd, lane, nl, red, sync))) {
      // 'none' (:110-113)
      for (int f = lane; f < n; f += nl) {
        double* c = seg + (int64_t)f * S;
        double cost;
        const int k = path_choose(c, (int)c[X + kSlotCnt], c[X + kSlotCog], NAN, 0, P.certWeight, &cost);
        c[X + kSlotPath] = k < 0 ? NAN : c[k];
      }
    }
    sync();
    if ((kMode & kPathSegs) && segs) {  // before the snake moves the path
      const double cost = path_cost(seg, S, W, n, P.certWeight, lane, nl, red, sync);
      if (lane == 0) {
        double* o = segs + 1 + (int64_t)kPathSegCells * nseg;
        o[0] = (double)sh[1], o[1] = (double)sh[2], o[2] = most, o[3] = cost;
      }
      ++nseg;
    }
    // snake() (:419-475); not run on a segment with a frame that has no candidate (in the
    // reference its first force_new is NA and it breaks at once)
    if (P.snakeStep > 0 && least > 0) {
      lo = path_reduce(lo, 1, lane, nl, red, sync);
      hi = path_reduce(hi, 2, lane, nl, red, sync);
      const double maxIter = floor((hi - lo) / P.snakeStep * 2);
      const double* p = seg + X + kSlotPath;
      double force_old = 1e10;
      for (double it = 1; it < maxIter; it += 1) {
        double sl, sr, part = 0;
        path_end_slopes(p, S, n, &sl, &sr);
        for (int f = lane; f < n; f += nl) {
          double* c = seg + (int64_t)f * S;
          const double force = path_force(c, c + W, (int)c[X + kSlotCnt], c[X + kSlotPath], path_grad(p, S, n, f, sl, sr),
                                          P.certWeight);
          c[X + kSlotAux] = force;
          part += fabs(force);
        }
        const double force_new = path_reduce(part, 0, lane, nl, red, sync) / n;
        const double force_delta = (force_old - force_new) / force_old;
        force_old = force_new;
        if (force_delta != force_delta || force_delta < P.snakeStep) break;
        for (int f = lane; f < n; f += nl) {
          double* c = seg + (int64_t)f * S;
          c[X + kSlotPath] = c[X + kSlotPath] + P.snakeStep * c[X + kSlotAux];
        }
        sync();
      }
    }
    for (int f = lane; f < n; f += nl) {
      double* c = seg + (int64_t)f * S;
      c[X + kSlotHz] = exp2(c[X + kSlotPath]);  // 2 ^ bestPath; NaN where the frame had no candidate
    }
  }
  sync();
  if ((kMode & kPathSegs) && segs && lane == 0) segs[0] = nseg;
  // medianSmoother (:670-681, reading the unsmoothed copies) and the final columns (:685-703)
  for (int f = lane; f < nf; f += nl) {
    double* row = rows + (int64_t)f * P.cols;
    if (src_rows != rows) {  // a table apart: the pair's own copy of the columns in front
      const double* src = src_rows + (int64_t)f * src_cols;
      for (int q = 0; q < c0; ++q) row[q] = src[q];
    }
    const double* c = scr + (int64_t)f * S;
    const int a = f - hw < 0 ? 0 : f - hw, b = f + hw > nf - 1 ? nf - 1 : f + hw;
    double pitch = c[X + kSlotHz], dom = c[X + kSlotDom];
    if (P.smooth_pitch && pitch == pitch)
      pitch = path_smooth(pitch, path_median(scr + (int64_t)a * S + X + kSlotHz, S, b - a + 1), P.smoothThres);
    if (P.smooth_dom && dom == dom)
      dom = path_smooth(dom, path_median(scr + (int64_t)a * S + X + kSlotDom, S, b - a + 1), P.smoothThres);
    const bool voiced = pitch == pitch;
    row[kPathDom] = dom;
    row[c0 + kPathPitch] = pitch;
    row[c0 + kPathAmplVoiced] = voiced ? row[kPathAmpl] : NAN;
    row[c0 + kPathVoiced] = voiced ? 1.0 : 0.0;
    row[c0 + kPathHarmonics] = NAN;
    if (!voiced)
      for (int q = kPathQ25; q <= kPathQ75; ++q) row[q] = NAN;
    row[kPathHNR] = path_to_dB(row[kPathHNR]);
  }
}

// One sound whose table is rewritten in place: rows holds the candidates and receives the result
template <class Sync, int kMode = 0>
SG_PATH_HD inline void path_sound(const PathPars& P, int nf, int hw, double* rows, double* scr, int lane, int nl,
                                  double* red, int64_t* sh, Sync sync, double* dd = nullptr, double* segs = nullptr) {
  path_sound_at<Sync, kMode>(P, nf, hw, rows, P.cols, rows, scr, lane, nl, red, sh, sync, dd, segs);
}

}  // namespace sg
