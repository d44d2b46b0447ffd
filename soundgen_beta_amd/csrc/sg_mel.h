// sg_mel.h — compareSounds() / getMelSpec() on the device (sg_mel.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "soundgen_hip.h"

namespace sg {

// tuneR melfcc geometry of one parameter set (host, fp64, R's operation order)
struct MelGeom {
  int winpts = 0, steppts = 0, nfft = 0, nfreqs = 0, nb = 0;
  double thr = 0;                      // 2^(throwaway / 10)
  std::vector<double> ham;             // hamming(winpts)
  std::vector<int32_t> band_k0, band_n, band_w0;  // per mel band: its bins' weights
  std::vector<double> w;
  std::vector<double> tw, twN;         // e^{-2 pi i t / M} (t < M/2), e^{-2 pi i k / nfft} (k < M), (re, im)
};
MelGeom mel_geom(const sg_mel_params& p);
// the same with melfcc's maxfreq and nbands given (ssm() passes its own)
MelGeom mel_geom(double sr, double windowLength, double step, double maxFreq, int nb, double throwaway);
int mel_frames(const MelGeom& g, int64_t len);

// getMelSpec of one waveform already on the device: nb x nk column-major into out
void mel_spec_device(const MelGeom& g, const double* d_x, int64_t len, std::vector<double>& out, int* nk,
                     hipStream_t s);
// compareSounds(targetSpec = tspec (host, nb x ncT, getMelSpec's value: already normalised),
// cand = each candidate of d_x): out[4 c + m] per method (cor, cosine, pixel, dtw), summary[c]
// (may be null). The pairs (target, c) through the kernels of compare_sounds_pairs_device, the
// target read as it stands; ncT = 0 is a target without a column, not an absent one.
void compare_sounds_device(const MelGeom& g, const double* tspec, int ncT, const float* d_x, const int64_t* offsets,
                           const int64_t* lengths, int64_t n, int methods, int penalize, double* out, double* summary,
                           hipStream_t s);

// The mel spectra of a batch of sounds kept in HBM (sg_mel_set_*): what the frame and
// kept-column kernels leave behind -- the raw band spectra, the kept-frame lists, nkept, min
// and max per sound and the sound table -- with the geometry they were computed under. The
// waveform itself is not kept. Sound c of d_x (float or double) is at offsets[c], lengths[c]
// samples; lengths[c] <= 0: skipped (no frame, NaN in every comparison).
struct MelRun;
struct MelSet {
  MelSet(sg_ctx* ctx, const sg_mel_params& p, const void* d_x, bool f64, const int64_t* offsets,
         const int64_t* lengths, int64_t n);
  ~MelSet();
  MelSet(const MelSet&) = delete;
  MelSet& operator=(const MelSet&) = delete;
  // getMelSpec of sound i: nb x nk column-major, as mel_spec_device
  void spec(int64_t i, std::vector<double>& out, int* nk) const;
  // the sets were computed under one geometry (winpts, steppts, nfft, nb, maxFreq, throwaway)
  bool same_geometry(const MelSet& o) const;

  sg_ctx* ctx;
  MelGeom g;
  double maxFreq, throwaway;
  int64_t n;
  std::vector<int32_t> ncols;  // kept columns per sound (0 for a skipped one)
  MelRun* r;
};
// compareSounds(target = sound pairs[2 p] of T, cand = sound pairs[2 p + 1] of C) for n_pairs
// pairs in one launch sequence (sg_mel_pair, sg_mel_pair_reduce; the only comparison path, which
// compare_sounds_device shares): out[4 p + m], summary[p]
// (may be null). The indices are the caller's to check. More than 2^31 - 1 column jobs:
// SG_E_UNSUPPORTED. profile: the device time of the two kernels is kept for
// sg_debug_mel_pair_kernel_ms.
void compare_sounds_pairs_device(const MelSet& T, const MelSet& C, const int32_t* pairs, int64_t n_pairs, int methods,
                                 int penalize, double* out, double* summary, hipStream_t s, bool profile);

}  // namespace sg

// the C ABI's handle of a MelSet
struct sg_mel_set {
  std::unique_ptr<sg::MelSet> set;
};
