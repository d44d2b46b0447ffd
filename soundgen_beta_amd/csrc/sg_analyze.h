// sg_analyze.h — the per-frame stage of analyze() (R/analyze.R:233-575,
// R/utilities_analyze.R:22-324): host decisions (sg_analyze.cpp) and the device
// launch sequence (sg_analyze.hip).
#pragma once
#include <cstdint>
#include <vector>

#include "sg_path.h"
#include "sg_spectrogram.h"
#include "sg_summary.h"
#include "soundgen_hip.h"

namespace sg {

constexpr int kAnlStages = 4;    // sg_debug_analyze_kernel_ms
constexpr int kAnlMaxCands = 8;  // nCands
constexpr int kAnlFixed = 15;    // columns before autocorCand / autocorCert
// columns of a frame's row
enum AnlCol { kAmpl = 0, kEntropy, kHNR, kDom, kPeakFreq, kPeakFreqCut, kMeanFreq, kQ25, kQ50, kQ75, kSlope, kDomCand,
              kDomCert, kCondSilence, kCondEntropy };

// What the stage decides from its arguments alone, validated. Every label has made
// R's 15-significant-digit character round trip (spectrogram.R:176, analyze.R:484).
struct AnlSetup {
  SpgSetup spg;            // getFrameBank / spectrogram(output = 'original'), zp = 0
  double silence = 0, entropyThres = 0, domThres = 0, autocorThres = 0;
  int nCands = 1, cols = 0;
  int do_autocor = 0, do_dom = 0;
  int rowLow = 0, rowHigh = 0;  // 1-based, inclusive: the entropy band (:466-467)
  int cut0 = 0, ncut = 0;       // the cut band freq > pitchFloor & freq < cutFreq: bins [cut0, cut0 + ncut)
  int pf_idx = 0;               // pitchFloor_idx, 1-based (utilities_analyze.R:216)
  int domW = 0, acW = 0;        // domSmooth_bins, autocorSmooth
  int lag0 = 0, nlag = 0;       // lags [lag0, lag0 + nlag) are read by getPitchAutocor
  std::vector<double> freq;     // 1000 * label of every bin (Hz)
  std::vector<double> xc;       // the cut band's freq - mean(freq), for the slope
  double sxx = 0;               // sum(xc^2)
  std::vector<double> lagf;     // label samplingRate / j of the used rows
};
AnlSetup anl_setup(const sg_analyze_params& p);
// the same for any non-empty subset of the four pitch methods: what the stage, pitch_candidates and analyze() share
// (the window, the frames, the columns up to cond_entropy), for the formants that run behind any of the three
AnlSetup anl_setup_any(const sg_analyze_params& p);
// the formants' order round(samplingRate / 1000) + 3 (sg_formants.h); SG_E_ARG for nFormants outside 1..8,
// SG_E_UNSUPPORTED for an order above 64
int formants_order(double samplingRate, int nFormants);
// SG_E_ARG for a window of wl samples that is not longer than the order
void formants_window(int wl, int order);
// frames of a sound of len samples: 0 for len <= wl
int anl_frames(const AnlSetup& S, int64_t len);
// 0-based first sample of frame f's amplitude window of wl + 1 samples
int64_t anl_ampl_start(const AnlSetup& S, int64_t len, int frames, int f);
// autoCorrelation_filter (:403-407) at the used lags, fp64
std::vector<double> anl_filter(const AnlSetup& S);

// pitch_candidates: the stage plus the cepstral and the spectral (BaNa) tracker
// (getPitchCep, R/utilities_analyze.R:337-407; getPitchSpec, :424-558). A row then has
// kAnlFixed + 6 nCands columns: autocorCand, autocorCert, cepCand, cepCert, specCand, specCert.
constexpr int kPitchStages = 6;  // sg_debug_pitch_kernel_ms: the four of analyze_frames, cepstrum, BaNa
struct PitchSetup : AnlSetup {
  int do_cep = 0, do_spec = 0;
  double pitchFloor = 0, pitchCeiling = 0;
  double cepThres = 0, specThres = 0, specPeak = 0, specSinglePeakCert = 0, specMerge = 0;
  int cepL = 0;            // length(frameZP): bins + 2 floor((cepZp - bins) / 2), or bins
  int cepPad = 0;          // zeros on either side of the frame
  int cepW = 0;            // the effective cepSmooth (after * round(cepZp / bins))
  int cepl = 0;            // L %/% 2 rows of the cepstrum are labelled
  int cep0 = 0, ncep = 0;  // rows [cep0, cep0 + ncep) (0-based: quefrency cep0 + 1 ...) lie in (pitchFloor, pitchCeiling)
  std::vector<double> cepf;  // their labels samplingRate / k / 2 * (L / bins)
  int specW = 0;           // getPitchSpec's width
};
PitchSetup pitch_setup(const sg_pitch_params& p);

// analyze(): pitch_candidates plus the tail behind the candidates (R/analyze.R:576-707,
// R/utilities_pitch_postprocessing.R; sg_path.h). A row then has kAnlFixed + 6 nCands +
// kPathCols columns: the candidates', then pitch, amplVoiced, voiced, harmonics.
constexpr int kTrackStages = 8;  // sg_debug_track_kernel_ms: the six of pitch_candidates, the path, the harmonics
struct TrackSetup : PitchSetup {
  PathPars path;            // the prior's shape, rate and normaliser, the resolved minVoicedCands, noRequired, ...
  double smooth = 0;        // <= 0: no medianSmoother
  std::vector<double> lab;  // the frequency label of every bin (kHz, after the round trip): `harmonics` reads it
};
// what the tail decides from p alone (of p.p only a.samplingRate, a.step, a.windowLength, a.overlap, a.nCands,
// a.pitchFloor, a.pitchCeiling and a.methods are read), validated
PathPars track_path_pars(const sg_analyze_params_full& p, double* smooth);
TrackSetup track_setup(const sg_analyze_params_full& p);
// floor(smoothing_ww / 2) for a sound of len samples and `frames` frames (:671-673); SG_E_UNSUPPORTED above kPathMaxWin
int track_hw(double smooth, double samplingRate, int64_t len, int frames);

// analyze(summary = TRUE): a sound's table in the buffer sg_anl_summary reads (sg_summary.h)
struct SumSound {
  int64_t row0;  // first double of its table
  int64_t len;   // samples (duration = len / samplingRate)
  int32_t nf, pad;
};
// one row of kSumCols doubles per sound into d_summary (device), from finished tables of `cols` columns on the device;
// kernel_ms (or nullptr): the device time of the kernel. Synchronises the stream.
void summary_device(const std::vector<SumSound>& snds, int cols, double samplingRate, const double* d_tables,
                    double* d_summary, hipStream_t s, double* kernel_ms);

// pitch: nullptr for analyze_frames (S is then a plain AnlSetup), else S itself; track:
// nullptr for analyze_frames and pitch_candidates, else S itself (then pitch is S too);
// d_summary: nullptr, or (with track) n_calls x kSumCols doubles of device memory that sg_anl_summary fills in the
// same launch sequence, its device time going to summary_ms
template <typename T>
void analyze_device(const AnlSetup& S, const T* d_x, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                    double* d_out, const int64_t* out_off, int32_t* frames_out, hipStream_t s, double* kernel_ms,
                    const PitchSetup* pitch = nullptr, const TrackSetup* track = nullptr, double* d_summary = nullptr,
                    double* summary_ms = nullptr);
// the path stage alone on n rows of P.cols doubles already on the device (sg_pitch_path); d_segs: nullptr, or
// path_seg_cells(frames) doubles on the device for the sound's segment list (sg_pitch_path_costs)
void path_device(const PathPars& P, int frames, int hw, double* d_rows, hipStream_t s, double* kernel_ms,
                 double* d_segs = nullptr);

// A parameter sweep of analyze(summary = TRUE) (sg_analyze_sweep): what the rows may share, decided from the
// resolved setups alone. Groups are numbered by first appearance.
//   frame group: equal SpgSetup, so equal frames and amplitude windows; owns |X|, the statistics, min(ampl)
//   store group (within a frame group; -1 without 'autocor'): also equal gates (silence, entropyThres, rowLow,
//     rowHigh) and lag band (lag0, nlag); owns the corrected autocorrelations of the gated frames
//   candidate group (within a frame group): every field of AnlSetup and PitchSetup equal; owns one candidate
//     table of kAnlFixed + 6 nCands columns per sound
constexpr int kSweepStages = 10;  // sg_debug_analyze_sweep_kernel_ms
constexpr int64_t kSweepWorkspaceCap = 1ll << 30;  // bytes of a store and of a chunk's pair tables, workspace_cap = 0
struct SweepPlan {
  std::vector<TrackSetup> S;  // per row
  std::vector<int32_t> frame_group, store_group, cand_group;
  int n_frame = 0, n_store = 0, n_cand = 0;
};
// every row through track_setup(); SG_E_* with "row r: " in front of the text for a refused row and for a row whose
// samplingRate is not rows[0]'s
SweepPlan anl_sweep_plan(const sg_analyze_params_full* rows, int64_t n_rows);
// the bytes sg_analyze_sweep_size reports: bytes[0] the largest frame group's |X| and candidate tables, bytes[1] the
// largest store that at least two candidate groups share (0: none), bytes[2] the largest tail workspace of one row
void anl_sweep_bytes(const SweepPlan& W, const int64_t* lengths, int64_t n_calls, int64_t* bytes);

}  // namespace sg
