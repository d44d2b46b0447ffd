/*
 * soundgen_hip.h — C-ABI of libsoundgen_hip.so, the MI355X-native engine for
 * soundgen's additive-source + formant-filter hot path.
 *
 * Reference interfaces this ABI replaces (nemochina2008/soundgen_beta, R):
 *   soundgen()            R/soundgen.R:208-862   -> sg_soundgen / sg_plan_batch+sg_execute
 *   generateHarmonics()   R/source.R:173-471     -> sg_generate_harmonics
 *   generateNoise()       R/source.R:57-138      -> sg_generate_noise
 *   getSpectralEnvelope() R/sourceSpectrum.R:261-566 -> sg_spectral_envelope
 *   getRolloff()          R/sourceSpectrum.R:71-186  -> sg_get_rolloff (host helper)
 *   seewave::stft/istft + z*env (R/soundgen.R:779-806) -> sg_formant_filter
 *
 * Conventions (mirroring R's .Call world):
 *   - plain pointers + sizes, doubles on the host side (R numeric vectors);
 *   - every function returns 0 or a negative SG_E_* code; no C++ exception
 *     ever crosses this boundary; sg_last_error() gives the message;
 *   - random draws are INJECTED (R draws them in the reference's order and
 *     passes them in): standard normals and standard uniforms are consumed
 *     sequentially in R's draw order (see DESIGN.md "Randomness").
 *   - "NA" anchors/formants are encoded as n == 0; NULL scalars as NaN.
 */
#ifndef SOUNDGEN_HIP_H
#define SOUNDGEN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_ABI_VERSION 5

enum {
  SG_OK = 0,
  SG_E_ARG = -1,         /* invalid argument (R: stop()) */
  SG_E_DOMAIN = -2,      /* R would error inside approx()/spline() etc. */
  SG_E_RANDOM = -3,      /* injected random stream exhausted */
  SG_E_UNSUPPORTED = -4, /* valid in R but not yet supported (e.g. loess) */
  SG_E_DEVICE = -5,      /* HIP runtime error */
  SG_E_CAPACITY = -6,    /* output buffer too small */
  SG_E_NOMEM = -7
};

/* A data.frame(time, value) of anchors. n == 0 encodes NA / NULL. */
typedef struct sg_anchors {
  int32_t n;
  const double* time;
  const double* value;
} sg_anchors;

/* A list of formants, each a data.frame(time, freq, amp, width) with
 * n_points[f] rows; arrays are concatenated over formants. n_formants == 0
 * encodes NA. f1_index is the position of the formant named "f1" (-1 if
 * absent; needed by the nasalization branch, R/sourceSpectrum.R:469-504). */
typedef struct sg_formants {
  int32_t n_formants;
  int32_t f1_index;
  const int32_t* n_points;
  const double* time;
  const double* freq;
  const double* amp;
  const double* width;
} sg_formants;

/* Random draws, consumed in the reference's draw order: standard normals
 * (rnorm), standard uniforms (runif) and gamma variates (rgamma). The arrays
 * are used first; once one is exhausted (or NULL) the matching callback is
 * called if set, else the call fails with SG_E_RANDOM. The R shim binds the
 * callbacks to R's own norm_rand()/unif_rand()/rgamma() so that draws follow
 * set.seed() exactly; tests inject arrays.
 * unif_n_cb (ABI 5, may be NULL): n consecutive uniforms into out, the same
 * values n unif_cb calls would return -- R: runif(n), i.e. unif_rand() in one C
 * loop. The planner takes generateNoise()'s runif(nr * nc) (R/source.R:111; ~8 k
 * draws per C5 call) through it in blocks instead of one callback per draw. */
typedef struct sg_random {
  const double* normals;
  int64_t n_normals;
  const double* uniforms;
  int64_t n_uniforms;
  double (*norm_cb)(void* user);
  double (*unif_cb)(void* user);
  double (*gamma_cb)(void* user, double shape, double rate);
  void* user;
  void (*unif_n_cb)(void* user, double* out, int64_t n);
} sg_random;

/* R's default random number generation (R 3.4.0: Mersenne-Twister,
 * Inversion normals), so that a seeded call draws what
 * `set.seed(seed); soundgen(...)` draws in R without R present. Replaces the
 * R runtime's unif_rand / norm_rand / exp_rand / rgamma (src/main/RNG.c,
 * src/nmath/{snorm,qnorm,sexp,rgamma}.c) reached by the reference through
 * runif/rnorm/rgamma calls, e.g. R/source.R:111, :278, :349,
 * R/utilities_math.R:212, :295, R/sourceSpectrum.R:384. sg_random_bind_rrng
 * points an sg_random's callbacks at one generator (one stream, so R's
 * interleaving of the draw kinds is kept). */
typedef struct sg_rrng sg_rrng;
int sg_rrng_create(int32_t seed, sg_rrng** out);  /* = set.seed(seed) */
void sg_rrng_destroy(sg_rrng* g);
void sg_rrng_set_seed(sg_rrng* g, int32_t seed);
double sg_rrng_unif(sg_rrng* g);                  /* runif(1) */
void sg_rrng_unif_n(sg_rrng* g, double* out, int64_t n); /* runif(n) (ABI 5) */
double sg_rrng_norm(sg_rrng* g);                  /* rnorm(1) */
double sg_rrng_exp(sg_rrng* g);                   /* rexp(1) */
double sg_rrng_gamma(sg_rrng* g, double shape, double scale); /* rgamma(1, shape, scale = scale) */
void sg_random_bind_rrng(sg_random* r, sg_rrng* g);

/* Formals of generateHarmonics(), R/source.R:173-205 (pitch and amplAnchors
 * are separate arguments). */
typedef struct sg_harm_params {
  double attackLen, nonlinBalance, nonlinDep, jitterDep, jitterLen;
  double vibratoFreq, vibratoDep, shimmerDep, creakyBreathy;
  double rolloff, rolloffOct, rolloffKHz, rolloffParab, rolloffParabHarm;
  double rolloffLip, rolloff_perAmpl, temperature, pitchDriftDep;
  double pitchDriftFreq, randomWalk_trendStrength, shortestEpoch, subFreq;
  double subDep, amDep, amFreq, overlap, samplingRate, pitchFloor;
  double pitchCeiling, pitchSamplingRate, throwaway;
} sg_harm_params;

/* Formals of soundgen(), R/soundgen.R:208-277. tempEffects is flattened in
 * the order sylLenDep, formDrift, formDisp, pitchDriftDep, pitchDriftFreq,
 * pitchAnchorsDep, noiseAnchorsDep, amplAnchorsDep. vocalTract NaN = NULL. */
typedef struct sg_soundgen_args {
  double repeatBout, nSyl, sylLen, pauseLen;
  sg_anchors pitchAnchors, pitchAnchorsGlobal;
  double temperature;
  double tempEffects[8];
  double maleFemale, creakyBreathy, nonlinBalance, nonlinDep;
  double jitterLen, jitterDep, vibratoFreq, vibratoDep, shimmerDep;
  double attackLen, rolloff, rolloffOct, rolloffKHz, rolloffParab;
  double rolloffParabHarm, rolloffLip;
  sg_formants formants;
  double formantDep, formantDepStoch, vocalTract;
  double subFreq, subDep, shortestEpoch, amDep, amFreq, amShape;
  sg_anchors noiseAnchors;
  sg_formants formantsNoise;
  double rolloffNoise;
  sg_anchors mouthAnchors, amplAnchors, amplAnchorsGlobal;
  double samplingRate, windowLength, overlap, addSilence;
  double pitchFloor, pitchCeiling, pitchSamplingRate, throwaway;
  int32_t invalidArgAction; /* 0 adjust, 1 abort, 2 ignore */
  /* max(unlist(lapply(formantsNoise, length))) evaluated on the caller's own
   * formantsNoise (R/soundgen.R:662-663): 1 for a vowel string, the number of
   * fields (4) for a list of formant lists. Noise formants are "moving" (one
   * envelope column per 10 ms) when it exceeds 1 or the mouth moves.
   * 0 = not supplied: treated as a list of formant lists (moving). */
  int32_t formantsNoise_rlen;
} sg_soundgen_args;

/* One call of a batch: either a whole soundgen() call or a bare
 * generateHarmonics() call on a given pitch contour. */
enum { SG_CALL_SOUNDGEN = 0, SG_CALL_HARMONICS = 1 };
typedef struct sg_call_desc {
  int32_t kind;
  /* SG_CALL_SOUNDGEN */
  const sg_soundgen_args* args;
  /* SG_CALL_HARMONICS */
  const double* pitch;
  int64_t pitch_len;
  const sg_harm_params* harm;
  sg_anchors amplAnchors;
  /* random draws for this call (both kinds) */
  sg_random random;
} sg_call_desc;

typedef struct sg_ctx sg_ctx;
typedef struct sg_plan sg_plan;

/* ---- context ---------------------------------------------------------- */
int sg_ctx_create(int device, sg_ctx** out);
void sg_ctx_destroy(sg_ctx* ctx);
const char* sg_last_error(const sg_ctx* ctx);
int sg_abi_version(void);
/* Fill the defaults of generateHarmonics()/soundgen() formals. */
void sg_default_harm_params(sg_harm_params* p);
void sg_default_soundgen_args(sg_soundgen_args* a);

/* ---- whole-node batch path: one process, several devices (ABI 3) --------
 * Replaces the single-device loop behind the R batch callers that north_star
 * keeps: soundgen_batch(), morph() (R/morph.R:200-208) and matchPars()
 * (R/matchPars.R:168-202), each a list of independent soundgen() calls.
 * A node is a list of device ordinals (a device may appear more than once;
 * NULL: 0 .. n - 1, and n <= 0 with NULL: every visible device). Planning needs
 * no device; each device's context is created on first execution. */
typedef struct sg_node sg_node;
typedef struct sg_node_plan sg_node_plan;
int sg_device_count(void);
int sg_node_create(const int32_t* devices, int32_t n, sg_node** out);
void sg_node_destroy(sg_node* node);
int32_t sg_node_size(const sg_node* node);
const char* sg_node_last_error(const sg_node* node);
/* Calls are assigned to the node's devices by LPT over an analytic cost per
 * call (samples x kept harmonic rows, STFT frames, per-sample assembly); each
 * device's shard is planned as one sg_plan. Lengths, offsets, statuses and
 * messages are those of the WHOLE batch in call order with sg_plan_batch's
 * layout, and every call's samples equal what sg_plan_batch of the whole batch
 * produces (a call's arithmetic does not depend on the batch around it). With
 * draw callbacks (R's RNG) the calls are first run in call order in a draws-only
 * pass that records each call's draws -- R's stream, R's order; a failing call ends
 * it as lapply() would -- and the shards are then planned, on host threads, from
 * the recorded draws (ABI 5: the recording pass no longer plans the device work).
 * Calls that carry only injected arrays are planned as given. */
int sg_node_plan_batch(sg_node* node, const sg_call_desc* calls, int64_t n_calls, sg_node_plan** out);
void sg_node_plan_destroy(sg_node_plan* plan);
int64_t sg_node_plan_n_calls(const sg_node_plan* plan);
int64_t sg_node_plan_total_samples(const sg_node_plan* plan);
int sg_node_plan_lengths(const sg_node_plan* plan, int64_t* out_len, int64_t* out_off);
int sg_node_plan_status(const sg_node_plan* plan, int32_t* out_status);
const char* sg_node_plan_call_message(const sg_node_plan* plan, int64_t i);
/* the node device index (0 .. size - 1) each call was assigned to */
int sg_node_plan_owner(const sg_node_plan* plan, int32_t* owner);
/* the analytic cost per call the assignment used (ns of one MI355X) */
int sg_node_plan_costs(const sg_node_plan* plan, double* cost);
int64_t sg_node_plan_shard_samples(const sg_node_plan* plan, int32_t k);
/* ABI 5: chunk plans of shard k (consecutive calls of the shard, <= SG_NODE_CHUNK
 * calls -- default 4096 -- and ~2^27 samples each: the unit of the execute pipeline) */
int32_t sg_node_plan_chunks(const sg_node_plan* plan, int32_t k);
/* ABI 5: 1 when a call failed in the shard planning after its recorded draws
 * succeeded (a failure behind a call's last draw that the draws-only recording pass
 * does not raise): later callback calls are then "not planned" as R's loop would
 * leave them, but their draws were consumed. 0 otherwise. */
int32_t sg_node_plan_diverged(const sg_node_plan* plan);
/* ABI 5: sg_plan_call_work per call of the whole batch (rows, flops: n_calls
 * doubles each, either may be NULL; unplanned calls are left untouched) */
int sg_node_plan_call_work(const sg_node_plan* plan, double* rows, double* fft_flops);
/* Synchronous: every device uploads, synthesizes its shard on its own streams
 * and copies it over its own link; each call's samples land in out_host at its
 * whole-batch offset (sg_node_plan_total_samples values in all). ABI 5: pipelined
 * by chunk (the D2H of a chunk overlaps the compute of the later ones and the host
 * scatter of the earlier one); the device output and two pinned staging slots of
 * the largest chunk stay allocated per device until sg_node_destroy. */
int sg_node_execute_to_host(sg_node* node, sg_node_plan* plan, double* out_host);
int sg_node_execute_to_host_f32(sg_node* node, sg_node_plan* plan, float* out_host);

/* ---- batch path (planned on host, executed on device) ------------------ */
/* All integer/length bookkeeping happens here, bit-exact with R. */
int sg_plan_batch(sg_ctx* ctx, const sg_call_desc* calls, int64_t n_calls,
                  sg_plan** out);
void sg_plan_destroy(sg_plan* plan);
int64_t sg_plan_n_calls(const sg_plan* plan);
int64_t sg_plan_total_samples(const sg_plan* plan);
/* per-call output length and offset into the packed output (int64 each) */
int sg_plan_lengths(const sg_plan* plan, int64_t* out_len, int64_t* out_off);
/* per-call status (0 ok or SG_E_*): a failed call marks its slot, the batch
 * does not abort (SURVEY §5 failure detection). */
int sg_plan_status(const sg_plan* plan, int32_t* out_status);
/* Bytes of device workspace the plan needs (descriptors + scratch). */
int64_t sg_plan_device_bytes(const sg_plan* plan);
/* Upload descriptors/inputs to HBM (outside any timed region). */
int sg_plan_upload(sg_ctx* ctx, sg_plan* plan);
/* After upload: free the plan's host copies of descriptors and inputs (a
 * 65,536-call preset batch holds ~0.7 MB per call on the host). Execution needs
 * nothing of the host plan: sg_execute and sg_execute_plans read the uploaded
 * device plan alone. Lengths, offsets, statuses, messages and the sg_plan_*
 * statistics keep working; re-upload does not.
 * The arrays are returned to the OS on a detached host thread, so the
 * call returns before their pages are unmapped.
 * No reference counterpart (R holds nothing between calls). */
int sg_plan_release_host(sg_plan* plan);
/* Run every kernel of the plan on `stream` (hipStream_t; NULL = the null
 * stream, ordered after earlier null-stream work such as torch's default stream)
 * writing fp32 samples into device buffer d_out (packed, offsets as above).
 * No host synchronisation inside; graph-capturable. */
int sg_execute(sg_ctx* ctx, sg_plan* plan, float* d_out, void* stream);
/* Several uploaded plans executed as ONE batch on `stream` (the outputs of
 * plan i go to d_outs[i], exactly as sg_execute(plans[i], d_outs[i]) would
 * write them): the harmonic chains of all plans run back to back on the
 * context's second stream, overlapping the spectral phases of the earlier
 * plans; everything is ordered after prior work on `stream` and joined back
 * to it. A plan may appear once. Replaces a loop of sg_execute over the 16k-call
 * chunks of one soundgen() batch (R/soundgen.R:208-862 per call). */
int sg_execute_plans(sg_ctx* ctx, sg_plan* const* plans, float* const* d_outs, int n, void* stream);
/* Profiling: when enabled, sg_execute brackets every sine-bank launch (one
 * per batch slice) and every sg_stft_ola launch with HIP events on the launch
 * stream; sg_profile_read
 * returns the average launch duration (ms) and the number of launches
 * recorded, and clears them. While profiling is on, the harmonic chain and
 * the noise phase (otherwise concurrent on the context's two streams) run one
 * after the other, so each recorded duration is the launch's own. */
int sg_set_profiling(sg_ctx* ctx, int on);
int sg_profile_read(sg_ctx* ctx, double* sine_ms_avg, int64_t* n);
/* Same for one kernel: SG_PROF_SINE_BANK (sg_sine_bank, generateHarmonics'
 * sine bank, R/source.R:389-419) or SG_PROF_STFT_OLA (sg_stft_ola, the fused
 * seewave stft/istft + overlap-add of R/soundgen.R:743-807 and R/source.R:88-131;
 * one event pair per phase launch). */
#define SG_PROF_SINE_BANK 0
#define SG_PROF_STFT_OLA 1
int sg_profile_read_kernel(sg_ctx* ctx, int kernel, double* ms_avg, int64_t* n);
int sg_synchronize(sg_ctx* ctx);
/* Synchronous convenience: upload (if needed), execute and copy the packed
 * output to host doubles: call i's samples land at out_host + offset[i]
 * (sg_plan_lengths), sg_plan_total_samples(plan) doubles in all. Random draws
 * happen only in sg_plan_batch, so a caller can size its buffer from the plan
 * before any sample is produced. */
int sg_execute_to_host(sg_ctx* ctx, sg_plan* plan, double* out_host);
/* Message of a failed call (status != 0). */
const char* sg_plan_call_message(const sg_plan* plan, int64_t i);
/* Per-kernel launch statistics of the last sg_execute (for roofline). */
int sg_plan_kernel_stats(const sg_plan* plan, int64_t* harm_samples,
                         int64_t* harm_terms, int64_t* harm_amp_bytes,
                         int64_t* fft_frames);
/* Wavetable spans of an uploaded plan (sg_set_sine_table): workgroups that
 * each build a table per execute, the samples they produce and the (sample, row) recurrence terms
 * those samples stand in for; zeros before upload. */
int sg_plan_table_stats(const sg_plan* plan, int64_t* tables, int64_t* samples, int64_t* terms);
/* sg_stft_ola work of the plan (fused seewave stft x envelope -> istft -> OLA,
 * R/soundgen.R:743-807, and generateNoise's istft, R/source.R:88-131): trimmed
 * output samples, algorithmic HBM bytes (source/uniforms + envelope columns +
 * output) and nominal flops (5 wl log2 wl per transform). */
int sg_plan_stft_stats(const sg_plan* plan, int64_t* samples, int64_t* alg_bytes, double* flops);
/* Sine-bank wave tasks of an uploaded plan by class (128-B descriptors, SgWTask):
 * counts[0] sg_sine_bank, [1] sg_sine_bank_pairs, [2] sg_sine_bank_tall,
 * [3] sg_sine_bank_tall_pairs, [4] sg_sine_bank_hp (zeros before upload). The
 * bench adds the descriptors to the kernels' algorithmic bytes. ABI 4. */
int sg_plan_sine_tasks(const sg_plan* plan, int64_t* counts);
/* Precision path of the plan (ABI 2): per call, the number of its bouts whose
 * formant filter runs in fp64 (source, pre-filter mix and forward STFT; the
 * planner's conditioning estimate of the fp32 round-off through the envelope
 * exceeded its threshold, env SG_HP_RHO, default 100; sg_set_fp64_policy: 0 never, 2 always);
 * totals of fp64 filter frames and sine-bank tasks. Any pointer may be NULL.
 * No reference counterpart: the R path is fp64 throughout. */
int sg_plan_precision(const sg_plan* plan, int32_t* call_fp64, int64_t* fp64_frames, int64_t* fp64_tasks);
/* Per call: the planner's conditioning estimate of the formant filter in fp32
 * (the largest over the call's filtered bouts; 0 when none was estimated):
 * bouts above the fp64 policy's threshold take the fp64 filter path. */
int sg_plan_conditioning(const sg_plan* plan, double* rho);
/* The same estimate for the pre-filter noise of each call's filtered bouts
 * (its fp32 inverse STFT's round-off against the formant envelope); above the
 * noise threshold those noise frames take the fp64 kernel. */
int sg_plan_noise_conditioning(const sg_plan* plan, double* rho);
/* Per-call device work the plan emits (ABI 2): sine-bank (sample, row) terms and
 * nominal FFT flops (5 wl log2 wl per transform), for load balancing across
 * GPUs (soundgen_beta_amd/dist.py). Either pointer may be NULL. */
int sg_plan_call_work(const sg_plan* plan, double* rows, double* fft_flops);
/* compareSounds() / getMelSpec() parameters (R/matchPars.R:313-325, :510-520
 * formals): windowLength and step in ms, overlap in %, throwaway in dB; step
 * NaN = windowLength * (1 - overlap / 100), maxFreq NaN = samplingRate / 2. */
typedef struct sg_mel_params {
  double samplingRate;
  double windowLength;
  double overlap;
  double step;
  double throwaway;
  double maxFreq;
  int32_t penalizeLengthDif;
  int32_t pad;
} sg_mel_params;
/* getMelSpec(s, ...) (R/matchPars.R:510-560: tuneR melfcc(spec_out = TRUE)
 * $aspectrum, frames with colMeans <= 2^(throwaway/10) dropped, log01) of one
 * host waveform, computed on the GPU in fp64: out (cap doubles) receives the
 * nb x nc matrix column-major; *nb and *nc are set (out may be NULL to size).
 * Windows of more than 4096 FFT points: SG_E_UNSUPPORTED. */
int sg_mel_spec(sg_ctx* ctx, const double* wave, int64_t len, const sg_mel_params* p, double* out, int64_t cap,
                int32_t* nb, int32_t* nc);
/* compareSounds(targetSpec = target, cand = candidate c, ...) for n candidates
 * in DEVICE memory (fp32, candidate c at d_wave + offsets[c], lengths[c]
 * samples; lengths[c] <= 0: skipped, NaN), against the host target spectrum
 * (nb x nc_target column-major, as sg_mel_spec returns it): out[4 c + m] for
 * m = cor, cosine, pixel, dtw (methods: bit m set = computed, else NaN; dtw is
 * the dtw package's symmetric2 normalizedDistance), summary[c] the mean of the
 * computed non-NA methods (compareSounds(summary = TRUE); may be NULL). One
 * launch sequence for the whole batch (R/matchPars.R:313-416, called per
 * candidate at :168, :202): the pairs (target, c) go through the kernels of
 * sg_compare_sounds_pairs with the target's columns read as they stand, are
 * reduced on the device, and five numbers per candidate come back. A target of
 * nc_target = 0 columns is a sound without a kept frame, not a skipped one:
 * 0 per method under penalizeLengthDif, NaN without it. */
int sg_compare_sounds_batch(sg_ctx* ctx, const double* target_spec, int32_t nb, int32_t nc_target,
                            const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n,
                            const sg_mel_params* p, int32_t methods, double* out, double* summary);
/* A set of mel spectra resident in DEVICE memory (an additive extension of ABI 5):
 * getMelSpec() of n sounds in device memory (fp32, or fp64 with is_f64 != 0; sound i at
 * d_wave + offsets[i], lengths[i] samples, the layout of sg_compare_sounds_batch;
 * lengths[i] <= 0: skipped), computed once under p and kept until sg_mel_set_destroy. The
 * waveform is not referenced after sg_mel_set_create returns. penalizeLengthDif of p is not
 * read here. */
typedef struct sg_mel_set sg_mel_set;
int sg_mel_set_create(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets,
                      const int64_t* lengths, int64_t n, const sg_mel_params* p, sg_mel_set** out);
/* The set's sounds, mel bands and (ncols: n values, may be NULL) kept columns per sound, 0 for
 * a skipped one. n and nb may be NULL. */
int sg_mel_set_info(const sg_mel_set* set, int64_t* n, int32_t* nb, int32_t* ncols);
/* getMelSpec of sound i of the set, as sg_mel_spec returns it: out (cap doubles; NULL to size)
 * receives the nb x *nc matrix column-major. For an fp64 set the values are sg_mel_spec's of
 * the same samples bit for bit. */
int sg_mel_set_spec(sg_mel_set* set, int64_t i, double* out, int64_t cap, int32_t* nc);
void sg_mel_set_destroy(sg_mel_set* set);
/* compareSounds(target = sound pairs[2 k] of `targets`, cand = sound pairs[2 k + 1] of
 * `cands`) for n_pairs pairs in one launch sequence: out[4 k + m] and summary[k] (may be NULL)
 * as sg_compare_sounds_batch defines them, reduced on the device; NaN where either sound was
 * skipped. The two sets may be one and the same; a pair's numbers do not depend on the other
 * pairs or on the other sounds of the sets, and equal sg_compare_sounds_batch's for the same
 * target spectrum and candidate samples bit for bit (one set of kernels serves both entries;
 * they differ in where the target's columns come from). SG_E_ARG, before any launch and with out
 * untouched: a NULL set, sets of different contexts or of different geometry (window, step and
 * FFT points, mel bands, maxFreq, throwaway), an index outside its set. More than 2^31 - 1
 * column jobs in one call: SG_E_UNSUPPORTED. n_pairs == 0 returns SG_OK and launches nothing. */
int sg_compare_sounds_pairs(sg_ctx* ctx, const sg_mel_set* targets, const sg_mel_set* cands, const int32_t* pairs,
                            int64_t n_pairs, int32_t methods, int32_t penalizeLengthDif, double* out,
                            double* summary);
/* compareSounds' 'dtw' method (R/matchPars.R:372-376): dtw::dtw(x, y,
 * distance.only = TRUE)$normalizedDistance with the dtw package defaults
 * (|x_i - y_j|, symmetric2, / (n + m)). Host only (ABI 2). */
int sg_dtw_symmetric2(const double* x, int64_t n, const double* y, int64_t m, double* out);
/* ssm() parameters (R/SSM.R:63-98 formals; an additive extension of ABI 5):
 * windowLength, step, ssmWin and kernelLen in ms, overlap in %. NaN = R's NULL
 * for step (windowLength * (1 - overlap / 100)), maxFreq (floor(samplingRate /
 * 2)) and nBands (100 * windowLength / 20). mfcc: the 1-based cepstral
 * coefficients of input 0 (R's MFCC; every index in 1..nBands, max >= 2).
 * input: 0 mfcc, 1 audiogram, 2 spectrum. norm: zeroOne per frame. simil: 0
 * cosine, 1 cor. normalize: 1 = the numeric-vector path (tuneR::normalize:
 * centre, / max|x|), 0 = the file path (samples used raw). */
typedef struct sg_ssm_params {
  double samplingRate;
  double windowLength;
  double overlap;
  double step;
  double ssmWin;
  double maxFreq;
  double nBands;
  double kernelLen;
  double kernelSD;
  const int32_t* mfcc;
  int32_t n_mfcc;
  int32_t input;
  int32_t norm;
  int32_t simil;
  int32_t normalize;
} sg_ssm_params;
/* ssm()'s integer decisions for a sound of len samples (host only, no device):
 * the melfcc frame count, the SSM's side n (selfsim's windows), selfsim's win
 * after its clamp to floor(n_frames / 2) and its odd-making rule, and
 * getNovelty's kernelSize (R/SSM.R:111-119, :228-244). len <= 1 (R's
 * length(x) > 1 test fails): n_frames = n = 0 and win is the unclamped value. */
int sg_ssm_size(int64_t len, const sg_ssm_params* p, int32_t* n_frames, int32_t* n, int32_t* win,
                int32_t* kernel_size);
/* ssm(wave, ...) of one host waveform on the GPU in fp64 (R/SSM.R:63-360:
 * melfcc, selfsim, getNovelty): ssm_out (n * n doubles, column-major; may be
 * NULL) and novelty_out (n doubles), n from sg_ssm_size. Limits: windows of at
 * most 4096 FFT points (SG_E_UNSUPPORTED); n * n <= 2^28 cells (n <= 16384),
 * for a batch the sum over its calls (SG_E_UNSUPPORTED); kernelSize >= 2 and
 * len >= 2 (SG_E_ARG). */
int sg_ssm(sg_ctx* ctx, const double* wave, int64_t len, const sg_ssm_params* p, double* ssm_out,
           double* novelty_out);
/* ssm() of n_calls sounds in DEVICE memory (fp32, call c at d_wave +
 * offsets[c], lengths[c] samples, the layout of sg_compare_sounds_batch), each
 * normalized on the device when p->normalize, in one launch sequence. n_out[c]
 * receives call c's n (0 for lengths[c] <= 1: skipped); its novelty goes to
 * novelty_out + novelty_off[c] (n doubles) and, if ssm_out is not NULL, its
 * matrix to ssm_out + ssm_off[c] (n * n doubles, column-major); both are host
 * memory. */
int sg_ssm_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                 const sg_ssm_params* p, int32_t* n_out, double* novelty_out, const int64_t* novelty_off,
                 double* ssm_out, const int64_t* ssm_off);
/* spectrogram() parameters (R/spectrogram.R:94-117 formals; an additive
 * extension of ABI 5): windowLength, step and zp as in R (ms, ms, points),
 * overlap and percentNoise in %. NaN = R's NULL for step (windowLength * (1 -
 * overlap / 100)). smoothFreq / smoothTime: the rolling medians' k (<= 1: off;
 * a whole odd number otherwise, SG_E_ARG if not). wn: 0 bartlett, 1 blackman, 2
 * flattop, 3 hamming, 4 hanning, 5 rectangle, 6 gaussian. method: 0 spectrum, 1
 * spectralDerivative. output: 0 original (|X|), 1 processed. */
typedef struct sg_spectrogram_params {
  double samplingRate;
  double windowLength;
  double step;
  double overlap;
  double zp;
  double smoothFreq;
  double smoothTime;
  double qTime;
  double percentNoise;
  double noiseReduction;
  double contrast;
  double brightness;
  int32_t wn;
  int32_t method;
  int32_t output;
  int32_t pad;
} sg_spectrogram_params;
/* spectrogram()'s integer decisions for a sound of len samples (host only, no
 * device): the window in points wl = floor(windowLength / 1000 * samplingRate /
 * 2) * 2, the FFT length n_fft = wl + max(floor((zp - wl) / 2) * 2, 0), bins =
 * n_fft / 2 and the frame count of getFrameBank's seq() (R/spectrogram.R:350;
 * 0 for len <= 1 or len < wl). Limits of the device transform: wl >= 4, bins <=
 * 2048 and bins a product of 2 and the odd primes <= 31; otherwise
 * SG_E_UNSUPPORTED, and sg_spectrogram_size_error() names zp as the way to a
 * supported length. */
int sg_spectrogram_size(int64_t len, const sg_spectrogram_params* p, int32_t* wl, int32_t* n_fft, int32_t* bins,
                        int32_t* frames);
/* The message of the calling thread's last failed sg_spectrogram_size ("" if none). */
const char* sg_spectrogram_size_error(void);
/* spectrogram(wave, ...) of one host waveform on the GPU in fp64: out receives
 * bins * frames doubles, frame after frame (R's column-major image of the bins x
 * frames matrix it returns). Limits: those of sg_spectrogram_size; len >= wl
 * (SG_E_ARG: R would index past the end); smoothTime <= bins and smoothFreq <=
 * frames (SG_E_ARG, zoo::rollmedian stops); fewer than 2^31 frames in one launch
 * sequence (SG_E_UNSUPPORTED). The rolling medians are exact for every odd k
 * but cost O(k^2) per cell: they are meant for small k. */
int sg_spectrogram(sg_ctx* ctx, const double* wave, int64_t len, const sg_spectrogram_params* p, double* out);
/* spectrogram() of n_calls sounds in DEVICE memory (fp32, call c at d_wave +
 * offsets[c], lengths[c] samples, the layout of sg_compare_sounds_batch) in one
 * launch sequence. Call c's matrix goes to d_out + out_off[c] in DEVICE memory
 * (bins * frames doubles as sg_spectrogram lays them out; the caller sizes d_out
 * with sg_spectrogram_size); bins_out[c] / frames_out[c] receive its shape. A
 * call with lengths[c] <= 1 or shorter than the window has 0 frames and writes
 * nothing. The call returns when the stream has finished. */
int sg_spectrogram_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                         int64_t n_calls, const sg_spectrogram_params* p, double* d_out, const int64_t* out_off,
                         int32_t* bins_out, int32_t* frames_out);
/* analyze()'s per-frame stage (R/analyze.R:233-575, R/utilities_analyze.R:22-324;
 * an additive extension of ABI 5). The formals after analyze()'s argument repairs
 * (:240-341; the caller makes them): silence, entropyThres, domThres and
 * autocorThres in [0, 1]; windowLength and step in ms, step NaN = R's NULL
 * (windowLength * (1 - overlap / 100)); zp in points; cutFreq, pitchFloor,
 * pitchCeiling and domSmooth in Hz; nCands a whole number in [1, 8]
 * (SG_E_UNSUPPORTED above 8); autocorSmooth NaN = R's NULL (2 * ceiling(7 *
 * samplingRate / 44100 / 2) - 1). wn as in sg_spectrogram_params. methods: bit 0
 * 'autocor', bit 1 'dom' (at least one; 'cep' and 'spec' are not built). */
typedef struct sg_analyze_params {
  double samplingRate;
  double silence;
  double windowLength;
  double step;
  double overlap;
  double zp;
  double cutFreq;
  double entropyThres;
  double pitchFloor;
  double pitchCeiling;
  double nCands;
  double domThres;
  double domSmooth;
  double autocorThres;
  double autocorSmooth;
  int32_t wn;
  int32_t methods;
} sg_analyze_params;
/* The stage's integer decisions for a sound of len samples (host only, no device):
 * the window in points, its wl / 2 bins, the frame count (0 for len <= wl), the
 * columns of a frame's row (15 + 2 nCands: ampl, entropy, HNR, dom, peakFreq,
 * peakFreqCut, meanFreq, quartile25, quartile50, quartile75, specSlope, domCand,
 * domCert, cond_silence, cond_entropy, autocorCand[nCands], autocorCert[nCands];
 * NaN = R's NA, the two gates 0 / 1), and the first and last lag of the
 * autocorrelation that getPitchAutocor reads (row j, lag j - 1, is labelled
 * samplingRate / j; the rows with pitchFloor < label < pitchCeiling). extra (8
 * int32 or NULL) receives rowLow, rowHigh (1-based, :466-467), the first bin
 * (0-based) and the size of the cut band, pitchFloor_idx (1-based), domSmooth_bins,
 * autocorSmooth and 0. All labels are decided after R's 15-significant-digit
 * character round trip. SG_E_ARG where the reference stops (zp padding the frame, no
 * label above 6 kHz, an empty lag range, a cut band under 2 bins) and for an even
 * or too-wide autocorSmooth; SG_E_UNSUPPORTED for the limits of sg_spectrogram_size
 * and nCands > 8. */
int sg_analyze_frames_size(int64_t len, const sg_analyze_params* p, int32_t* wl, int32_t* bins, int32_t* frames,
                           int32_t* cols, int32_t* lag_first, int32_t* lag_last, int32_t* extra);
/* The message of the calling thread's last failed sg_analyze_frames_size /
 * sg_analyze_frames_ampl_starts ("" if none). */
const char* sg_analyze_frames_size_error(void);
/* Host only: the 0-based first sample of the wl + 1 samples whose RMS is frame
 * f's ampl, floor(seq(1, len - wl, length.out = frames)[f]) - 1 (:456-459), for
 * f < n (n = the frame count of sg_analyze_frames_size). */
int sg_analyze_frames_ampl_starts(int64_t len, const sg_analyze_params* p, int64_t* starts, int32_t n);
/* The stage for one host waveform on the GPU in fp64: out receives frames * cols
 * doubles, row after row. SG_E_ARG for len <= wl (the reference's amplitude window
 * leaves the sound); fewer than 2^31 frames in one launch sequence. */
int sg_analyze_frames(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params* p, double* out);
/* The stage for n_calls sounds in DEVICE memory (fp32, call c at d_wave +
 * offsets[c], lengths[c] samples) in one launch sequence. Call c's table goes to
 * d_out + out_off[c] in DEVICE memory (frames * cols doubles; the caller sizes
 * d_out with sg_analyze_frames_size); frames_out[c] receives its rows. A call
 * with lengths[c] <= wl has 0 frames and writes nothing. Returns when the stream
 * has finished. */
int sg_analyze_frames_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                            int64_t n_calls, const sg_analyze_params* p, double* d_out, const int64_t* out_off,
                            int32_t* frames_out);
/* pitch_candidates: analyze()'s per-frame stage with all four pitch trackers (an
 * additive extension of ABI 5): sg_analyze_frames plus the cepstral tracker
 * (getPitchCep, R/utilities_analyze.R:337-407) and the spectral one (getPitchSpec,
 * :424-558, a modified BaNa). a: as for sg_analyze_frames, except a.methods: bit 0
 * 'autocor', bit 1 'dom', bit 2 'cep', bit 3 'spec' (at least one). The formals
 * after analyze()'s repairs (:343-363; the caller makes them): cepThres, specThres,
 * specPeak and specSinglePeakCert in [0, 1]; specMerge (semitones) >= 0; specSmooth
 * in Hz; cepZp in points; cepSmooth NaN = R's NULL (2 * ceiling(31 * samplingRate /
 * 44100 / 2) - 1). specHNRslope is accepted and unused: analyze() passes HNR = NULL
 * (:134), so the peak threshold is specPeak. */
typedef struct sg_pitch_params {
  sg_analyze_params a;
  double cepThres;
  double cepSmooth;
  double cepZp;
  double specThres;
  double specPeak;
  double specSinglePeakCert;
  double specHNRslope;
  double specSmooth;
  double specMerge;
} sg_pitch_params;
/* The integer decisions for a sound of len samples (host only, no device): the
 * frame count (0 for len <= wl), the columns of a row (15 + 6 nCands: the 15 of
 * sg_analyze_frames_size, then autocorCand, autocorCert, cepCand, cepCert, specCand,
 * specCert, nCands each) and, in extra (24 int32 or NULL): wl, bins, lag_first,
 * lag_last, rowLow, rowHigh, the cut band's first bin and size, pitchFloor_idx,
 * domSmooth_bins, autocorSmooth (as sg_analyze_frames_size gives them), then L =
 * length(frameZP) (bins + 2 floor((cepZp - bins) / 2) for cepZp >= bins, else bins),
 * the effective cepSmooth (* round(cepZp / bins) when padded), l = L %/% 2, the first
 * row (0-based) and the number of rows of the cepstrum with pitchFloor < samplingRate
 * / k / 2 * (L / bins) < pitchCeiling, getPitchSpec's width 2 * ceiling((specSmooth /
 * bin + 1) * 20 / bin / 2) - 1, and zeros. The refusals of sg_analyze_frames_size
 * hold whatever a.methods is. Where 'cep' is asked for: SG_E_ARG for an even
 * effective cepSmooth (zoo's even-width alignment is not restated) and for an empty
 * cepstral band (the reference's rollapply gets an empty series); SG_E_UNSUPPORTED
 * when L cannot be transformed: L even needs L / 2, L odd needs L itself, 31-smooth
 * and <= 2048. Where 'spec' is asked for: SG_E_ARG for a width below 1. A smoothing
 * window wider than its band is not refused: it finds no peak, as in zoo. Errors
 * through sg_analyze_frames_size_error. */
int sg_pitch_candidates_size(int64_t len, const sg_pitch_params* p, int32_t* frames, int32_t* cols, int32_t* extra);
/* Host only: the labels (Hz) of the n = extra[15] rows of the cepstral band. */
int sg_pitch_candidates_cep_labels(const sg_pitch_params* p, double* labels, int32_t n);
/* sg_analyze_frames / sg_analyze_frames_batch with rows of 15 + 6 nCands columns.
 * With a.methods within bits 0..1 the shared columns equal sg_analyze_frames' bit
 * for bit; the columns of a method not asked for are NaN. */
int sg_pitch_candidates(sg_ctx* ctx, const double* wave, int64_t len, const sg_pitch_params* p, double* out);
int sg_pitch_candidates_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                              int64_t n_calls, const sg_pitch_params* p, double* d_out, const int64_t* out_off,
                              int32_t* frames_out);
/* analyze(): sg_pitch_candidates plus the tail behind the candidates (an additive
 * extension of ABI 5; R/analyze.R:576-707, R/utilities_pitch_postprocessing.R): the
 * prior, findVoicedSegments, pathfinder per voiced segment (interpolate, pathfinding
 * 'none' / 'fast' / 'exact', snake), medianSmoother and the final columns. p: as for
 * sg_pitch_candidates. priorMean / priorSD (semitones): the prior applies when both are
 * numbers (NaN = not numeric: no prior; SG_E_ARG unless positive). minVoicedCands: NaN
 * = 'autom' (also taken when < 1 or above the number of methods). shortestSyl,
 * shortestPause in ms (shortestPause >= 0). interpolWin: a whole number of frames (<= 0:
 * no interpolation). certWeight in [0, 1]. snakeStep <= 0 or NaN: no snake. smooth <= 0
 * or NaN: no smoothing. pathfinding: 0 'none', 1 'fast', 2 'slow' (SG_E_UNSUPPORTED:
 * simulated annealing on R's random stream is not built), 3 'exact' (not in the
 * reference: the path that minimises the reference's own costPerPath(), the cost 'slow'
 * anneals, found by dynamic programming over a segment's frames; deterministic, no random
 * stream; the tail's workspace grows by 2 + 3 nCands doubles per frame); any other value
 * is SG_E_ARG. smoothVars: bit 0 'pitch', bit
 * 1 'dom'. SG_E_UNSUPPORTED also for interpolWin or half the smoothing window above 64
 * frames and for 0 < snakeStep < 0.005. */
typedef struct sg_analyze_params_full {
  sg_pitch_params p;
  double priorMean;
  double priorSD;
  double minVoicedCands;
  double shortestSyl;
  double shortestPause;
  double interpolWin;
  double interpolTol;
  double interpolCert;
  double certWeight;
  double snakeStep;
  double smooth;
  int32_t pathfinding;
  int32_t smoothVars;
} sg_analyze_params_full;
/* The integer decisions for a sound of len samples (host only, no device): the frame
 * count, the columns of a row (15 + 6 nCands + 4: those of sg_pitch_candidates_size,
 * then pitch, amplVoiced, voiced (0 / 1), harmonics) and, in extra (8 int32 or NULL):
 * minVoicedCands resolved, noRequired = max(1, ceiling(shortestSyl / step)),
 * nToleratedNA = floor(shortestPause / step), hw = floor(round(smooth * frames /
 * duration / 10) / 2) (R's round: half to even), interpolWin, and zeros. The refusals of
 * sg_pitch_candidates_size hold. Errors through sg_analyze_frames_size_error. */
int sg_analyze_size(int64_t len, const sg_analyze_params_full* p, int32_t* frames, int32_t* cols, int32_t* extra);
/* sg_pitch_candidates / sg_pitch_candidates_batch with rows of 15 + 6 nCands + 4 columns:
 * the columns analyze() does not rewrite equal sg_pitch_candidates' bit for bit; HNR and
 * harmonics are in dB, dom is smoothed (if asked for), the quartiles are NaN for unvoiced
 * frames. A sound's table is the same bit for bit alone and in any batch. */
int sg_analyze(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params_full* p, double* out);
int sg_analyze_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_analyze_params_full* p, double* d_out, const int64_t* out_off, int32_t* frames_out);
/* The tail alone, from a HOST table of `frames` rows of 15 + 6 nCands columns (a
 * sg_pitch_candidates table, or the caller's own candidates) of a sound of len samples
 * (len decides the smoothing window): out receives frames rows of 15 + 6 nCands + 4
 * columns; harmonics, which needs the spectrum, is NaN. Of p->p only a.samplingRate,
 * a.step, a.windowLength, a.overlap, a.nCands, a.pitchFloor, a.pitchCeiling and a.methods
 * are read. */
int sg_pitch_path(sg_ctx* ctx, const double* table, int32_t frames, int64_t len, const sg_analyze_params_full* p,
                  double* out);
/* sg_pitch_path plus the list of the sound's voiced segments (an additive extension of ABI
 * 5): *n_segments of them (at most `frames`), 4 doubles each in `segments` (room for 4 *
 * frames doubles): the first and the last frame (1-based), nrow (the largest number of
 * candidates in a frame, after interpolation: the rows left when the all-NA rows are
 * dropped) and the value costPerPath() (R/utilities_pitch_postprocessing.R:347-372)
 * gives for the path handed to the snake: certWeight * mean(|path - centre of gravity|) +
 * (1 - certWeight) * mean(costJumps(path[f], path[f + 1])), both means with na.rm = TRUE;
 * NaN where a mean has no term (a one-frame segment, or no two neighbouring frames with a
 * path value). Any pathfinding sg_pitch_path takes; for a one-row segment the cost of its
 * only path. `out` is what sg_pitch_path gives, bit for bit. */
int sg_pitch_path_costs(sg_ctx* ctx, const double* table, int32_t frames, int64_t len, const sg_analyze_params_full* p,
                        double* out, double* segments, int32_t* n_segments);
/* analyze(summary = TRUE) (an additive extension of ABI 5; R/analyze.R:770-796): one row
 * of SG_ANALYZE_SUMMARY_COLS doubles per sound from its finished table: duration (s: the
 * sound's len / samplingRate), voiced (the proportion of voiced frames), then <var>_mean,
 * <var>_median, <var>_sd over the frames where the variable is not NaN, for ampl,
 * amplVoiced, dom, entropy, harmonics, HNR, meanFreq, peakFreq, peakFreqCut, pitch,
 * quartile25, quartile50, quartile75, specSlope (the reference's sort() of the column
 * names under a case-insensitive collation; the C locale would put HNR first: the names
 * identify the cells). R's arithmetic in fp64: the mean is sum / n refined once by the
 * mean of the residuals, the sd is the two-pass variance about the refined mean over n -
 * 1 (NaN for n < 2), the median is exact (a zero comes out as +0.0); NaN for no value;
 * +-Inf are ordinary values. A sound without frames (not longer than the window, or len <
 * 0) gets SG_ANALYZE_SUMMARY_COLS NaN. A sound's row is the same bit for bit alone, in any
 * batch and at any position of it. */
#define SG_ANALYZE_SUMMARY_COLS 44
/* Host only: the name of cell i of a row ("duration", "voiced", "ampl_mean", ...); NULL
 * outside 0 .. SG_ANALYZE_SUMMARY_COLS - 1. Valid until the thread's next call. */
const char* sg_analyze_summary_name(int32_t i);
/* The summary stage alone, from a HOST table of `frames` rows of cols = 15 + 6 nCands + 4
 * doubles (an sg_analyze table, or the caller's own) of a sound of len samples; out
 * receives SG_ANALYZE_SUMMARY_COLS doubles of host memory. */
int sg_analyze_summary(sg_ctx* ctx, const double* table, int32_t frames, int32_t cols, int32_t nCands, int64_t len,
                       double samplingRate, double* out);
/* sg_analyze_batch followed by the summary kernel in the same launch sequence: d_tables,
 * out_off and frames_out exactly as sg_analyze_batch's d_out, out_off and frames_out (the
 * tables are the same bit for bit and stay valid); d_summary (device memory) receives
 * n_calls x SG_ANALYZE_SUMMARY_COLS doubles, row c for call c. */
int sg_analyze_summary_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                             int64_t n_calls, const sg_analyze_params_full* p, double* d_tables, const int64_t* out_off,
                             int32_t* frames_out, double* d_summary);
/* sg_analyze for one sound from host memory with its summary row: out (host, the table of
 * sg_analyze, or NULL when only the row is wanted) and summary (host,
 * SG_ANALYZE_SUMMARY_COLS doubles). Refuses what sg_analyze refuses. */
int sg_analyze_summary_sound(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params_full* p, double* out,
                             double* summary);
/* analyze()'s formant tracks (R/analyze.R:486-502; an additive extension of ABI 5): for every
 * frame that passed cond_silence, phonTools::findformants(frame, samplingRate, verify = FALSE)
 * with its defaults, restated from phonTools 0.2-2.1 as documented (phonTools is not in the
 * reference tree: PARITY UNPINNED, like sg_dtw_symmetric2). Linear prediction of order
 * round(samplingRate / 1000) + 3 (pre-emphasis at 50 Hz, minus the mean, a Hann window,
 * autocorrelation, Levinson-Durbin where phonTools solves by LU), all roots of the predictor by
 * the Aberth-Ehrlich iteration in fp64, formant = round(atan2(Im z, Re z) samplingRate / (2 pi),
 * 2), bandwidth = -(samplingRate / pi) log|z|, ordered by formant, kept where bandwidth < 600 &
 * formant > 200 & formant < samplingRate / 2. A row holds f1_freq, f1_width, f2_freq, ...:
 * 2 nFormants doubles, NaN = NA (a frame not analysed, fewer kept roots, a frame whose
 * autocorrelation Levinson-Durbin refuses or whose iteration does not settle in 64 steps).
 * round(x, 2) is nearbyint(100 x) / 100 in fp64 (R multiplies in long double). A frame's row is
 * the same bit for bit alone, in any batch and at any position of it.
 * Host only: the order and cols = 2 nFormants. SG_E_ARG unless 1 <= nFormants <= 8;
 * SG_E_UNSUPPORTED for an order above 64 (samplingRate >= 61.5 kHz): one root per lane of a
 * wave. SG_E_ARG too where p's window is not longer than the order (windowLength = 1 ms at
 * 44.1 kHz: 44 samples for order 47; the reference's solve() fails on every such frame), and
 * what sg_analyze_frames_size refuses. Errors through sg_analyze_frames_size_error. */
int sg_formants_size(const sg_analyze_params* p, int32_t nFormants, int32_t* order, int32_t* cols);
/* The formant tables of n_calls sounds in DEVICE memory (as for sg_analyze_frames_batch) behind
 * their finished tables from sg_analyze_frames_batch, sg_pitch_candidates_batch or
 * sg_analyze_batch (d_tables, out_off, frames as those calls left them; table_cols their
 * columns; of p only what the three share is read, and p->methods may name any of the four
 * methods): call c's frames[c] x 2 nFormants table goes to d_fmt + fmt_off[c] in DEVICE memory.
 * A call without frames (frames[c] == 0: not longer than the window, or failed) writes nothing.
 * Returns when the stream has finished. */
int sg_formants_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                      const sg_analyze_params* p, int32_t nFormants, const double* d_tables, const int64_t* out_off,
                      int32_t table_cols, const int32_t* frames, double* d_fmt, const int64_t* fmt_off);
/* One sound from host memory: sg_analyze_frames for the gate, then the formants; out (host)
 * receives frames x 2 nFormants doubles. Refuses what sg_analyze_frames refuses. */
int sg_formants_sound(sg_ctx* ctx, const double* wave, int64_t len, const sg_analyze_params* p, int32_t nFormants, double* out);
/* The two kernels alone on nframes caller-given frames of n samples each (host, row after row;
 * order < n <= 4096): no gate, no normalisation, no analysis window; fs is findformants' fs.
 * out (host) receives nframes x 2 nFormants doubles. */
int sg_formants_frames(sg_ctx* ctx, const double* frames, int32_t n, int32_t nframes, double fs, int32_t nFormants,
                       double* out);
/* phonTools::findformants(sound, fs, verify = FALSE) on a whole sound of any length (matchPars'
 * initial formants, R/matchPars.R:130; an additive extension of ABI 5): the steps above with
 * the Hann window over all len samples, no gate, no normalisation, no analysis window. The
 * sound is cut into chunks of `chunk` samples; the mean and every lag are sums of per-chunk
 * sums folded in chunk order, so that a sound's row is the same bit for bit alone, in any
 * batch and at any position of it. A row is 2 * 8 doubles: (formant, bandwidth) pairs in
 * ascending order of formant, NaN behind the kept ones; more than 8 kept roots are not
 * returned.
 * Host only, no GPU call: the order round(fs / 1000) + 3, the chunk size and the chunks of a
 * sound of len samples (0 for len <= 0). SG_E_UNSUPPORTED for an order above 64 and for a len
 * whose chunk count does not fit an int32. */
int sg_formants_whole_size(double fs, int64_t len, int32_t* order, int32_t* chunk, int64_t* nchunks);
/* One sound from host memory; out (host) receives the 16 doubles. SG_E_ARG for len <= order. */
int sg_formants_whole(sg_ctx* ctx, const double* wave, int64_t len, double fs, double* out);
/* n_calls sounds in DEVICE memory (as for sg_analyze_frames_batch): call c's row goes to
 * d_out + 16 c in DEVICE memory. A call with lengths[c] <= order (a failed call's length < 0
 * too) gets a NaN row. Returns when the stream has finished. */
int sg_formants_whole_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths,
                            int64_t n_calls, double fs, double* d_out);
/* segment() (an additive extension of ABI 5; R/segment.R:79-219, R/utilities_segment.R):
 * the smoothed Hilbert envelope of the whole sound (seewave::env(envt = "hil", msmooth =
 * c(windowLength_points, overlap)): a transform of 2^ceiling(log2(len)) points), the
 * syllables, the bursts and the summary row, fp64. shortestPause NaN = NULL / NA (no
 * merging); interburst NaN = NULL (median(sylLen) * interburstMult, or shortestSyl without
 * a syllable), otherwise >= 0 (SG_E_ARG). overlap is clamped to 0..99 as the reference
 * does. mode 0: segment(); mode 1: Mod(seewave::hilbert(wave)) alone, un-padded by the
 * reference's rule and not normalized (only len is read of the other fields' effects).
 * workspace_cap: bytes of transform workspace one chunk of a batch may take (0: the
 * default, sg_segment.h; a larger sound runs alone); results do not depend on it.
 * SG_E_ARG where the reference stops (len < 2, a smoothing window of 0 or 1 points: len
 * == 2 among them); SG_E_UNSUPPORTED for more than 2^22 transform points. */
typedef struct sg_segment_params {
  double samplingRate;
  double windowLength;
  double overlap;
  double shortestSyl;
  double shortestPause;
  double sylThres;
  double interburst;
  double interburstMult;
  double burstThres;
  double peakToTrough;
  int32_t troughLeft;
  int32_t troughRight;
  int32_t mode;
  int32_t reserved;
  int64_t workspace_cap;
} sg_segment_params;
/* The integer decisions for a sound of len samples (host only, no device): log2 of the
 * transform length, the envelope's values (mode 0: the smoothed envelope's, mode 1: the
 * un-padded transform's: len, or len - 1 for len = 2^p - 1), the points of a smoothing
 * window (mode 0) and the doubles of the sound's output. Mode 0's cells (m = *n_env):
 * [0] m [1] rows of the syllable table [2] 1 if a syllable was found (0: one row,
 * syllable = 0, NaN elsewhere) [3] bursts [4] timestep, ms [5] threshold [6] interburst,
 * ms [7] floor(interburst / timestep); [8 .. 18] nSyl, sylLen_mean, sylLen_median,
 * sylLen_sd, pauseLen_mean, pauseLen_median, pauseLen_sd, nBursts, interburst_mean,
 * interburst_median, interburst_sd (NaN for NA); from 19 the envelope (m); from 19 + m the
 * syllable table, rows x (syllable, start, end, sylLen, pauseLen), room for (m + 1) / 2
 * rows; behind it the burst table, bursts x (time, ampl, interburstInt), room for m rows;
 * then m cells of scratch. Mode 1's cells: the envelope. Errors through
 * sg_segment_size_error. */
int sg_segment_size(int64_t len, const sg_segment_params* p, int32_t* log2n, int32_t* n_env, int32_t* points,
                    int64_t* cells);
const char* sg_segment_size_error(void);
/* Host only, mode 0: the n = *n_env smoothing windows of the sound and the envelope's time
 * step in ms. Point j of a window is the envelope's value first + j (0-based), and first +
 * j + 1 from j = jump on: R's from:to adds in fp64 from a fractional from, and a from a
 * rounding error below a whole number makes the truncated indices skip one value where
 * the sum rounds up (jump = points: nothing skipped). */
int sg_segment_windows(int64_t len, const sg_segment_params* p, int64_t* first, int64_t* points, int64_t* jump,
                       int32_t n, double* timestep);
/* One sound from host memory; out: *cells doubles of host memory. */
int sg_segment(sg_ctx* ctx, const double* wave, int64_t len, const sg_segment_params* p, double* out);
/* n_calls sounds already in device memory (d_wave + offsets[c], lengths[c] samples) into
 * d_out + out_off[c] (device memory; out_off has n_calls + 1 entries, and out_off[c + 1] -
 * out_off[c] must hold the sound's cells: SG_E_CAPACITY). Mode 0 only. A sound of fewer
 * than three samples (the reference stops) takes 19 cells: zeros, and a NaN summary with
 * nSyl = nBursts = 0. A sound's cells are the same bit for bit alone (from the same fp32
 * samples), in any batch and under any workspace_cap. Nothing is launched when a sound is
 * refused. */
int sg_segment_batch(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_segment_params* p, double* d_out, const int64_t* out_off);
/* A parameter sweep of segment(summary = TRUE) (an additive extension of ABI 5; what
 * optimizePars() evaluates, R/optimize.R:206-234): n_rows parameter rows over n_calls sounds
 * laid out as for sg_segment_batch. d_out (device memory): n_rows x n_calls x 11 doubles, the
 * summary row (cells 8 .. 18 of sg_segment_size's layout, NaN for NA) of sound c under
 * rows[r] at (r * n_calls + c) * 11; a sound of fewer than three samples has nSyl = nBursts
 * = 0 and NaN elsewhere. samplingRate, mode (0) and workspace_cap are those of rows[0]; a
 * row that differs in one of them is SG_E_ARG. The raw envelope is computed once per sound,
 * the smoothed one once per sound and (windowLength, clamped overlap), and all pairs of a
 * chunk of rows run in one launch; workspace_cap also bounds the bytes of the tables one such
 * chunk keeps (at least one row runs). A pair's eleven cells are sg_segment_batch's bit for
 * bit, whatever rows and sounds share the sweep and whatever the cap. A row refused for any
 * sound refuses the sweep before anything is launched; the text names the row and the sound. */
int sg_segment_sweep(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_segment_params* rows, int64_t n_rows, double* d_out);
/* 1 - cor(x, key, use = 'pairwise.complete.obs') per row of a device matrix of n_rows x
 * n_calls x width doubles (width 11: sg_segment_sweep's; 44: sg_analyze_summary_batch's, one
 * row), x = column `column` of the row's n_calls sounds; key: n_calls doubles of host
 * memory; NaN = NA on either side (the pair is dropped). fit: n_rows doubles of host memory;
 * NaN for fewer than two complete pairs or a side whose values are all equal (R: NA). A
 * row's value does not depend on the other rows. */
int sg_sweep_fitness(sg_ctx* ctx, const double* d_matrix, int64_t n_rows, int64_t n_calls, int32_t width, int32_t column,
                     const double* key, double* fit);
/* Process-wide: whether sg_segment_sweep's tail copies a pair's envelope to LDS first (1,
 * the default; an envelope of more than 8192 values is read in place either way) or reads
 * it in place (0). The results are the same bit for bit; for measurements. */
int sg_set_sweep_staging(int32_t mode);
/* A parameter sweep of analyze(summary = TRUE) (an additive extension of ABI 5; what
 * optimizePars() evaluates for analyzeFolder, R/optimize.R:95-108, :206-234): n_rows parameter
 * rows over n_calls sounds laid out as for sg_analyze_batch. d_out (device memory): n_rows x
 * n_calls x SG_ANALYZE_SUMMARY_COLS doubles, the row of sound c under rows[r] at (r * n_calls
 * + c) * 44; a sound without frames under a row has 44 NaN. Each stage runs once per distinct
 * set of the resolved decisions it reads, never of the raw arguments (step = NaN with overlap
 * = 50 and windowLength = 50 is step = 25; autocorSmooth = NaN is its default):
 *   frame group      equal window, step in points, window type and bins: the spectrogram, the
 *                    amplitudes and min(ampl) once; frame groups run one after another
 *   store group      within a frame group, for rows with 'autocor': also equal gates (silence,
 *                    entropyThres, the entropy band) and lag band. Where two candidate groups or
 *                    more share one and its nlag doubles per frame fit workspace_cap, the first
 *                    keeps the gated frames' corrected autocorrelations and the others only pick
 *                    their peaks (autocorThres, autocorSmooth, nCands) from them
 *   candidate group  within a frame group: every decision of the per-frame kernels equal; one
 *                    table of 15 + 6 nCands columns per sound, which the tail never rewrites
 * The tail (path, harmonics, summary) runs for all (row, sound) pairs of a chunk of rows in one
 * launch each; workspace_cap (bytes; 0: 1 GiB) bounds a store and the pair tables of a chunk
 * (at least one row runs). A pair's 44 cells are sg_analyze_summary_batch's bit for bit,
 * whatever rows and sounds share the sweep, in whatever order, under any cap, with the store on
 * or off. Every row must have rows[0]'s samplingRate. A row that sg_analyze_size refuses (for
 * any sound: the smoothing window) refuses the sweep before anything is launched; the text
 * names the row ("row r: ", "row r, sound c: "). */
int sg_analyze_sweep(sg_ctx* ctx, const float* d_wave, const int64_t* offsets, const int64_t* lengths, int64_t n_calls,
                     const sg_analyze_params_full* rows, int64_t n_rows, int64_t workspace_cap, double* d_out);
/* Host only, no device: the three group numbers of every row (n_rows int32 each), numbered by
 * first appearance; store_group is -1 for a row without 'autocor'. Store and candidate groups
 * are numbered over the whole sweep; each lies within one frame group. Refuses what
 * sg_analyze_sweep refuses from the rows alone; errors through sg_analyze_frames_size_error. */
int sg_analyze_sweep_plan(const sg_analyze_params_full* rows, int64_t n_rows, int32_t* frame_group, int32_t* store_group,
                          int32_t* cand_group);
/* Host only: bytes[0] = the device memory the largest frame group keeps while it runs (its |X|
 * frames and candidate tables), bytes[1] = the largest store the sweep would build (one that
 * two candidate groups or more share; 0 if there is none), bytes[2] = the largest tail
 * workspace of one row (its pair tables and scratch over all sounds). Also refuses a smoothing
 * window above 64 frames for any (row, sound). */
int sg_analyze_sweep_size(const int64_t* lengths, int64_t n_calls, const sg_analyze_params_full* rows, int64_t n_rows,
                          int64_t* bytes);
/* Process-wide, for measurements and tests; the results are the same bit for bit under either
 * mode. 1 (the default): the autocorrelation store; 0: every candidate group computes its own
 * autocorrelations, as it does where a store does not fit workspace_cap. SG_E_ARG for any other
 * mode, which leaves the mode in force. */
int sg_set_analyze_sweep_store(int32_t mode);
/* Process-wide policy of the fp64 filter path for later sg_plan_batch calls:
 * mode 0 never, 1 when the conditioning estimate exceeds rho (default 100),
 * 2 every filtered bout. SG_E_ARG for an invalid mode or rho. */
int sg_set_fp64_policy(int32_t mode, double rho);
/* Process-wide source of the harmonic amplitude matrices for later
 * sg_plan_batch calls: 0 (default) built on the device at upload from
 * per-glottal-cycle parameters, 1 built on the host and uploaded (the
 * reference-order host restatement; tests compare the two). */
int sg_set_amp_policy(int32_t host_built);
/* Process-wide handling of generateNoise()'s uniforms read from injected draw
 * arrays, for later sg_plan_batch calls: 1 (default) the planner records each
 * noise item's range of the caller's array, copies the union of the ranges
 * once and the device expands the items at upload; 0 each item's draws are
 * copied into the plan (the same values either way; tests compare the two).
 * The arrays are read during sg_plan_batch only. */
int sg_set_uniform_gather(int32_t on);
/* Process-wide switch of the sine bank's wavetable path, for plans uploaded
 * later (sg_plan_upload, or the first sg_execute of a plan): 1 (default)
 * long runs of constant-amplitude, linear-phase tasks (static tones) sample a
 * per-span table of the harmonic sum by cubic Hermite interpolation
 * (sg_sine_bank_tab); 0 every task runs the row recurrence. */
int sg_set_sine_table(int32_t on);
/* Release the planner's process-wide cache of freed host blocks (kept for the
 * next plan, capped by SG_HOST_CACHE_MB or 8 GB / LOCAL_WORLD_SIZE). Returns
 * the bytes released. Safe at any time; later plans refill it. */
int64_t sg_host_cache_trim(void);
/* The amplitude blocks sg_amp_build writes at upload, evaluated on the host by
 * the same code (tests; no device needed): n = sg_plan_amp_count(plan) floats. */
int64_t sg_plan_amp_count(const sg_plan* plan);
int sg_plan_debug_amps(const sg_plan* plan, float* out, int64_t n);

/* ---- function-level entries mirroring the R API (synchronous) ---------- */
int sg_generate_harmonics(sg_ctx* ctx, const double* pitch, int64_t len,
                          const sg_harm_params* p, sg_anchors amplAnchors,
                          const sg_random* rnd, double* out, int64_t cap,
                          int64_t* out_len);
int sg_soundgen(sg_ctx* ctx, const sg_soundgen_args* a, const sg_random* rnd,
                double* out, int64_t cap, int64_t* out_len);
/* generateNoise(len, noiseAnchors, rolloffNoise, attackLen,
 * windowLength_points, samplingRate, overlap, throwaway, filterNoise);
 * filterNoise is nr x filter_nc column-major (NULL/0 = NA). */
int sg_generate_noise(sg_ctx* ctx, int64_t len, sg_anchors noiseAnchors,
                      double rolloffNoise, double attackLen,
                      int32_t windowLength_points, double samplingRate,
                      double overlap, double throwaway,
                      const double* filterNoise, int32_t filter_nc,
                      const sg_random* rnd, double* out);
/* getSpectralEnvelope(nr, nc, formants, formantDep, rolloffLip,
 * mouthAnchors, mouthOpenThres, openMouthBoost, vocalTract, temperature,
 * formDrift, formDisp, formantDepStoch, smoothLinearFactor, samplingRate,
 * speedSound) -> out[nr*nc] column-major. */
int sg_spectral_envelope(sg_ctx* ctx, int32_t nr, int32_t nc,
                         const sg_formants* formants, double formantDep,
                         double rolloffLip, sg_anchors mouthAnchors,
                         double mouthOpenThres, double openMouthBoost,
                         double vocalTract, double temperature,
                         double formDrift, double formDisp,
                         double formantDepStoch, double smoothLinearFactor,
                         double samplingRate, double speedSound,
                         const sg_random* rnd, double* out);
/* STFT(hamming) x envelope -> ISTFT(hann OLA) -> /max, R/soundgen.R:743-807.
 * env is nr x env_nc (env_nc == 1: stationary). out cap >= len. */
int sg_formant_filter(sg_ctx* ctx, const double* sound, int64_t len,
                      const double* env, int32_t env_nc,
                      int32_t windowLength_points, double overlap,
                      double* out, int64_t cap, int64_t* out_len);
/* getSmoothContour(anchors, len, thisIsPitch, method, valueFloor,
 * valueCeiling, samplingRate)  R/smoothContours.R:53-227 (exported,
 * NAMESPACE:10); method 0 = 'loess' (R's default), 1 = 'spline'. The
 * planner's own contour (host, fp64). out holds len doubles; *out_len = 0 when
 * R returns NA (no anchors, len 0). len = -1 is R's len = NULL: the anchor
 * times are in ms and len = floor(duration_ms * samplingRate / 1000) (out must
 * then hold that many doubles). */
int sg_get_smooth_contour(sg_anchors anchors, int64_t len, int32_t thisIsPitch, int32_t method, int32_t has_floor,
                          double valueFloor, int32_t has_ceil, double valueCeiling, double samplingRate, double* out,
                          int64_t* out_len);
/* getRolloff() (host helper; R returns H x nGC). out cap = nHarmonics*nGC.
 * rolloffParabCeiling NaN = NULL (R/sourceSpectrum.R:77, :105-107). */
int sg_get_rolloff(const double* pitch_per_gc, int32_t n_gc,
                   int32_t nHarmonics, double rolloff, double rolloffOct,
                   double rolloffParab, double rolloffParabHarm,
                   double rolloffParabCeiling, double rolloffKHz,
                   double baseline, double throwaway,
                   double samplingRate, double* out, int32_t* out_rows);

/* ---- output writer: seewave::savewav (R/soundgen.R:856, R/morph.R:205) --- */
/* 16-bit PCM of every call of an executed plan, as savewav(wave, f) converts a
 * waveform (tuneR::normalize(unit = "16", level = min(max(wave), 1)): center,
 * scale by level / max|x| unless that is ~0, round(x * 32767) half to even).
 * d_in: the plan's packed fp32 output; d_out: int16 at the same offsets. */
int sg_pcm16(sg_ctx* ctx, sg_plan* plan, const float* d_in, int16_t* d_out, void* stream);
/* The same conversion for one host waveform in R's fp64 arithmetic (on the
 * GPU); rescale NULL, or {lower, upper} for savewav(rescale = ...). */
int sg_savewav_pcm(sg_ctx* ctx, const double* wave, int64_t n, const double* rescale, int16_t* pcm_out);
/* The file tuneR::writeWave(extensible = TRUE) writes for a mono 16-bit Wave. */
int sg_wav_write(const char* path, const int16_t* pcm, int64_t n, int32_t samplingRate);

/* Reference data tables the planner restates (pinned by tests/test_rda_fixtures.py
 * against the decoded .rda files):
 *   permittedValues rows 1..33 (data/permittedValues.rda, R/presets.R:22-56):
 *     name, default, low, high of soundgen()'s range-checked arguments;
 *   noiseThresholdsDict$q1/$q2[nonlinBalance + 1] (R/sysdata.rda,
 *     data-raw/noiseThresholdsDict.R), which = 1 or 2. */
int sg_permitted_value(int32_t i, const char** name, double* def_low_high);
double sg_noise_threshold(int32_t which, double nonlinBalance);

/* Test hook, no reference counterpart: the wavefront FFT stages used inside
 * the fused STFT/ISTFT kernel, on nframes frames of wl/2 complex points
 * (interleaved re, im, in place semantics: out = DFT(in), unscaled; inverse
 * bit 0 uses exp(+2 pi i nk / M); bit 1, for wl = 2204 only, runs the radix-29
 * stage on the VALU as sg_stft_ola_noise does instead of on the matrix pipe).
 * SG_E_UNSUPPORTED if wl is not on that path. */
int sg_debug_wave_fft(sg_ctx* ctx, int32_t wl, int32_t inverse, int32_t nframes,
                      const float* in, float* out);
/* Test hook, no reference counterpart: the fp64 transform under spectrogram(),
 * analyze()'s frames and cepstrum, segment() and the fp64 formant-filter frames
 * (fft64, sg_fft64_dev.h), alone: out = DFT(in) of nframes frames of M complex
 * points (host, interleaved re, im), unscaled; inverse != 0 uses
 * exp(+2 pi i nk / M). SG_E_UNSUPPORTED, checked before anything else (ctx may be
 * NULL then, out is left alone), for M < 1, M > 2048 or M not 31-smooth. */
int sg_debug_fft64(sg_ctx* ctx, int32_t M, int32_t inverse, int32_t nframes,
                   const double* in, double* out);
/* Test hook, no reference counterpart: the six sine-bank kernels (sg_sine_bank,
 * _pairs, _tall, _tall_pairs, _hp, _tab) on caller-built wave tasks, through the
 * product's classifier and launchers. tasks: ntasks records of 128 bytes laid out as
 * SgWTask (csrc/sg_dev.h); amps: namps floats, the columns the tasks' a_off / d_off
 * index; wlen: elements of the epoch scratch the tasks' w_off + j index; jobs
 * (NULL with njobs 0: none): njobs records of 32 bytes laid out as SgTabJob with
 * flags 0, whose tasks run on the wavetable path; env: the flat amplitude
 * envelope of every syllable with a task flagged SG_TASK_ENV (4).
 * Every byte of the three outputs is first set to 0xFF on the device (a NaN in
 * either precision), then each class is launched once and the table jobs once per
 * logn: W (wlen floats) and W64 (wlen doubles) receive the fp32 and the fp64
 * scratch, taskmax (ntasks floats) the per-task maxima, cls (ntasks) each task's
 * class: 0 sg_sine_bank, 1 _pairs, 2 _tall, 3 _tall_pairs, 4 _hp, 5 _tab.
 * SG_E_ARG, before anything touches the device, unless every task has
 *   1 <= len <= 1024; R > 0 and a multiple of 16; 0 < Rn <= R, a multiple of 4;
 *   j0 >= 0; 0 <= mbase <= 2^30; 0 <= w_off + j0 and w_off + j0 + len <= wlen;
 *   0 <= a_off, d_off and a_off + R, d_off + R <= namps; 0 <= dj0 <= dj1; syl >= 0;
 *   flags within 1 | 2 | 4 | 8, not 2 and 4 together; finite coefficients;
 *   the tasks of one syl next to each other,
 * and every job
 *   flags 0; 1 <= n <= 64; 0 <= t0, t0 + n <= ntasks, past the job before it;
 *   8 <= logn <= 11; 4 <= Rn <= 96; 0 <= a_off, a_off + Rn <= namps; every task of
 *   it with flags 1 | 2 exactly, R <= 96 and the job's a_off and Rn,
 * and 1 <= ntasks <= 2^20, 1 <= wlen <= 2^26, 1 <= namps <= 2^26, env finite. */
int sg_debug_sine_bank(sg_ctx* ctx, const void* tasks, int64_t ntasks, const float* amps, int64_t namps,
                       int64_t wlen, const void* jobs, int64_t njobs, double env,
                       float* W, double* W64, float* taskmax, int32_t* cls);
/* Test hook, no reference counterpart: the tile map of ssm()'s Gram kernel
 * (sg_ssm_gram, one wavefront per 16 x 16 tile on the fp64 matrix pipe). feat
 * holds n vectors of L doubles one after another (host); out (host, n * n
 * doubles, column-major) receives their unnormalised Gram matrix
 * out[i + j n] = sum_k feat[i L + k] feat[j L + k]. */
int sg_debug_ssm_gram(sg_ctx* ctx, const double* feat, int32_t L, int32_t n, double* out);
/* Measurement hook: the device milliseconds of the 7 stages of the last sg_ssm /
 * sg_ssm_batch run on a context with sg_set_profiling on (between events on the
 * stream): stats, frames, feat, winstat, gram, novelty, out (7 doubles). */
int sg_debug_ssm_kernel_ms(double* out);
/* Measurement hook: the device milliseconds of the 12 stages of the last
 * sg_spectrogram / sg_spectrogram_batch run on a context with sg_set_profiling on
 * (between events on the stream; 0 for a stage its argument switched off): stats,
 * frames, derivative, median along bins, median along frames, frame quantile and
 * range, log, entropy, entropy quantile, noise spectrum, subtraction, power and
 * scale (12 doubles). */
int sg_debug_spectrogram_kernel_ms(double* out);
/* Measurement hook: the device milliseconds of the 4 stages of the last
 * sg_analyze_frames / sg_analyze_frames_batch run on a context with
 * sg_set_profiling on: the spectrogram (statistics and |X| frames), the frame
 * amplitudes, the spectral descriptives and dom, the autocorrelation and its
 * peaks (4 doubles). */
int sg_debug_analyze_kernel_ms(double* out);
/* The same for the last sg_pitch_candidates / sg_pitch_candidates_batch run: the 4
 * stages above, then the cepstrum and its peaks, then the spectral peaks and the
 * BaNa candidates (6 doubles; 0 for a stage that was not launched). */
int sg_debug_pitch_kernel_ms(double* out);
/* The same for the last sg_analyze / sg_analyze_batch / sg_pitch_path run: the 6 stages
 * above, then the path stage (segments, pathfinder, smoother, final columns), then the
 * harmonics (8 doubles; sg_pitch_path runs the seventh alone). */
int sg_debug_track_kernel_ms(double* out);
/* The device milliseconds of the summary kernel of the last sg_analyze_summary /
 * sg_analyze_summary_batch / sg_analyze_summary_sound run (1 double); the stages before it
 * are sg_debug_track_kernel_ms's, unchanged. */
int sg_debug_summary_kernel_ms(double* out);
/* The device milliseconds of sg_fmt_lags and sg_fmt_roots in the last profiled sg_formants* run
 * (2 doubles), and, of the last run, profiled or not (counts: 3 int64, or NULL): the frames
 * that hit the iteration cap, the frames analysed, and the Aberth iterations those took. */
int sg_debug_formants_kernel_ms(double* out, int64_t* counts);
/* The same for the last sg_formants_whole / sg_formants_whole_batch run: the device
 * milliseconds of the mean (chunk sums and their fold), the chunk lags, the fold of the lags
 * and sg_fmt_roots (4 doubles), and the three counters over the sounds analysed. */
int sg_debug_formants_whole_kernel_ms(double* out, int64_t* counts);
/* The same for the last sg_segment / sg_segment_batch run, summed over the chunks of a
 * batch: the normalization statistics, the forward columns with their twiddle (or the
 * whole transform of a sound of at most 2048 points), the rows (forward, the Hilbert
 * multiplier, inverse, twiddle), the inverse columns with Mod and the un-padding, the
 * smoothing, and the tail (syllables, bursts, summary) (6 doubles). */
int sg_debug_segment_kernel_ms(double* out);
/* The same six stages for the last sg_segment_sweep: the first four once per sound, the
 * smoothing summed over the envelope groups, the tail summed over the chunks of rows. */
int sg_debug_sweep_kernel_ms(double* out);
/* The device milliseconds of the last profiled sg_analyze_sweep, summed over its frame groups,
 * candidate groups and chunks of rows (10 doubles): spectrogram, amplitude, descriptives and
 * dom, autocorrelation (full: sg_anl_acf with or without the store), autocorrelation (peaks
 * only: sg_anl_acf_peaks from the store), cepstrum, BaNa, path, harmonics, summary. A stage runs
 * from its stamp to the next stage's: it carries the host's preparation of the next launch. */
int sg_debug_analyze_sweep_kernel_ms(double* out);
/* The device milliseconds of sg_mel_pair and sg_mel_pair_reduce in the last profiled
 * sg_compare_sounds_pairs (2 doubles). */
int sg_debug_mel_pair_kernel_ms(double* out);

/* ---- stft(), istft() and invert_spectrogram(): sound from a spectrogram (an additive
 * extension of ABI 5; no reference counterpart). p is spectrogram()'s parameter block and
 * binds the same decisions: wl, the pad of zp, N = wl + 2 pad, M = N / 2 bins, the frame
 * starts of getFrameBank's seq(), the window; smoothing, denoising, method and output are not
 * read beyond their validation. Every refusal of sg_spectrogram_size applies with the same
 * code and text, before anything is launched and before ctx is looked at.
 *
 * A spectrum is stored frame after frame with `rows` cells a frame: rows = M (the shape of
 * spectrogram()'s matrix: DC in, Nyquist out) or M + 1 (with the Nyquist bin); anything else is
 * SG_E_ARG. A complex cell is two doubles (re, im).
 *   Analysis A: frame i is w[t] x[s_i + t], zero-padded as getFrameBank pads it; bins 0 .. M of
 *   its N-point DFT, unscaled.
 *   Synthesis A+ (least squares): the M + 1 bins extended Hermitian (a missing Nyquist bin is
 *   0), the real part of the inverse DFT / N, the pad dropped, then x^[t] = sum_i w[t - s_i]
 *   y_i[t - s_i] / sum_i w[t - s_i]^2 over the frames that cover t, in frame order. A sample whose
 *   denominator is 0 (no frame covers it, or only zeros of the window do) is 0. No other floor.
 * The sound that comes back is in the domain of getFrameBank's normalised sound: the original
 * scale is not in a spectrogram. */
/* Host only, no device: for a sound of len samples wl, n_fft, bins (= M) and frames as
 * sg_spectrogram_size gives them, the samples A+ returns (len), and the bytes of workspace the
 * sound takes inside sg_spg_istft_batch / sg_invert_spectrogram_batch. rows: 0, or a row
 * count to validate. */
int sg_invert_size(int64_t len, const sg_spectrogram_params* p, int32_t rows, int32_t* wl, int32_t* n_fft, int32_t* bins,
                   int32_t* frames, int64_t* samples, int64_t* workspace_bytes);
/* The message of the calling thread's last failed sg_invert_size ("" if none). */
const char* sg_invert_size_error(void);
/* A of n_calls sounds in DEVICE memory (call c: lengths[c] samples at offsets[c] of d_wave,
 * fp32, or fp64 when is_f64), each normalised as getFrameBank normalises it (the statistics are
 * spectrogram()'s, bit for bit). d_out (device): call c's frames x rows complex cells at complex
 * cell out_off[c]. A sound shorter than the window has no frames. */
int sg_spg_stft_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                      int64_t n_calls, const sg_spectrogram_params* p, int32_t rows, double* d_out,
                      const int64_t* out_off);
/* A+ of n_calls spectra in DEVICE memory (call c: frames x rows complex cells at complex cell
 * spec_off[c] of d_spec, frames as sg_invert_size gives them for lengths[c]). d_out (device)
 * receives lengths[c] doubles at out_off[c]. */
int sg_spg_istft_batch(sg_ctx* ctx, const double* d_spec, const int64_t* spec_off, const int64_t* lengths, int64_t n_calls,
                       const sg_spectrogram_params* p, int32_t rows, double* d_out, const int64_t* out_off);
/* Griffin & Lim's alternating projections on n_calls magnitude matrices in DEVICE memory (call
 * c: frames x rows doubles at mag_off[c] of d_mag, as sg_spectrogram_batch leaves them; d_phase:
 * the initial phases in the same layout, or NULL for zero). X_0 = S exp(i phi_0); n_iter times
 * x = A+ X, Z = A x, X = S Z / |Z| on the constrained bins (X = S where |Z| = 0; the Nyquist bin of
 * an M-row matrix is unconstrained, starts at 0 and is carried through); d_out (device) receives
 * A+ X, lengths[c] doubles at out_off[c], and serves as x in between. err_out (host, n_calls x
 * n_iter doubles, call-major, or NULL): e_k = sqrt(sum (|A x_k| - S)^2 / sum S^2) over the
 * constrained bins, k = 1 .. n_iter (NaN for a sound without frames or with S = 0). The batch
 * runs in chunks of consecutive sounds whose workspaces (sg_invert_size) fit workspace_cap bytes
 * (0: 1 GiB; at least one sound a chunk); one launch sequence per iteration serves a chunk, with
 * no wait inside the loop. A sound's samples and errors are the same bit for bit alone, in any
 * batch, at any position and under any cap. SG_E_ARG for a negative or NaN magnitude. */
int sg_invert_spectrogram_batch(sg_ctx* ctx, const double* d_mag, const int64_t* mag_off, const double* d_phase,
                                const int64_t* lengths, int64_t n_calls, const sg_spectrogram_params* p, int32_t rows,
                                int32_t n_iter, int64_t workspace_cap, double* d_out, const int64_t* out_off,
                                double* err_out);
/* The device milliseconds of the last of the three on a context with sg_set_profiling on, summed
 * over iterations and chunks (6 doubles): normalisation statistics, the forward frames (with the
 * projection inside the iteration), X_0, the inverse frames, the overlap-add, the error fold. */
int sg_debug_invert_kernel_ms(double* out);

/* ---- time_stretch(), shift_pitch() and resample(): a phase vocoder between A and A+ above and a
 * band-limited resampler (an additive extension of ABI 5; no reference counterpart). fp64, no
 * floating-point atomics: a sound's samples are the same bit for bit alone, in any batch, at any
 * position and under any workspace cap. Formants move with the pitch; there is no transient
 * handling and no phase locking.
 *
 *   Time stretch. X = A x without getFrameBank's normalisation, M + 1 rows, F_in frames starting at
 *   s_i; the output has out_len samples, F_out frames starting at t_j, g_j = t_j - t_j-1, and a
 *   position q_j in [0, F_in - 1] per output frame. i = min(floor(q_j), F_in - 1), a = q_j - i,
 *   i1 = min(i + 1, F_in - 1), h = s_i1 - s_i;
 *     m_j[k] = (1 - a) |X_i[k]| + a |X_i1[k]|,
 *     d = arg X_i1[k] - arg X_i[k] - 2 pi ((k h) mod N) / N, wrapped d -= 2 pi rint(d / 2 pi), (d / h)_j = d / h
 *     (0 where h = 0),
 *     psi_0[k] = arg X_i(0)[k], psi_j[k] = psi_j-1[k] + 2 pi ((k g_j) mod N) / N + g_j (d / h)_j-1, wrapped alike
 *     after every step,
 *   X'_j[k] = m_j[k] exp(i psi_j[k]) and the result is A+ X'. With q_j = j and out_len = len, X' = X up to
 *   rounding.
 *   Resample. up and down reduced by their gcd, D = max(up, down), n_out = ceil(n up / down):
 *     y[r] = sum_m x[m] (up / D) sinc(num / D) (1 + cos(pi num / (16 D))) / 2,  num = r down - m up,
 *   over 0 <= m < n with |num| < 16 D in ascending m; sin(pi num / D) is taken on num reduced mod 2 D
 *   (exactly 0 at the non-zero multiples of D), so up = down returns x bit for bit. */
/* Host only, no device. With p: for a sound of len samples and an output of out_len, the frames of
 * both (frames_in, frames_out) and the bytes of workspace the sound takes inside
 * sg_time_stretch_batch; every refusal of sg_spectrogram_size applies with its code and text.
 * With p = NULL: for len samples and the ratio up : down, n_out and the most taps an output sample
 * has. SG_E_ARG for up or down below 1 or at 2^31 and above, max / min above 64 after reduction, or
 * n_out at 2^31 and above. The outputs of the other form may be NULL. */
int sg_stretch_size(int64_t len, const sg_spectrogram_params* p, int64_t out_len, int64_t up, int64_t down, int32_t* frames_in,
                    int32_t* frames_out, int64_t* workspace_bytes, int64_t* n_out, int64_t* taps);
/* The message of the calling thread's last failed sg_stretch_size ("" if none). */
const char* sg_stretch_size_error(void);
/* The vocoder on n_calls sounds in DEVICE memory (call c: lengths[c] samples at offsets[c] of
 * d_wave, fp32, or fp64 when is_f64). out_lengths[c]: the samples of call c's result, written as
 * doubles at out_off[c] of d_out (device). positions (HOST): call c's pos_count[c] positions at
 * positions[pos_off[c]]. SG_E_ARG, before ctx is looked at, for a count that is not the frame count
 * of out_lengths[c], a position that is NaN or outside [0, F_in - 1], or an output shorter than the
 * window. A sound shorter than the window has no frames, as in sg_spg_stft_batch: its count and
 * positions are not read and its result is out_lengths[c] zeros. The batch runs in chunks of
 * consecutive sounds whose workspaces (sg_stretch_size) fit workspace_cap bytes (0: 1 GiB; at least
 * one sound a chunk). d_spec (device, or NULL): receives X', F_out x (M + 1) complex cells at
 * complex cell spec_off[c]. */
int sg_time_stretch_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                          int64_t n_calls, const sg_spectrogram_params* p, const int64_t* out_lengths, const double* positions,
                          const int64_t* pos_off, const int64_t* pos_count, double* d_out, const int64_t* out_off,
                          int64_t workspace_cap, double* d_spec, const int64_t* spec_off);
/* The resampler on n_calls sounds in DEVICE memory, call c by up[c] : down[c]: n_out doubles
 * (sg_stretch_size) at out_off[c] of d_out (device). The refusals are sg_stretch_size's, before
 * ctx is looked at. */
int sg_resample_batch(sg_ctx* ctx, const void* d_wave, int32_t is_f64, const int64_t* offsets, const int64_t* lengths,
                      int64_t n_calls, const int64_t* up, const int64_t* down, double* d_out, const int64_t* out_off);
/* The device milliseconds of the last of the two on a context with sg_set_profiling on, summed
 * over chunks (5 doubles): the resampler, the forward frames, the vocoder, the inverse frames, the
 * overlap-add. */
int sg_debug_stretch_kernel_ms(double* out);

#ifdef __cplusplus
}
#endif
#endif /* SOUNDGEN_HIP_H */
