"""Loader of the in-tree HIP library soundgen_beta_amd/lib/libsoundgen_hip.so.

There is no CPU fallback: if the library is missing or the GPU is not
usable, calls raise. (The planner entry points work without a GPU so host
bookkeeping can be tested on CPU; every synthesis call needs the device.)
"""
import ctypes as C
import os
import re

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SG_HIP_LIB") or os.path.join(_HERE, "lib", "libsoundgen_hip.so")  # override: experiments
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "soundgen_hip.h")

_lib = None
# the planner's default threshold on its fp32 conditioning estimate of a formant
# filter (sg_set_fp64_policy; DESIGN.md §5 "fp64 path")
HP_RHO_DEFAULT = 100.0


class SoundgenError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (_abi.SG_ERR_NAMES.get(code, code), msg))
        self.code = code


def declared_symbols():
    """Function names declared in include/soundgen_hip.h."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(sg_[a-z_0-9]+)\s*\(", txt)))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    # Share torch's HIP runtime when torch is present: torch/lib/libamdhip64.so
    # has the same SONAME as /opt/rocm's, so importing torch first makes our
    # NEEDED entry resolve to that copy (one runtime, valid device pointers).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("libsoundgen_hip.so not built (run __graft_entry__.build()): %s" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    dp = C.POINTER(C.c_double)
    i64 = C.c_int64
    i64p = C.POINTER(C.c_int64)
    L.sg_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sg_ctx_destroy.argtypes = [vp]
    L.sg_last_error.argtypes = [vp]
    L.sg_last_error.restype = C.c_char_p
    L.sg_plan_batch.argtypes = [vp, C.POINTER(_abi.sg_call_desc), i64, C.POINTER(vp)]
    L.sg_plan_destroy.argtypes = [vp]
    L.sg_plan_n_calls.argtypes = [vp]
    L.sg_plan_n_calls.restype = i64
    L.sg_plan_total_samples.argtypes = [vp]
    L.sg_plan_total_samples.restype = i64
    L.sg_plan_lengths.argtypes = [vp, i64p, i64p]
    L.sg_plan_status.argtypes = [vp, C.POINTER(C.c_int32)]
    L.sg_plan_call_message.argtypes = [vp, i64]
    L.sg_plan_call_message.restype = C.c_char_p
    L.sg_plan_device_bytes.argtypes = [vp]
    L.sg_plan_device_bytes.restype = i64
    L.sg_plan_upload.argtypes = [vp, vp]
    L.sg_plan_release_host.argtypes = [vp]
    L.sg_execute.argtypes = [vp, vp, vp, vp]
    L.sg_execute_plans.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, vp]
    L.sg_set_profiling.argtypes = [vp, C.c_int]
    L.sg_profile_read.argtypes = [vp, dp, i64p]
    L.sg_profile_read_kernel.argtypes = [vp, C.c_int, dp, i64p]
    L.sg_plan_stft_stats.argtypes = [vp, i64p, i64p, dp]
    L.sg_plan_conditioning.argtypes = [vp, dp]
    L.sg_plan_noise_conditioning.argtypes = [vp, dp]
    L.sg_plan_precision.argtypes = [vp, C.POINTER(C.c_int32), i64p, i64p]
    L.sg_set_fp64_policy.argtypes = [C.c_int32, C.c_double]
    L.sg_set_amp_policy.argtypes = [C.c_int32]
    L.sg_set_uniform_gather.argtypes = [C.c_int32]
    if hasattr(L, "sg_plan_sine_tasks"):  # ABI 4 (an older library still loads for A/B runs)
        L.sg_plan_sine_tasks.argtypes = [vp, i64p]
    L.sg_set_sine_table.argtypes = [C.c_int32]
    L.sg_plan_table_stats.argtypes = [C.c_void_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.sg_host_cache_trim.argtypes = []
    L.sg_host_cache_trim.restype = i64
    L.sg_get_smooth_contour.argtypes = [_abi.sg_anchors, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                        C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double),
                                        C.POINTER(C.c_int64)]
    L.sg_plan_amp_count.restype = C.c_int64
    L.sg_plan_amp_count.argtypes = [C.c_void_p]
    L.sg_plan_debug_amps.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
    L.sg_plan_call_work.argtypes = [vp, dp, dp]
    L.sg_dtw_symmetric2.argtypes = [dp, i64, dp, i64, dp]
    L.sg_mel_spec.argtypes = [vp, dp, i64, C.POINTER(_abi.sg_mel_params), dp, i64, C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32)]
    L.sg_compare_sounds_batch.argtypes = [vp, dp, C.c_int32, C.c_int32, vp, i64p, i64p, i64,
                                          C.POINTER(_abi.sg_mel_params), C.c_int32, dp, dp]
    if hasattr(L, "sg_mel_set_create"):  # resident mel spectra and pair scoring: additive to ABI 5
        i32p = C.POINTER(C.c_int32)
        L.sg_mel_set_create.argtypes = [vp, vp, C.c_int32, i64p, i64p, i64, C.POINTER(_abi.sg_mel_params),
                                        C.POINTER(vp)]
        L.sg_mel_set_info.argtypes = [vp, i64p, i32p, i32p]
        L.sg_mel_set_spec.argtypes = [vp, i64, dp, i64, i32p]
        L.sg_mel_set_destroy.argtypes = [vp]
        L.sg_mel_set_destroy.restype = None
        L.sg_compare_sounds_pairs.argtypes = [vp, vp, vp, i32p, i64, C.c_int32, C.c_int32, dp, dp]
        L.sg_debug_mel_pair_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_ssm_size"):  # ssm(): an additive extension of ABI 5 (a host-only build lacks it)
        i32p = C.POINTER(C.c_int32)
        L.sg_ssm_size.argtypes = [i64, C.POINTER(_abi.sg_ssm_params), i32p, i32p, i32p, i32p]
        L.sg_ssm.argtypes = [vp, dp, i64, C.POINTER(_abi.sg_ssm_params), dp, dp]
        L.sg_ssm_batch.argtypes = [vp, vp, i64p, i64p, i64, C.POINTER(_abi.sg_ssm_params), i32p, dp, i64p, dp,
                                   i64p]
        L.sg_debug_ssm_gram.argtypes = [vp, dp, C.c_int32, C.c_int32, dp]
        L.sg_debug_ssm_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_spectrogram_size"):  # spectrogram(): likewise additive, absent from a host-only build
        i32p = C.POINTER(C.c_int32)
        spp = C.POINTER(_abi.sg_spectrogram_params)
        L.sg_spectrogram_size.argtypes = [i64, spp, i32p, i32p, i32p, i32p]
        L.sg_spectrogram_size_error.argtypes = []
        L.sg_spectrogram_size_error.restype = C.c_char_p
        L.sg_spectrogram.argtypes = [vp, dp, i64, spp, dp]
        L.sg_spectrogram_batch.argtypes = [vp, vp, i64p, i64p, i64, spp, vp, i64p, i32p, i32p]
        L.sg_debug_spectrogram_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_invert_size"):  # stft(), istft(), invert_spectrogram(): likewise additive
        i32p = C.POINTER(C.c_int32)
        spp = C.POINTER(_abi.sg_spectrogram_params)
        L.sg_invert_size.argtypes = [i64, spp, C.c_int32, i32p, i32p, i32p, i32p, i64p, i64p]
        L.sg_invert_size_error.argtypes = []
        L.sg_invert_size_error.restype = C.c_char_p
        L.sg_spg_stft_batch.argtypes = [vp, vp, C.c_int32, i64p, i64p, i64, spp, C.c_int32, vp, i64p]
        L.sg_spg_istft_batch.argtypes = [vp, vp, i64p, i64p, i64, spp, C.c_int32, vp, i64p]
        L.sg_invert_spectrogram_batch.argtypes = [vp, vp, i64p, vp, i64p, i64, spp, C.c_int32, C.c_int32, i64, vp, i64p,
                                                  dp]
        L.sg_debug_invert_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_stretch_size"):  # time_stretch(), shift_pitch(), resample(): likewise additive
        i32p = C.POINTER(C.c_int32)
        spp = C.POINTER(_abi.sg_spectrogram_params)
        L.sg_stretch_size.argtypes = [i64, spp, i64, i64, i64, i32p, i32p, i64p, i64p, i64p]
        L.sg_stretch_size_error.argtypes = []
        L.sg_stretch_size_error.restype = C.c_char_p
        L.sg_time_stretch_batch.argtypes = [vp, vp, C.c_int32, i64p, i64p, i64, spp, i64p, dp, i64p, i64p, vp, i64p, i64, vp,
                                            i64p]
        L.sg_resample_batch.argtypes = [vp, vp, C.c_int32, i64p, i64p, i64, i64p, i64p, vp, i64p]
        L.sg_debug_stretch_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_debug_fft64"):  # the fp64 transform alone (tests/test_fft64.py): likewise additive
        L.sg_debug_fft64.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    if hasattr(L, "sg_debug_sine_bank"):  # the sine-bank kernels on caller-built tasks (tests/test_sine_bank.py)
        L.sg_debug_sine_bank.argtypes = [vp, vp, i64, C.POINTER(C.c_float), i64, i64, vp, i64, C.c_double,
                                         C.POINTER(C.c_float), dp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    if hasattr(L, "sg_analyze_frames_size"):  # analyze()'s per-frame stage: likewise additive
        i32p = C.POINTER(C.c_int32)
        app = C.POINTER(_abi.sg_analyze_params)
        L.sg_analyze_frames_size.argtypes = [i64, app, i32p, i32p, i32p, i32p, i32p, i32p, i32p]
        L.sg_analyze_frames_size_error.argtypes = []
        L.sg_analyze_frames_size_error.restype = C.c_char_p
        L.sg_analyze_frames_ampl_starts.argtypes = [i64, app, i64p, C.c_int32]
        L.sg_analyze_frames.argtypes = [vp, dp, i64, app, dp]
        L.sg_analyze_frames_batch.argtypes = [vp, vp, i64p, i64p, i64, app, vp, i64p, i32p]
        L.sg_debug_analyze_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_pitch_candidates_size"):  # the cepstral and spectral trackers: likewise additive
        i32p = C.POINTER(C.c_int32)
        ppp = C.POINTER(_abi.sg_pitch_params)
        L.sg_pitch_candidates_size.argtypes = [i64, ppp, i32p, i32p, i32p]
        L.sg_pitch_candidates_cep_labels.argtypes = [ppp, dp, C.c_int32]
        L.sg_pitch_candidates.argtypes = [vp, dp, i64, ppp, dp]
        L.sg_pitch_candidates_batch.argtypes = [vp, vp, i64p, i64p, i64, ppp, vp, i64p, i32p]
        L.sg_debug_pitch_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_analyze_size"):  # analyze()'s tail behind the candidates: likewise additive
        i32p = C.POINTER(C.c_int32)
        fpp = C.POINTER(_abi.sg_analyze_params_full)
        L.sg_analyze_size.argtypes = [i64, fpp, i32p, i32p, i32p]
        L.sg_analyze.argtypes = [vp, dp, i64, fpp, dp]
        L.sg_analyze_batch.argtypes = [vp, vp, i64p, i64p, i64, fpp, vp, i64p, i32p]
        L.sg_pitch_path.argtypes = [vp, dp, C.c_int32, i64, fpp, dp]
        if hasattr(L, "sg_pitch_path_costs"):  # the segments and their path costs: likewise additive
            L.sg_pitch_path_costs.argtypes = [vp, dp, C.c_int32, i64, fpp, dp, dp, i32p]
        L.sg_debug_track_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_analyze_summary"):  # analyze(summary = TRUE): likewise additive
        i32p = C.POINTER(C.c_int32)
        fpp = C.POINTER(_abi.sg_analyze_params_full)
        L.sg_analyze_summary_name.argtypes = [C.c_int32]
        L.sg_analyze_summary_name.restype = C.c_char_p
        L.sg_analyze_summary.argtypes = [vp, dp, C.c_int32, C.c_int32, C.c_int32, i64, C.c_double, dp]
        L.sg_analyze_summary_batch.argtypes = [vp, vp, i64p, i64p, i64, fpp, vp, i64p, i32p, vp]
        L.sg_analyze_summary_sound.argtypes = [vp, dp, i64, fpp, dp, dp]
        L.sg_debug_summary_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_formants_size"):  # analyze()'s formant tracks: likewise additive
        i32p = C.POINTER(C.c_int32)
        app = C.POINTER(_abi.sg_analyze_params)
        L.sg_formants_size.argtypes = [app, C.c_int32, i32p, i32p]
        L.sg_formants_batch.argtypes = [vp, vp, i64p, i64p, i64, app, C.c_int32, vp, i64p, C.c_int32, i32p, vp, i64p]
        L.sg_formants_sound.argtypes = [vp, dp, i64, app, C.c_int32, dp]
        L.sg_formants_frames.argtypes = [vp, dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, dp]
        L.sg_debug_formants_kernel_ms.argtypes = [dp, i64p]
    if hasattr(L, "sg_formants_whole_size"):  # findformants on a whole sound (matchPars): likewise additive
        i32p = C.POINTER(C.c_int32)
        L.sg_formants_whole_size.argtypes = [C.c_double, i64, i32p, i32p, i64p]
        L.sg_formants_whole.argtypes = [vp, dp, i64, C.c_double, dp]
        L.sg_formants_whole_batch.argtypes = [vp, vp, i64p, i64p, i64, C.c_double, vp]
        L.sg_debug_formants_whole_kernel_ms.argtypes = [dp, i64p]
    if hasattr(L, "sg_segment_size"):  # segment(): likewise additive
        i32p = C.POINTER(C.c_int32)
        gpp = C.POINTER(_abi.sg_segment_params)
        L.sg_segment_size.argtypes = [i64, gpp, i32p, i32p, i32p, i64p]
        L.sg_segment_size_error.argtypes = []
        L.sg_segment_size_error.restype = C.c_char_p
        L.sg_segment_windows.argtypes = [i64, gpp, i64p, i64p, i64p, C.c_int32, dp]
        L.sg_segment.argtypes = [vp, dp, i64, gpp, dp]
        L.sg_segment_batch.argtypes = [vp, vp, i64p, i64p, i64, gpp, vp, i64p]
        L.sg_debug_segment_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_segment_sweep"):  # parameter sweeps of segment(): likewise additive
        gpp = C.POINTER(_abi.sg_segment_params)
        L.sg_segment_sweep.argtypes = [vp, vp, i64p, i64p, i64, gpp, i64, vp]
        L.sg_sweep_fitness.argtypes = [vp, vp, i64, i64, C.c_int32, C.c_int32, dp, dp]
        L.sg_set_sweep_staging.argtypes = [C.c_int32]
        L.sg_debug_sweep_kernel_ms.argtypes = [dp]
    if hasattr(L, "sg_analyze_sweep"):  # parameter sweeps of analyze(): likewise additive
        i32p = C.POINTER(C.c_int32)
        fpp = C.POINTER(_abi.sg_analyze_params_full)
        L.sg_analyze_sweep.argtypes = [vp, vp, i64p, i64p, i64, fpp, i64, i64, vp]
        L.sg_analyze_sweep_plan.argtypes = [fpp, i64, i32p, i32p, i32p]
        L.sg_analyze_sweep_size.argtypes = [i64p, i64, fpp, i64, i64p]
        L.sg_set_analyze_sweep_store.argtypes = [C.c_int32]
        L.sg_debug_analyze_sweep_kernel_ms.argtypes = [dp]
    L.sg_rrng_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.sg_rrng_destroy.argtypes = [vp]
    L.sg_rrng_set_seed.argtypes = [vp, C.c_int32]
    for f in ("unif", "norm", "exp"):
        getattr(L, "sg_rrng_" + f).argtypes = [vp]
        getattr(L, "sg_rrng_" + f).restype = C.c_double
    L.sg_rrng_gamma.argtypes = [vp, C.c_double, C.c_double]
    L.sg_rrng_gamma.restype = C.c_double
    L.sg_random_bind_rrng.argtypes = [C.POINTER(_abi.sg_random), vp]
    L.sg_plan_kernel_stats.argtypes = [vp, i64p, i64p, i64p, i64p]
    L.sg_synchronize.argtypes = [vp]
    L.sg_execute_to_host.argtypes = [vp, vp, dp]
    L.sg_generate_harmonics.argtypes = [vp, dp, i64, C.POINTER(_abi.sg_harm_params), _abi.sg_anchors,
                                        C.POINTER(_abi.sg_random), dp, i64, i64p]
    L.sg_soundgen.argtypes = [vp, C.POINTER(_abi.sg_soundgen_args), C.POINTER(_abi.sg_random), dp, i64, i64p]
    L.sg_formant_filter.argtypes = [vp, dp, i64, dp, C.c_int32, C.c_int32, C.c_double, dp, i64, i64p]
    L.sg_generate_noise.argtypes = [vp, i64, _abi.sg_anchors, C.c_double, C.c_double, C.c_int32, C.c_double,
                                    C.c_double, C.c_double, dp, C.c_int32, C.POINTER(_abi.sg_random), dp]
    L.sg_spectral_envelope.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(_abi.sg_formants), C.c_double,
                                       C.c_double, _abi.sg_anchors, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.POINTER(_abi.sg_random), dp]
    L.sg_get_rolloff.argtypes = [dp, C.c_int32, C.c_int32] + [C.c_double] * 9 + [dp, C.POINTER(C.c_int32)]
    fp = C.POINTER(C.c_float)
    L.sg_debug_wave_fft.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, fp, fp]
    i16p = C.POINTER(C.c_int16)
    L.sg_pcm16.argtypes = [vp, vp, vp, vp, vp]
    L.sg_savewav_pcm.argtypes = [vp, dp, i64, dp, i16p]
    L.sg_wav_write.argtypes = [C.c_char_p, i16p, i64, C.c_int32]
    L.sg_permitted_value.argtypes = [C.c_int32, C.POINTER(C.c_char_p), dp]
    L.sg_noise_threshold.argtypes = [C.c_int32, C.c_double]
    L.sg_noise_threshold.restype = C.c_double
    L.sg_abi_version.restype = C.c_int
    # whole-node batch path (sg_node.cpp; ABI 3, chunks and divergence ABI 5). Guarded
    # like sg_plan_sine_tasks: an older library still loads for A/B runs
    if not hasattr(L, "sg_node_create"):
        _lib = L
        return L
    L.sg_device_count.restype = C.c_int
    L.sg_node_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(vp)]
    L.sg_node_destroy.argtypes = [vp]
    L.sg_node_size.argtypes = [vp]
    L.sg_node_size.restype = C.c_int32
    L.sg_node_last_error.argtypes = [vp]
    L.sg_node_last_error.restype = C.c_char_p
    L.sg_node_plan_batch.argtypes = [vp, vp, i64, C.POINTER(vp)]
    L.sg_node_plan_destroy.argtypes = [vp]
    L.sg_node_plan_n_calls.argtypes = [vp]
    L.sg_node_plan_n_calls.restype = i64
    L.sg_node_plan_total_samples.argtypes = [vp]
    L.sg_node_plan_total_samples.restype = i64
    L.sg_node_plan_lengths.argtypes = [vp, i64p, i64p]
    L.sg_node_plan_status.argtypes = [vp, C.POINTER(C.c_int32)]
    L.sg_node_plan_call_message.argtypes = [vp, i64]
    L.sg_node_plan_call_message.restype = C.c_char_p
    L.sg_node_plan_owner.argtypes = [vp, C.POINTER(C.c_int32)]
    L.sg_node_plan_costs.argtypes = [vp, dp]
    L.sg_node_plan_shard_samples.argtypes = [vp, C.c_int32]
    L.sg_node_plan_shard_samples.restype = i64
    L.sg_node_execute_to_host.argtypes = [vp, vp, dp]
    L.sg_node_execute_to_host_f32.argtypes = [vp, vp, C.POINTER(C.c_float)]
    if hasattr(L, "sg_node_plan_chunks"):
        L.sg_node_plan_chunks.argtypes = [vp, C.c_int32]
        L.sg_node_plan_chunks.restype = C.c_int32
        L.sg_node_plan_diverged.argtypes = [vp]
        L.sg_node_plan_diverged.restype = C.c_int32
        L.sg_node_plan_call_work.argtypes = [vp, dp, dp]
    if hasattr(L, "sg_rrng_unif_n"):
        L.sg_rrng_unif_n.argtypes = [vp, dp, i64]
    _lib = L
    return L


def check(rc, ctx=None):
    if rc < 0:
        msg = lib().sg_last_error(ctx).decode() if ctx is not None else ""
        raise SoundgenError(rc, msg)
    return rc


def raise_code(rc, msg, value_error=False):
    """The return-code policy of the analysis features: SoundgenError(rc, msg), or, for the modules
    that say so, ValueError for SG_E_ARG (-1)."""
    if value_error and rc == -1:
        raise ValueError(msg)
    raise SoundgenError(rc, msg)


def host_check(rc, reader, value_error=False):
    """Nothing for rc >= 0; otherwise raises with the text that reader() returns (a *_size_error
    reader after a host-only entry point, sg_last_error behind a context)."""
    if rc < 0:
        raise_code(rc, reader().decode(), value_error)


class Context:
    """A device context (one HIP stream on one GPU)."""

    def __init__(self, device=0):
        self.device = device
        self.ptr = C.c_void_p()
        rc = lib().sg_ctx_create(device, C.byref(self.ptr))
        if rc < 0:
            raise SoundgenError(rc, "sg_ctx_create(%d) failed (no usable GPU?)" % device)

    def close(self):
        if self.ptr:
            lib().sg_ctx_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Node:
    """Several devices driven from this process (sg_node_*): a batch is sharded
    over them by calls (LPT), each device synthesizes its shard and copies it over
    its own link. devices: ordinals (repeats allowed: a 2-way node on one GPU), or
    None for every visible device. Planning works without a GPU."""

    def __init__(self, devices=None):
        L = lib()
        self.ptr = C.c_void_p()
        if devices is None:
            rc = L.sg_node_create(None, 0, C.byref(self.ptr))
        else:
            d = (C.c_int32 * len(devices))(*devices)
            rc = L.sg_node_create(d, len(devices), C.byref(self.ptr))
        if rc < 0:
            raise SoundgenError(rc, "sg_node_create failed (no usable GPU?)")
        self.size = int(L.sg_node_size(self.ptr))

    def check(self, rc):
        if rc < 0:
            raise SoundgenError(rc, lib().sg_node_last_error(self.ptr).decode())
        return rc

    def close(self):
        if self.ptr:
            lib().sg_node_destroy(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------ marshalling of the *_batch entry points
def batch_layout(offsets, lengths):
    """The calls of a packed batch as the library reads them: (offs, lens, nc, p_offs,
    p_lens), contiguous int64 arrays (keep them alive across the call) and their pointers."""
    import numpy as np
    i64p = C.POINTER(C.c_int64)
    offs = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64))
    return offs, lens, len(offs), offs.ctypes.data_as(i64p), lens.ctypes.data_as(i64p)


def out_offsets(cells):
    """Where each call's output starts in one packed buffer, from the cells of every
    call: nc + 1 int64 (the last is the total), and the pointer."""
    import numpy as np
    ooff = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    return ooff, ooff.ctypes.data_as(C.POINTER(C.c_int64))


def device_out(data, n):
    """An fp64 tensor of n cells (at least 1) beside `data`, once the caller's work
    on data's device is done: the library runs on its own stream."""
    import torch
    out = torch.empty(max(int(n), 1), dtype=torch.float64, device=data.device)
    torch.cuda.synchronize(data.device)
    return out


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
