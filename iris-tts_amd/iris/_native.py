"""ctypes binding of the C-ABI declared in ``include/iris_hifigan.h``.

The shared library is built in-tree by ``iris-tts_amd/csrc/Makefile`` (``__graft_entry__.build()``).
There is no fallback: if the library is missing or does not load, every entry point raises
``NativeLibraryError`` -- the product path never computes on the CPU.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

MAX_STAGES = 8
MAX_KERNELS = 8
MAX_DILATIONS = 8
ABI_VERSION = 4
MAX_PLAN_LAUNCHES = 96

DTYPE_F32 = 0
DTYPE_BF16 = 1
DTYPE_F32_SPLIT = 2

STATUS_INVALID_ARGUMENT = 1
STATUS_UNSUPPORTED = 4
STATUS_WORKSPACE_TOO_SMALL = 5
STATUS_NOT_PREPARED = 6

LIB_NAME = "libiris_hifigan.so"
CSRC_DIR = Path(__file__).resolve().parent.parent / "csrc"


class NativeLibraryError(RuntimeError):
    """The HIP extension is missing, stale or failed to load."""


class NativeCallError(RuntimeError):
    """A C-ABI call returned a non-zero status."""

    def __init__(self, fn: str, status: int, message: str):
        super().__init__(f"{fn} failed with status {status}: {message}")
        self.status = status


class Config(ctypes.Structure):
    """``iris_hifigan_config``"""

    _fields_ = [
        ("in_channels", ctypes.c_int32),
        ("upsample_initial_channel", ctypes.c_int32),
        ("num_upsamples", ctypes.c_int32),
        ("upsample_rates", ctypes.c_int32 * MAX_STAGES),
        ("upsample_kernel_sizes", ctypes.c_int32 * MAX_STAGES),
        ("num_kernels", ctypes.c_int32),
        ("resblock_kernel_sizes", ctypes.c_int32 * MAX_KERNELS),
        ("num_dilations", ctypes.c_int32 * MAX_KERNELS),
        ("resblock_dilations", (ctypes.c_int32 * MAX_DILATIONS) * MAX_KERNELS),
        ("pre_kernel_size", ctypes.c_int32),
        ("post_kernel_size", ctypes.c_int32),
        ("lrelu_slope", ctypes.c_float),
    ]


class LaunchRecord(ctypes.Structure):
    """``iris_hifigan_launch_record``"""

    _fields_ = [
        ("kind", ctypes.c_int32),
        ("stage", ctypes.c_int32),
        ("step", ctypes.c_int32),
        ("launches", ctypes.c_int32),
        ("flops", ctypes.c_double),
        ("bytes", ctypes.c_double),
        ("ms", ctypes.c_float),
        ("reserved2", ctypes.c_float),
    ]


class WorkspaceMap(ctypes.Structure):
    """``iris_hifigan_workspace_map``"""

    _fields_ = [
        ("pre_offset", ctypes.c_uint64),
        ("up_offset", ctypes.c_uint64),
        ("y_offset", ctypes.c_uint64 * MAX_KERNELS),
        ("xt_offset", ctypes.c_uint64 * MAX_KERNELS),
        ("total_bytes", ctypes.c_uint64),
        ("element_bytes", ctypes.c_int32),
        ("launches", ctypes.c_int32),
    ]


class PlanLaunch(ctypes.Structure):
    """``iris_hifigan_plan_launch``"""

    _fields_ = [
        ("kernel", ctypes.c_char * 80),
        ("grid", ctypes.c_uint32 * 3),
        ("block", ctypes.c_uint32),
        ("lds_bytes", ctypes.c_uint64),
    ]


class Plan(ctypes.Structure):
    """``iris_hifigan_plan``"""

    _fields_ = [
        ("workspace_bytes", ctypes.c_uint64),
        ("n_launches", ctypes.c_int32),
        ("cu_count", ctypes.c_int32),
        ("passes", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("launches", PlanLaunch * MAX_PLAN_LAUNCHES),
    ]


# name -> (restype, argtypes); must list every symbol of include/iris_hifigan.h
_c = ctypes
_vp, _i32, _u64, _f = _c.c_void_p, _c.c_int32, _c.c_uint64, _c.c_float
_fp = _c.POINTER(_c.c_float)
SYMBOLS = {
    "iris_hifigan_abi_version": (_i32, []),
    "iris_hifigan_last_error": (_c.c_char_p, []),
    "iris_hifigan_weight_count": (_i32, [_c.POINTER(Config), _c.POINTER(_u64)]),
    "iris_hifigan_create": (_i32, [_c.POINTER(Config), _fp, _u64, _c.POINTER(_vp)]),
    "iris_hifigan_destroy": (_i32, [_vp]),
    "iris_hifigan_prepare": (_i32, [_vp, _i32]),
    "iris_hifigan_release_host_weights": (_i32, [_vp]),
    "iris_hifigan_pause_profiling": (_i32, [_vp, _i32]),
    "iris_hifigan_describe_plan": (_i32, [_c.POINTER(Config), _i32, _i32, _i32, _i32, _c.POINTER(Plan)]),
    "iris_hifigan_workspace_bytes": (_i32, [_vp, _i32, _i32, _i32, _c.POINTER(_u64)]),
    "iris_hifigan_forward": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _u64, _i32, _vp]),
    "iris_hifigan_forward_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _i32, _vp]),
    "iris_hifigan_forward_pcm16": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _f, _vp, _u64, _i32, _vp]),
    "iris_hifigan_workspace_layout": (_i32, [_vp, _i32, _i32, _i32, _c.POINTER(WorkspaceMap)]),
    "iris_hifigan_forward_until": (_i32, [_vp, _vp, _i32, _i32, _vp, _u64, _i32, _i32, _i32, _c.POINTER(_i32), _vp]),
    "iris_hifigan_hop_length": (_i32, [_vp, _c.POINTER(_i32)]),
    "iris_hifigan_set_profiling": (_i32, [_vp, _i32]),
    "iris_hifigan_read_profile": (_i32, [_vp, _c.POINTER(LaunchRecord), _i32, _c.POINTER(_i32)]),
    "iris_hifigan_op_conv1d": (_i32, [_vp, _fp, _fp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _i32, _vp]),
    "iris_hifigan_op_conv_transpose1d": (_i32, [_vp, _fp, _fp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_conv_post": (_i32, [_vp, _vp, _vp, _fp, _fp, _vp, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_pcm16": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_g711": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "iris_hifigan_op_mrf_step": (_i32, [_c.POINTER(_vp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_vp), _c.POINTER(_vp), _vp,
                                       _i32, _i32, _i32, _c.POINTER(_i32), _c.POINTER(_i32), _f, _i32, _vp]),
    "iris_hifigan_op_mrf_pair": (_i32, [_c.POINTER(_vp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp),
                                       _c.POINTER(_vp), _vp, _i32, _i32, _i32, _c.POINTER(_i32), _c.POINTER(_i32), _f, _i32, _vp]),
    "iris_hifigan_op_mrf_pair_bf16": (_i32, [_c.POINTER(_vp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp),
                                            _c.POINTER(_vp), _i32, _i32, _i32, _i32, _c.POINTER(_i32), _c.POINTER(_i32), _f, _vp]),
    "iris_hifigan_op_mrf_pair_mean_bf16": (_i32, [_c.POINTER(_vp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp), _c.POINTER(_fp),
                                                 _vp, _i32, _i32, _i32, _i32, _c.POINTER(_i32), _c.POINTER(_i32), _f, _vp]),
    "iris_hifigan_op_conv1d_bf16": (_i32, [_vp, _fp, _fp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_conv_transpose1d_bf16": (_i32, [_vp, _fp, _fp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_conv1d_f32s": (_i32, [_vp, _fp, _fp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_hifigan_op_conv_transpose1d_f32s": (_i32, [_vp, _fp, _fp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f, _vp]),
    "iris_postnet_create": (_i32, [_i32, _i32, _i32, _i32, _fp, _u64, _c.POINTER(_vp)]),
    "iris_postnet_destroy": (_i32, [_vp]),
    "iris_postnet_workspace_bytes": (_i32, [_vp, _i32, _i32, _c.POINTER(_u64)]),
    "iris_postnet_forward": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _u64, _vp]),
    "iris_postnet_forward_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
}

# the sample-rate conversion stage (iris.resample): bound by load() like SYMBOLS
_i64, _d = _c.c_int64, _c.c_double
_ip, _i64p = _c.POINTER(_i32), _c.POINTER(_i64)
RESAMPLER_SYMBOLS = {
    "iris_resampler_design": (_i32, [_i32, _i32, _i32, _d, _d, _ip, _ip, _ip, _fp, _u64]),
    "iris_resampler_create": (_i32, [_i32, _i32, _i32, _d, _d, _c.POINTER(_vp)]),
    "iris_resampler_destroy": (_i32, [_vp]),
    "iris_resampler_info": (_i32, [_vp, _ip, _ip, _ip, _ip]),
    "iris_resampler_out_range": (_i32, [_vp, _i64, _i64, _i64p, _i64p]),
    "iris_resampler_forward": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _f, _vp]),
}

# its window form and its G.711 store form (iris.resample: ResamplerSession, forward(encoding=)): bound by load() like SYMBOLS,
# and kept apart from RESAMPLER_SYMBOLS, which stays the stage's first six functions
RESAMPLER_WINDOW_SYMBOLS = {
    "iris_resampler_forward_g711": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _i64, _i32, _vp, _vp]),
    "iris_resampler_window_plan": (_i32, [_vp, _i64, _i64, _i64, _i32, _i64p, _i64p]),
    "iris_resampler_forward_window": (_i32, [_vp, _vp, _i32, _i32, _i64, _i64, _i32, _vp, _i32, _vp]),
}

# output forms of the resampler's window and G.711 entry points (include/iris_hifigan.h: IRIS_OUT_*)
OUT_F32, OUT_PCM16, OUT_ULAW, OUT_ALAW = 0, 1, 3, 4
OUT_FORMS = {"f32": OUT_F32, "pcm16": OUT_PCM16, "ulaw": OUT_ULAW, "alaw": OUT_ALAW}



class VaeDecoderConfig(ctypes.Structure):
    """``iris_vae_decoder_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("n_mels", "cond_dim", "model_channels", "latent_dim", "decoder_blocks",
                                             "wavenet_kernel_size", "down_stages", "flow_layers", "flow_hidden")]


VAE_TAP_LAT_COND, VAE_TAP_DEC_IN, VAE_TAP_DEC_OUT = 0, 1, 2

# the VAE decoder stage (iris.vae): bound by load() like SYMBOLS
_u64p = _c.POINTER(_u64)
VAE_SYMBOLS = {
    "iris_vae_decoder_weight_count": (_i32, [_c.POINTER(VaeDecoderConfig), _u64p]),
    "iris_vae_decoder_create": (_i32, [_c.POINTER(VaeDecoderConfig), _fp, _u64, _c.POINTER(_vp)]),
    "iris_vae_decoder_destroy": (_i32, [_vp]),
    "iris_vae_decoder_workspace_bytes": (_i32, [_vp, _i32, _i32, _u64p]),
    "iris_vae_decoder_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_vae_decoder_forward_ragged": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "iris_vae_decoder_forward_posterior": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_vae_decoder_forward_posterior_ragged": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "iris_vae_decoder_launch_count": (_i32, [_vp, _i32, _i32, _ip]),
    "iris_vae_decoder_tap": (_i32, [_vp, _i32, _i32, _i32, _u64p, _u64p]),
}


class VaeEncoderConfig(ctypes.Structure):
    """``iris_vae_encoder_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("n_mels", "cond_dim", "model_channels", "latent_dim", "num_wavenet_blocks",
                                             "wavenet_kernel_size", "down_stages")]


VAE_ENC_TAP_H_IN, VAE_ENC_TAP_H_OUT, VAE_ENC_TAP_LAT_H = 0, 1, 2

# the VAE posterior encoder stage (iris.vae.VAEPosteriorEncoder): bound by load() like SYMBOLS
VAE_ENCODER_SYMBOLS = {
    "iris_vae_encoder_weight_count": (_i32, [_c.POINTER(VaeEncoderConfig), _u64p]),
    "iris_vae_encoder_create": (_i32, [_c.POINTER(VaeEncoderConfig), _fp, _u64, _c.POINTER(_vp)]),
    "iris_vae_encoder_destroy": (_i32, [_vp]),
    "iris_vae_encoder_workspace_bytes": (_i32, [_vp, _i32, _i32, _u64p]),
    "iris_vae_encoder_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_vae_encoder_launch_count": (_i32, [_vp, _i32, _i32, _ip]),
    "iris_vae_encoder_tap": (_i32, [_vp, _i32, _i32, _i32, _u64p, _u64p]),
}

# the ragged forward of the posterior encoder (iris.vae: encode_device(lengths=)): bound by load() like SYMBOLS.  It takes an
# iris_vae_encoder handle but is named outside the iris_vae_encoder_* family, which keeps its seven functions.
VAE_POSTERIOR_SYMBOLS = {
    "iris_vae_posterior_encode_ragged": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
}

# the masked VAE losses (iris.vae.vae_losses): bound by load() like SYMBOLS
VAE_LOSSES_SYMBOLS = {
    "iris_vae_losses_workspace_bytes": (_i32, [_i32, _i32, _i32, _i32, _i32, _u64p]),
    "iris_vae_losses": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
}


class PhonemeEncoderConfig(ctypes.Structure):
    """``iris_phoneme_encoder_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("vocab_size", "embed_dim", "num_blocks", "num_heads", "ffn_dim", "max_length")]


class DurationPredictorConfig(ctypes.Structure):
    """``iris_duration_predictor_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("in_dim", "hidden_dim", "num_layers", "kernel_size", "max_frames_per_phoneme")]


# the text stage (iris.encoder): bound by load() like SYMBOLS
_pec, _dpc = _c.POINTER(PhonemeEncoderConfig), _c.POINTER(DurationPredictorConfig)
TEXT_SYMBOLS = {
    "iris_phoneme_encoder_weight_count": (_i32, [_pec, _u64p]),
    "iris_phoneme_encoder_workspace_bytes": (_i32, [_pec, _i32, _i32, _u64p]),
    "iris_phoneme_encoder_launch_count": (_i32, [_pec, _i32, _i32, _ip]),
    "iris_phoneme_encoder_create": (_i32, [_pec, _fp, _u64, _c.POINTER(_vp)]),
    "iris_phoneme_encoder_destroy": (_i32, [_vp]),
    "iris_phoneme_encoder_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _u64, _vp]),
    "iris_phoneme_encoder_tap": (_i32, [_pec, _i32, _i32, _u64p, _u64p]),
    "iris_duration_predictor_weight_count": (_i32, [_dpc, _u64p]),
    "iris_duration_predictor_workspace_bytes": (_i32, [_dpc, _i32, _i32, _u64p]),
    "iris_duration_predictor_launch_count": (_i32, [_dpc, _i32, _i32, _ip]),
    "iris_duration_predictor_create": (_i32, [_dpc, _fp, _u64, _c.POINTER(_vp)]),
    "iris_duration_predictor_destroy": (_i32, [_vp]),
    "iris_duration_predictor_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "iris_duration_predictor_tap": (_i32, [_dpc, _i32, _i32, _u64p, _u64p]),
    "iris_length_scan": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "iris_length_regulate": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
}



class MelFrontendConfig(ctypes.Structure):
    """``iris_mel_frontend_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "n_fft", "hop_length", "win_length", "n_mels", "reserved")] + [
        ("fmin", ctypes.c_double), ("fmax", ctypes.c_double)]


MEL_SAMPLES_F32, MEL_SAMPLES_I16 = 0, 1

# the mel front-end (iris.mel): bound by load() like SYMBOLS
_mfc = _c.POINTER(MelFrontendConfig)
MEL_SYMBOLS = {
    "iris_mel_frontend_design": (_i32, [_mfc, _ip, _fp, _u64, _fp, _u64]),
    "iris_mel_frontend_workspace_bytes": (_i32, [_mfc, _i32, _i32, _u64p]),
    "iris_mel_frontend_launch_count": (_i32, [_mfc, _i32, _i32, _ip]),
    "iris_mel_frontend_create": (_i32, [_mfc, _c.POINTER(_vp)]),
    "iris_mel_frontend_destroy": (_i32, [_vp]),
    "iris_mel_frontend_forward": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _u64, _vp]),
    "iris_mel_frontend_forward_ragged": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
}


class GriffinLimConfig(ctypes.Structure):
    """``iris_griffin_lim_config``"""

    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "n_fft", "hop_length", "win_length", "n_mels", "n_iter")] + [
        ("fmin", ctypes.c_double), ("fmax", ctypes.c_double), ("nnls_iters", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("momentum", ctypes.c_double), ("nnls_step", ctypes.c_double)]


# the Griffin-Lim vocoder (iris.griffin_lim): bound by load() like SYMBOLS
_glc = _c.POINTER(GriffinLimConfig)
GRIFFIN_LIM_SYMBOLS = {
    "iris_griffin_lim_design": (_i32, [_glc, _ip, _fp, _u64, _fp, _u64, _fp, _u64, _fp, _u64]),
    "iris_griffin_lim_workspace_bytes": (_i32, [_glc, _i32, _i32, _u64p]),
    "iris_griffin_lim_launch_count": (_i32, [_glc, _i32, _i32, _ip]),
    "iris_griffin_lim_create": (_i32, [_glc, _fp, _u64, _c.POINTER(_vp)]),
    "iris_griffin_lim_destroy": (_i32, [_vp]),
    "iris_griffin_lim_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _u64, _vp]),
    "iris_griffin_lim_forward_ragged": (_i32, [_vp, _vp, _vp, _u64, _i32, _i32, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_griffin_lim_draw_phase": (_i32, [_vp, _u64, _i32, _i32, _i32, _vp, _vp]),
}

# the bias denoiser (iris.denoiser): bound by load() like SYMBOLS; it takes the mel front-end's config
DENOISER_SYMBOLS = {
    "iris_denoiser_workspace_bytes": (_i32, [_mfc, _i32, _i32, _u64p]),
    "iris_denoiser_launch_count": (_i32, [_mfc, _i32, _i32, _ip]),
    "iris_denoiser_estimate_launch_count": (_i32, [_mfc, _i32, _ip]),
    "iris_denoiser_create": (_i32, [_mfc, _fp, _c.POINTER(_vp)]),
    "iris_denoiser_destroy": (_i32, [_vp]),
    "iris_denoiser_set_bias": (_i32, [_vp, _vp, _vp]),
    "iris_denoiser_estimate_bias": (_i32, [_vp, _vp, _i32, _vp, _vp, _u64, _vp]),
    "iris_denoiser_forward": (_i32, [_vp, _vp, _i32, _i32, _vp, _f, _vp, _vp, _u64, _vp]),
    "iris_denoiser_window_range": (_i32, [_mfc, _i64, _i32, _i32, _i64p, _i64p]),
    "iris_denoiser_window_workspace_bytes": (_i32, [_mfc, _i32, _i32, _u64p]),
    "iris_denoiser_window_launch_count": (_i32, [_mfc, _i32, _i32, _i64, _i32, _ip]),
    "iris_denoiser_forward_window": (_i32, [_vp, _vp, _i32, _i32, _i64, _i32, _f, _vp, _vp, _u64, _vp]),
}

# the time stretch (iris.time_stretch): bound by load() like SYMBOLS; it takes the mel front-end's config and a double rate
TIME_STRETCH_SYMBOLS = {
    "iris_time_stretch_out_samples": (_i32, [_mfc, _i32, _d, _ip, _ip]),
    "iris_time_stretch_workspace_bytes": (_i32, [_mfc, _i32, _i32, _d, _u64p]),
    "iris_time_stretch_launch_count": (_i32, [_mfc, _i32, _i32, _d, _ip]),
    "iris_time_stretch_create": (_i32, [_mfc, _c.POINTER(_vp)]),
    "iris_time_stretch_destroy": (_i32, [_vp]),
    "iris_time_stretch_forward": (_i32, [_vp, _vp, _i32, _i32, _d, _vp, _vp, _u64, _vp]),
    "iris_time_stretch_forward_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _d, _vp, _vp, _vp, _u64, _vp]),
    "iris_time_stretch_state_bytes": (_i32, [_mfc, _i32, _u64p]),
    "iris_time_stretch_window_plan": (_i32, [_mfc, _d, _i64, _i32, _i32, _i64, _i64p, _i64p, _i64p, _i64p]),
    "iris_time_stretch_window_workspace_bytes": (_i32, [_mfc, _i32, _i32, _d, _u64p]),
    "iris_time_stretch_window_launch_count": (_i32, [_mfc, _i32, _i32, _d, _i64, _i32, _i64, _ip]),
    "iris_time_stretch_forward_window": (_i32, [_vp, _vp, _i32, _i32, _i64, _i32, _d, _i64, _vp, _vp, _vp, _u64, _vp]),
}



class AssembleConfig(ctypes.Structure):
    """``iris_assemble_config``"""

    _fields_ = [("frame_length", ctypes.c_int32), ("hop_length", ctypes.c_int32), ("top_db", ctypes.c_float), ("ref", ctypes.c_float),
                ("pad_samples", ctypes.c_int32), ("fade_samples", ctypes.c_int32), ("pause_samples", ctypes.c_int32)]


# silence trim and sentence join (iris.assemble): bound by load() like SYMBOLS
_asc = _c.POINTER(AssembleConfig)
ASSEMBLE_SYMBOLS = {
    "iris_assemble_out_capacity": (_i32, [_asc, _i32, _i32, _i64p]),
    "iris_assemble_workspace_bytes": (_i32, [_asc, _i32, _i32, _u64p]),
    "iris_assemble_launch_count": (_i32, [_asc, _i32, _i32, _ip]),
    "iris_assemble_create": (_i32, [_asc, _c.POINTER(_vp)]),
    "iris_assemble_destroy": (_i32, [_vp]),
    "iris_assemble_forward": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
    "iris_assemble_trim_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
}


class LoudnessConfig(ctypes.Structure):
    """``iris_loudness_config``"""

    _fields_ = [("sample_rate", ctypes.c_int32), ("target_lufs", ctypes.c_float), ("max_gain_db", ctypes.c_float),
                ("peak_ceiling", ctypes.c_float)]


# BS.1770 loudness and the gain to a target (iris.loudness): bound by load() like SYMBOLS
LOUDNESS_DESIGN_DOUBLES = 144
_ldc = _c.POINTER(LoudnessConfig)
LOUDNESS_SYMBOLS = {
    "iris_loudness_design": (_i32, [_ldc, _c.POINTER(_d), _u64]),
    "iris_loudness_workspace_bytes": (_i32, [_ldc, _i32, _i32, _u64p]),
    "iris_loudness_launch_count": (_i32, [_ldc, _i32, _i32, _i32, _ip]),
    "iris_loudness_create": (_i32, [_ldc, _c.POINTER(_vp)]),
    "iris_loudness_destroy": (_i32, [_vp]),
    "iris_loudness_normalize_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_loudness_measure_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _u64, _vp]),
}



class LimiterConfig(ctypes.Structure):
    """``iris_limiter_config``"""

    _fields_ = [("ceiling", ctypes.c_float), ("lookahead", ctypes.c_int32)]


# the look-ahead true-peak limiter (iris.limiter): bound by load() like SYMBOLS
LIMITER_BANK_FLOATS = 36
_lmc = _c.POINTER(LimiterConfig)
LIMITER_SYMBOLS = {
    "iris_limiter_design": (_i32, [_lmc, _fp, _u64]),
    "iris_limiter_workspace_bytes": (_i32, [_lmc, _i32, _i32, _u64p]),
    "iris_limiter_launch_count": (_i32, [_lmc, _i32, _i32, _i32, _ip]),
    "iris_limiter_create": (_i32, [_lmc, _c.POINTER(_vp)]),
    "iris_limiter_destroy": (_i32, [_vp]),
    "iris_limiter_forward_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _u64, _vp]),
    "iris_limiter_measure_ragged": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _u64, _vp]),
    "iris_limiter_window_range": (_i32, [_lmc, _i64, _i32, _i32, _i64p, _i64p]),
    "iris_limiter_window_workspace_bytes": (_i32, [_lmc, _i32, _i32, _u64p]),
    "iris_limiter_window_launch_count": (_i32, [_lmc, _i32, _i32, _i64, _i32, _ip]),
    "iris_limiter_forward_window": (_i32, [_vp, _vp, _i32, _i32, _i64, _i32, _vp, _i32, _vp, _vp, _u64, _vp]),
}


class LimiterWindowItem(ctypes.Structure):
    """``iris_limiter_window_item``"""

    _fields_ = [("origin", ctypes.c_int64), ("Lw", ctypes.c_int32), ("final", ctypes.c_int32)]


class ResamplerWindowItem(ctypes.Structure):
    """``iris_resampler_window_item``"""

    _fields_ = [("origin", ctypes.c_int64), ("n_next", ctypes.c_int64), ("Lw", ctypes.c_int32), ("final", ctypes.c_int32)]


# groups of windows, one utterance per row (iris.stream_group): bound by load() like SYMBOLS, and kept apart from LIMITER_SYMBOLS
# and RESAMPLER_WINDOW_SYMBOLS, which stay the one-utterance forms
WINDOW_GROUP_MAX = 64                           # include/iris_hifigan.h: IRIS_WINDOW_GROUP_MAX
_lwi, _rwi = _c.POINTER(LimiterWindowItem), _c.POINTER(ResamplerWindowItem)
WINDOW_GROUP_SYMBOLS = {
    "iris_limiter_windows_workspace_bytes": (_i32, [_lmc, _i32, _i32, _u64p]),
    "iris_limiter_windows_launch_count": (_i32, [_lmc, _i32, _lwi, _ip]),
    "iris_limiter_forward_windows": (_i32, [_vp, _vp, _i32, _i32, _lwi, _vp, _i32, _i32, _vp, _vp, _u64, _vp]),
    "iris_resampler_forward_windows": (_i32, [_vp, _vp, _i32, _i32, _rwi, _vp, _i32, _i32, _vp]),
}

# the spectral-distance stage (iris.metrics): bound by load() like SYMBOLS; its config is a host array [n_res][3] of int32
SPECTRAL_DISTANCE_MAX_RES = 4                   # csrc/spectral_distance.h: kMaxRes
SPECTRAL_DISTANCE_SYMBOLS = {
    "iris_spectral_distance_workspace_bytes": (_i32, [_ip, _i32, _i32, _i32, _u64p]),
    "iris_spectral_distance_launch_count": (_i32, [_ip, _i32, _i32, _i32, _ip]),
    "iris_spectral_distance_create": (_i32, [_ip, _i32, _c.POINTER(_vp)]),
    "iris_spectral_distance_destroy": (_i32, [_vp]),
    "iris_spectral_distance_forward": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _u64, _vp]),
}

_lib: Optional[ctypes.CDLL] = None


def library_path() -> Path:
    override = os.environ.get("IRIS_HIFIGAN_LIB")
    return Path(override) if override else CSRC_DIR / LIB_NAME


def load() -> ctypes.CDLL:
    """Loads (once) and returns the library with typed entry points."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not path.exists():
        raise NativeLibraryError(
            f"HIP extension not built: {path} is missing. Build it with "
            f"`make -C {CSRC_DIR}` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the vocoder path.")
    try:
        # torch must own the process's HIP runtime first so that both see the same libamdhip64
        import torch  # noqa: F401
        lib = ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL)
    except OSError as exc:
        raise NativeLibraryError(f"could not load {path}: {exc}") from exc
    for name, (restype, argtypes) in {**SYMBOLS, **RESAMPLER_SYMBOLS, **RESAMPLER_WINDOW_SYMBOLS, **VAE_SYMBOLS, **VAE_ENCODER_SYMBOLS, **VAE_POSTERIOR_SYMBOLS, **VAE_LOSSES_SYMBOLS, **TEXT_SYMBOLS, **MEL_SYMBOLS,
                                      **GRIFFIN_LIM_SYMBOLS, **DENOISER_SYMBOLS, **TIME_STRETCH_SYMBOLS, **ASSEMBLE_SYMBOLS,
                                      **LOUDNESS_SYMBOLS, **LIMITER_SYMBOLS, **WINDOW_GROUP_SYMBOLS, **SPECTRAL_DISTANCE_SYMBOLS}.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise NativeLibraryError(f"{path} does not export {name}; rebuild the extension") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    version = lib.iris_hifigan_abi_version()
    if version != ABI_VERSION:
        raise NativeLibraryError(f"{path} has ABI version {version}, binding expects {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(fn_name: str, status: int) -> None:
    if status != 0:
        msg = load().iris_hifigan_last_error()
        raise NativeCallError(fn_name, status, msg.decode("utf-8", "replace") if msg else "")


def describe_plan(cfg, batch: int, frames: int, dtype_code: int = DTYPE_F32, cu_count: int = 0) -> dict:
    """Launch plan of one forward, computed on the host alone (``iris_hifigan_describe_plan``: no device needed,
    nothing is launched): workspace bytes and, per launch, kernel name, grid, block and dynamic LDS."""
    lib = load()
    plan = Plan()
    ccfg = make_config(cfg)
    check("iris_hifigan_describe_plan", lib.iris_hifigan_describe_plan(ctypes.byref(ccfg), batch, frames, dtype_code, cu_count,
                                                                       ctypes.byref(plan)))
    n = min(plan.n_launches, MAX_PLAN_LAUNCHES)
    return {"workspace_bytes": int(plan.workspace_bytes), "n_launches": int(plan.n_launches), "cu_count": int(plan.cu_count),
            "passes": int(plan.passes),
            "launches": [{"kernel": plan.launches[i].kernel.decode(), "grid": tuple(plan.launches[i].grid),
                          "block": int(plan.launches[i].block), "lds_bytes": int(plan.launches[i].lds_bytes)} for i in range(n)]}


def make_config(cfg) -> Config:
    """``GeneratorConfig`` -> ``iris_hifigan_config`` (validates the fixed-size limits)."""
    if cfg.num_upsamples > MAX_STAGES:
        raise ValueError(f"at most {MAX_STAGES} upsample stages are supported, got {cfg.num_upsamples}")
    if cfg.num_kernels > MAX_KERNELS:
        raise ValueError(f"at most {MAX_KERNELS} MRF kernels are supported, got {cfg.num_kernels}")
    c = Config()
    c.in_channels = cfg.in_channels
    c.upsample_initial_channel = cfg.upsample_initial_channel
    c.num_upsamples = cfg.num_upsamples
    for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        c.upsample_rates[i] = u
        c.upsample_kernel_sizes[i] = k
    c.num_kernels = cfg.num_kernels
    for j, (k, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
        if len(dils) > MAX_DILATIONS:
            raise ValueError(f"at most {MAX_DILATIONS} dilations per ResBlock are supported")
        c.resblock_kernel_sizes[j] = k
        c.num_dilations[j] = len(dils)
        for m, d in enumerate(dils):
            c.resblock_dilations[j][m] = d
    c.pre_kernel_size = cfg.pre_kernel_size
    c.post_kernel_size = cfg.post_kernel_size
    c.lrelu_slope = cfg.lrelu_slope
    return c
