"""ctypes binding of ``include/ls_hip.h`` (the C-ABI of the gfx950 engine).

There is deliberately NO fallback: if ``libls_hip.so`` is missing or fails to load, importing the
engine raises; nothing in the product path ever routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)

LS_SAMPLER_DDPM, LS_SAMPLER_DDIM, LS_SAMPLER_PLMS, LS_SAMPLER_DDIM_REVERSE = 0, 1, 2, 3
LS_NOISE_TAPE, LS_NOISE_PHILOX, LS_NOISE_TORCH_DEVICE = 0, 1, 2
LS_PRECISION_FP32, LS_PRECISION_BF16X3 = 0, 1


class LsConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("njoints", "nfeats", "nframes", "n_prefix_tokens", "n_pre_seq",
                                         "latent_dim", "layers", "audio_len", "n_speakers", "n_emotions",
                                         "device", "reserved")]


class LsSchedule(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("reserved", C.c_int32), ("timestep_map", c_i64p)] + [
        (n, c_f64p) for n in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod", "posterior_mean_coef1",
                              "posterior_mean_coef2", "posterior_log_variance_clipped", "alphas_cumprod",
                              "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")]


class LsCond(C.Structure):
    _fields_ = [("batch", C.c_int32), ("on_device", C.c_int32), ("audio_input", C.c_void_p),
                ("origin_x", C.c_void_p), ("vid_indices", C.c_void_p), ("emo", C.c_void_p), ("scale", C.c_void_p)]


class LsSampleArgs(C.Structure):
    _fields_ = [("sampler", C.c_int32), ("noise_mode", C.c_int32), ("skip_timesteps", C.c_int32),
                ("const_noise", C.c_int32), ("on_device", C.c_int32), ("use_graph", C.c_int32),
                ("clip_denoised", C.c_int32), ("two_pass_always", C.c_int32), ("eta", C.c_float), ("n_dump", C.c_int32), ("dump_steps", c_i32p), ("dump_out", C.c_void_p),
                ("x_init", C.c_void_p), ("init_image", C.c_void_p), ("eps_tape", C.c_void_p),
                ("noise_tape", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
                ("out", C.c_void_p), ("seg_begin", C.c_int32), ("seg_count", C.c_int32), ("inpaint_mask", C.c_void_p),
                ("inpainted_motion", C.c_void_p), ("inpaint_noise", C.c_void_p), ("inpaint_noised", C.c_int32), ("plms_order", C.c_int32)]


class LsLongCond(C.Structure):
    _fields_ = [("batch", C.c_int32), ("n_windows", C.c_int32), ("on_device", C.c_int32), ("encoder_chunk", C.c_int32),
                ("audio_samples", C.c_int64), ("audio", C.c_void_p), ("seed_poses", C.c_void_p), ("vid_indices", C.c_void_p),
                ("emo", C.c_void_p), ("scale", C.c_void_p)]


class LsLongSampleArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised",
                                         "two_pass_always")] + [
        ("eta", C.c_float), ("x_init", C.c_void_p), ("eps_tape", C.c_void_p), ("noise_tape", C.c_void_p), ("seed", C.c_uint64),
        ("sample_offset", C.c_uint64), ("sag", C.c_void_p), ("text_features", C.c_void_p), ("timeline", C.c_void_p), ("windows", C.c_void_p)]


class LsLongEditArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised",
                                         "two_pass_always")] + [
        ("eta", C.c_float), ("inpaint_noised", C.c_int32), ("windows_capacity", C.c_int32), ("frame_lo", c_i32p), ("frame_hi", c_i32p),
        ("channels", C.c_void_p), ("timeline", C.c_void_p), ("windows", C.c_void_p), ("windows_run", c_i32p), ("n_windows_run", c_i32p),
        ("x_init", C.c_void_p), ("eps_tape", C.c_void_p), ("noise_tape", C.c_void_p), ("inpaint_noise", C.c_void_p),
        ("seed", C.c_uint64), ("sample_offset", C.c_uint64)]


class LsLongEditCompactArgs(C.Structure):
    _fields_ = LsLongEditArgs._fields_ + [("rows_run", c_i32p)]


class LsLongStreamCond(C.Structure):
    _fields_ = [("batch", C.c_int32), ("on_device", C.c_int32), ("seed_poses", C.c_void_p), ("vid_indices", C.c_void_p), ("scale", C.c_void_p)]


class LsLongStreamPushArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised",
                                         "two_pass_always")] + [
        ("eta", C.c_float), ("closing", C.c_int32), ("capacity", C.c_int32), ("n_samples", C.c_int64), ("audio", C.c_void_p),
        ("emo", C.c_void_p), ("sag", C.c_void_p), ("text_features", C.c_void_p), ("x_init", C.c_void_p), ("eps_tape", C.c_void_p),
        ("noise_tape", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64), ("frames", C.c_void_p),
        ("n_frames", c_i32p), ("n_windows", c_i32p)]


class LsLongPoolJoinArgs(C.Structure):
    _fields_ = [("slot", C.c_int32), ("on_device", C.c_int32), ("seed_poses", C.c_void_p), ("vid_index", C.c_void_p), ("scale", C.c_void_p),
                ("emo", C.c_void_p), ("text_features", C.c_void_p)]


class LsLongPoolPushArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sampler", "noise_mode", "skip_timesteps", "on_device", "use_graph", "clip_denoised",
                                         "two_pass_always")] + [
        ("eta", C.c_float), ("capacity", C.c_int32), ("reserved", C.c_int32), ("n_max", C.c_int64), ("audio", C.c_void_p),
        ("lengths", c_i64p), ("closing", c_i32p), ("given", c_i32p), ("emo", C.c_void_p), ("sag", C.c_void_p), ("text_features", C.c_void_p),
        ("x_init", C.c_void_p), ("eps_tape", C.c_void_p), ("noise_tape", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("frames", C.c_void_p), ("n_frames", c_i32p), ("n_rounds", c_i32p)]


class LsForwardArgs(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("no_sync", C.c_int32), ("x", C.c_void_p), ("timesteps", C.c_void_p),
                ("eps_cond", C.c_void_p), ("eps_uncond", C.c_void_p), ("out_cond", C.c_void_p),
                ("out_uncond", C.c_void_p), ("out_cfg", C.c_void_p), ("trace", C.c_void_p)]


class LsStepArgs(C.Structure):
    _fields_ = [("sampler", C.c_int32), ("index", C.c_int32), ("on_device", C.c_int32), ("eta", C.c_float),
                ("clip_denoised", C.c_int32), ("two_pass_always", C.c_int32), ("x", C.c_void_p), ("eps_cond", C.c_void_p), ("eps_uncond", C.c_void_p), ("noise", C.c_void_p),
                ("sample", C.c_void_p), ("pred_xstart", C.c_void_p), ("indices", C.c_void_p), ("no_sync", C.c_int32),
                ("indices_on_device", C.c_int32), ("inpaint_mask", C.c_void_p), ("inpainted_motion", C.c_void_p), ("inpaint_noise", C.c_void_p)]


class LsPlmsStepArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("index", "order", "n_hist", "on_device", "clip_denoised", "two_pass_always", "no_sync", "reserved")] + [
        ("x", C.c_void_p), ("eps_cond", C.c_void_p), ("eps_uncond", C.c_void_p), ("eps_cond2", C.c_void_p), ("eps_uncond2", C.c_void_p),
        ("hist", C.c_void_p * 3), ("sample", C.c_void_p), ("pred_xstart", C.c_void_p), ("eps_out", C.c_void_p)]


class LsVbTermsArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("index", "on_device", "indices_on_device", "clip_denoised")] + [
        (n, C.c_void_p) for n in ("indices", "x_start", "x_t", "pred_xstart", "noise", "vb_out", "xstart_mse_out", "mse_out", "pred_out")]


class LsBpdArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("noise_mode", "on_device", "use_graph", "clip_denoised", "two_pass_always", "col_begin", "col_count",
                                         "reserved")] + [("x_start", C.c_void_p), ("noise_tape", C.c_void_p), ("eps_tape", C.c_void_p),
                                                         ("seed", C.c_uint64), ("sample_offset", C.c_uint64), ("vb", C.c_void_p),
                                                         ("xstart_mse", C.c_void_p), ("mse", C.c_void_p)]


class LsSagConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("njoints", "nfeats", "nframes", "latent_dim", "ff_size", "num_layers",
                                         "num_heads", "n_pre_poses", "device", "reserved")]


class LsClipTextConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("device", "vocab_size", "context_length", "width", "heads", "layers", "embed_dim")]


class LsPostConfig(C.Structure):
    _fields_ = [("njoints", C.c_int32), ("n_pairs", C.c_int32), ("n_pose_joints", C.c_int32), ("thres", C.c_float),
                ("pair_a", C.c_int32 * 8), ("pair_b", C.c_int32 * 8), ("change_angle", C.c_float * 8),
                ("bone_parent", C.c_int32 * 16), ("bone_child", C.c_int32 * 16), ("bone_len", C.c_float * 16),
                ("mean_dir_vec", C.c_float * 48)]


class LsBeatMetricsArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "njoints", "on_device", "order", "align_series", "reserved")] + [
        ("series_joint", C.c_int32 * 6)] + [(n, C.c_float) for n in ("threshold", "scale", "sigma", "fps")] + [
        (n, C.c_void_p) for n in ("pred", "target", "semantic", "onset_times", "onset_offsets", "success", "srgr_sum", "vel",
                                  "beat_mask", "align")]


class LsOnsetsArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "length", "on_device", "pad_mode")] + [
        (n, C.c_float) for n in ("sr", "sr_pick", "fmax", "delta")] + [
        (n, C.c_void_p) for n in ("audio", "envelope", "mel_db", "rms", "oenv", "count", "onset_raw", "onset_bt", "onset_bt_rms",
                                  "kernel_ms")]


class LsTedAlignArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "n_frames", "on_device", "onset_cols")] + [
        (n, C.c_double) for n in ("fps", "sigma", "sr")] + [("hop", C.c_int32), ("reserved", C.c_int32)] + [
        (n, C.c_void_p) for n in ("beat_mask", "onset_frames", "onset_count", "align_sum", "n_beats")]


class LsPostStreamPushArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("on_device", "K", "beat_capacity", "reserved")] + [
        (n, C.c_void_p) for n in ("frames", "counts", "finish", "aligned", "pose", "angle_diff", "decoded", "euler_deg", "beat_mask",
                                  "beat_first", "beat_count")]


class LsIngestPlanArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "n_poses", "n_ext", "stride", "beat", "frame_cap", "window_cap", "n_frames",
                                         "n_windows", "reserved")] + [("fps", C.c_double), ("sr", C.c_double)] + [
        (n, C.c_void_p) for n in ("n_raw", "start_time", "end_time", "audio_len", "word_offsets", "word_times", "frame_offsets",
                                  "frame_clip", "frame_lo", "frame_hi", "frame_frac", "window_offsets", "win_clip", "win_first",
                                  "win_audio_start", "win_n_pad", "win_has_words")]


class LsTedIngestArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "on_device", "n_poses", "n_ext", "n_frames", "n_windows", "audio_out_len",
                                         "reserved")] + [("cfg", C.POINTER(LsPostConfig))] + [
        (n, C.c_void_p) for n in ("mean_pose", "n_raw", "audio_len", "frame_offsets", "frame_clip", "frame_lo", "frame_hi",
                                  "frame_frac", "win_clip", "win_first", "win_audio_start", "win_has_words", "raw_poses", "audio",
                                  "resampled", "dir_vec", "pose_seq", "vec_seq", "x", "audio_out", "stats", "verdict")]


class LsBeatIngestArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "on_device", "n_poses", "njoints", "n_windows", "audio_out_len")] + [
        (n, C.c_void_p) for n in ("mean_pose", "std_pose", "n_raw", "audio_len", "win_clip", "win_first", "win_audio_start",
                                  "win_has_words", "poses", "audio", "rot6d", "x", "audio_out", "verdict")]


class LsTiming(C.Structure):
    _fields_ = [("prepare_ms", C.c_float), ("loop_ms", C.c_float), ("total_ms", C.c_float),
                ("n_step_launches", C.c_int32), ("graph_replayed", C.c_int32), ("single_pass", C.c_int32),
                ("tape_upload_ms", C.c_float), ("n_segments", C.c_int32), ("step_path", C.c_int32),
                ("tail_samples", C.c_int32), ("tail_path", C.c_int32), ("tail2_samples", C.c_int32), ("tail2_path", C.c_int32), ("n_cus", C.c_int32), ("coop_slices", C.c_int32)]


class LsTrainConfig(C.Structure):
    _fields_ = [("model", LsConfig), ("lambda_vel", C.c_float), ("kld_weight", C.c_float), ("diffusion_steps", C.c_int32),
                ("reserved", C.c_int32)]


class LsTrainBatch(C.Structure):
    _fields_ = [("batch", C.c_int32), ("on_device", C.c_int32), ("x_start", C.c_void_p), ("t", C.c_void_p), ("noise", C.c_void_p),
                ("drop", C.c_void_p), ("eps", C.c_void_p), ("audio_input", C.c_void_p), ("origin_x", C.c_void_p),
                ("vid_indices", C.c_void_p), ("emo", C.c_void_p)]


class LsTrainTerms(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("rot_mse", "vel_mse", "kld", "loss", "total", "fwd_ms", "bwd_ms", "reserved")]


class LsEvalConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("pose_dim", "n_frames", "base", "hidden1", "hidden2", "device")]


class LsScoreConfig(C.Structure):
    _fields_ = [("sr", C.c_float), ("sr_pick", C.c_float), ("pad_mode", C.c_int32), ("fmax", C.c_float), ("delta", C.c_float),
                ("hop", C.c_int32), ("onset_source", C.c_int32), ("max_chunk", C.c_int32), ("fps", C.c_double), ("sigma", C.c_double),
                ("time_rate", C.c_double)]


class LsScoreStreamPushArgs(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("n_max", C.c_int32), ("beat_capacity", C.c_int32), ("reserved", C.c_int32),
                ("audio", C.c_void_p), ("lengths", C.c_void_p), ("beats", C.c_void_p), ("beat_first", C.c_void_p), ("beat_count", C.c_void_p)]


class LsScoreStreamOutputs(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("cols", C.c_int32)] + [(n, C.c_void_p) for n in (
        "n_frames", "count", "onset_raw", "onset_bt", "onset_bt_rms", "oenv", "mel_db", "rms", "align_sum", "n_beats", "align")]


class LsResampleArgs(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("batch", "on_device", "dtype", "channels")] + [
        ("row_stride", C.c_int64), ("audio", C.c_void_p), ("lengths", c_i64p)] + [(n, C.c_int32) for n in ("in_sr", "out_sr", "zeros", "reserved")] + [
        ("beta", C.c_double), ("rolloff", C.c_double), ("out", C.c_void_p), ("out_stride", C.c_int64), ("out_lengths", c_i64p)]


class LsResampleStreamPushArgs(C.Structure):
    _fields_ = [("on_device", C.c_int32), ("n_max", C.c_int32), ("out_capacity", C.c_int64), ("audio", C.c_void_p), ("lengths", c_i32p),
                ("finish", c_i32p), ("out", C.c_void_p), ("out_first", c_i64p), ("out_count", c_i64p)]


EXPORTS = ("ls_abi_version", "ls_create", "ls_destroy", "ls_last_error", "ls_set_weight", "ls_commit_weights",
           "ls_set_schedule", "ls_prepare", "ls_prepare_async", "ls_long_prepare", "ls_long_prepare_ragged", "ls_long_plan_drop", "ls_long_sample", "ls_long_edit_plan", "ls_long_edit", "ls_long_edit_sag", "ls_long_edit_plan_compact", "ls_long_prepare_edit", "ls_long_edit_compact", "ls_long_edit_plan_mask", "ls_long_edit_mask", "ls_long_prepare_edit_mask", "ls_long_edit_compact_mask", "ls_long_edit_mask_pairs", "ls_long_stream_plan", "ls_long_stream_open", "ls_long_stream_push", "ls_long_stream_info", "ls_long_pool_plan", "ls_long_pool_open", "ls_long_pool_join", "ls_long_pool_push", "ls_long_pool_info", "ls_sample", "ls_forward", "ls_step", "ls_plms_step", "ls_q_sample", "ls_vb_terms", "ls_bpd", "ls_read",
           "ls_get_timing", "ls_synchronize", "ls_stream_order", "ls_stream", "ls_sag_stream", "ls_train_stream", "ls_eval_stream", "ls_philox_x_init", "ls_set_row_keys", "ls_long_pool_keyed", "ls_long_pool_set_key", "ls_long_pool_keys", "ls_long_pool_pin_plan", "ls_long_pool_pins", "ls_long_pool_pin", "ls_long_pool_unpin", "ls_long_pool_pin_tape", "ls_long_pool_pin_info", "ls_torch_randn_advance", "ls_torch_randn", "ls_set_torch_ring_bytes", "ls_shard_range", "ls_set_precision", "ls_set_path", "ls_plan_query", "ls_plan_coop_slices", "ls_trng_randn", "ls_trng_fill_steps", "ls_trng_stats", "ls_trng_set_jump", "ls_trng_jump_check", "ls_trng_pairs_debug", "ls_sag_create", "ls_sag_destroy", "ls_sag_last_error",
           "ls_sag_set_weight", "ls_sag_commit_weights", "ls_sag_decode", "ls_sag_decode_async", "ls_sag_last_decode_ms",
           "ls_sag_enc_create", "ls_sag_enc_destroy", "ls_sag_enc_last_error", "ls_sag_enc_set_weight", "ls_sag_enc_commit_weights",
           "ls_sag_enc_encode", "ls_sag_enc_encode_async", "ls_sag_enc_last_encode_ms", "ls_sag_enc_stream",
           "ls_clip_text_create", "ls_clip_text_destroy", "ls_clip_text_last_error", "ls_clip_text_set_weight", "ls_clip_text_commit_weights",
           "ls_clip_text_encode", "ls_clip_text_encode_async", "ls_clip_text_last_encode_ms", "ls_clip_text_stream", "ls_clip_text_plan", "ls_ted_post", "ls_beat_post", "ls_beat_metrics", "ls_beat_ldiv", "ls_onsets", "ls_onsets_tables",
           "ls_ted_post_timeline", "ls_beat_post_timeline", "ls_beat_metrics_timeline", "ls_ted_beat_align",
           "ls_onsets_ragged", "ls_onsets_long", "ls_ted_post_timeline_ragged", "ls_beat_post_timeline_ragged", "ls_beat_metrics_timeline_ragged", "ls_ragged_tiles",
           "ls_post_stream_plan", "ls_post_stream_check", "ls_post_stream_open", "ls_post_stream_push", "ls_post_stream_info", "ls_post_stream_close",
           "ls_post_stream_last_error",
           "ls_score_stream_plan", "ls_score_stream_open", "ls_score_stream_push", "ls_score_stream_finish", "ls_score_stream_info",
           "ls_score_stream_close", "ls_score_stream_last_error",
           "ls_resample_ratio", "ls_resample_plan", "ls_resample_taps", "ls_resample", "ls_resample_stream_open", "ls_resample_stream_push",
           "ls_resample_stream_reset", "ls_resample_stream_info", "ls_resample_stream_close", "ls_resample_stream_last_error",
           "ls_ingest_plan", "ls_ted_ingest", "ls_beat_ingest",
           "ls_train_create", "ls_train_destroy", "ls_train_last_error", "ls_train_set_schedule", "ls_train_param_count",
           "ls_train_flat_size", "ls_train_param_info", "ls_train_set_weight", "ls_train_get_weight", "ls_train_forward_backward",
           "ls_train_adamw", "ls_train_read", "ls_train_get_moment", "ls_train_set_moment", "ls_train_get_step", "ls_train_set_step",
           "ls_eval_create", "ls_eval_destroy", "ls_eval_last_error", "ls_eval_set_weight", "ls_eval_commit_weights", "ls_eval_features")

_lib = None


class EngineError(RuntimeError):
    pass


_lib_override = None


def use_library(path: str) -> None:
    """Developer tooling only (tools/ab_variants.py, tools/phase_profile.py): bind an alternative build of the library.
    Must be called, in code, before the first engine is created; no environment variable selects the binary."""
    global _lib_override
    if _lib is not None:
        raise EngineError("use_library() must be called before the library is loaded")
    _lib_override = os.path.abspath(path)


def library_path() -> str:
    return _lib_override or _build.LIB


def torch_randn_advance(n, n_cu, max_threads_per_cu) -> int:
    """Offset advance of torch's device generator for one float32 ``torch.randn(n)`` (ls_torch_randn_advance; no GPU needed)."""
    return int(load_library().ls_torch_randn_advance(int(n), int(n_cu), int(max_threads_per_cu)))


def load_library(build_if_missing: bool = True):
    """dlopen libls_hip.so (building it in-tree first if it is missing or stale and hipcc is present)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64; if libls_hip.so pulled in /opt/rocm's copy
    # first, torch's later initialisation reports "No HIP GPUs are available".  Importing torch first makes the
    # loader resolve our NEEDED libamdhip64.so.N to the copy torch already mapped (same SONAME).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    path = library_path()
    if build_if_missing and _lib_override is None and _build.is_stale():
        try:
            _build.build_library()
        except Exception as e:      # no hipcc on this box: fall through to whatever .so travelled here
            if not os.path.exists(path):
                raise EngineError(f"libls_hip.so is missing and could not be built: {e}") from e
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: run `python -m livelyspeaker_amd.build` (no CPU fallback exists)")
    lib = C.CDLL(path)
    lib.ls_abi_version.restype = C.c_int
    lib.ls_set_schedule.argtypes = [C.c_void_p, C.POINTER(LsSchedule)]
    lib.ls_prepare.argtypes = [C.c_void_p, C.POINTER(LsCond)]
    lib.ls_prepare_async.argtypes = [C.c_void_p, C.POINTER(LsCond)]
    lib.ls_sample.argtypes = [C.c_void_p, C.POINTER(LsSampleArgs)]
    lib.ls_long_prepare.argtypes = [C.c_void_p, C.POINTER(LsLongCond)]
    lib.ls_long_sample.argtypes = [C.c_void_p, C.POINTER(LsLongSampleArgs)]
    lib.ls_long_prepare_ragged.argtypes = [C.c_void_p, C.POINTER(LsLongCond), C.c_void_p]
    lib.ls_long_plan_drop.argtypes = [C.c_int32, C.c_int32, C.c_void_p, c_i32p, c_i32p, c_i32p, C.c_int32, c_i32p]
    lib.ls_long_edit.argtypes = [C.c_void_p, C.POINTER(LsLongEditArgs)]
    lib.ls_long_edit_sag.argtypes = [C.c_void_p, C.POINTER(LsLongEditArgs), C.c_void_p, C.c_void_p]
    lib.ls_long_edit_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i32p, c_i32p, c_i32p]
    lib.ls_long_edit_plan_compact.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i32p, C.c_void_p, C.c_int32, c_i32p, c_i32p,
                                              c_i32p, C.c_int32, c_i32p, C.c_int32, c_i32p, c_i32p]
    lib.ls_long_prepare_edit.argtypes = [C.c_void_p, C.POINTER(LsLongCond), C.c_void_p, c_i32p, c_i32p, C.c_void_p]
    lib.ls_long_edit_compact.argtypes = [C.c_void_p, C.POINTER(LsLongEditCompactArgs), C.c_void_p, C.c_void_p]
    lib.ls_long_edit_plan_mask.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, c_i32p, c_i32p, c_i32p, C.c_int32,
                                           c_i32p, C.c_int32, c_i32p, c_i32p]
    lib.ls_long_edit_mask.argtypes = [C.c_void_p, C.POINTER(LsLongEditArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_long_prepare_edit_mask.argtypes = [C.c_void_p, C.POINTER(LsLongCond), C.c_void_p, C.c_void_p]
    lib.ls_long_edit_compact_mask.argtypes = [C.c_void_p, C.POINTER(LsLongEditCompactArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_long_edit_mask_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_i32p, C.c_void_p]
    lib.ls_long_stream_plan.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32, c_i64p, c_i64p]
    lib.ls_long_stream_open.argtypes = [C.c_void_p, C.POINTER(LsLongStreamCond)]
    lib.ls_long_stream_push.argtypes = [C.c_void_p, C.POINTER(LsLongStreamPushArgs)]
    lib.ls_long_stream_info.argtypes = [C.c_void_p, c_i64p]
    lib.ls_long_pool_plan.argtypes = [C.c_int32, C.c_int32, c_i64p, c_i64p, c_i64p, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p, C.c_int32, c_i32p, c_i32p]
    lib.ls_long_pool_open.argtypes = [C.c_void_p, C.c_int32]
    lib.ls_long_pool_join.argtypes = [C.c_void_p, C.POINTER(LsLongPoolJoinArgs)]
    lib.ls_long_pool_push.argtypes = [C.c_void_p, C.POINTER(LsLongPoolPushArgs)]
    lib.ls_long_pool_keyed.argtypes = [C.c_void_p, C.c_int32]
    lib.ls_long_pool_set_key.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    lib.ls_long_pool_keys.argtypes = [C.c_int32, C.POINTER(C.c_uint64), c_i64p, c_i32p, C.POINTER(C.c_uint64), C.c_int32, c_i32p]
    lib.ls_long_pool_pin_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, c_i64p, c_i32p, c_i32p, c_i64p, c_i32p, C.c_int32, c_i32p, c_i32p, c_i32p, C.c_int32, c_i32p, c_i32p]
    lib.ls_long_pool_pins.argtypes = [C.c_void_p, C.c_int32]
    lib.ls_long_pool_pin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_i64p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.ls_long_pool_unpin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, c_i64p]
    lib.ls_long_pool_pin_tape.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    lib.ls_long_pool_pin_info.argtypes = [C.c_void_p, C.c_int32, c_i32p, c_i64p]
    lib.ls_set_row_keys.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int32]
    lib.ls_long_pool_info.argtypes = [C.c_void_p, C.c_int32, c_i64p, c_i64p, c_i64p, c_i32p, c_i64p]
    lib.ls_post_stream_plan.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, c_i64p, c_i32p]
    lib.ls_post_stream_check.argtypes = [C.c_int32, C.c_int32, C.c_int32, c_i64p, C.c_int32, c_i32p, c_i32p, C.c_int32, c_i64p, c_i32p]
    lib.ls_post_stream_open.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(LsPostConfig), C.c_int32, C.c_int32, c_i32p, C.POINTER(C.c_void_p)]
    lib.ls_post_stream_push.argtypes = [C.c_void_p, C.POINTER(LsPostStreamPushArgs)]
    lib.ls_post_stream_info.argtypes = [C.c_void_p, c_i64p, c_i64p]
    lib.ls_post_stream_close.argtypes = [C.c_void_p]
    lib.ls_post_stream_close.restype = None
    lib.ls_post_stream_last_error.argtypes = [C.c_void_p]
    lib.ls_post_stream_last_error.restype = C.c_char_p
    lib.ls_score_stream_plan.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int32, c_i64p, c_i32p]
    lib.ls_score_stream_open.argtypes = [C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(LsScoreConfig), C.POINTER(C.c_void_p)]
    lib.ls_score_stream_push.argtypes = [C.c_void_p, C.POINTER(LsScoreStreamPushArgs)]
    lib.ls_score_stream_finish.argtypes = [C.c_void_p, c_i32p, C.POINTER(LsScoreStreamOutputs)]
    lib.ls_score_stream_info.argtypes = [C.c_void_p, c_i64p, c_i64p, c_i64p, c_i64p]
    lib.ls_score_stream_close.argtypes = [C.c_void_p]
    lib.ls_score_stream_close.restype = None
    lib.ls_score_stream_last_error.argtypes = [C.c_void_p]
    lib.ls_score_stream_last_error.restype = C.c_char_p
    lib.ls_resample_ratio.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [c_i64p] * 6
    lib.ls_resample_plan.argtypes = [C.c_int64] * 5 + [C.c_int32, c_i64p, c_i64p]
    lib.ls_resample_taps.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, c_f64p, c_f32p]
    lib.ls_resample.argtypes = [C.c_int, C.POINTER(LsResampleArgs)]
    lib.ls_resample_stream_open.argtypes = [C.c_int] + [C.c_int32] * 6 + [C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_void_p)]
    lib.ls_resample_stream_push.argtypes = [C.c_void_p, C.POINTER(LsResampleStreamPushArgs)]
    lib.ls_resample_stream_reset.argtypes = [C.c_void_p, C.c_int32]
    lib.ls_resample_stream_info.argtypes = [C.c_void_p, c_i64p, c_i64p, c_i64p]
    lib.ls_resample_stream_close.argtypes = [C.c_void_p]
    lib.ls_resample_stream_close.restype = None
    lib.ls_resample_stream_last_error.argtypes = [C.c_void_p]
    lib.ls_resample_stream_last_error.restype = C.c_char_p
    lib.ls_forward.argtypes = [C.c_void_p, C.POINTER(LsForwardArgs)]
    lib.ls_step.argtypes = [C.c_void_p, C.POINTER(LsStepArgs)]
    lib.ls_plms_step.argtypes = [C.c_void_p, C.POINTER(LsPlmsStepArgs)]
    lib.ls_q_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_vb_terms.argtypes = [C.c_void_p, C.POINTER(LsVbTermsArgs)]
    lib.ls_bpd.argtypes = [C.c_void_p, C.POINTER(LsBpdArgs)]
    lib.ls_read.argtypes = [C.c_void_p, C.c_char_p, c_f32p, C.c_size_t]
    lib.ls_read.restype = C.c_longlong
    lib.ls_get_timing.argtypes = [C.c_void_p, C.POINTER(LsTiming)]
    lib.ls_synchronize.argtypes = [C.c_void_p]
    lib.ls_stream_order.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    # what every handle family declares alike (include/ls_hip.h); the trainer has no commit_weights, its set_weight writes the master parameters
    for pre, cfg in (("ls_", LsConfig), ("ls_sag_", LsSagConfig), ("ls_sag_enc_", LsSagConfig), ("ls_clip_text_", LsClipTextConfig),
                     ("ls_train_", LsTrainConfig), ("ls_eval_", LsEvalConfig)):
        def fn(name, pre=pre):
            return getattr(lib, pre + name)
        fn("create").argtypes = [C.POINTER(cfg), C.POINTER(C.c_void_p)]
        fn("destroy").argtypes, fn("destroy").restype = [C.c_void_p], None
        fn("last_error").argtypes, fn("last_error").restype = [C.c_void_p], C.c_char_p
        fn("set_weight").argtypes = [C.c_void_p, C.c_char_p, c_f32p, C.c_size_t]
        if pre != "ls_train_":
            fn("commit_weights").argtypes = [C.c_void_p]
        fn("stream").argtypes, fn("stream").restype = [C.c_void_p], C.c_void_p
    lib.ls_philox_x_init.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    lib.ls_torch_randn_advance.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.ls_torch_randn_advance.restype = C.c_uint64
    lib.ls_torch_randn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p, C.c_int]
    lib.ls_set_torch_ring_bytes.argtypes = [C.c_void_p, C.c_uint64]
    lib.ls_set_precision.argtypes = [C.c_void_p, C.c_int]
    lib.ls_set_path.argtypes = [C.c_void_p, C.c_int]
    lib.ls_plan_query.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    lib.ls_plan_coop_slices.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ls_trng_randn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    lib.ls_trng_fill_steps.argtypes = [C.c_void_p, C.c_size_t] + [C.c_int] * 7 + [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.ls_trng_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.ls_trng_pairs_debug.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
    lib.ls_shard_range.argtypes = [C.c_int64, C.c_int32, C.c_int32, c_i64p, c_i64p]
    lib.ls_sag_decode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_sag_decode_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_sag_last_decode_ms.argtypes = [C.c_void_p]
    lib.ls_sag_last_decode_ms.restype = C.c_float
    lib.ls_sag_enc_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_sag_enc_encode_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_sag_enc_last_encode_ms.argtypes = [C.c_void_p]
    lib.ls_sag_enc_last_encode_ms.restype = C.c_float
    lib.ls_clip_text_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ls_clip_text_encode_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ls_clip_text_last_encode_ms.argtypes = [C.c_void_p]
    lib.ls_clip_text_last_encode_ms.restype = C.c_float
    lib.ls_clip_text_plan.argtypes = [c_i64p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.ls_ted_post.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(LsPostConfig), C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p]
    lib.ls_beat_post.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_beat_metrics.argtypes = [C.c_int, C.POINTER(LsBeatMetricsArgs)]
    lib.ls_beat_ldiv.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, c_f64p]
    lib.ls_onsets.argtypes = [C.c_int, C.POINTER(LsOnsetsArgs)]
    lib.ls_ted_post_timeline.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(LsPostConfig), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
    lib.ls_beat_post_timeline.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_beat_metrics_timeline.argtypes = [C.c_int, C.c_int, C.POINTER(LsBeatMetricsArgs)]
    lib.ls_ted_beat_align.argtypes = [C.c_int, C.POINTER(LsTedAlignArgs)]
    lib.ls_onsets_ragged.argtypes = [C.c_int, C.POINTER(LsOnsetsArgs), C.c_void_p]
    lib.ls_onsets_long.argtypes = [C.c_int, C.POINTER(LsOnsetsArgs)]
    lib.ls_ted_post_timeline_ragged.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(LsPostConfig), C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_beat_post_timeline_ragged.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ls_beat_metrics_timeline_ragged.argtypes = [C.c_int, C.c_int, C.c_void_p, C.POINTER(LsBeatMetricsArgs)]
    lib.ls_ragged_tiles.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.ls_onsets_tables.argtypes = [C.c_float, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    lib.ls_ingest_plan.argtypes = [C.POINTER(LsIngestPlanArgs)]
    lib.ls_ted_ingest.argtypes = [C.c_int, C.POINTER(LsTedIngestArgs)]
    lib.ls_beat_ingest.argtypes = [C.c_int, C.POINTER(LsBeatIngestArgs)]
    lib.ls_train_set_schedule.argtypes = [C.c_void_p, c_f64p, c_f64p, c_i64p]
    lib.ls_train_param_count.argtypes = [C.c_void_p]
    lib.ls_train_flat_size.argtypes = [C.c_void_p]
    lib.ls_train_flat_size.restype = C.c_int64
    lib.ls_train_param_info.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, c_i64p, c_i64p]
    lib.ls_train_get_weight.argtypes = [C.c_void_p, C.c_char_p, c_f32p, C.c_size_t]
    lib.ls_train_forward_backward.argtypes = [C.c_void_p, C.POINTER(LsTrainBatch), C.c_void_p, C.POINTER(LsTrainTerms)]
    lib.ls_train_adamw.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]
    lib.ls_train_read.argtypes = [C.c_void_p, C.c_char_p, c_f32p, C.c_size_t]
    lib.ls_train_get_moment.argtypes = [C.c_void_p, C.c_int, C.c_char_p, c_f32p, C.c_size_t]
    lib.ls_train_set_moment.argtypes = [C.c_void_p, C.c_int, C.c_char_p, c_f32p, C.c_size_t]
    lib.ls_train_get_step.argtypes = [C.c_void_p]
    lib.ls_train_get_step.restype = C.c_int64
    lib.ls_train_set_step.argtypes = [C.c_void_p, C.c_int64]
    lib.ls_eval_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if lib.ls_abi_version() != 5:
        raise EngineError("libls_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _is_cuda(a) -> bool:
    return hasattr(a, "is_cuda") and bool(a.is_cuda)


# torch's name of a marshalled dtype, by table: numpy's own dtype.name costs microseconds per call
_TORCH_NAMES = {np.float32: "float32", np.float64: "float64", np.int32: "int32", np.int64: "int64", np.uint8: "uint8"}


class _Marshal:
    """Turns a group of arrays (numpy / torch CPU / torch CUDA) into raw pointers for one ABI call.
    If ANY member is a CUDA tensor the whole group is passed as device pointers (on_device=1) and outputs
    are torch CUDA tensors; otherwise everything is host numpy.  Keeps the converted buffers alive."""

    def __init__(self, device_index: int, *members, stream=None):
        self.on_device = any(_is_cuda(m) for m in members if m is not None)
        self.device_index = device_index
        self.stream = stream        # the handle's HIP stream (ls_stream & co.): inputs are ordered in front of it, not host-synchronised
        self.keep = []
        if self.on_device:
            import torch
            self.torch = torch
            self.dev = torch.device("cuda", device_index)

    def f32(self, a, shape=None):
        return self._conv(a, np.float32, shape)

    def i64(self, a, shape=None):
        return self._conv(a, np.int64, shape)

    def i32(self, a, shape=None):
        return self._conv(a, np.int32, shape)

    def u8(self, a, shape=None):
        """bool / byte mask -> bytes"""
        return self._conv(a, np.uint8, shape)

    def _conv(self, a, dtype, shape):
        if a is None:
            return None
        if self.on_device:
            t = self.torch.as_tensor(a)
            t = t.to(device=self.dev, dtype=getattr(self.torch, _TORCH_NAMES[dtype])).contiguous()
            if shape is not None:
                assert tuple(t.shape) == tuple(shape), (tuple(t.shape), tuple(shape))
            self.keep.append(t)
            return C.c_void_p(t.data_ptr())
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        n = np.ascontiguousarray(a, dtype=dtype)
        if shape is not None:
            assert tuple(n.shape) == tuple(shape), (n.shape, tuple(shape))
        self.keep.append(n)
        return n.ctypes.data_as(C.c_void_p)

    def ready(self):
        """Call right before the ABI call.  The engine's streams are non-blocking (nothing orders them against torch's), and the
        inputs -- as well as the dtype / contiguity conversions `_conv` may have just enqueued (e.g. the strided `emo[:, 0]` of
        the BEAT callers) and the allocation of the outputs -- belong to torch's current stream: the handle's stream is made to
        wait for that stream's work so far (an event, ls_stream_order) instead of the host waiting for it."""
        if self.on_device:
            ts = self.torch.cuda.current_stream(self.dev)
            if self.stream is None or load_library().ls_stream_order(self.device_index, C.c_void_p(ts.cuda_stream), C.c_void_p(self.stream)) != 0:
                ts.synchronize()

    def done_async(self):
        """After a no_sync ABI call: torch's current stream waits for the handle's work (outputs, and inputs it still reads), so
        consumers on that stream and the allocator's reuse of the marshalled temporaries stay ordered without a host wait."""
        if self.on_device:
            ts = self.torch.cuda.current_stream(self.dev).cuda_stream
            if self.stream is None or load_library().ls_stream_order(self.device_index, C.c_void_p(self.stream), C.c_void_p(ts)) != 0:
                raise EngineError("ls_stream_order failed")

    def out(self, shape, dtype=np.float32):
        """(object, pointer) for an output of this call: float32, uint8, int32 or float64."""
        if self.on_device:
            t = self.torch.empty(tuple(shape), dtype=getattr(self.torch, _TORCH_NAMES[dtype]), device=self.dev)
            return t, C.c_void_p(t.data_ptr())
        n = np.empty(tuple(shape), dtype)
        return n, n.ctypes.data_as(C.c_void_p)


def call(name, *args):
    """Call the handle-less export ``name``; a non-zero return raises.  The export is looked up by name at every call."""
    rc = getattr(load_library(), name)(*args)
    if rc != 0:
        raise EngineError(f"{name} failed ({rc})")


def host_lengths(values, batch, least, most, name):
    """The valid lengths of a ragged call as a contiguous host int32 [batch] (the engine reads them on the host in both modes)."""
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    n = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.int64)
    if n.shape != (batch,):
        raise ValueError(f"{name} must hold one length per clip: got {n.size} for {batch} clips")
    if n.size and (n.min() < least or n.max() > most):
        raise ValueError(f"{name} must lie in [{least}, {most}], got {n.min()} .. {n.max()}")
    return n.astype(np.int32)


def stream_order(device_index: int, first, then) -> None:
    """Work enqueued on stream ``then`` from now on waits for what stream ``first`` holds so far (an event; no host wait).  Streams are
    raw handles: ``Engine._stream`` / ``SagEngine._stream`` or ``torch.cuda.current_stream().cuda_stream``."""
    if load_library().ls_stream_order(int(device_index), C.c_void_p(first), C.c_void_p(then)) != 0:
        raise EngineError("ls_stream_order failed")


def _order_after_torch(device_index: int, stream) -> None:
    """Make a handle's stream wait for the work enqueued so far on torch's current stream of that device."""
    import torch
    ts = torch.cuda.current_stream(torch.device("cuda", device_index))
    if stream is None or load_library().ls_stream_order(device_index, C.c_void_p(ts.cuda_stream), C.c_void_p(stream)) != 0:
        ts.synchronize()


def _np32(a) -> np.ndarray:
    """Host fp32 C-contiguous view/copy of a numpy array or CPU torch tensor."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def plan_query(batch, dataset="ted", single_pass=False, precision="fp32", n_cus=256):
    """The step plan `auto` makes for ``batch`` clips (no GPU needed): ([(family, first, count), ...], model ms per step); family as in
    ``Engine.timing()['step_path']`` (0 fused, 1 batch-level, 2 sample-split, 3 one-pass-per-workgroup)."""
    lib = load_library()
    out = (C.c_int * 10)()
    ms = C.c_float()
    rc = lib.ls_plan_query(int(dataset != "ted"), int(batch), int(bool(single_pass)), {"fp32": 0, "bf16x3": 1, "fp32_mfma": 2}.get(precision, precision), int(n_cus), out, C.byref(ms))
    if rc != 0:
        raise EngineError(f"ls_plan_query failed ({rc})")
    return [(out[1 + 3 * i], out[2 + 3 * i], out[3 + 3 * i]) for i in range(out[0])], float(ms.value)


def long_plan_drop(audio_lengths, audio_len):
    """ls_long_plan_drop (no GPU needed): (slot -> clip int32 [B], windows per slot int32 [B], active clips per window int32 [W_max])."""
    lib = load_library()
    lens = np.ascontiguousarray(np.asarray(audio_lengths).reshape(-1), dtype=np.int64)
    B = int(lens.size)
    row, wins, nw = np.empty(B, np.int32), np.empty(B, np.int32), C.c_int32()
    ptr = lambda a: a.ctypes.data_as(c_i32p)      # noqa: E731
    if B < 1 or lib.ls_long_plan_drop(B, int(audio_len), lens.ctypes.data_as(C.c_void_p), ptr(row), ptr(wins), None, 0, C.byref(nw)) != 0:
        raise ValueError(f"audio_lengths must hold at least one length, each >= 1: got {lens.tolist()}")
    active = np.empty(int(nw.value), np.int32)
    if lib.ls_long_plan_drop(B, int(audio_len), lens.ctypes.data_as(C.c_void_p), None, None, ptr(active), int(nw.value), C.byref(nw)) != 0:
        raise EngineError("ls_long_plan_drop failed")
    return row, wins, active


def long_edit_plan(lo, hi, n_windows, n_frames=34, n_pre=4):
    """ls_long_edit_plan (no GPU needed): the windows a timeline edit of the per-clip frame ranges [lo[b], hi[b]) runs, ascending, as a
    list.  A range outside the timeline or with lo > hi raises ``ValueError``."""
    lib = load_library()
    lo = np.ascontiguousarray(np.asarray(lo).reshape(-1), dtype=np.int32)
    hi = np.ascontiguousarray(np.asarray(hi).reshape(-1), dtype=np.int32)
    W = int(n_windows)
    flags, n = np.zeros(max(W, 1), np.int32), C.c_int32()
    ptr = lambda a: a.ctypes.data_as(c_i32p)      # noqa: E731
    if lo.shape != hi.shape or lib.ls_long_edit_plan(int(lo.size), W, int(n_frames), int(n_pre), ptr(lo), ptr(hi), ptr(flags), C.byref(n)) != 0:
        raise ValueError(f"frame ranges must hold one 0 <= lo <= hi <= {int(n_frames) + (W - 1) * (int(n_frames) - int(n_pre))} per clip, "
                         f"got lo {lo.tolist()} hi {hi.tolist()} for {W} windows")
    return [w for w in range(W) if flags[w]]


def long_edit_plan_compact(lo, hi, n_windows, channels=None, frames=None, n_frames=34, n_pre=4):
    """ls_long_edit_plan_compact (no GPU needed): the clip-windows a COMPACT timeline edit runs, as a list of ``(w, rows)`` -- the
    windows that run, ascending, each with the clips that have an editable element in it, ascending (int32 arrays).  ``channels``: bool /
    byte [B, C] or None (every channel; a clip without a selected channel is in no window); ``frames``: int [B] or None -- clip b has
    only the windows its own ``frames[b]`` frames hold.  A range outside its clip's timeline, ``lo > hi`` or a ``frames[b]`` that is no
    stitched length raises ``ValueError``.  The list is empty when no clip has an editable element."""
    lib = load_library()
    lo = np.ascontiguousarray(np.asarray(lo).reshape(-1), dtype=np.int32)
    hi = np.ascontiguousarray(np.asarray(hi).reshape(-1), dtype=np.int32)
    B, W = int(lo.size), int(n_windows)
    ch = None if channels is None else np.ascontiguousarray(np.asarray(channels).reshape(B, -1) != 0, dtype=np.uint8)
    fr = None if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(c_i32p)      # noqa: E731
    chp, nch = (None, 0) if ch is None else (ch.ctypes.data_as(C.c_void_p), int(ch.shape[1]))
    nw, npairs = C.c_int32(), C.c_int32()
    head = (B, W, int(n_frames), int(n_pre), ptr(lo), ptr(hi), chp, nch, ptr(fr))
    if lo.shape != hi.shape or (fr is not None and fr.shape != lo.shape) or \
            lib.ls_long_edit_plan_compact(*head, None, None, 0, None, 0, C.byref(nw), C.byref(npairs)) != 0:
        raise ValueError(f"frame ranges must hold one 0 <= lo <= hi <= frames[b] per clip (frames[b] = 34 + 30 k, at most "
                         f"{int(n_frames) + (W - 1) * (int(n_frames) - int(n_pre))}), got lo {lo.tolist()} hi {hi.tolist()} frames "
                         f"{None if fr is None else fr.tolist()} for {W} windows")
    wins, counts, rows = np.empty(max(nw.value, 1), np.int32), np.empty(max(nw.value, 1), np.int32), np.empty(max(npairs.value, 1), np.int32)
    if lib.ls_long_edit_plan_compact(*head, ptr(wins), ptr(counts), int(nw.value), ptr(rows), int(npairs.value), C.byref(nw), C.byref(npairs)) != 0:
        raise EngineError("ls_long_edit_plan_compact failed")
    offs = np.concatenate([[0], np.cumsum(counts[:nw.value])]).astype(np.int64)
    return [(int(wins[e]), rows[offs[e]:offs[e + 1]].copy()) for e in range(nw.value)]


def long_edit_plan_mask(mask, n_windows, frames=None, n_frames=34, n_pre=4):
    """ls_long_edit_plan_mask (no GPU needed): the clip-windows a timeline edit by ELEMENT MASK runs, as ``long_edit_plan_compact``'s
    list of ``(w, rows)``.  ``mask``: host bool / bytes [B, C, N] with N = n_frames + (n_windows - 1)(n_frames - n_pre), non-zero =
    editable; the pair (b, w) is in the plan iff clip b has a set element on a frame w owns.  ``frames``: int [B] or None.  A set
    element at or beyond ``frames[b]`` or a ``frames[b]`` that is no stitched length raises ``ValueError``."""
    lib = load_library()
    W = int(n_windows)
    N = int(n_frames) + (W - 1) * (int(n_frames) - int(n_pre))
    m = np.asarray(mask)
    if m.ndim != 3 or m.shape[0] < 1 or m.shape[1] < 1 or m.shape[2] != N:
        raise ValueError(f"an element mask is [B, channels, {N}] for {W} windows, got {list(m.shape)}")
    m = np.ascontiguousarray(m != 0, dtype=np.uint8)
    B = int(m.shape[0])
    fr = None if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(c_i32p)      # noqa: E731
    nw, npairs = C.c_int32(), C.c_int32()
    head = (B, W, int(n_frames), int(n_pre), m.ctypes.data_as(C.c_void_p), int(m.shape[1]), ptr(fr))
    if (fr is not None and fr.shape != (B,)) or lib.ls_long_edit_plan_mask(*head, None, None, 0, None, 0, C.byref(nw), C.byref(npairs)) != 0:
        raise ValueError(f"an element mask must not be set at or beyond its clip's frames[b] (frames[b] = 34 + 30 k, at most {N}); frames "
                         f"{None if fr is None else fr.tolist()} for {W} windows")
    wins, counts, rows = np.empty(max(nw.value, 1), np.int32), np.empty(max(nw.value, 1), np.int32), np.empty(max(npairs.value, 1), np.int32)
    if lib.ls_long_edit_plan_mask(*head, ptr(wins), ptr(counts), int(nw.value), ptr(rows), int(npairs.value), C.byref(nw), C.byref(npairs)) != 0:
        raise EngineError("ls_long_edit_plan_mask failed")
    offs = np.concatenate([[0], np.cumsum(counts[:nw.value])]).astype(np.int64)
    return [(int(wins[e]), rows[offs[e]:offs[e + 1]].copy()) for e in range(nw.value)]


def long_stream_plan(samples_before, samples_new, audio_len, closing=False):
    """ls_long_stream_plan (no GPU needed): ``(first_window, n_windows)`` a push of ``samples_new`` samples runs on a stream that holds
    ``samples_before``; ``closing`` adds the zero-padded windows the total still owes.  Closing an empty stream raises ``ValueError``."""
    first, n = C.c_int64(), C.c_int64()
    if load_library().ls_long_stream_plan(int(samples_before), int(samples_new), int(audio_len), int(bool(closing)), C.byref(first), C.byref(n)) != 0:
        raise ValueError(f"no windows for {samples_before} + {samples_new} samples (closing={bool(closing)}): counts must be >= 0, "
                         "and a stream that is closed must hold a sample")
    return int(first.value), int(n.value)


def long_pool_plan(samples_in, windows_run, samples_new, closing, open, audio_len):
    """ls_long_pool_plan (no GPU needed): ``(rounds, frames)`` of one push of a session pool.  ``rounds`` is a list of lists -- round r
    holds, ascending, the slots that run their window ``windows_run[s] + r`` in it -- and ``frames`` int32 [S] the frames each slot gets.
    The five arrays are host sequences [S].  Samples for a slot that is not open, closing a slot that was fed no sample, or a negative
    count raise ``ValueError``."""
    lib = load_library()
    i64 = lambda a: np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int64)      # noqa: E731
    i32 = lambda a: np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)      # noqa: E731
    fed, ran, new, closing, open = i64(samples_in), i64(windows_run), i64(samples_new), i32(closing), i32(open)
    S = int(fed.size)
    if not (ran.size == new.size == closing.size == open.size == S):
        raise ValueError(f"one entry per slot: got {[a.size for a in (fed, ran, new, closing, open)]}")
    p64, p32 = (lambda a: a.ctypes.data_as(c_i64p)), (lambda a: a.ctypes.data_as(c_i32p))
    wins, frames, n_rounds, n_entries = np.zeros(max(S, 1), np.int32), np.zeros(max(S, 1), np.int32), C.c_int32(), C.c_int32()

    def run(slots, cap):
        return lib.ls_long_pool_plan(S, int(audio_len), p64(fed), p64(ran), p64(new), p32(closing), p32(open), p32(wins), p32(frames), slots, cap,
                                     C.byref(n_rounds), C.byref(n_entries))

    if run(None, 0) != 0:
        raise ValueError(f"no plan for samples_in {fed.tolist()} windows_run {ran.tolist()} + {new.tolist()} (closing {closing.tolist()}, open "
                         f"{open.tolist()}): counts must be >= 0 and consistent, samples go to open slots only, and a slot that is closed must hold a sample")
    flat = np.zeros(max(int(n_entries.value), 1), np.int32)
    if run(p32(flat), int(n_entries.value)) != 0:
        raise EngineError("ls_long_pool_plan failed")
    rounds, at = [], 0
    for r in range(int(n_rounds.value)):
        A = int((wins[:S] > r).sum())
        rounds.append([int(s) for s in flat[at:at + A]])
        at += A
    return rounds, frames[:S].copy()


def long_pool_pin_plan(windows_run, n_windows, pins, n_frames=34, n_pre=4):
    """ls_long_pool_pin_plan (no GPU needed): the sampling calls of one push of a session with pinned poses, as a list of ``(round,
    pinned, slots)`` in the order they run.  ``windows_run`` / ``n_windows``: host sequences [S] (``n_windows[s]``: the windows slot s
    runs in the push, ``len([r for r in rounds if s in r])`` of ``long_pool_plan``); ``pins``: per slot the pending pinned frames, a
    sequence of S sequences of series frames in any order (None: no pins).  Round r is its unpinned slots, ascending, as one plain
    call, then its pinned ones, ascending, as one inpainting call; an empty half is no call.  Negative counts or frames, or a wrong
    number of entries, raise ``ValueError``."""
    lib = load_library()
    ran = np.ascontiguousarray(np.asarray(windows_run).reshape(-1), dtype=np.int64)
    wins = np.ascontiguousarray(np.asarray(n_windows).reshape(-1), dtype=np.int32)
    S = int(ran.size)
    if wins.size != S or (pins is not None and len(pins) != S):
        raise ValueError(f"one entry per slot: got {[ran.size, wins.size] + ([] if pins is None else [len(pins)])}")
    first = frames = None
    if pins is not None:
        per = [np.asarray(list(p), dtype=np.int64).reshape(-1) for p in pins]
        first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([p.size for p in per])]), dtype=np.int32)
        frames = np.ascontiguousarray(np.concatenate(per + [np.zeros(1, np.int64)]), dtype=np.int64)      # never empty: the pointer is real
    p64, p32 = (lambda a: None if a is None else a.ctypes.data_as(c_i64p)), (lambda a: None if a is None else a.ctypes.data_as(c_i32p))
    n_calls, n_entries = C.c_int32(), C.c_int32()

    def run(rows, counts, pinned, rounds):
        return lib.ls_long_pool_pin_plan(S, int(n_frames), int(n_pre), p64(ran), p32(wins), p32(first), p64(frames), p32(rows), 0 if rows is None else rows.size,
                                         p32(counts), p32(pinned), p32(rounds), 0 if counts is None else counts.size, C.byref(n_calls), C.byref(n_entries))

    if S < 1 or run(None, None, None, None) != 0:
        raise ValueError(f"no pin plan for windows_run {ran.tolist()} n_windows {wins.tolist()} pins {pins!r}: counts and frames must be >= 0")
    rows = np.zeros(max(int(n_entries.value), 1), np.int32)
    counts, pinned, rounds = (np.zeros(max(int(n_calls.value), 1), np.int32) for _ in range(3))
    if run(rows, counts, pinned, rounds) != 0:
        raise EngineError("ls_long_pool_pin_plan failed")
    calls, at = [], 0
    for q in range(int(n_calls.value)):
        calls.append((int(rounds[q]), bool(pinned[q]), [int(s) for s in rows[at:at + int(counts[q])]]))
        at += int(counts[q])
    return calls


def long_pool_keys(keys, windows_run, n_windows):
    """ls_long_pool_keys (no GPU needed): the key table of one push of a keyed session pool, uint64 [sum n_windows], in
    ``long_pool_plan``'s row order -- the row of slot s in round r draws at ``keys[s] + ((windows_run[s] + r) << 48)``.  A key of
    a slot that runs a window outside ``[0, 2^48)`` raises ``ValueError``, a window index that reaches 2^16 ``EngineError``."""
    lib = load_library()
    for k in keys:
        if not 0 <= int(k) < 1 << 64:
            raise ValueError(f"key {k} outside [0, 2^64)")
    k64 = np.ascontiguousarray([int(k) for k in keys], dtype=np.uint64)
    ran = np.ascontiguousarray(np.asarray(windows_run).reshape(-1), dtype=np.int64)
    wins = np.ascontiguousarray(np.asarray(n_windows).reshape(-1), dtype=np.int32)
    S = int(k64.size)
    if not (ran.size == wins.size == S):
        raise ValueError(f"one entry per slot: got {[a.size for a in (k64, ran, wins)]}")
    pu64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))      # noqa: E731
    n = C.c_int32()
    rc = lib.ls_long_pool_keys(S, pu64(k64), ran.ctypes.data_as(c_i64p), wins.ctypes.data_as(c_i32p), None, 0, C.byref(n))
    if rc == -2:        # LS_ESTATE
        raise EngineError("ls_long_pool_keys: a clip of a keyed pool runs at most 2^16 windows")
    if rc != 0:
        raise ValueError(f"no key table for keys {k64.tolist()} windows_run {ran.tolist()} n_windows {wins.tolist()}: keys stay below 2^48, counts are >= 0")
    out = np.zeros(max(int(n.value), 1), np.uint64)
    if lib.ls_long_pool_keys(S, pu64(k64), ran.ctypes.data_as(c_i64p), wins.ctypes.data_as(c_i32p), pu64(out), int(n.value), C.byref(n)) != 0:
        raise EngineError("ls_long_pool_keys failed")
    return out[:int(n.value)].copy()


POST_STREAM_MAX_CHUNK = 256      # LS_POST_STREAM_MAX_CHUNK
POST_STREAM_MAX_ORDER = 8        # LS_POST_STREAM_MAX_ORDER


def post_stream_plan(dataset, n_before, n_new, finishing=False, order=2):
    """ls_post_stream_plan (no GPU needed): ``(beat_first, beat_count)``, the beat entries a push of ``n_new`` frames decides on a
    series that holds ``n_before`` -- frames of the TED beat mask, velocity indices of the BEAT series.  A negative count, an order
    outside [1, 8] (BEAT) or finishing a series without a frame raise ``ValueError``."""
    first, count = C.c_int64(), C.c_int32()
    if dataset not in ("ted", "beat") or load_library().ls_post_stream_plan(int(dataset == "beat"), int(order), int(n_before), int(n_new),
                                                                           int(bool(finishing)), C.byref(first), C.byref(count)) != 0:
        raise ValueError(f"no plan for dataset {dataset!r}, order {order}, {n_before} + {n_new} frames (finishing={bool(finishing)}): counts "
                         "must be >= 0, a BEAT order in [1, 8], and a series that is finished must hold a frame")
    return int(first.value), int(count.value)


def post_stream_check(dataset, order, frames_in, K, counts, finish, beat_capacity=None):
    """ls_post_stream_check (no GPU needed): what a push refuses ahead of any launch.  Returns ``(beat_first int64 [S], beat_count int32
    [S])``; ``beat_capacity=None`` asks for the counts alone.  Raises ``ValueError`` for what the engine answers with LS_EINVAL or
    LS_ESTATE."""
    n = np.ascontiguousarray(np.asarray(frames_in).reshape(-1), dtype=np.int64)
    S = int(n.size)
    k = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
    fin = np.zeros(S, np.int32) if finish is None else np.ascontiguousarray(np.asarray(finish).reshape(-1)).astype(bool).astype(np.int32)
    if k.shape != (S,) or fin.shape != (S,):
        raise ValueError(f"one count and one finish flag per slot: got {k.size} and {fin.size} for {S} slots")
    if k.size and (k.min() < 0 or k.max() > int(K)):
        raise ValueError(f"counts must lie in [0, {int(K)}], got {k.min()} .. {k.max()}")
    k = k.astype(np.int32)
    first, count = np.zeros(max(S, 1), np.int64), np.zeros(max(S, 1), np.int32)
    cap = (POST_STREAM_MAX_CHUNK + POST_STREAM_MAX_ORDER) if beat_capacity is None else int(beat_capacity)
    rc = load_library().ls_post_stream_check(int(dataset == "beat"), int(order), S, n.ctypes.data_as(c_i64p), int(K), k.ctypes.data_as(c_i32p),
                                             fin.ctypes.data_as(c_i32p), cap, first.ctypes.data_as(c_i64p), count.ctypes.data_as(c_i32p))
    if rc == -2:
        raise ValueError(f"finish on a slot without a frame: frames_in {n.tolist()}, counts {k.tolist()}, finish {fin.tolist()}")
    if rc != 0:
        raise ValueError(f"refused: at most {POST_STREAM_MAX_CHUNK} frames per push (got K = {int(K)}), counts in [0, K], a BEAT order in [1, 8], "
                         f"beat_capacity {cap} >= every slot's entries")
    return first[:S].copy(), count[:S].copy()


SCORE_STREAM_MAX_BEATS = 4096    # LS_SCORE_STREAM_MAX_BEATS


def score_stream_plan(pad_mode, samples_before, n_new, finishing=False):
    """ls_score_stream_plan (no GPU needed): ``(frame_first, frame_count)``, the audio frames a push of ``n_new`` samples decides on a
    series that holds ``samples_before``.  ``pad_mode``: 0 constant, 1 reflect.  Raises ``ValueError`` for what the engine refuses."""
    first, count = C.c_int64(), C.c_int32()
    if load_library().ls_score_stream_plan(int(pad_mode), int(samples_before), int(n_new), int(bool(finishing)), C.byref(first), C.byref(count)) != 0:
        raise ValueError(f"no plan for pad_mode {pad_mode}, {samples_before} + {n_new} samples (finishing={bool(finishing)}): counts must be >= 0 "
                         "and at most 2^31 - 2048 in all, a series that is finished must hold a sample, and more than 1024 under reflect padding")
    return int(first.value), int(count.value)


class ScoreStreamEngine:
    """One ``ls_score_stream`` handle: ``capacity`` slots of spectra and motion beats on one GPU (``postprocess.open_score_stream``)."""

    def __init__(self, dataset, capacity, max_audio_frames, max_beat_entries, cfg, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.device, self.S = int(device), int(capacity)
        rc = self.lib.ls_score_stream_open(self.device, int(dataset == "beat"), self.S, int(max_audio_frames), int(max_beat_entries), C.byref(cfg),
                                           C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise EngineError(f"ls_score_stream_open failed ({rc}): {self.lib.ls_score_stream_last_error(None).decode()}")

    def _check(self, name, rc):
        if rc != 0:
            msg = self.lib.ls_score_stream_last_error(self.h).decode()
            raise (ValueError if rc in (-1, -2) else EngineError)(f"{name} failed ({rc}): {msg}")

    def push(self, args: "LsScoreStreamPushArgs"):
        self._check("ls_score_stream_push", self.lib.ls_score_stream_push(self.h, C.byref(args)))

    def finish(self, flags, outputs: "LsScoreStreamOutputs"):
        self._check("ls_score_stream_finish", self.lib.ls_score_stream_finish(self.h, flags.ctypes.data_as(c_i32p), C.byref(outputs)))

    def info(self) -> dict:
        a, b, c, nbytes = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64), np.zeros(self.S, np.int64), C.c_int64()
        if self.lib.ls_score_stream_info(self.h, a.ctypes.data_as(c_i64p), b.ctypes.data_as(c_i64p), c.ctypes.data_as(c_i64p), C.byref(nbytes)) != 0:
            raise EngineError("ls_score_stream_info failed")
        return {"samples_in": a, "frames_done": b, "beats_in": c, "device_bytes": int(nbytes.value)}

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ls_score_stream_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RESAMPLE_MAX_CHANNELS = 8        # LS_RESAMPLE_MAX_CHANNELS
RESAMPLE_DTYPES = {"float32": 0, "int16": 1}      # LS_RESAMPLE_F32, LS_RESAMPLE_I16


def resample_ratio(in_sr, out_sr, zeros=32) -> dict:
    """ls_resample_ratio (no GPU needed): ``up``, ``down``, ``half``, ``taps_per_output``, ``carry_len`` and ``n_taps`` of a rate pair.
    ``ValueError`` for a rate or ``zeros`` below 1, ``EngineError`` for more than 2^22 taps."""
    v = [C.c_int64() for _ in range(6)]
    for name, x in (("in_sr", in_sr), ("out_sr", out_sr), ("zeros", zeros)):
        if isinstance(x, bool) or int(x) != x or not 1 <= int(x) < 1 << 31:
            raise ValueError(f"{name} must be an integer in [1, 2^31), got {x!r}")
    rc = load_library().ls_resample_ratio(int(in_sr), int(out_sr), int(zeros), *[C.byref(x) for x in v])
    if rc == -5:        # LS_EUNSUPPORTED
        raise EngineError(f"{in_sr} -> {out_sr} Hz with {zeros} zeros needs more than 2^22 taps")
    if rc != 0:
        raise ValueError(f"no ratio for {in_sr} -> {out_sr} Hz with {zeros} zeros: all three must be >= 1")
    return dict(zip(("up", "down", "half", "taps_per_output", "carry_len", "n_taps"), (int(x.value) for x in v)))


def resample_ratio_plan(up, down, half, n_before, n_new, finishing=False):
    """ls_resample_plan (no GPU needed): ``(out_first, out_count)``, the outputs a push of ``n_new`` samples decides on a series that
    holds ``n_before``; ``finishing`` adds what the end of the series still owes.  ``ValueError`` for what the engine refuses."""
    first, count = C.c_int64(), C.c_int64()
    args = [int(v) for v in (up, down, half, n_before, n_new)]
    if any(not -(1 << 63) <= v < 1 << 63 for v in args) or load_library().ls_resample_plan(*args, int(bool(finishing)), C.byref(first), C.byref(count)) != 0:
        raise ValueError(f"no plan for up {up}, down {down}, half {half}, {n_before} + {n_new} samples (finishing={bool(finishing)}): up and down "
                         "must be >= 1, half and the counts >= 0 and at most 2^62 (also times up), and a series that is finished must hold a sample")
    return int(first.value), int(count.value)


def resample_taps(up, down, zeros=32, beta=12.0, rolloff=0.95):
    """ls_resample_taps (no GPU needed): ``(h64, h32)``, the ``2 * zeros * max(up, down) + 1`` taps in double and rounded to float32."""
    q = max(int(up), int(down))
    if int(up) < 1 or int(down) < 1 or int(zeros) < 1 or not float(beta) >= 0 or not 0 < float(rolloff) <= 1:
        raise ValueError(f"up, down and zeros must be >= 1, beta >= 0 and rolloff in (0, 1]: got {up}, {down}, {zeros}, {beta}, {rolloff}")
    if 2 * int(zeros) * q + 1 > 1 << 22:
        raise EngineError(f"up {up}, down {down} with {zeros} zeros needs {2 * int(zeros) * q + 1} taps, above 2^22")
    h64, h32 = np.empty(2 * int(zeros) * q + 1, np.float64), np.empty(2 * int(zeros) * q + 1, np.float32)
    rc = load_library().ls_resample_taps(int(up), int(down), int(zeros), float(beta), float(rolloff), h64.ctypes.data_as(c_f64p), h32.ctypes.data_as(c_f32p))
    if rc != 0:
        raise EngineError(f"ls_resample_taps failed ({rc})")
    return h64, h32


class ResampleStreamEngine:
    """One ``ls_resample_stream`` handle: ``capacity`` slots of resampler state on one GPU (``audio_io.open_resample_stream``)."""

    def __init__(self, capacity, in_sr, out_sr, channels, dtype, zeros, beta, rolloff, max_chunk, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.device, self.S = int(device), int(capacity)
        rc = self.lib.ls_resample_stream_open(self.device, self.S, int(in_sr), int(out_sr), int(channels), RESAMPLE_DTYPES[dtype], int(zeros), float(beta),
                                              float(rolloff), int(max_chunk), C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise EngineError(f"ls_resample_stream_open failed ({rc}): {self.lib.ls_resample_stream_last_error(None).decode()}")

    def push(self, args: "LsResampleStreamPushArgs"):
        rc = self.lib.ls_resample_stream_push(self.h, C.byref(args))
        if rc != 0:
            msg = self.lib.ls_resample_stream_last_error(self.h).decode()
            raise (ValueError if rc == -1 else EngineError)(f"ls_resample_stream_push failed ({rc}): {msg}")

    def reset(self, slot):
        if self.lib.ls_resample_stream_reset(self.h, int(slot)) != 0:
            raise ValueError(f"ls_resample_stream_reset: {self.lib.ls_resample_stream_last_error(self.h).decode()}")

    def info(self) -> dict:
        a, b, nbytes = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64), C.c_int64()
        if self.lib.ls_resample_stream_info(self.h, a.ctypes.data_as(c_i64p), b.ctypes.data_as(c_i64p), C.byref(nbytes)) != 0:
            raise EngineError("ls_resample_stream_info failed")
        return {"samples_in": a, "outputs_done": b, "device_bytes": int(nbytes.value)}

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ls_resample_stream_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PostStreamEngine:
    """One ``ls_post_stream`` handle: ``capacity`` slots of post-processing state on one GPU (see ``postprocess.open_post_stream``)."""

    def __init__(self, dataset, capacity, device=0, cfg=None, njoints=47, order=2, series_joints=(0,) * 6):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.device, self.S = int(device), int(capacity)
        joints = (C.c_int32 * 6)(*[int(j) for j in series_joints])
        rc = self.lib.ls_post_stream_open(self.device, int(dataset == "beat"), self.S, C.byref(cfg) if cfg is not None else None, int(njoints),
                                          int(order), joints, C.byref(self.h))
        if rc != 0:
            self.h = C.c_void_p()
            raise EngineError(f"ls_post_stream_open failed ({rc}): {self.lib.ls_post_stream_last_error(None).decode()}")

    def push(self, args: "LsPostStreamPushArgs"):
        rc = self.lib.ls_post_stream_push(self.h, C.byref(args))
        if rc != 0:
            raise EngineError(f"ls_post_stream_push failed ({rc}): {self.lib.ls_post_stream_last_error(self.h).decode()}")

    def info(self) -> dict:
        n, nbytes = np.zeros(self.S, np.int64), C.c_int64()
        if self.lib.ls_post_stream_info(self.h, n.ctypes.data_as(c_i64p), C.byref(nbytes)) != 0:
            raise EngineError("ls_post_stream_info failed")
        return {"frames_in": n, "device_bytes": int(nbytes.value)}

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ls_post_stream_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def plan_coop_slices(groups, dataset="ted", n_cus=256):
    """Slice workgroups per (sample, CFG pass) the sample-split kernel uses for ``groups`` (sample, pass) groups: 8, 4 or 2."""
    lib = load_library()
    rc = lib.ls_plan_coop_slices(int(dataset != "ted"), int(groups), int(n_cus))
    if rc < 0:
        raise EngineError(f"ls_plan_coop_slices failed ({rc})")
    return rc


class _Handle:
    """What the six wrappers share: one C handle of the ``ls_<prefix>*`` family (``_prefix`` is ``"ls_"``, ``"ls_sag_"``, ...)."""

    _prefix = "ls_"

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    def _create(self, cfg):
        self.lib = load_library()
        self.cfg = cfg
        self.h = C.c_void_p()
        rc = self._fn("create")(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            raise EngineError(f"{self._prefix}create failed ({rc}): {self._fn('last_error')(None).decode()}")
        self._stream = self._fn("stream")(self.h)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise EngineError(f"{what} failed ({rc}): {self._fn('last_error')(self.h).decode()}")
        return rc

    def _set_weights(self, sd: dict, commit=True):
        for k, v in sd.items():
            a = _np32(v)
            self._check(self._fn("set_weight")(self.h, k.encode(), a.ctypes.data_as(c_f32p), a.size), f"{self._prefix}set_weight({k})")
        if commit:
            self._check(self._fn("commit_weights")(self.h), f"{self._prefix}commit_weights")


class Engine(_Handle):
    """One handle = one GPU. Thin, typed wrapper over the C-ABI; all arrays in/out are host numpy
    (torch CUDA tensors on the same device may be passed to ``sample``/``prepare`` via ``*_device``)."""

    #: which kernels the steps of a 34-frame model run on when the caller does not say: "auto" (the sample-split kernel for small
    #: batches, one workgroup per sample or per (sample, pass) otherwise), "fused", "batch", "coop", "pass" (ls_set_path)
    default_path = "auto"

    def __init__(self, njoints, nfeats, n_prefix_tokens, audio_len, n_emotions=0, nframes=34, n_pre_seq=4,
                 latent_dim=512, layers=8, n_speakers=1400, device=0, path=None):
        self._create(LsConfig(njoints, nfeats, nframes, n_prefix_tokens, n_pre_seq, latent_dim, layers, audio_len,
                              n_speakers, n_emotions, device, 0))
        self.path = path or Engine.default_path
        if nframes != 34:
            self.path = "batch"                       # other frame counts have only the batch-level kernels (ls_set_path refuses the rest)
        elif self.path != "auto":
            self.set_path(self.path)
        self.J, self.F, self.T, self.D = njoints, nfeats, nframes, latent_dim
        self.S = nframes + n_prefix_tokens
        self.layers = layers
        self.device = device
        self.batch = 0
        self.n_steps = 0
        self._keep = []

    def set_precision(self, mode):
        """'fp32' (default: fp32-accurate split-bf16 channel mixing in the fused step kernel, fp32 MFMA elsewhere), 'fp32_mfma'
        (fp32 MFMA everywhere, the pre-split arithmetic) or 'bf16x3' (split-precision channel mixing on the bf16 matrix cores)."""
        code = {"fp32": 0, "bf16x3": 1, "fp32_mfma": 2}.get(mode, mode)
        self._check(self.lib.ls_set_precision(self.h, int(code)), "ls_set_precision")
        self.precision = mode

    def set_path(self, mode):
        """'auto' (default: the sample-split kernel for small batches, one workgroup per sample otherwise), 'fused', 'batch'
        (batch-level kernels, 21 launches per step), 'coop' (sample-split kernel), 'pass' (one workgroup per (sample, CFG pass), two per
        CU), 'pass4' (its 4-wave form at every grid size), 'coop8' / 'coop4' / 'coop2' (the sample-split kernel with that many channel
        slices per (sample, CFG pass)); applies from the next prepare().  None = 'auto'.  On a long-sequence model (145-160 tokens) 'auto'
        runs the sampling loop on the one-launch mixer where every launch is at least 7/8 full, 'batch' forces the batch-level kernels and
        'coop' the mixer at every batch size; the other modes raise (ls_set_path in include/ls_hip.h)."""
        mode = "auto" if mode is None else mode
        code = {"auto": 0, "fused": 1, "batch": 2, "coop": 3, "pass": 4, "pass4": 5, "coop4": 6, "coop2": 7, "coop8": 8}.get(mode, mode)
        self._check(self.lib.ls_set_path(self.h, int(code)), "ls_set_path")
        self.path = mode

    # ---- weights / schedule --------------------------------------------------------------------
    def load_state_dict(self, sd: dict):
        self._set_weights(sd)

    def set_schedule(self, sched):
        """sched: object with the GaussianDiffusion table attributes + timestep_map."""
        tabs = {}
        s = LsSchedule()
        s.n_steps = int(sched.num_timesteps)
        tmap = np.ascontiguousarray(np.asarray(sched.timestep_map), dtype=np.int64)
        s.timestep_map = tmap.ctypes.data_as(c_i64p)
        for name, _ in LsSchedule._fields_[3:]:
            tabs[name] = np.ascontiguousarray(getattr(sched, name), dtype=np.float64)
            assert tabs[name].shape == (s.n_steps,), name
            setattr(s, name, tabs[name].ctypes.data_as(c_f64p))
        self._check(self.lib.ls_set_schedule(self.h, C.byref(s)), "ls_set_schedule")
        self.n_steps = s.n_steps

    # ---- per call --------------------------------------------------------------------------------
    def prepare(self, y: dict, wait: bool = True):
        """Once-per-call stage.  ``wait=False`` (ls_prepare_async) only enqueues it on the engine's stream: the next sample / forward /
        step is ordered behind it, and work on other streams (the SAG decode) overlaps it.  The marshalled inputs are kept alive on
        this object until the next prepare, by which time a synchronising call has long consumed them."""
        emo = y.get("emo") if self.cfg.n_prefix_tokens == 2 else None
        if emo is not None:
            # scripts_beat/model/RAG.py:125 reads y['emo'][:, 0] only, whatever the width: a bare [B] vector, [B, 1] or any padded
            # [B, W] is accepted and presented to the ABI in its [B, T] form (column 0 repeated)
            if getattr(emo, "ndim", 2) not in (1, 2):
                raise EngineError(f"y['emo'] must be [B] or [B, W], got shape {tuple(emo.shape)}")
            col = emo if emo.ndim == 1 else emo[:, 0]
            if hasattr(col, "expand") and not isinstance(col, np.ndarray):
                emo = col[:, None].expand(col.shape[0], self.T)
            else:
                emo = np.broadcast_to(np.asarray(col)[:, None], (len(col), self.T))
        m = _Marshal(self.device, y["audio_input"], y["origin_x"], y["vid_indices"], y["scale"], emo, stream=self._stream)
        B = int(y["audio_input"].shape[0])
        c = LsCond(B, int(m.on_device), m.f32(y["audio_input"], (B, self.cfg.audio_len)),
                   m.f32(y["origin_x"], (B, self.J, self.F, self.T)), m.i64(y["vid_indices"], (B,)),
                   m.i64(emo, (B, self.T)), m.f32(y["scale"], (B,)))
        m.ready()
        if wait:
            self._check(self.lib.ls_prepare(self.h, C.byref(c)), "ls_prepare")
            self._prepare_inputs = None
        else:
            self._check(self.lib.ls_prepare_async(self.h, C.byref(c)), "ls_prepare_async")
            self._prepare_inputs = (m, y)       # device buffers (and any converted copies) stay valid while the copies are in flight
            if m.on_device:
                # conv1 reads a device-resident waveform IN PLACE (no ingest copy): whatever the caller enqueues next on torch's stream --
                # e.g. refilling the same batch buffer -- has to wait for the engine's stream, exactly like the outputs of a no_sync call
                m.done_async()
        self.batch = B

    def _xshape(self):
        return (self.batch, self.J, self.F, self.T)

    def forward(self, x, t, eps_c, eps_u, trace=False):
        m = _Marshal(self.device, x, t, eps_c, eps_u, stream=self._stream)
        B, D = self.batch, self.D
        eps_c = eps_c.reshape(B, D)
        eps_u = eps_u.reshape(B, D)
        oc, poc = m.out(self._xshape())
        ou, pou = m.out(self._xshape())
        og, pog = m.out(self._xshape())
        tr, ptr = m.out((B, self.layers + 1, 2 * self.S, D)) if trace else (None, None)
        a = LsForwardArgs(int(m.on_device), 0, m.f32(x, self._xshape()), m.i64(t, (B,)), m.f32(eps_c, (B, D)),
                          m.f32(eps_u, (B, D)), poc, pou, pog, ptr)
        m.ready()
        self._check(self.lib.ls_forward(self.h, C.byref(a)), "ls_forward")
        return (oc, ou, og, tr) if trace else (oc, ou, og)

    def step(self, sampler, index, x, eps_c, eps_u, noise, eta=0.0, clip_denoised=False, two_pass_always=False, indices=None,
             no_sync=False, inpaint=None):
        """One p_sample / ddim_sample step.  ``indices``: one schedule index per sample ([B] int64; numpy / CPU tensor = validated
        on the host, CUDA tensor = never read by the host) instead of the uniform ``index``.  ``no_sync`` (device tensors only):
        return without waiting for the GPU; the outputs are ordered behind the step on torch's current stream."""
        inp = inpaint or (None, None, None)          # (mask, motion, q_sample noise or None): p_mean_variance's inpainting branch
        m = _Marshal(self.device, x, eps_c, eps_u, noise, inp[1], stream=self._stream)
        B, D = self.batch, self.D
        out, pout = m.out(self._xshape())
        x0, px0 = m.out(self._xshape())
        pidx, idx_dev = None, 0
        if indices is not None:
            if _is_cuda(indices):
                if not m.on_device:
                    raise EngineError("device `indices` need device tensors for the other arguments")
                t = indices.to(dtype=m.torch.int64).contiguous()
                if tuple(t.shape) != (B,):
                    raise EngineError(f"indices must be [{B}], got {tuple(t.shape)}")
                m.keep.append(t)
                pidx, idx_dev = C.c_void_p(t.data_ptr()), 1
            else:
                n = np.ascontiguousarray(indices.detach().cpu().numpy() if hasattr(indices, "detach") else indices, dtype=np.int64)
                if n.shape != (B,):
                    raise EngineError(f"indices must be [{B}], got {n.shape}")
                m.keep.append(n)
                pidx = n.ctypes.data_as(C.c_void_p)
        nosync = int(bool(no_sync) and m.on_device)
        a = LsStepArgs(sampler, int(index), int(m.on_device), eta, int(clip_denoised), int(two_pass_always), m.f32(x, self._xshape()),
                       m.f32(eps_c.reshape(B, D)), m.f32(eps_u.reshape(B, D)), m.f32(noise, self._xshape()), pout, px0, pidx, nosync, idx_dev,
                       m.u8(inp[0], self._xshape()), m.f32(inp[1], self._xshape()), m.f32(inp[2], self._xshape()))
        m.ready()
        self._check(self.lib.ls_step(self.h, C.byref(a)), "ls_step")
        if nosync:
            m.done_async()
            self._inflight = m          # marshalled copies stay referenced until the next call replaces them
        return out, x0

    def plms_step(self, index, order, x, eps, hist=(), eps2=None, clip_denoised=False, two_pass_always=False, no_sync=False):
        """One plms_sample step at the uniform schedule ``index``.  ``eps`` = (cond, uncond) style draws of the evaluation, ``eps2`` those
        of the second evaluation of a loop's first step (``hist`` empty); ``hist``: the old eps planes, oldest first (at most the last
        three are read).  Returns (sample, pred_xstart, eps plane of this step)."""
        hist = list(hist)[-3:]
        e2 = eps2 or (None, None)
        m = _Marshal(self.device, x, eps[0], eps[1], e2[0], e2[1], *hist, stream=self._stream)
        B, D = self.batch, self.D
        out, pout = m.out(self._xshape())
        x0, px0 = m.out(self._xshape())
        ep, pep = m.out(self._xshape())
        nosync = int(bool(no_sync) and m.on_device)
        a = LsPlmsStepArgs()
        a.index, a.order, a.n_hist, a.on_device = int(index), int(order), len(hist), int(m.on_device)
        a.clip_denoised, a.two_pass_always, a.no_sync = int(clip_denoised), int(two_pass_always), nosync
        a.x = m.f32(x, self._xshape())
        a.eps_cond, a.eps_uncond = m.f32(eps[0].reshape(B, D)), m.f32(eps[1].reshape(B, D))
        if eps2 is not None:
            a.eps_cond2, a.eps_uncond2 = m.f32(eps2[0].reshape(B, D)), m.f32(eps2[1].reshape(B, D))
        for j, hp in enumerate(hist):
            a.hist[j] = m.f32(hp, self._xshape())
        a.sample, a.pred_xstart, a.eps_out = pout, px0, pep
        m.ready()
        self._check(self.lib.ls_plms_step(self.h, C.byref(a)), "ls_plms_step")
        if nosync:
            m.done_async()
            self._inflight = m
        return out, x0, ep

    def sample(self, sampler=LS_SAMPLER_DDPM, x_init=None, eps_tape=None, noise_tape=None, init_image=None,
               skip_timesteps=0, eta=0.0, const_noise=False, dump_steps=None, philox_seed=None, sample_offset=0,
               use_graph=True, clip_denoised=False, device_out=False, two_pass_always=False, segment=None, inpaint=None,
               torch_state=None, torch_ring_bytes=256 << 20, plms_order=0, row_keys=None):
        """Run the whole loop. TAPE mode when tapes are given, PHILOX mode when ``philox_seed`` is, TORCH_DEVICE mode when
        ``torch_state`` = (seed, offset) of torch's device generator is (the loop makes torch's device draws itself; ``x_init`` None =
        it draws x_T too; the caller moves the generator on).  ``row_keys`` uint64 [B] (PHILOX): row b draws at ``row_keys[b]`` in place of
        ``sample_offset + b`` (ls_set_row_keys; set for this call alone, its draws go through the ring of ``torch_ring_bytes``).  Outputs are torch CUDA tensors if any input is one (or ``device_out``),
        else numpy."""
        inp = inpaint or (None, None, None, False)     # (mask, motion, q_sample noise tape or None, re-noise?): the inpainting branch
        m = self._marshal([x_init, eps_tape, noise_tape, init_image, inp[1]], device_out)
        a = LsSampleArgs()
        a.sampler, a.skip_timesteps, a.const_noise, a.on_device = sampler, skip_timesteps, int(const_noise), int(m.on_device)
        a.use_graph, a.eta, a.clip_denoised = int(use_graph), eta, int(clip_denoised)
        a.two_pass_always = int(two_pass_always)
        n_exec = self.n_steps - skip_timesteps
        a.plms_order = int(plms_order)  # LS_SAMPLER_PLMS: eps_tape holds n_exec + 1 evaluations, there is no step noise
        if segment is not None:         # (first executed-step counter, count): one piece of a TAPE-mode loop, tapes hold these steps only
            a.seg_begin, a.seg_count = int(segment[0]), int(segment[1])
            n_tape, last = a.seg_count, a.seg_begin + a.seg_count == n_exec
        else:
            n_tape, last = n_exec, True
        if torch_state is not None:
            a.noise_mode = LS_NOISE_TORCH_DEVICE
            a.seed, a.sample_offset = int(torch_state[0]) & 0xFFFFFFFFFFFFFFFF, int(torch_state[1])
            self._check(self.lib.ls_set_torch_ring_bytes(self.h, int(torch_ring_bytes)), "ls_set_torch_ring_bytes")
        elif philox_seed is None:
            a.noise_mode = LS_NOISE_TAPE
            a.eps_tape = m.f32(eps_tape, (n_tape + (sampler == LS_SAMPLER_PLMS), 2, self.batch, self.D))
            a.noise_tape = m.f32(noise_tape, (n_tape,) + self._xshape())
        else:
            a.noise_mode = LS_NOISE_PHILOX
            a.seed, a.sample_offset = int(philox_seed), int(sample_offset)
        a.x_init = m.f32(x_init, self._xshape())
        a.init_image = m.f32(init_image, self._xshape())
        if inp[0] is not None:
            a.inpaint_mask = m.u8(inp[0], self._xshape())
            a.inpainted_motion = m.f32(inp[1], self._xshape())
            a.inpaint_noised = int(bool(inp[3]))
            if inp[2] is not None:
                a.inpaint_noise = m.f32(inp[2], (n_tape,) + self._xshape())
        out, a.out = m.out(self._xshape())
        dumps = None
        if dump_steps:
            ds = np.ascontiguousarray(dump_steps, dtype=np.int32)
            dumps, a.dump_out = m.out((len(ds),) + self._xshape())
            a.n_dump, a.dump_steps = len(ds), ds.ctypes.data_as(c_i32p)
            m.keep.append(ds)
        m.ready()
        if row_keys is not None:
            rk = np.ascontiguousarray(row_keys, dtype=np.uint64).reshape(-1)
            self._check(self.lib.ls_set_torch_ring_bytes(self.h, int(torch_ring_bytes)), "ls_set_torch_ring_bytes")
            self._check(self.lib.ls_set_row_keys(self.h, rk.ctypes.data_as(C.POINTER(C.c_uint64)), int(rk.size)), "ls_set_row_keys")
        try:
            self._check(self.lib.ls_sample(self.h, C.byref(a)), "ls_sample")
        finally:
            if row_keys is not None:
                self._check(self.lib.ls_set_row_keys(self.h, None, 0), "ls_set_row_keys")
        if not last:
            self._segment_inputs = m     # page-locked host tapes of this segment: referenced until the next segment call has returned
            return None
        self._segment_inputs = None
        return (out, dumps) if dump_steps else out

    def _marshal(self, members, device_out=False):
        """A ``_Marshal`` of one call's arrays; ``device_out`` adds a device member, so that the outputs come back as device tensors."""
        if device_out:
            import torch
            members = list(members) + [torch.empty(1, device=torch.device("cuda", self.device))]
        return _Marshal(self.device, *members, stream=self._stream)

    # ---- long-form synthesis ---------------------------------------------------------------------
    def _chain_sampler(self, a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta):
        """The eight fields every chained-window call opens with (ls_long_sample_args & co.); returns n_exec."""
        a.sampler, a.skip_timesteps, a.on_device, a.use_graph = int(sampler), int(skip_timesteps), int(m.on_device), int(bool(use_graph))
        a.clip_denoised, a.two_pass_always, a.eta = int(bool(clip_denoised)), int(bool(two_pass_always)), float(eta)
        return self.n_steps - skip_timesteps

    def _chain_noise(self, a, m, lead, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset, inpaint_noise=None, packed=False):
        """TAPE mode (``philox_seed`` None) with the draws of ``lead`` windows -- ``packed``: of ``lead`` clip-windows, window after window
        at its own batch; ``lead`` None: the call runs no window and takes no tapes -- or PHILOX mode."""
        if philox_seed is not None:
            a.noise_mode = LS_NOISE_PHILOX
            a.seed, a.sample_offset = int(philox_seed), int(sample_offset)
            return
        a.noise_mode = LS_NOISE_TAPE
        if lead is None:
            return
        B, D, x = self.batch, self.D, self._xshape()
        a.x_init = m.f32(x_init, (lead,) + (x[1:] if packed else x))
        a.eps_tape = m.f32(eps_tape, (lead * n_exec * 2 * D,) if packed else (lead, n_exec, 2, B, D))
        a.noise_tape = m.f32(noise_tape, (lead * n_exec * self.J * self.F * self.T,) if packed else (lead, n_exec) + x)
        if inpaint_noise is not None:
            a.inpaint_noise = m.f32(inpaint_noise, (lead, n_exec) + x)

    def _chain_frames(self, a, m, rows, cap):
        """The output of a session's push, ``frames`` [rows, J, F, cap]: the call gets its address unless it has no column."""
        frames, pframes = m.out((rows, self.J, self.F, cap))
        if cap:
            a.frames = pframes
        return frames

    def long_prepare(self, audio, seed_poses, vid_indices, scale, emo=None, n_windows=1, encoder_chunk=None, audio_lengths=None):
        """Once-per-call stage of a long-form call (ls_long_prepare): ``audio`` [B, L] is encoded once for all ``n_windows`` windows
        (zero-padded at the end when short), ``seed_poses`` [B, J, F, n_pre_seq] condition window 0, ``emo`` [W, B] (BEAT).  Replaces
        whatever ``prepare`` left resident.

        ``audio_lengths`` (host [B]): ls_long_prepare_ragged -- every clip runs only the windows its own length needs
        (``long_plan_drop``); ``audio``, ``seed_poses`` and ``audio_lengths`` are in the caller's clip order, ``vid_indices``, ``scale``
        and ``emo`` in slot order, ``n_windows`` is the longest clip's count.  ``long_sample`` then takes packed tapes and slot-ordered
        ``text_features`` (include/ls_hip.h)."""
        B, W = int(audio.shape[0]), int(n_windows)
        npre = int(self.cfg.n_pre_seq)
        m = _Marshal(self.device, audio, seed_poses, vid_indices, scale, emo, stream=self._stream)
        c = LsLongCond(B, W, int(m.on_device), int(encoder_chunk or 0), int(audio.shape[1]), m.f32(audio, (B, int(audio.shape[1]))),
                       m.f32(seed_poses, (B, self.J, self.F, npre)), m.i64(vid_indices, (B,)), m.i64(emo, (W, B)), m.f32(scale, (B,)))
        m.ready()
        if audio_lengths is None:
            self._check(self.lib.ls_long_prepare(self.h, C.byref(c)), "ls_long_prepare")
            self.window_batches = None
        else:
            lens = np.ascontiguousarray(np.asarray(audio_lengths).reshape(-1), dtype=np.int64)
            assert lens.shape == (B,), (lens.shape, B)
            self._check(self.lib.ls_long_prepare_ragged(self.h, C.byref(c), lens.ctypes.data_as(C.c_void_p)), "ls_long_prepare_ragged")
            self.window_batches = [int(n) for n in long_plan_drop(lens, self.cfg.audio_len)[2]]
        self.batch, self.n_windows = B, W

    def long_sample(self, sampler=LS_SAMPLER_DDIM, x_init=None, eps_tape=None, noise_tape=None, skip_timesteps=0, eta=0.0,
                    philox_seed=None, sample_offset=0, use_graph=True, clip_denoised=False, two_pass_always=False, device_out=False,
                    sag=None, text_features=None, return_windows=False):
        """The chained windows of the last ``long_prepare`` (ls_long_sample).  TAPE mode with ``x_init`` [W, B, J, F, T], ``eps_tape``
        [W, n_exec, 2, B, D] and ``noise_tape`` [W, n_exec, B, J, F, T]; PHILOX mode with ``philox_seed``.  ``sag``: a SagEngine whose
        decode of (origin_x_w, ``text_features`` [W, B, D]) starts every window.  Returns the timeline [B, J, F, T + (W-1)(T-n_pre)]
        (and the raw windows [W, B, J, F, T])."""
        B, W, D = self.batch, self.n_windows, self.D
        bw = getattr(self, "window_batches", None)      # a ragged call: packed tapes, window after window at its own batch
        m = self._marshal([x_init, eps_tape, noise_tape, text_features], device_out)
        a = LsLongSampleArgs()
        n_exec = self._chain_sampler(a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta)
        self._chain_noise(a, m, sum(bw) if bw else W, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset, packed=bool(bw))
        if sag is not None:
            a.sag = sag.h
            a.text_features = m.f32(text_features, (W, B, D))
        n_frames = self.T + (W - 1) * (self.T - int(self.cfg.n_pre_seq))
        timeline, a.timeline = m.out((B, self.J, self.F, n_frames))
        windows = None
        if return_windows:
            windows, a.windows = m.out((W,) + self._xshape())
        m.ready()
        self._check(self.lib.ls_long_sample(self.h, C.byref(a)), "ls_long_sample")
        return (timeline, windows) if return_windows else timeline

    def long_edit(self, timeline, frame_lo, frame_hi, channels=None, sampler=LS_SAMPLER_DDIM, x_init=None, eps_tape=None, noise_tape=None,
                  inpaint_noise=None, inpaint_noised=False, skip_timesteps=0, eta=0.0, philox_seed=None, sample_offset=0, use_graph=True,
                  clip_denoised=False, two_pass_always=False, device_out=False, return_windows=False, sag=None, text_features=None, mask=None):
        """Re-synthesise the frames [frame_lo[b], frame_hi[b]) (host int [B]) of ``timeline`` [B, J, F, T + (W-1)(T-n_pre)] on the
        channels ``channels`` (host bytes [B, J*F]; None = all) with the conditioning of the last ``long_prepare`` (ls_long_edit): only
        the windows of ``long_edit_plan`` run, everything else is kept bit for bit.  TAPE mode takes the draws of those We windows,
        ascending: ``x_init`` [We, B, J, F, T], ``eps_tape`` [We, n_exec, 2, B, D], ``noise_tape`` and (``inpaint_noised``)
        ``inpaint_noise`` [We, n_exec, B, J, F, T]; PHILOX mode ``philox_seed``.  Returns (a new timeline, the windows that ran) and, with
        ``return_windows``, their raw samples [We, B, J, F, T]; the caller's timeline is not written.

        ``sag`` (a SagEngine) with ``text_features`` [W, B, D]: the scripted edit (ls_long_edit_sag) -- every window that runs starts
        from the decoder's output on its editable elements and from its slice elsewhere, at every ``skip_timesteps``; rows of
        ``text_features`` for windows that do not run are not read.  One without the other is the engine's to refuse.

        ``mask`` (bool / bytes [B, J*F, N], host or device, NON-ZERO = EDITABLE; with ``frame_lo = frame_hi = channels = None``): the
        edit by element mask (ls_long_edit_mask) -- window w runs iff some clip has a set element on a frame it owns
        (``long_edit_mask_plan``), and everything above holds with that rule in place of the rectangle."""
        B, W, D = self.batch, self.n_windows, self.D
        npre = int(self.cfg.n_pre_seq)
        n_frames = self.T + (W - 1) * (self.T - npre)
        lo = hi = ch = None
        if frame_lo is not None or mask is None:        # together with a mask: the engine's to refuse
            lo = np.ascontiguousarray(np.asarray(frame_lo).reshape(-1), dtype=np.int32)
            hi = np.ascontiguousarray(np.asarray(frame_hi).reshape(-1), dtype=np.int32)
            assert lo.shape == hi.shape == (B,), (lo.shape, hi.shape, B)
        if channels is not None:
            ch = np.ascontiguousarray(np.asarray(channels).reshape(B, self.J * self.F) != 0, dtype=np.uint8)
        if mask is not None:
            plan = [w for w, _ in self.long_edit_mask_plan(mask, W)]
        else:
            try:        # a clip without a selected channel is not edited; what the plan cannot take is the engine's to refuse
                plan = long_edit_plan(lo, np.where(ch.any(axis=1), hi, lo) if ch is not None else hi, W, self.T, npre)
            except ValueError:
                plan = []
        We = len(plan)
        m = self._marshal([timeline, x_init, eps_tape, noise_tape, inpaint_noise, text_features, mask], device_out)
        a = LsLongEditArgs()
        n_exec = self._chain_sampler(a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta)
        a.inpaint_noised = int(bool(inpaint_noised))
        if lo is not None:
            a.frame_lo, a.frame_hi = lo.ctypes.data_as(c_i32p), hi.ctypes.data_as(c_i32p)
        if ch is not None:
            a.channels = ch.ctypes.data_as(C.c_void_p)
        maskp = m.u8(mask, (B, self.J * self.F, n_frames))
        self._chain_noise(a, m, We, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset,
                          inpaint_noise=inpaint_noise if inpaint_noised else None)
        shape = (B, self.J, self.F, n_frames)
        assert tuple(int(s) for s in timeline.shape) == shape, (tuple(timeline.shape), shape)
        if m.on_device:         # a copy of the caller's timeline: the engine edits it in place
            out = m.torch.empty(shape, dtype=m.torch.float32, device=m.dev)
            out.copy_(m.torch.as_tensor(timeline))
            a.timeline = C.c_void_p(out.data_ptr())
        else:
            out = np.array(timeline.detach().cpu().numpy() if hasattr(timeline, "detach") else timeline, dtype=np.float32, order="C", copy=True)
            a.timeline = out.ctypes.data_as(C.c_void_p)
        windows = None
        if return_windows and We:
            windows, a.windows = m.out((We,) + self._xshape())
        ran, n_ran = np.full(max(W, 1), -1, np.int32), C.c_int32(0)
        a.windows_run, a.windows_capacity, a.n_windows_run = ran.ctypes.data_as(c_i32p), W, C.pointer(n_ran)
        text = m.f32(text_features, (W, B, D))
        m.ready()
        if mask is not None:
            self._check(self.lib.ls_long_edit_mask(self.h, C.byref(a), None if sag is None else sag.h, text, maskp), "ls_long_edit_mask")
        elif sag is None and text_features is None:
            self._check(self.lib.ls_long_edit(self.h, C.byref(a)), "ls_long_edit")
        else:
            self._check(self.lib.ls_long_edit_sag(self.h, C.byref(a), None if sag is None else sag.h, text), "ls_long_edit_sag")
        ran = [int(w) for w in ran[:int(n_ran.value)]]
        assert ran == plan, (ran, plan)
        return (out, ran, windows) if return_windows else (out, ran)

    def long_edit_mask_pairs(self, mask, n_windows, frames=None):
        """The pair flags of an element mask as the device computes them (ls_long_edit_mask_pairs; ``k_edit_mask_pairs``): uint8
        [n_windows, B], 1 where clip b has a set element on a frame window w owns.  ``mask``: bool / bytes [B, J*F, N], host (uploaded
        first) or device (read in place; only the flags cross to the host).  ``frames``: host int [B] or None.  A set element at or
        beyond ``frames[b]`` is the engine's to refuse."""
        B, W = int(mask.shape[0]), int(n_windows)
        n_frames = self.T + (W - 1) * (self.T - int(self.cfg.n_pre_seq))
        fr = None if frames is None else np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int32)
        assert fr is None or fr.shape == (B,), (fr.shape, B)
        m = _Marshal(self.device, mask, stream=self._stream)
        maskp = m.u8(mask, (B, self.J * self.F, n_frames))
        flags = np.zeros((W, B), np.uint8)
        m.ready()
        self._check(self.lib.ls_long_edit_mask_pairs(self.h, maskp, int(m.on_device), B, W, None if fr is None else fr.ctypes.data_as(c_i32p),
                                                     flags.ctypes.data_as(C.c_void_p)), "ls_long_edit_mask_pairs")
        return flags

    def long_edit_mask_plan(self, mask, n_windows, frames=None):
        """The clip-windows of an element mask [B, J*F, N] as ``[(w, rows)]``.  A host mask: ``long_edit_plan_mask`` (no GPU; a set
        element beyond ``frames[b]``: ``ValueError``).  A device mask stays on the device: the plan is read off the W * B pair flags
        of ``long_edit_mask_pairs``, as the engine reads it."""
        if _is_cuda(mask):
            flags = self.long_edit_mask_pairs(mask, n_windows, frames)
            return [(w, np.flatnonzero(flags[w]).astype(np.int32)) for w in range(int(n_windows)) if flags[w].any()]
        host = mask.detach().numpy() if hasattr(mask, "detach") else np.asarray(mask)
        return long_edit_plan_mask(host, n_windows, frames, self.T, int(self.cfg.n_pre_seq))

    def long_prepare_edit(self, audio, seed_poses, vid_indices, scale, frame_lo, frame_hi, channels=None, emo=None, n_windows=1,
                          encoder_chunk=None, audio_lengths=None, mask=None):
        """Once-per-call stage of a COMPACT timeline edit (ls_long_prepare_edit): the conditioning of ``long_prepare``, everything in
        the caller's clip order, plus the edit's ranges (host int [B]) and ``channels`` (host bytes [B, J*F]; None = all).  Only the
        clip-windows of ``long_edit_plan_compact`` go through the WavEncoder.  ``audio_lengths`` (host [B]): clips of different
        lengths -- ``n_windows`` is the longest clip's count, a clip has only its own windows, and ``audio`` at and beyond a clip's
        length is never read.  Sets ``edit_plan``: the list of ``(w, rows)``.

        ``mask`` (bool / bytes [B, J*F, N], host or device, non-zero = editable; with ``frame_lo = frame_hi = channels = None``): the
        plan of the element mask (ls_long_prepare_edit_mask; ``long_edit_mask_plan``)."""
        B, W = int(audio.shape[0]), int(n_windows)
        npre = int(self.cfg.n_pre_seq)
        assert mask is None or (frame_lo is None and frame_hi is None and channels is None), "the prepare takes a mask or ranges"
        lo = hi = ch = None
        if mask is None:
            lo = np.ascontiguousarray(np.asarray(frame_lo).reshape(-1), dtype=np.int32)
            hi = np.ascontiguousarray(np.asarray(frame_hi).reshape(-1), dtype=np.int32)
            assert lo.shape == hi.shape == (B,), (lo.shape, hi.shape, B)
            ch = None if channels is None else np.ascontiguousarray(np.asarray(channels).reshape(B, self.J * self.F) != 0, dtype=np.uint8)
        lens = frames = None
        if audio_lengths is not None:
            lens = np.ascontiguousarray(np.asarray(audio_lengths).reshape(-1), dtype=np.int64)
            assert lens.shape == (B,), (lens.shape, B)
        m = _Marshal(self.device, audio, seed_poses, vid_indices, scale, emo, mask, stream=self._stream)
        c = LsLongCond(B, W, int(m.on_device), int(encoder_chunk or 0), int(audio.shape[1]), m.f32(audio, (B, int(audio.shape[1]))),
                       m.f32(seed_poses, (B, self.J, self.F, npre)), m.i64(vid_indices, (B,)), m.i64(emo, (W, B)), m.f32(scale, (B,)))
        maskp = m.u8(mask, (B, self.J * self.F, self.T + (W - 1) * (self.T - npre)))
        m.ready()
        lensp = None if lens is None else lens.ctypes.data_as(C.c_void_p)
        if mask is not None:
            self._check(self.lib.ls_long_prepare_edit_mask(self.h, C.byref(c), lensp, maskp), "ls_long_prepare_edit_mask")
        else:
            self._check(self.lib.ls_long_prepare_edit(self.h, C.byref(c), lensp, lo.ctypes.data_as(c_i32p), hi.ctypes.data_as(c_i32p),
                                                      None if ch is None else ch.ctypes.data_as(C.c_void_p)), "ls_long_prepare_edit")
        if lens is not None:        # frames per clip: what ls_long_plan_drop's window counts stitch to
            row, wins, _ = long_plan_drop(lens, self.cfg.audio_len)
            frames = np.empty(B, np.int32)
            frames[row] = self.T + (wins - 1) * (self.T - npre)
        self.edit_plan = self.long_edit_mask_plan(mask, W, frames) if mask is not None else long_edit_plan_compact(lo, hi, W, ch, frames, self.T, npre)
        self.batch, self.n_windows, self.window_batches = B, W, None

    def long_edit_compact(self, timeline, frame_lo, frame_hi, channels=None, sampler=LS_SAMPLER_DDIM, x_init=None, eps_tape=None,
                          noise_tape=None, inpaint_noise=None, inpaint_noised=False, skip_timesteps=0, eta=0.0, philox_seed=None,
                          sample_offset=0, use_graph=True, clip_denoised=False, two_pass_always=False, device_out=False, return_windows=False,
                          sag=None, text_features=None, mask=None):
        """The planned clip-windows of the last ``long_prepare_edit`` (ls_long_edit_compact): window w is one sampling call at batch
        ``len(rows)`` on its rows.  ``frame_lo`` / ``frame_hi`` / ``channels`` repeat the prepared ones.  TAPE mode takes packed
        tapes, window after window at its own batch: ``x_init`` [n_pairs, J, F, T], flat ``eps_tape`` / ``noise_tape`` /
        ``inpaint_noise`` holding per window [n_exec, 2, A_w, D] / [n_exec, A_w, J, F, T]; PHILOX mode ``philox_seed`` (clip b of
        window w draws at ``sample_offset + b + (w << 48)``).  ``sag`` with ``text_features`` [W, B, D] in clip order: the scripted
        edit.  Returns (a new timeline, the plan ``[(w, rows)]``) and, with ``return_windows``, the raw samples [n_pairs, J, F, T].

        ``mask`` (with ``frame_lo = frame_hi = channels = None``): the element mask ``long_prepare_edit(mask=)`` was given
        (ls_long_edit_compact_mask); one whose clip-windows differ from the prepared ones is the engine's to refuse."""
        B, W, D = self.batch, self.n_windows, self.D
        n_frames = self.T + (W - 1) * (self.T - int(self.cfg.n_pre_seq))
        lo = hi = None
        if frame_lo is not None or mask is None:        # together with a mask: the engine's to refuse
            lo = np.ascontiguousarray(np.asarray(frame_lo).reshape(-1), dtype=np.int32)
            hi = np.ascontiguousarray(np.asarray(frame_hi).reshape(-1), dtype=np.int32)
            assert lo.shape == hi.shape == (B,), (lo.shape, hi.shape, B)
        ch = None if channels is None else np.ascontiguousarray(np.asarray(channels).reshape(B, self.J * self.F) != 0, dtype=np.uint8)
        plan = getattr(self, "edit_plan", None) or []
        n_pairs = sum(len(rows) for _, rows in plan)
        m = self._marshal([timeline, x_init, eps_tape, noise_tape, inpaint_noise, text_features, mask], device_out)
        a = LsLongEditCompactArgs()
        n_exec = self._chain_sampler(a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta)
        a.inpaint_noised = int(bool(inpaint_noised))
        if lo is not None:
            a.frame_lo, a.frame_hi = lo.ctypes.data_as(c_i32p), hi.ctypes.data_as(c_i32p)
        if ch is not None:
            a.channels = ch.ctypes.data_as(C.c_void_p)
        maskp = m.u8(mask, (B, self.J * self.F, n_frames))
        self._chain_noise(a, m, n_pairs, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset, packed=True)
        if philox_seed is None and inpaint_noised:
            a.inpaint_noise = m.f32(inpaint_noise, (n_pairs * n_exec * self.J * self.F * self.T,))
        shape = (B, self.J, self.F, n_frames)
        assert tuple(int(s) for s in timeline.shape) == shape, (tuple(timeline.shape), shape)
        if m.on_device:         # a copy of the caller's timeline: the engine edits it in place
            out = m.torch.empty(shape, dtype=m.torch.float32, device=m.dev)
            out.copy_(m.torch.as_tensor(timeline))
            a.timeline = C.c_void_p(out.data_ptr())
        else:
            out = np.array(timeline.detach().cpu().numpy() if hasattr(timeline, "detach") else timeline, dtype=np.float32, order="C", copy=True)
            a.timeline = out.ctypes.data_as(C.c_void_p)
        windows = None
        if return_windows and n_pairs:
            windows, a.windows = m.out((n_pairs, self.J, self.F, self.T))
        ran, n_ran, n_rows = np.full(max(W, 1), -1, np.int32), C.c_int32(0), C.c_int32(0)
        a.windows_run, a.windows_capacity, a.n_windows_run, a.rows_run = ran.ctypes.data_as(c_i32p), W, C.pointer(n_ran), C.pointer(n_rows)
        text = m.f32(text_features, (W, B, D))
        m.ready()
        if mask is not None:
            self._check(self.lib.ls_long_edit_compact_mask(self.h, C.byref(a), None if sag is None else sag.h, text, maskp), "ls_long_edit_compact_mask")
        else:
            self._check(self.lib.ls_long_edit_compact(self.h, C.byref(a), None if sag is None else sag.h, text), "ls_long_edit_compact")
        ran = [int(w) for w in ran[:int(n_ran.value)]]
        self.rows_run = int(n_rows.value)          # the clip-windows that ran (ls_long_edit_compact_args.rows_run)
        assert ran == [w for w, _ in plan] and self.rows_run == n_pairs, (ran, plan, self.rows_run)
        return (out, plan, windows) if return_windows else (out, plan)

    # ---- streaming long-form synthesis -----------------------------------------------------------
    def long_stream_open(self, seed_poses, vid_indices, scale):
        """Open a stream at batch B (ls_long_stream_open): a session of B slots, every slot joined here.  Replaces whatever ``prepare`` /
        ``long_prepare`` / ``long_pool_open`` left resident; any of those ends the stream in turn."""
        B = int(seed_poses.shape[0])
        m = _Marshal(self.device, seed_poses, vid_indices, scale, stream=self._stream)
        c = LsLongStreamCond(B, int(m.on_device), m.f32(seed_poses, (B, self.J, self.F, int(self.cfg.n_pre_seq))), m.i64(vid_indices, (B,)),
                             m.f32(scale, (B,)))
        m.ready()
        self._check(self.lib.ls_long_stream_open(self.h, C.byref(c)), "ls_long_stream_open")
        self.batch, self.n_windows, self.window_batches = B, 0, None

    def long_stream_push(self, audio, closing=False, emo=None, sag=None, text_features=None, sampler=LS_SAMPLER_DDIM, x_init=None,
                         eps_tape=None, noise_tape=None, skip_timesteps=0, eta=0.0, philox_seed=None, sample_offset=0, use_graph=True,
                         clip_denoised=False, two_pass_always=False, device_out=False, inpaint_noise=None):
        """Feed ``audio`` [B, n] (n >= 0) to the open stream and run the k windows that complete (ls_long_stream_push; ``closing``: also
        the zero-padded ones still owed).  ``emo`` [B] / ``text_features`` [B, D] replace the held conditioning.  TAPE mode takes the
        draws of exactly those k windows (``x_init`` [k, B, J, F, T], ``eps_tape`` [k, n_exec, 2, B, D], ``noise_tape`` [k, n_exec, B, J, F,
        T]; ``long_stream_plan`` tells k), PHILOX mode ``philox_seed``.  ``inpaint_noise`` (TAPE mode on the TED model, a stream with pins):
        the re-noise draws of the kp windows that run pinned, [kp, n_exec, B, J, F, T] (``long_pool_pin_tape``).  Returns
        ``(frames [B, J, F, 34 | 30 per window], k)``."""
        B, D = self.batch, self.D
        n = int(audio.shape[1])
        assert tuple(int(s) for s in audio.shape) == (B, n), (tuple(audio.shape), B)
        info = self.long_stream_info()
        first, k = long_stream_plan(info["samples_in"], n, self.cfg.audio_len, closing)
        npre = int(self.cfg.n_pre_seq)
        cap = k * (self.T - npre) + (npre if (k and first == 0) else 0)
        m = self._marshal([audio if n else None, emo, text_features] + ([x_init, eps_tape, noise_tape, inpaint_noise] if k else []), device_out)
        a = LsLongStreamPushArgs()
        n_exec = self._chain_sampler(a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta)
        a.closing, a.capacity, a.n_samples = int(bool(closing)), cap, n
        if n:
            a.audio = m.f32(audio, (B, n))
        a.emo = m.i64(emo, (B,))
        if sag is not None:
            a.sag = sag.h
            a.text_features = m.f32(text_features, (B, D))
        self._chain_noise(a, m, k or None, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset)
        frames = self._chain_frames(a, m, B, cap)
        n_frames, n_windows = C.c_int32(-1), C.c_int32(-1)
        a.n_frames, a.n_windows = C.pointer(n_frames), C.pointer(n_windows)
        renoise = self._pin_tape(m, inpaint_noise if k else None)
        m.ready()
        renoise()
        self._check(self.lib.ls_long_stream_push(self.h, C.byref(a)), "ls_long_stream_push")
        assert (int(n_frames.value), int(n_windows.value)) == (cap, k), (n_frames.value, n_windows.value, cap, k)
        if k == 0:          # nothing was waited for: torch's stream must not reuse the chunk before the engine's stream has read it
            m.done_async()
        return frames, k

    def long_stream_info(self) -> dict:
        """ls_long_stream_info of the current (or last) stream: samples_in, windows_run, frames_out, and device_bytes -- what the
        session holds for its B slots, as ``long_pool_info`` counts it."""
        out = (C.c_int64 * 4)()
        self._check(self.lib.ls_long_stream_info(self.h, out), "ls_long_stream_info")
        return {"samples_in": int(out[0]), "windows_run": int(out[1]), "frames_out": int(out[2]), "device_bytes": int(out[3])}

    # ---- session pool: streams that join and leave ------------------------------------------------
    def long_pool_open(self, capacity):
        """A pool of ``capacity`` slots (ls_long_pool_open): everything a round can touch is allocated here.  Replaces whatever
        ``prepare`` / ``long_prepare`` / ``long_stream_open`` left resident; any of those ends the pool in turn."""
        self._check(self.lib.ls_long_pool_open(self.h, int(capacity)), "ls_long_pool_open")
        self.batch, self.n_windows, self.window_batches = int(capacity), 0, None

    def long_pool_keyed(self, on=True):
        """PHILOX draws that follow the clip (ls_long_pool_keyed): on a pool nobody has joined yet."""
        self._check(self.lib.ls_long_pool_keyed(self.h, int(bool(on))), "ls_long_pool_keyed")

    def long_pool_set_key(self, slot, key):
        """The key in [0, 2^48) of the clip in ``slot`` of a keyed pool (ls_long_pool_set_key): after its join, ahead of its first window."""
        self._check(self.lib.ls_long_pool_set_key(self.h, int(slot), int(key)), "ls_long_pool_set_key")

    def long_pool_join(self, slot, seed_poses, vid_index, scale, emo=None, text_features=None):
        """Fill the free slot ``slot`` (ls_long_pool_join): ``seed_poses`` [J, F, n_pre], one speaker id, one scale, and the held
        ``emo`` id (BEAT) / ``text_features`` [D]."""
        as1 = lambda a: None if a is None else (a.reshape(1) if hasattr(a, "reshape") else np.asarray(a).reshape(1))      # noqa: E731
        vid_index, scale, emo = as1(vid_index), as1(scale), as1(emo)
        m = _Marshal(self.device, seed_poses, vid_index, scale, emo, text_features, stream=self._stream)
        a = LsLongPoolJoinArgs(int(slot), int(m.on_device), m.f32(seed_poses, (self.J, self.F, int(self.cfg.n_pre_seq))), m.i64(vid_index, (1,)),
                               m.f32(scale, (1,)), m.i64(emo, (1,)), m.f32(text_features, (self.D,)))
        m.ready()
        self._check(self.lib.ls_long_pool_join(self.h, C.byref(a)), "ls_long_pool_join")

    def long_pool_push(self, audio, lengths, closing=None, emo=None, text_features=None, given=None, sag=None, sampler=LS_SAMPLER_DDIM,
                       x_init=None, eps_tape=None, noise_tape=None, skip_timesteps=0, eta=0.0, philox_seed=None, sample_offset=0,
                       use_graph=True, clip_denoised=False, two_pass_always=False, device_out=False, inpaint_noise=None):
        """Feed the ragged chunk ``audio`` [S, n_max] -- ``lengths`` [S] (host) samples per slot -- and run the rounds of
        ``long_pool_plan`` (ls_long_pool_push).  ``closing`` [S] (host): the slot leaves after the windows it is owed.  ``emo`` [S] /
        ``text_features`` [S, D] replace the held conditioning of the slots whose ``given`` [S] (host) has bit 0 / bit 1 set.  TAPE mode
        takes the draws packed round after round at each round's batch A (``x_init`` [sum A, J, F, T], flat ``eps_tape`` / ``noise_tape``
        holding per round [n_exec, 2, A, D] / [n_exec, A, J, F, T]), PHILOX mode ``philox_seed`` (a keyed pool, ``long_pool_keyed``, draws
        at the slots' keys and does not read ``sample_offset``).  A pool with pending pins (``long_pool_pin``) runs the calls of
        ``long_pool_pin_plan`` in place of bare rounds: the tapes are then packed call after call, and ``inpaint_noise`` (TAPE mode on
        the TED model) holds the re-noise draws of the pinned calls, flat, per call [n_exec, A, J, F, T].  Returns ``(frames [S, J, F, K], counts
        int32 [S], rounds)`` with K the most frames any slot got; a slot's row is zero behind its own count."""
        info = self.long_pool_info()        # of the last pool, whatever has been prepared on the handle since
        S, D = info["capacity"], self.D
        n = int(audio.shape[1])
        assert tuple(int(s) for s in audio.shape) == (S, n), (tuple(audio.shape), S)
        lens = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int64)
        cl = np.ascontiguousarray(np.zeros(S) if closing is None else np.asarray(closing).reshape(-1), dtype=np.int32)
        gv = None if given is None else np.ascontiguousarray(np.asarray(given).reshape(-1), dtype=np.int32)
        assert lens.shape == cl.shape == (S,) and (gv is None or gv.shape == (S,)), (lens.shape, cl.shape, S)
        rounds, per_slot = long_pool_plan(info["samples_in"], info["windows_run"], lens, cl, info["open"], self.cfg.audio_len)
        cap, rows = int(per_slot.max()), sum(len(r) for r in rounds)
        m = self._marshal([audio if n else None, emo, text_features] + ([x_init, eps_tape, noise_tape, inpaint_noise] if rows else []), device_out)
        a = LsLongPoolPushArgs()
        n_exec = self._chain_sampler(a, m, sampler, skip_timesteps, use_graph, clip_denoised, two_pass_always, eta)
        a.capacity, a.n_max = cap, n
        if n:
            a.audio = m.f32(audio, (S, n))
        a.lengths, a.closing = lens.ctypes.data_as(c_i64p), cl.ctypes.data_as(c_i32p)
        if gv is not None:
            a.given = gv.ctypes.data_as(c_i32p)
        a.emo = m.i64(emo, (S,))
        if sag is not None:
            a.sag = sag.h
        a.text_features = m.f32(text_features, (S, D))
        self._chain_noise(a, m, rows or None, n_exec, x_init, eps_tape, noise_tape, philox_seed, sample_offset, packed=True)
        frames = self._chain_frames(a, m, S, cap)
        counts, n_rounds = np.full(S, -1, np.int32), C.c_int32(-1)
        a.n_frames, a.n_rounds = counts.ctypes.data_as(c_i32p), C.pointer(n_rounds)
        renoise = self._pin_tape(m, inpaint_noise if rows else None)
        m.ready()
        renoise()
        self._check(self.lib.ls_long_pool_push(self.h, C.byref(a)), "ls_long_pool_push")
        assert counts.tolist() == per_slot.tolist() and int(n_rounds.value) == len(rounds), (counts, per_slot, n_rounds.value, rounds)
        if not rounds:      # nothing was waited for: torch's stream must not reuse the chunk before the engine's stream has read it
            m.done_async()
        return frames, counts, rounds

    # ---- pinned poses for frames a session has yet to make (a pool and a stream alike) -----------
    def long_pool_pins(self, horizon):
        """Enable pins on the open session (ls_long_pool_pins): a pool nobody has joined, a stream nothing was pushed to.  ``horizon``
        >= nframes: a pin may name a frame in ``[frames_out, frames_out + horizon)``.  The store and the inpainting planes are allocated here."""
        self._check(self.lib.ls_long_pool_pins(self.h, int(horizon)), "ls_long_pool_pins")

    def long_pool_pin(self, slot, frames, poses, mask=None):
        """Pin elements of K frames the clip in ``slot`` has not returned yet (ls_long_pool_pin): ``frames`` [K] host ints (series
        frames, distinct), ``poses`` [J, F, K], ``mask`` [J, F, K] bool (True = pinned; None: the whole pose), host or device."""
        fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int64)
        K = int(fr.size)
        m = _Marshal(self.device, poses, mask, stream=self._stream)
        pp, pm = m.f32(poses, (self.J, self.F, K)), m.u8(mask, (self.J, self.F, K))
        m.ready()
        self._check(self.lib.ls_long_pool_pin(self.h, int(slot), K, fr.ctypes.data_as(c_i64p), pp, pm, int(m.on_device)), "ls_long_pool_pin")

    def long_pool_unpin(self, slot, frames=None):
        """Drop the pins of ``frames`` (host ints) of ``slot``, or with None all of them (ls_long_pool_unpin)."""
        if frames is None:
            self._check(self.lib.ls_long_pool_unpin(self.h, int(slot), 0, None), "ls_long_pool_unpin")
            return
        fr = np.ascontiguousarray(np.asarray(frames).reshape(-1), dtype=np.int64)
        self._check(self.lib.ls_long_pool_unpin(self.h, int(slot), int(fr.size), fr.ctypes.data_as(c_i64p)), "ls_long_pool_unpin")

    def _pin_tape(self, m, inpaint_noise):
        """The re-noise tape of the coming push's pinned calls through ``m``; returns the call that hands it over (ls_long_pool_pin_tape),
        to be made once ``m`` is ready.  None: nothing to hand over."""
        if inpaint_noise is None:
            return lambda: None
        n = int(np.prod(tuple(inpaint_noise.shape)))
        ptr = m.f32(inpaint_noise)
        return lambda: self._check(self.lib.ls_long_pool_pin_tape(self.h, ptr, n, int(m.on_device)), "ls_long_pool_pin_tape")

    def long_pool_pin_info(self) -> dict:
        """ls_long_pool_pin_info: ``pending`` int32 [S] -- the pinned frames of each slot whose window has yet to run -- and the ints
        ``horizon`` and ``ring`` (0 where the session has no pins)."""
        S = self.long_pool_info()["capacity"] or int(self.batch or 0)
        pend, misc = np.zeros(max(S, 1), np.int32), (C.c_int64 * 2)()
        self._check(self.lib.ls_long_pool_pin_info(self.h, S, pend.ctypes.data_as(c_i32p), misc), "ls_long_pool_pin_info")
        return {"pending": pend[:S].copy(), "horizon": int(misc[0]), "ring": int(misc[1])}

    def long_pool_info(self) -> dict:
        """ls_long_pool_info of the current (or last) pool: per-slot numpy arrays samples_in, windows_run, frames_out (int64) and open
        (bool), and the ints capacity, device_bytes, rounds, is_open."""
        misc = (C.c_int64 * 4)()
        self._check(self.lib.ls_long_pool_info(self.h, 0, None, None, None, None, misc), "ls_long_pool_info")
        S = int(misc[0])
        fed, ran, out = (np.zeros(max(S, 1), np.int64) for _ in range(3))
        opened = np.zeros(max(S, 1), np.int32)
        p64 = lambda a: a.ctypes.data_as(c_i64p)      # noqa: E731
        self._check(self.lib.ls_long_pool_info(self.h, S, p64(fed), p64(ran), p64(out), opened.ctypes.data_as(c_i32p), misc), "ls_long_pool_info")
        return {"samples_in": fed[:S], "windows_run": ran[:S], "frames_out": out[:S], "open": opened[:S].astype(bool), "capacity": S,
                "device_bytes": int(misc[1]), "rounds": int(misc[2]), "is_open": bool(misc[3])}

    def q_sample(self, index, x_start, noise):
        m = _Marshal(self.device, x_start, noise, stream=self._stream)
        out, pout = m.out(tuple(x_start.shape))
        n = int(np.prod(x_start.shape))
        m.ready()
        self._check(self.lib.ls_q_sample(self.h, index, int(m.on_device), n, m.f32(x_start), m.f32(noise), pout), "ls_q_sample")
        return out

    def vb_terms(self, x_start, x_t, pred_xstart, noise=None, index=0, indices=None, clip_denoised=False):
        """k_vb_terms alone on caller-given planes [B, J, F, T] (ls_vb_terms): the second half of _vb_terms_bpd plus the two MSEs of
        calc_bpd_loop.  ``indices`` ([B] int64, numpy / CPU tensor = validated on the host, CUDA tensor = clamped on the device) or the
        uniform ``index``.  Returns (vb [B], xstart_mse [B], mse [B] or None without ``noise``, the pred_xstart plane used)."""
        m = _Marshal(self.device, x_start, x_t, pred_xstart, noise, stream=self._stream)
        B = self.batch
        vb, pvb = m.out((B,))
        xs, pxs = m.out((B,))
        ms, pms = m.out((B,)) if noise is not None else (None, None)
        px, ppx = m.out(self._xshape())
        a = LsVbTermsArgs()
        a.index, a.on_device, a.clip_denoised = int(index), int(m.on_device), int(bool(clip_denoised))
        if indices is not None:
            if _is_cuda(indices):
                if not m.on_device:
                    raise EngineError("device `indices` need device tensors for the other arguments")
                t = indices.to(dtype=m.torch.int64).contiguous()
                shape, a.indices, a.indices_on_device = tuple(t.shape), C.c_void_p(t.data_ptr()), 1
            else:
                t = np.ascontiguousarray(indices.detach().cpu().numpy() if hasattr(indices, "detach") else indices, dtype=np.int64)
                shape, a.indices = t.shape, t.ctypes.data_as(C.c_void_p)
            if tuple(shape) != (B,):
                raise EngineError(f"indices must be [{B}], got {tuple(shape)}")
            m.keep.append(t)
        a.x_start, a.x_t = m.f32(x_start, self._xshape()), m.f32(x_t, self._xshape())
        a.pred_xstart, a.noise = m.f32(pred_xstart, self._xshape()), m.f32(noise, self._xshape())
        a.vb_out, a.xstart_mse_out, a.mse_out, a.pred_out = pvb, pxs, pms, ppx
        m.ready()
        self._check(self.lib.ls_vb_terms(self.h, C.byref(a)), "ls_vb_terms")
        return vb, xs, ms, px

    def bpd(self, x_start, out, columns=None, noise_tape=None, eps_tape=None, philox_seed=None, sample_offset=0, use_graph=True,
            clip_denoised=True, two_pass_always=False):
        """Columns ``columns`` = (first, count) (default: all) of calc_bpd_loop (ls_bpd) into ``out`` = (vb, xstart_mse, mse), three
        float32 C-contiguous [B, n_steps] arrays (all numpy, or all torch CUDA tensors on this GPU) of which only those columns are
        written.  TAPE mode with ``noise_tape`` [count, B, J, F, T] and ``eps_tape`` [count, 2, B, D]; PHILOX mode with ``philox_seed``."""
        k0, n = (0, self.n_steps) if columns is None else (int(columns[0]), int(columns[1]))
        m = _Marshal(self.device, x_start, noise_tape, eps_tape, *out, stream=self._stream)
        a = LsBpdArgs()
        a.on_device, a.use_graph, a.clip_denoised = int(m.on_device), int(bool(use_graph)), int(bool(clip_denoised))
        a.two_pass_always, a.col_begin, a.col_count = int(bool(two_pass_always)), k0, n
        a.x_start = m.f32(x_start, self._xshape())
        if philox_seed is None:
            a.noise_mode = LS_NOISE_TAPE
            a.noise_tape = m.f32(noise_tape, (n,) + self._xshape())
            a.eps_tape = m.f32(eps_tape, (n, 2, self.batch, self.D))
        else:
            a.noise_mode = LS_NOISE_PHILOX
            a.seed, a.sample_offset = int(philox_seed), int(sample_offset)
        ptrs = []
        for o in out:
            ok = (tuple(o.shape) == (self.batch, self.n_steps) and
                  (_is_cuda(o) and o.is_contiguous() and str(o.dtype) == "torch.float32" if m.on_device else
                   isinstance(o, np.ndarray) and o.dtype == np.float32 and o.flags.c_contiguous))
            if not ok:
                raise EngineError(f"bpd: outputs must be float32 C-contiguous [{self.batch}, {self.n_steps}] "
                                  f"{'CUDA tensors' if m.on_device else 'numpy arrays'}")
            ptrs.append(C.c_void_p(o.data_ptr()) if m.on_device else o.ctypes.data_as(C.c_void_p))
        a.vb, a.xstart_mse, a.mse = ptrs
        m.ready()
        self._check(self.lib.ls_bpd(self.h, C.byref(a)), "ls_bpd")
        return out

    def torch_randn(self, seed, offset, out):
        """Fill the CUDA float32 tensor ``out`` (contiguous, on this engine's GPU) with what ``torch.randn(out.numel())`` draws from a
        device generator at (seed, offset); the generator is neither read nor moved.  Waits for the GPU."""
        import torch
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()):
            raise EngineError("torch_randn: out must be a contiguous float32 CUDA tensor")
        torch.cuda.synchronize(out.device)
        self._check(self.lib.ls_torch_randn(self.h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), out.numel(), C.c_void_p(out.data_ptr()), 0),
                    "ls_torch_randn")
        return out

    def philox_x_init(self, batch, seed, sample_offset=0) -> np.ndarray:
        out = np.empty((batch, self.J, self.F, self.T), np.float32)
        self._check(self.lib.ls_philox_x_init(self.h, batch, int(seed), int(sample_offset), 0,
                                              out.ctypes.data_as(C.c_void_p)), "ls_philox_x_init")
        return out

    def read(self, name: str) -> np.ndarray:
        shapes = {"audio_feat": (self.batch, self.T, 256), "static_c": (self.batch, self.T, self.D),
                  "static_u": (self.batch, self.T, self.D), "z_mu": (self.batch, self.D),
                  "z_logvar": (self.batch, self.D), "z_std": (self.batch, self.D), "temb": (self.n_steps, self.D)}
        out = np.empty(shapes[name], np.float32)
        n = self._check(self.lib.ls_read(self.h, name.encode(), out.ctypes.data_as(c_f32p), out.size), f"ls_read({name})")
        assert n == out.size
        return out

    def synchronize(self):
        """Wait for everything enqueued on the engine's stream (an asynchronous prepare included)."""
        self._check(self.lib.ls_synchronize(self.h), "ls_synchronize")

    def timing(self) -> dict:
        t = LsTiming()
        self.lib.ls_get_timing(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in LsTiming._fields_}


class SagEngine(_Handle):
    """ctypes wrapper of the SAG decoder handle (ls_sag_*): Decoder_TRANSFORMER.forward on the GPU."""

    _prefix = "ls_sag_"

    def __init__(self, njoints=9, nfeats=3, nframes=34, latent_dim=512, ff_size=1024, num_layers=3, num_heads=4,
                 n_pre_poses=4, device=0):
        self._create(LsSagConfig(njoints, nfeats, nframes, latent_dim, ff_size, num_layers, num_heads, n_pre_poses, device, 0))
        self.J, self.F, self.T, self.D, self.device = njoints, nfeats, nframes, latent_dim, device
        self._async_inputs = None

    def load_state_dict(self, sd: dict):
        self._set_weights(sd)

    def last_decode_ms(self) -> float:
        return float(self.lib.ls_sag_last_decode_ms(self.h))

    def decode(self, x, z, mask=None, wait=True):
        """``wait=False`` (device tensors only): enqueue on the decoder's stream and return at once; the output tensor is complete once
        that stream has reached this point -- ``order_after(self, other_engine)`` / ``stream_order`` puts a consumer behind it."""
        m = _Marshal(self.device, x, z, mask, stream=self._stream)
        B = int(x.shape[0])
        out, pout = m.out((B, self.J, self.F, self.T))
        pmask = m.u8(mask)
        m.ready()
        if not wait:
            if not m.on_device:
                raise EngineError("decode(wait=False) needs device tensors")
            self._check(self.lib.ls_sag_decode_async(self.h, B, m.f32(x, (B, self.J, self.F, self.T)), m.f32(z, (B, self.D)), pmask, pout),
                        "ls_sag_decode_async")
            self._async_inputs = m          # the marshalled inputs stay referenced until the next decode on this (in-order) stream
            return out
        self._check(self.lib.ls_sag_decode(self.h, B, int(m.on_device), m.f32(x, (B, self.J, self.F, self.T)),
                                           m.f32(z, (B, self.D)), pmask, pout), "ls_sag_decode")
        self._async_inputs = None
        return out


class SagEncoderEngine(_Handle):
    """ctypes wrapper of the SAG encoder handle (ls_sag_enc_*): Encoder_TRANSFORMER.forward (eval mode) on the GPU."""

    _prefix = "ls_sag_enc_"

    def __init__(self, njoints=9, nfeats=3, nframes=34, latent_dim=512, ff_size=1024, num_layers=3, num_heads=4, device=0):
        self._create(LsSagConfig(njoints, nfeats, nframes, latent_dim, ff_size, num_layers, num_heads, 0, device, 0))
        self.J, self.F, self.T, self.D, self.device = njoints, nfeats, nframes, latent_dim, device
        self._async_inputs = None

    def load_state_dict(self, sd: dict):
        self._set_weights(sd)

    def last_encode_ms(self) -> float:
        return float(self.lib.ls_sag_enc_last_encode_ms(self.h))

    def encode(self, x, mask=None, wait=True):
        """x [B, J, F, T], mask [B, T] bool (False = padded frame) or None -> mu [B, latent]: numpy in, numpy out; device tensors in, a
        device tensor out.  ``wait=False`` (device tensors only): enqueue on the encoder's stream and return at once, without a host
        wait.  torch's current stream is ordered behind the encode, so torch operations on ``mu`` issued from now on see it complete; a
        consumer on another stream (the decoder's) is put behind it with ``stream_order(device, self._stream, that_stream)``."""
        shape = tuple(int(s) for s in x.shape)
        if len(shape) != 4 or shape[1:] != (self.J, self.F, self.T):
            raise ValueError(f"x must be [B, {self.J}, {self.F}, {self.T}], got {list(shape)}")
        B = shape[0]
        if B < 1:
            raise ValueError("x holds no clip")
        if mask is not None and tuple(int(s) for s in mask.shape) != (B, self.T):
            raise ValueError(f"mask must be [{B}, {self.T}], got {list(mask.shape)}")
        m = _Marshal(self.device, x, mask, stream=self._stream)
        if not wait and not m.on_device:
            raise EngineError("encode(wait=False) needs device tensors")
        px, pmask = m.f32(x, shape), m.u8(mask, (B, self.T))
        out, pout = m.out((B, self.D))
        m.ready()
        if not wait:
            self._check(self.lib.ls_sag_enc_encode_async(self.h, B, px, pmask, pout), "ls_sag_enc_encode_async")
            m.done_async()
            self._async_inputs = m          # the marshalled inputs stay referenced until the next encode on this (in-order) stream
            return out
        self._check(self.lib.ls_sag_enc_encode(self.h, B, int(m.on_device), px, pmask, pout), "ls_sag_enc_encode")
        self._async_inputs = None
        return out


def clip_text_plan(tokens, vocab_size=49408):
    """The packing plan of ``tokens`` [B, context] int64 (ls_clip_text_plan; no GPU needed): ``(eot [B], row0 [B], total)`` with
    ``eot = tokens.argmax(-1)`` (first position of the maximum), ``row0`` the exclusive prefix of ``eot + 1`` and ``total`` the packed row
    count.  Raises on an id outside ``[0, vocab_size)``."""
    if hasattr(tokens, "detach"):
        tokens = tokens.detach().cpu().numpy()
    t = np.ascontiguousarray(tokens, dtype=np.int64)
    if t.ndim != 2 or t.shape[0] < 1:
        raise ValueError(f"tokens must be [B, context], got {list(t.shape)}")
    B = t.shape[0]
    eot, row0, total = np.empty(B, np.int32), np.empty(B, np.int32), C.c_int64()
    rc = load_library().ls_clip_text_plan(t.ctypes.data_as(c_i64p), B, t.shape[1], int(vocab_size), eot.ctypes.data_as(C.POINTER(C.c_int32)),
                                          row0.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total))
    if rc != 0:
        raise EngineError(f"ls_clip_text_plan failed ({rc}): a token id lies outside [0, {int(vocab_size)})")
    return eot, row0, int(total.value)


class ClipTextEngine(_Handle):
    """ctypes wrapper of the CLIP text encoder handle (ls_clip_text_*): ``clip_model.encode_text(text).float()`` on the GPU."""

    _prefix = "ls_clip_text_"

    def __init__(self, vocab_size=49408, context_length=77, width=512, heads=8, layers=12, embed_dim=512, device=0):
        self._create(LsClipTextConfig(device, vocab_size, context_length, width, heads, layers, embed_dim))
        self.context, self.E, self.device = context_length, embed_dim, device
        self._async_inputs = None

    def load_state_dict(self, sd: dict):
        self._set_weights(sd)

    def last_encode_ms(self) -> float:
        return float(self.lib.ls_clip_text_last_encode_ms(self.h))

    def encode(self, tokens, wait=True, prune=True, device_out=False):
        """tokens [B, context] integer ids -> features [B, embed_dim].  Host tokens are planned on the host; device tokens cost the
        call's one host wait (the plan's B + 1 ints come back, because the GEMM grids need the packed row count).  The output is a
        device tensor when the tokens are one or ``device_out`` is set, numpy otherwise.  ``wait=False`` (device output only): the
        rest of the encode is enqueued on the encoder's stream; torch's current stream is ordered behind it, a consumer on another
        stream with ``stream_order(device, self._stream, that_stream)``.  ``prune=False`` computes all context rows of every sample
        (same bits; there to test and time the packing against)."""
        shape = tuple(int(s) for s in tokens.shape)
        if len(shape) != 2 or shape[1] != self.context:
            raise ValueError(f"tokens must be [B, {self.context}], got {list(shape)}")
        B = shape[0]
        if B < 1:
            raise ValueError("tokens hold no sentence")
        m = _Marshal(self.device, tokens, stream=self._stream)
        tokens_dev = m.on_device
        ptok = m.i64(tokens, shape)
        if device_out and not tokens_dev:          # host tokens, device output: the output side of the marshal alone is on the device
            import torch
            m.on_device, m.torch, m.dev = True, torch, torch.device("cuda", self.device)
        if not wait and not m.on_device:
            raise EngineError("encode(wait=False) needs a device output")
        out, pout = m.out((B, self.E))
        m.ready()
        if not wait:
            self._check(self.lib.ls_clip_text_encode_async(self.h, B, int(tokens_dev), ptok, int(bool(prune)), pout), "ls_clip_text_encode_async")
            m.done_async()
            self._async_inputs = m          # the marshalled inputs stay referenced until the next encode on this (in-order) stream
            return out
        mode = 1 if tokens_dev else (2 if m.on_device else 0)
        self._check(self.lib.ls_clip_text_encode(self.h, B, mode, ptok, int(bool(prune)), pout), "ls_clip_text_encode")
        self._async_inputs = None
        return out


class Trainer(_Handle):
    """ctypes wrapper of the training-step handle (ls_train_*).  Master parameters, gradients and Adam moments are flat
    device arrays; ``grad`` is a torch CUDA tensor owned by this object so a data-parallel caller can all-reduce it
    (RCCL) between ``forward_backward`` and ``adamw``."""

    _prefix = "ls_train_"

    def __init__(self, njoints, nfeats, n_prefix_tokens, audio_len, n_emotions=0, nframes=34, n_pre_seq=4, layers=8,
                 n_speakers=1400, device=0, diffusion_steps=1000, lambda_vel=1.0, kld_weight=0.01):
        import torch
        self._create(LsTrainConfig(LsConfig(njoints, nfeats, nframes, n_prefix_tokens, n_pre_seq, 512, layers, audio_len, n_speakers,
                                            n_emotions, device, 0), lambda_vel, kld_weight, diffusion_steps, 0))
        self.J, self.F, self.T, self.device, self.n_prefix = njoints, nfeats, nframes, device, n_prefix_tokens
        self.params = {}
        key = C.create_string_buffer(256)
        off, num = C.c_int64(), C.c_int64()
        for i in range(self.lib.ls_train_param_count(self.h)):
            self._check(self.lib.ls_train_param_info(self.h, i, key, 256, C.byref(off), C.byref(num)), "ls_train_param_info")
            self.params[key.value.decode()] = (int(off.value), int(num.value))
        self.flat_size = int(self.lib.ls_train_flat_size(self.h))
        self.grad = torch.zeros(self.flat_size, dtype=torch.float32, device=torch.device("cuda", device))
        self.shapes = {}

    def load_state_dict(self, sd: dict):
        self.shapes.update((k, tuple(np.shape(v))) for k, v in sd.items())
        self._set_weights(sd, commit=False)      # ls_train_set_weight writes the master parameters directly

    def state_dict(self) -> dict:
        out = {}
        for k, (_, n) in self.params.items():
            a = np.empty(n, np.float32)
            self._check(self.lib.ls_train_get_weight(self.h, k.encode(), a.ctypes.data_as(c_f32p), n), f"ls_train_get_weight({k})")
            out[k] = a.reshape(self.shapes.get(k, (n,)))
        return out

    def set_schedule(self, sched):
        """sched: anything with .sqrt_alphas_cumprod, .sqrt_one_minus_alphas_cumprod (fp64) and .timestep_map."""
        a = np.ascontiguousarray(sched.sqrt_alphas_cumprod, dtype=np.float64)
        b = np.ascontiguousarray(sched.sqrt_one_minus_alphas_cumprod, dtype=np.float64)
        m = np.ascontiguousarray(sched.timestep_map, dtype=np.int64)
        if not (len(a) == len(b) == len(m) == self.cfg.diffusion_steps):
            raise EngineError("schedule length does not match diffusion_steps")
        self._check(self.lib.ls_train_set_schedule(self.h, a.ctypes.data_as(c_f64p), b.ctypes.data_as(c_f64p), m.ctypes.data_as(c_i64p)),
                    "ls_train_set_schedule")

    def forward_backward(self, x_start, t, noise, y: dict, drop, eps) -> dict:
        """One forward + loss + backward; gradients land in ``self.grad`` (flat, device). Returns the loss terms."""
        import torch
        m = _Marshal(self.device, x_start, noise, drop, eps, y["audio_input"], y["origin_x"], y["vid_indices"], y.get("emo"), stream=self._stream)
        B = int(x_start.shape[0])
        xs = (B, self.J, self.F, self.T)
        tt = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.int64)
        assert tt.shape == (B,)
        tb = LsTrainBatch(B, int(m.on_device), m.f32(x_start, xs), tt.ctypes.data_as(C.c_void_p), m.f32(noise, xs), m.f32(drop, (B,)),
                          m.f32(np.asarray(eps).reshape(B, 512) if not hasattr(eps, "detach") else eps.reshape(B, 512), (B, 512)),
                          m.f32(y["audio_input"]), m.f32(y["origin_x"], xs), m.i64(y["vid_indices"], (B,)),
                          m.i64(y["emo"], (B, self.T)) if self.n_prefix == 2 else None)
        terms = LsTrainTerms()
        m.ready()
        _order_after_torch(self.device, self._stream)     # whatever last touched self.grad on torch's stream (zero_, an all-reduce)
        self._check(self.lib.ls_train_forward_backward(self.h, C.byref(tb), C.c_void_p(self.grad.data_ptr()), C.byref(terms)),
                    "ls_train_forward_backward")
        return {n: float(getattr(terms, n)) for n in ("rot_mse", "vel_mse", "kld", "loss", "total", "fwd_ms", "bwd_ms")}

    def grads(self) -> dict:
        g = self.grad.detach().cpu().numpy()
        return {k: g[o:o + n].reshape(self.shapes.get(k, (n,))).copy() for k, (o, n) in self.params.items()}

    def adamw(self, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        _order_after_torch(self.device, self._stream)     # an all-reduce of self.grad may still be in flight: ordered, not waited for
        self._check(self.lib.ls_train_adamw(self.h, C.c_void_p(self.grad.data_ptr()), lr, betas[0], betas[1], eps, weight_decay),
                    "ls_train_adamw")

    def optimizer_state(self) -> dict:
        """{'step': int, 'exp_avg': {key: array}, 'exp_avg_sq': {key: array}} (what opt%09d.pt holds, train_loop.py:222-227)."""
        out = {"step": int(self.lib.ls_train_get_step(self.h)), "exp_avg": {}, "exp_avg_sq": {}}
        for which, name in ((1, "exp_avg"), (2, "exp_avg_sq")):
            for k, (_, n) in self.params.items():
                a = np.empty(n, np.float32)
                self._check(self.lib.ls_train_get_moment(self.h, which, k.encode(), a.ctypes.data_as(c_f32p), n), "ls_train_get_moment")
                out[name][k] = a.reshape(self.shapes.get(k, (n,)))
        return out

    def load_optimizer_state(self, st: dict):
        for which, name in ((1, "exp_avg"), (2, "exp_avg_sq")):
            for k, v in st[name].items():
                a = _np32(v)
                self._check(self.lib.ls_train_set_moment(self.h, which, k.encode(), a.ctypes.data_as(c_f32p), a.size), "ls_train_set_moment")
        self._check(self.lib.ls_train_set_step(self.h, int(st["step"])), "ls_train_set_step")

    def read(self, name: str, shape) -> np.ndarray:
        a = np.empty(tuple(shape), np.float32)
        self._check(self.lib.ls_train_read(self.h, name.encode(), a.ctypes.data_as(c_f32p), a.size), f"ls_train_read({name})")
        return a


class EvalEngine(_Handle):
    """ctypes wrapper of the FGD feature extractor (ls_eval_*): PoseEncoderConv in eval mode on the GPU."""

    _prefix = "ls_eval_"

    def __init__(self, pose_dim=27, n_frames=34, base=32, hidden=(256, 128), device=0):
        self._create(LsEvalConfig(pose_dim, n_frames, base, hidden[0], hidden[1], device))
        self.pose_dim, self.T, self.base, self.device = pose_dim, n_frames, base, device

    def load_state_dict(self, sd: dict):
        self._set_weights(sd)

    def features(self, poses):
        m = _Marshal(self.device, poses, stream=self._stream)
        B = int(poses.shape[0])
        out, pout = m.out((B, self.base))
        m.ready()
        self._check(self.lib.ls_eval_features(self.h, B, int(m.on_device), m.f32(poses, (B, self.T, self.pose_dim)), pout), "ls_eval_features")
        return out
