"""ctypes binding of libseedvc_hip.so (C ABI in include/seedvc_hip.h).

PyTorch is used only for device memory and streams: tensors are passed as raw device pointers and
the current HIP stream handle.  There is NO CPU fallback: a missing library raises ImportError here,
and every entry point raises RuntimeError with the library's message on failure.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libseedvc_hip.so")

EXPORTS = [
    "svc_abi_version", "svc_last_error",
    "svc_dit_create", "svc_dit_create_ex", "svc_dit_precision", "svc_dit_destroy", "svc_dit_set_microbatch", "svc_dit_set_fused_min_rows", "svc_dit_set_fused_seams", "svc_dit_fused_available", "svc_dit_set_graphs", "svc_cfm_sample", "svc_dit_forward",
    "svc_cfm_sample_seeded", "svc_cfm_noise_draws", "svc_cfm_sample_rows", "svc_cfm_rows_plan", "svc_hift_forward_seeded", "svc_hift_noise_draws",
    "svc_bigvgan_create", "svc_bigvgan_destroy", "svc_bigvgan_forward", "svc_bigvgan_forward_ragged", "svc_bigvgan_set_microbatch",
    "svc_hift_create", "svc_hift_destroy", "svc_hift_forward", "svc_hift_forward_ragged", "svc_hift_set_microbatch",
    "svc_anti_alias_act_fwd",
    "svc_ar_create", "svc_ar_destroy", "svc_ar_reset", "svc_ar_forward_generate", "svc_ar_decode_step", "svc_ar_sample", "svc_ar_generate",
    "svc_ar_set_max_batch", "svc_ar_prefill_slot", "svc_ar_decode_step_batch", "svc_ar_generate_batch",
    "svc_ar_generate_batch_seeded", "svc_ar_exp_draws", "svc_v2_assemble_cond", "svc_mel_strip_prompt",
    "svc_ar_prefill_batch", "svc_ar_set_prefill_rows", "svc_ar_prefill_passes", "svc_ar_admit", "svc_ar_run", "svc_ar_retire",
    "svc_ar_session_active",
    "svc_lr_create", "svc_lr_destroy", "svc_lr_forward", "svc_crossfade",
    "svc_chunks_gather_cond", "svc_chunks_assemble", "svc_chunks_emit", "svc_sola_step", "svc_rt_push", "svc_rt_push_tiles", "svc_rt_ring_floats",
    "svc_rt_out", "svc_rt_push_gated", "svc_rt_out_dev", "svc_rt_pitch_state_words", "svc_rt_pitch",
    "svc_rt_pitch_cache_words", "svc_rt_pitch_ring_words", "svc_rt_pitch_win",
    "svc_vad_create", "svc_vad_destroy", "svc_vad_rows", "svc_vad_history", "svc_vad_state_floats", "svc_vad_scores", "svc_vad_detect",
    "svc_vad_step",
    "svc_campplus_create", "svc_campplus_destroy", "svc_campplus_forward", "svc_kaldi_fbank_frames", "svc_kaldi_fbank",
    "svc_kaldi_fbank_ragged", "svc_campplus_forward_ragged",
    "svc_mel_create", "svc_mel_destroy", "svc_mel_frames", "svc_mel_forward", "svc_mel_forward_ragged", "svc_mel_min_len",
    "svc_resampler_create", "svc_resampler_destroy", "svc_resample_len", "svc_resampler_tile", "svc_resample",
    "svc_rmvpe_create", "svc_rmvpe_destroy", "svc_rmvpe_frames", "svc_rmvpe_min_len", "svc_rmvpe_set_plane_budget", "svc_rmvpe_set_timing", "svc_rmvpe_last_timing", "svc_rmvpe_mel",
    "svc_rmvpe_salience", "svc_rmvpe_decode", "svc_rmvpe_f0", "svc_f0_adjust",
    "svc_whisper_create", "svc_whisper_destroy", "svc_whisper_n_windows", "svc_whisper_rows", "svc_whisper_set_window_group",
    "svc_whisper_set_timing", "svc_whisper_last_timing", "svc_whisper_mel", "svc_whisper_encode", "svc_whisper_content",
    "svc_w2v_create", "svc_w2v_destroy", "svc_w2v_frames", "svc_w2v_n_windows", "svc_w2v_rows", "svc_w2v_set_window_group",
    "svc_w2v_set_timing", "svc_w2v_last_timing", "svc_w2v_normalize", "svc_w2v_features", "svc_w2v_posconv", "svc_w2v_encode",
    "svc_w2v_content", "svc_w2v_create_ex",
    "svc_astral_create", "svc_astral_destroy", "svc_astral_n_windows", "svc_astral_rows", "svc_astral_set_window_group",
    "svc_astral_set_timing", "svc_astral_last_timing", "svc_astral_ssl", "svc_astral_convnext", "svc_astral_logits", "svc_astral_tokens",
    "svc_astral_tokens_heads", "svc_op_bsq_index", "svc_tokens_reduce",
    "svc_prof_enable", "svc_prof_collect",
    "svc_op_linear", "svc_op_conv1d", "svc_op_conv1d_ex", "svc_op_conv1d_last_took", "svc_op_dit_panel", "svc_op_conv_transpose1d", "svc_op_attention", "svc_op_attention_ex", "svc_op_rmsnorm",
    "svc_op_layernorm", "svc_op_layernorm_gelu", "svc_op_act_cl", "svc_op_hift_signal", "svc_op_ar_sampler",
    "svc_op_ar_attn", "svc_op_ar_linear", "svc_op_kgemm", "svc_op_permute_vt", "svc_op_lr", "svc_op_attention_x3",
    "svc_bigvgan_plan_size", "svc_bigvgan_plan_name", "svc_bigvgan_plan_get", "svc_bigvgan_plan_set", "svc_bigvgan_plan_reset",
    "svc_bigvgan_calibrate", "svc_hift_plan_size", "svc_hift_plan_name", "svc_hift_plan_get", "svc_hift_plan_set",
    "svc_hift_plan_reset", "svc_hift_calibrate", "svc_op_range_census", "svc_op_weight_census", "svc_op_plan_fake",
    "svc_op_plan_apply",
]


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4)]


class DitConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "version", "hidden_dim", "num_heads", "depth", "in_channels", "content_dim", "style_dim",
        "final_layer_type", "time_as_token", "style_as_token", "uvit_skip_connection", "long_skip_connection",
        "style_condition", "wn_hidden_dim", "wn_num_layers", "wn_kernel_size", "wn_dilation_rate")]


class CfmArgs(C.Structure):
    _fields_ = [("B", C.c_int), ("T", C.c_int), ("P", C.c_int),
                ("mu", C.c_void_p), ("prompt", C.c_void_p), ("style", C.c_void_p), ("z", C.c_void_p),
                ("x_lens", C.POINTER(C.c_int64)), ("prompt_lens", C.POINTER(C.c_int64)),
                ("n_timesteps", C.c_int), ("temperature", C.c_float), ("cfg_rate", C.c_float * 2),
                ("random_voice", C.c_int), ("out", C.c_void_p)]


class CfmRow(C.Structure):
    """svc_cfm_row_t: the sampler settings of one utterance (svc_cfm_sample_rows)."""
    _fields_ = [("n_timesteps", C.c_int32), ("temperature", C.c_float), ("cfg_rate", C.c_float * 2), ("random_voice", C.c_int32)]


class BigVGANConfig(C.Structure):
    _fields_ = [("num_mels", C.c_int), ("upsample_initial_channel", C.c_int), ("num_upsamples", C.c_int),
                ("num_kernels", C.c_int), ("upsample_rates", C.c_int * 8), ("upsample_kernel_sizes", C.c_int * 8),
                ("resblock_kernel_sizes", C.c_int * 4), ("resblock_dilation_sizes", (C.c_int * 3) * 4),
                ("use_tanh_at_final", C.c_int), ("use_bias_at_final", C.c_int), ("snake_logscale", C.c_int),
                ("snakebeta", C.c_int), ("precision", C.c_int)]


class HiftConfig(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("base_channels", C.c_int), ("nb_harmonics", C.c_int),
                ("sampling_rate", C.c_int), ("nsf_alpha", C.c_float), ("nsf_sigma", C.c_float),
                ("nsf_voiced_threshold", C.c_float), ("num_upsamples", C.c_int), ("upsample_rates", C.c_int * 4),
                ("upsample_kernel_sizes", C.c_int * 4), ("istft_n_fft", C.c_int), ("istft_hop", C.c_int),
                ("num_kernels", C.c_int), ("resblock_kernel_sizes", C.c_int * 4),
                ("resblock_dilation_sizes", (C.c_int * 3) * 4), ("source_resblock_kernel_sizes", C.c_int * 4),
                ("source_resblock_dilation_sizes", (C.c_int * 3) * 4), ("lrelu_slope", C.c_float),
                ("audio_limit", C.c_float), ("f0_cond_channels", C.c_int), ("precision", C.c_int)]


class ArConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dim", "n_head", "n_local_heads", "head_dim", "n_layer", "intermediate_size",
                                       "vocab_size", "max_seq_len")] + [("rope_base", C.c_float), ("norm_eps", C.c_float)]


class ArRequest(C.Structure):
    """svc_ar_request_t: one request of svc_ar_admit."""
    _fields_ = [("slot", C.c_int32), ("S", C.c_int32), ("exp_noise", C.c_void_p), ("seed", C.c_uint64), ("max_new", C.c_int32),
                ("min_tokens_before_eos", C.c_int32), ("temperature", C.c_float), ("top_p", C.c_float),
                ("repetition_penalty", C.c_float), ("tokens_out", C.c_void_p)]


class CampplusConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("feat_dim", "embedding_size", "growth_rate", "bn_size", "init_channels", "m_channels", "n_blocks")] + \
               [("block_layers", C.c_int * 4), ("block_kernel", C.c_int * 4), ("block_dilation", C.c_int * 4), ("seg_len", C.c_int)]


class RmvpeConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_mels", "en_de_layers", "inter_layers", "n_blocks", "en_out_channels", "gru_hidden", "n_bins")]


class WhisperConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_mels", "d_model", "n_heads", "n_layers", "ffn_dim", "max_source_positions", "precision")]


class W2vConfig(C.Structure):
    _fields_ = [("conv_dim", C.c_int), ("n_conv", C.c_int), ("conv_kernel", C.c_int * 8), ("conv_stride", C.c_int * 8)] + \
               [(n, C.c_int) for n in ("d_model", "n_heads", "n_layers", "ffn_dim", "pos_k", "pos_groups", "feat_extract_norm_layer",
                                       "do_stable_layer_norm", "conv_bias", "window_samples", "precision")]


class W2vExt(C.Structure):
    _fields_ = [("do_normalize", C.c_int), ("feat_proj_layer_norm", C.c_int)]


class AstralHeadConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dim", "intermediate_dim", "n_blocks", "bits", "dw_kernel")]


class AstralConfig(C.Structure):
    _fields_ = [("ssl", W2vConfig), ("n_heads", C.c_int), ("head", AstralHeadConfig * 2)]


class VadConfig(C.Structure):
    """svc_vad_config_t: the detector's thresholds (frames of 10 ms) and the default run length of svc_vad_scores."""
    _fields_ = [("p_max", C.c_float)] + [(n, C.c_int32) for n in ("win", "on_count", "off_count", "lookback", "end_silence",
                                                                  "max_segment", "seg_rows")]


class LrConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("channels", "in_channels", "out_channels", "is_discrete", "codebook_size", "n_convs",
                                       "interpolate", "has_final_conv", "f0_condition", "n_f0_bins")]


class Conv1dEx(C.Structure):
    """svc_conv1d_ex_t: the arguments of svc_op_conv1d_ex (test aid)."""
    _fields_ = [("x", C.c_void_p), ("a_hi", C.c_void_p), ("a_lo", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("B", "L", "Cin", "Cout", "k", "dilation", "pad_left", "Lout", "dtype")] + \
               [("seq_len", C.POINTER(C.c_int32)), ("res", C.c_void_p), ("res2", C.c_void_p),
                ("out_scale", C.c_float), ("act", C.c_int32), ("act_slope", C.c_float), ("c_rows", C.c_int32), ("c_off", C.c_int32),
                ("post_a", C.c_void_p), ("post_ib", C.c_void_p), ("next_p8", C.c_int32), ("bm", C.c_int32), ("force_gemm", C.c_int32),
                ("y", C.c_void_p), ("plane_hi", C.c_void_p), ("plane_lo", C.c_void_p), ("took", C.c_int32)]


class DitPanel(C.Structure):
    """svc_dit_panel_t: the arguments of svc_op_dit_panel (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("D", "I", "gated", "tm", "M", "Lout", "seq_rows", "row_off", "n_seq")] + \
               [("eps", C.c_float), ("add_one", C.c_int32)] + \
               [(n, C.c_int32) for n in ("do_post", "do_skip", "do_qkv", "do_final", "seam")] + \
               [(n, C.c_void_p) for n in ("wo", "w1", "w3", "w2", "wskip", "wqkv", "w_merge")] + \
               [("ldw", C.c_int32), ("C", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("head_wa", "head_w2", "gate_a", "gate_f", "g_ffn", "w_f", "b_f", "g_attn", "w_a", "b_a", "bskip",
                                          "g_fin", "w_fin", "b_fin", "head_b0", "head_b2", "tok_time", "tok_style",
                                          "ao", "skip_in", "x16", "x", "st_term", "c16", "n16", "qk", "vt")] + \
               [("vt_seq_stride", C.c_int64), ("vt_ld", C.c_int64), ("vt_mode", C.c_int32),
                ("v32", C.c_void_p), ("ldv", C.c_int32), ("head_C", C.c_int32), ("rope", C.c_void_p), ("q_scale", C.c_float),
                ("npre", C.c_int32), ("time_first", C.c_int32), ("T", C.c_int32)]


class Attention(C.Structure):
    """svc_attention_t: the arguments of svc_op_attention_ex (test aid)."""
    _fields_ = [(n, C.c_void_p) for n in ("q", "k", "vt", "out", "out32")] + \
               [(n, C.c_int64) for n in ("ld_qk", "vt_seq_stride", "vt_ld", "ld_out")] + \
               [(n, C.c_int32) for n in ("n_seq", "H", "seq_rows", "Tq", "q_start")] + \
               [("kv_len", C.POINTER(C.c_int64))] + \
               [(n, C.c_int32) for n in ("kv_len_const", "vt_perm", "qt_form")]


class ActCl(C.Structure):
    """svc_act_cl_t: the arguments of svc_op_act_cl (test aid)."""
    _fields_ = [("x", C.c_void_p), ("y_hi", C.c_void_p), ("y_lo", C.c_void_p), ("ldx", C.c_int64), ("ldy", C.c_int64),
                ("out_f16", C.c_int32), ("lo_fmt", C.c_int32), ("taps", C.c_float * 12), ("a", C.c_void_p), ("inv_b", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("B", "C", "L", "mode")] + [("slope", C.c_float), ("lens", C.POINTER(C.c_int32))]


class HiftSignal(C.Structure):
    """svc_hift_signal_t: the arguments of svc_op_hift_signal (test aid)."""
    _fields_ = [("stage", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("in", "phase0", "noise", "lin_w", "lin_b", "out", "out_lo")] + \
               [(n, C.c_int32) for n in ("B", "n_utt", "NH", "up")] + \
               [(n, C.c_float) for n in ("sr", "sine_amp", "noise_std", "voiced_thr", "limit")] + \
               [(n, C.c_int32) for n in ("S", "S_in", "F")] + [("Lw", C.c_int64)] + \
               [(n, C.c_int32) for n in ("ld", "C", "vd", "mode")] + [("slope", C.c_float)] + \
               [(n, C.POINTER(C.c_int32)) for n in ("src", "len", "lw", "nf")]


class Census(C.Structure):
    """svc_census_t: one range-census record (csrc/range_census.hip)."""
    _fields_ = [(n, C.c_int64) for n in ("n", "n_hi_clamp", "n_hi_sub", "n_lo_flush", "n_lo_clamp")] + \
               [(n, C.c_double) for n in ("max_hi", "s_hi2", "s_hi_err2", "s_lo2", "s_lo_err2")]


class PlanRow(C.Structure):
    """svc_plan_row_t: one report row of svc_bigvgan_calibrate / svc_hift_calibrate."""
    _fields_ = [(n, C.c_int32) for n in ("index", "veto", "L", "reserved")] + \
               [(n, C.c_double) for n in ("rho", "eta", "omega_hi", "omega_lo")] + [("census", Census)]


class RangeCensus(C.Structure):
    """svc_range_census_t: the arguments of svc_op_range_census (test aid)."""
    _fields_ = [("hi", C.c_void_p), ("lo", C.c_void_p)] + [(n, C.c_int32) for n in ("B", "L", "C", "ld")] + \
               [("lens", C.POINTER(C.c_int32)), ("out", C.POINTER(Census))]


class ArSampler(C.Structure):
    """svc_ar_sampler_t: the arguments of svc_op_ar_sampler (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("form", "V", "D", "B", "max_new", "Lmax")] + \
               [("logits", C.c_void_p), ("prev", C.c_void_p), ("n_prev", C.c_int32), ("suppress", C.c_int32)] + \
               [(n, C.c_float) for n in ("rep_pen", "temperature", "top_p")] + \
               [("exp_noise", C.c_void_p), ("seed", C.c_uint64), ("step", C.c_int32)] + \
               [(n, C.c_void_p) for n in ("idx_out", "probs_out", "toks", "noise", "emb", "next_x")] + \
               [(n, C.POINTER(C.c_int32)) for n in ("s_cnt", "s_done", "s_max_new", "s_min_before_eos", "s_eos")] + \
               [(n, C.POINTER(C.c_float)) for n in ("s_temperature", "s_top_p", "s_rep_pen")] + \
               [("s_seed", C.POINTER(C.c_uint64)), ("s_has_noise", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32))]


class ArAttn(C.Structure):
    """svc_ar_attn_t: the arguments of svc_op_ar_attn (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "H", "Hkv", "Lmax", "n_slots", "n")] + \
               [("x", C.c_void_p), ("ldq", C.c_int64), ("kc", C.c_void_p), ("vc", C.c_void_p), ("rope", C.c_void_p)] + \
               [(n, C.POINTER(C.c_int32)) for n in ("slots", "seq_S", "pos")] + \
               [("y16", C.c_void_p), ("q_out", C.c_void_p), ("hres", C.c_void_p), ("eps", C.c_float), ("wo", C.c_void_p),
                ("part", C.c_void_p)]


class ArLinear(C.Structure):
    """svc_ar_linear_t: the arguments of svc_op_ar_linear (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("path", "role", "D", "I", "H", "Hkv", "V", "Lmax", "rows", "n_slots")] + \
               [("x", C.c_void_p), ("gamma", C.c_void_p), ("eps", C.c_float), ("W", C.c_void_p), ("W2", C.c_void_p)] + \
               [(n, C.c_void_p) for n in ("res", "part", "out32", "out16", "out2", "q_out", "kc", "vc", "rope")] + \
               [(n, C.POINTER(C.c_int32)) for n in ("slots", "pos")]


class KGemm(C.Structure):
    """svc_kgemm_t: the arguments of svc_op_kgemm (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("dtype", "epi", "form", "n_src")] + \
               [("a_src", C.c_void_p * 4), ("a_rows", C.c_int64 * 4), ("a_K", C.c_int32 * 4), ("n_taps", C.c_int32),
                ("tap_src", C.c_int32 * 48), ("tap_shift", C.c_int32 * 48), ("tap_K", C.c_int32 * 48), ("w", C.c_void_p), ("w_rows", C.c_int64)] + \
               [(n, C.c_int32) for n in ("M", "N", "Lout", "a_seq_rows", "a_off", "a_stride", "a_len", "pad_mode", "reflect_min")] + \
               [("seq_len", C.POINTER(C.c_int32)), ("a_seq_map", C.POINTER(C.c_int32)), ("c_seq_rows", C.c_int32), ("c_off", C.c_int32),
                ("c_rows", C.c_int64), ("ldc", C.c_int64), ("c32", C.c_void_p), ("c16", C.c_void_p), ("c16_lo", C.c_void_p),
                ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("ld_rowvec", C.c_int64), ("gate", C.c_void_p), ("ld_gate", C.c_int64),
                ("res", C.c_void_p), ("res2", C.c_void_p), ("post_a", C.c_void_p), ("post_ib", C.c_void_p), ("post_n", C.c_int32),
                ("out_scale", C.c_float), ("act", C.c_int32), ("act_slope", C.c_float), ("post_relu", C.c_int32), ("vec_ok", C.c_int32),
                ("rope", C.c_void_p), ("rope_rows", C.c_int32), ("rope_D", C.c_int32), ("q_scale", C.c_float),
                ("vt", C.c_void_p), ("vt_ld", C.c_int64), ("vt_mode", C.c_int32), ("check_only", C.c_int32)]


class LrOp(C.Structure):
    """svc_lr_op_t: the arguments of svc_op_lr (test aid)."""
    _fields_ = [(n, C.c_int32) for n in ("stage", "B", "tout_max", "C", "ld")] + \
               [("ylens", C.POINTER(C.c_int32)), ("x", C.c_void_p), ("feat", C.c_void_p), ("ld_feat", C.c_int64), ("tin_max", C.c_int32),
                ("tokens", C.c_void_p), ("emb", C.c_void_p), ("in_lens", C.POINTER(C.c_int32)), ("interpolate", C.c_int32),
                ("f0", C.c_void_p), ("tf0_max", C.c_int32), ("f0_lens", C.POINTER(C.c_int32)), ("f0_emb", C.c_void_p),
                ("f0_mask", C.c_void_p), ("n_bins", C.c_int32), ("stats", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("eps", C.c_float), ("out", C.c_void_p), ("ld_out", C.c_int32), ("N", C.c_int32), ("check_only", C.c_int32)]


_lib = None


def lib():
    """Loads the shared library (once).  No fallback: the HIP path is the product."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
        l = C.CDLL(LIB_PATH)
        l.svc_last_error.restype = C.c_char_p
        if l.svc_abi_version() != 1:
            raise ImportError("libseedvc_hip.so ABI version mismatch")
        # the streaming splice: the pieces' rows, lengths and ranges as HOST int32 arrays, their output offsets as HOST int64
        l.svc_chunks_emit.argtypes = ([C.c_void_p, C.c_longlong, C.c_int] + [C.POINTER(C.c_int32)] * 6 + [C.POINTER(C.c_int64), C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p])
        l.svc_sola_step.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32),
                                    C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_rt_push.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        # the live block step: the gate thresholds and the speech flags as HOST arrays
        l.svc_rt_push_gated.argtypes = l.svc_rt_push.argtypes[:-1] + [C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_rt_out.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
        # svc_rt_out with DEVICE mute flags behind the host ones
        a = l.svc_rt_out.argtypes
        l.svc_rt_out_dev.argtypes = a[:10] + [C.c_void_p] + a[10:]
        # FSMN-VAD: lengths, row counts and slots as HOST int32 arrays, totals as a HOST int64 array, sample counts as C long
        l.svc_vad_create.argtypes = [C.POINTER(VadConfig), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_vad_destroy.argtypes = [C.c_void_p]
        l.svc_vad_destroy.restype = None
        l.svc_vad_rows.argtypes = [C.c_long, C.c_int]
        l.svc_vad_rows.restype = C.c_long
        l.svc_vad_history.argtypes = [C.c_long]
        l.svc_vad_history.restype = C.c_long
        l.svc_vad_state_floats.argtypes = [C.c_int]
        l.svc_vad_state_floats.restype = C.c_longlong
        l.svc_vad_scores.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_vad_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_vad_step.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_long, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                   C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p]
        # the streams' pitch step: slots, auto flags and semitones as HOST arrays
        l.svc_rt_pitch_state_words.argtypes = [C.c_int]
        l.svc_rt_pitch_state_words.restype = C.c_longlong
        l.svc_rt_pitch.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int,
                                   C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_float,
                                   C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p]
        # the same on the context's tail: window, guard, the slots' cache rows and rings of counted bins
        l.svc_rt_pitch_cache_words.argtypes = l.svc_rt_pitch_ring_words.argtypes = [C.c_int, C.c_int]
        l.svc_rt_pitch_cache_words.restype = l.svc_rt_pitch_ring_words.restype = C.c_longlong
        l.svc_rt_pitch_win.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_float), C.c_int, C.c_float, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                       C.c_void_p, C.c_void_p]
        l.svc_rt_push_tiles.argtypes = [C.c_int]
        l.svc_rt_ring_floats.argtypes = [C.c_int, C.c_int]
        l.svc_rt_ring_floats.restype = C.c_longlong
        l.svc_hift_forward_ragged.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_op_conv1d_ex.argtypes = [C.POINTER(Conv1dEx), C.c_void_p]
        l.svc_op_dit_panel.argtypes = [C.POINTER(DitPanel), C.c_void_p]
        l.svc_op_attention_ex.argtypes = [C.POINTER(Attention), C.c_void_p]
        l.svc_op_act_cl.argtypes = [C.POINTER(ActCl), C.c_void_p]
        l.svc_op_hift_signal.argtypes = [C.POINTER(HiftSignal), C.c_void_p]
        # precision plan of the fp16p8 vocoders: vetoes as HOST bytes, report rows and lengths as HOST arrays
        u8p = C.POINTER(C.c_uint8)
        for voc in ("bigvgan", "hift"):
            getattr(l, f"svc_{voc}_plan_size").argtypes = [C.c_void_p]
            getattr(l, f"svc_{voc}_plan_name").argtypes = [C.c_void_p, C.c_int]
            getattr(l, f"svc_{voc}_plan_name").restype = C.c_char_p
            getattr(l, f"svc_{voc}_plan_get").argtypes = [C.c_void_p, u8p, C.c_int]
            getattr(l, f"svc_{voc}_plan_set").argtypes = [C.c_void_p, u8p, C.c_int]
            getattr(l, f"svc_{voc}_plan_reset").argtypes = [C.c_void_p]
        l.svc_bigvgan_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float,
                                            C.POINTER(PlanRow), C.c_int, C.c_void_p]
        l.svc_hift_calibrate.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_int, C.c_float, C.POINTER(PlanRow), C.c_int, C.c_void_p]
        l.svc_op_range_census.argtypes = [C.POINTER(RangeCensus), C.c_void_p]
        l.svc_op_weight_census.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p]
        l.svc_op_plan_fake.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        l.svc_op_plan_apply.argtypes = [C.c_void_p, C.POINTER(PlanRow), C.c_int, C.c_float]
        l.svc_op_ar_sampler.argtypes = [C.POINTER(ArSampler), C.c_void_p]
        l.svc_op_ar_attn.argtypes = [C.POINTER(ArAttn), C.c_void_p]
        l.svc_op_ar_linear.argtypes = [C.POINTER(ArLinear), C.c_void_p]
        l.svc_op_kgemm.argtypes = [C.POINTER(KGemm), C.c_void_p]
        l.svc_op_permute_vt.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p]
        l.svc_op_lr.argtypes = [C.POINTER(LrOp), C.c_void_p]
        l.svc_op_attention_x3.argtypes = [C.c_void_p] * 4 + [C.c_int] * 5 + [C.POINTER(C.c_int64), C.c_void_p]
        l.svc_dit_create_ex.argtypes = [C.POINTER(DitConfig), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_dit_precision.argtypes = [C.c_void_p]
        # seeded noise: 64-bit seeds by value and as HOST arrays
        l.svc_cfm_sample_seeded.argtypes = [C.c_void_p, C.POINTER(CfmArgs), C.POINTER(C.c_uint64), C.c_void_p]
        l.svc_cfm_noise_draws.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        # per-utterance sampler settings: the rows, the seeds and the plan's outputs as HOST arrays
        l.svc_cfm_sample_rows.argtypes = [C.c_void_p, C.POINTER(CfmArgs), C.POINTER(CfmRow), C.POINTER(C.c_uint64), C.c_void_p]
        l.svc_cfm_rows_plan.argtypes = [C.c_int, C.POINTER(CfmRow), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        l.svc_hift_forward_seeded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_uint64),
                                              C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_hift_noise_draws.argtypes = [C.c_uint64, C.c_int, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]
        # reference front-end, ragged: lengths as HOST int32 arrays
        l.svc_mel_forward_ragged.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_float, C.c_void_p,
                                             C.c_void_p]
        l.svc_kaldi_fbank_ragged.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_void_p]
        l.svc_campplus_forward_ragged.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        i32p = C.POINTER(C.c_int32)
        # resampler: the taps table and the lengths as HOST arrays, sample counts as C long
        l.svc_resampler_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, i32p, C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_resampler_destroy.argtypes = [C.c_void_p]
        l.svc_resampler_destroy.restype = None
        l.svc_resample_len.argtypes = [C.c_int, C.c_int, C.c_long]
        l.svc_resample_len.restype = C.c_long
        l.svc_resampler_tile.argtypes = [C.c_void_p]
        l.svc_resampler_tile.restype = C.c_long
        l.svc_resample.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_long, C.c_void_p, C.c_long, C.c_void_p]
        # RMVPE: lengths as HOST int32 arrays, semitones as a HOST float array
        l.svc_rmvpe_create.argtypes = [C.POINTER(RmvpeConfig), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_rmvpe_set_plane_budget.argtypes = [C.c_void_p, C.c_longlong]
        l.svc_rmvpe_set_timing.argtypes = [C.c_void_p, C.c_int]
        l.svc_rmvpe_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.svc_rmvpe_mel.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_rmvpe_salience.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_rmvpe_decode.argtypes = [C.c_void_p, i32p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        l.svc_rmvpe_f0.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        l.svc_f0_adjust.argtypes = [C.c_void_p, i32p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                    C.c_void_p, C.c_void_p, C.c_void_p]
        # Whisper content encoder: lengths as HOST int32 arrays, sample counts of the window plan as C long
        l.svc_whisper_create.argtypes = [C.POINTER(WhisperConfig), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_whisper_destroy.argtypes = [C.c_void_p]
        l.svc_whisper_n_windows.argtypes = [C.c_int, C.c_int, C.c_long]
        l.svc_whisper_rows.argtypes = [C.c_int, C.c_int, C.c_long]
        l.svc_whisper_set_window_group.argtypes = [C.c_void_p, C.c_int]
        l.svc_whisper_set_timing.argtypes = [C.c_void_p, C.c_int]
        l.svc_whisper_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.svc_whisper_mel.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_whisper_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_whisper_content.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        # wav2vec 2.0 content encoder: lengths and row counts as HOST int32 arrays, sample counts as C long
        cp = C.POINTER(W2vConfig)
        l.svc_w2v_create.argtypes = [cp, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_w2v_create_ex.argtypes = [cp, C.POINTER(W2vExt), C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_w2v_destroy.argtypes = [C.c_void_p]
        l.svc_w2v_frames.argtypes = [cp, C.c_long]
        l.svc_w2v_frames.restype = C.c_long
        l.svc_w2v_n_windows.argtypes = [cp, C.c_int, C.c_long]
        l.svc_w2v_rows.argtypes = [cp, C.c_int, C.c_long]
        l.svc_w2v_set_window_group.argtypes = [C.c_void_p, C.c_int]
        l.svc_w2v_set_timing.argtypes = [C.c_void_p, C.c_int]
        l.svc_w2v_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.svc_w2v_normalize.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_w2v_features.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        l.svc_w2v_posconv.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_w2v_encode.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_w2v_content.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        # ASTRAL tokenizer: lengths and row counts as HOST int32 arrays; token buffers are device int32
        ap = C.POINTER(AstralConfig)
        l.svc_astral_create.argtypes = [ap, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_void_p, C.POINTER(C.c_void_p)]
        l.svc_astral_destroy.argtypes = [C.c_void_p]
        l.svc_astral_n_windows.argtypes = [ap, C.c_int, C.c_long]
        l.svc_astral_rows.argtypes = [ap, C.c_int, C.c_long]
        l.svc_astral_set_window_group.argtypes = [C.c_void_p, C.c_int]
        l.svc_astral_set_timing.argtypes = [C.c_void_p, C.c_int]
        l.svc_astral_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        l.svc_astral_ssl.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        l.svc_astral_convnext.argtypes = [C.c_void_p, C.c_int, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_astral_logits.argtypes = [C.c_void_p, C.c_int, C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        l.svc_op_bsq_index.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
        l.svc_tokens_reduce.argtypes = [C.c_void_p, i32p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_astral_tokens.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        l.svc_astral_tokens_heads.argtypes = [C.c_void_p, C.c_void_p, i32p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        l.svc_op_layernorm_gelu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
        l.svc_op_layernorm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p]
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        raise RuntimeError("seedvc_hip: " + (lib().svc_last_error() or b"unknown error").decode())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def f32c(t, device=None):
    """contiguous fp32 device tensor"""
    t = t.detach()
    if device is not None:
        t = t.to(device)
    return t.to(torch.float32).contiguous()


def make_descs(state_dict, device):
    """state_dict -> (TensorDesc array, keep-alive list). Non-float entries (masks, index buffers) are skipped."""
    keep, items = [], []
    for k, v in state_dict.items():
        if not torch.is_tensor(v) or not (v.is_floating_point()):
            continue
        if v.dim() > 4:
            continue
        t = f32c(v, device)
        keep.append(t)
        items.append((k, t))
    arr = (TensorDesc * len(items))()
    for i, (k, t) in enumerate(items):
        kb = k.encode()
        keep.append(kb)
        arr[i].name = kb
        arr[i].data = t.data_ptr()
        arr[i].ndim = t.dim()
        for j in range(4):
            arr[i].shape[j] = t.shape[j] if j < t.dim() else 1
    return arr, len(items), keep


def int_list(v):
    """list / tensor / array of integers -> list of Python ints."""
    return [int(x) for x in (v.tolist() if torch.is_tensor(v) else v)]


def i64_host(values):
    if values is None:
        return None
    vals = [int(v) for v in values]
    return (C.c_int64 * len(vals))(*vals)


def i32_host(values):
    """Python ints -> a HOST int32 array (lengths and slots travel as kernel arguments)."""
    return (C.c_int32 * len(values))(*values)


def seed_ints(seeds, n, what):
    """seeds (list / tensor of n integers in [0, 2^64)) -> list of ints; ValueError for a wrong count or a seed out of range."""
    vals = int_list(seeds)
    if len(vals) != n:
        raise ValueError(f"{what}: {len(vals)} seeds for {n} utterances")
    for v in vals:
        if not 0 <= v < 1 << 64:
            raise ValueError(f"{what}: seed {v} is outside [0, 2^64)")
    return vals


def seeds_host(seeds, n, what):
    """The same as a HOST uint64 array for the seeded calls."""
    return (C.c_uint64 * n)(*seed_ints(seeds, n, what))
