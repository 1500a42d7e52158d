"""ctypes binding of libfacppg_hip.so (C ABI: include/facppg.h).

The library is the product: if it is missing, or there is no GPU, the synthesis path raises --
there is no CPU fallback (the CPU restatement lives in oracle/ and is test infrastructure).
``import torch`` happens before ``CDLL`` on purpose: libfacppg_hip.so needs ``libamdhip64.so.7``
and must bind to the copy PyTorch-ROCm already loaded, so that torch's streams and device
pointers are valid inside the kernels' launches.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede CDLL, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libfacppg_hip.so")

_lib = None


class FacppgError(RuntimeError):
    pass


class WgConfig(ctypes.Structure):
    """facppg_wg_config (include/facppg.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_mel_channels", "hop_length", "n_flows", "n_group", "n_early_every", "n_early_size",
        "wn_layers", "wn_channels", "wn_kernel_size", "upsample_kernel", "alternate_halves")]


class TacoConfig(ctypes.Structure):
    """facppg_taco_config (include/facppg.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_symbols", "symbols_embedding_dim", "encoder_kernel_size", "encoder_n_convolutions", "encoder_embedding_dim",
        "n_acoustic_feat_dims", "prenet_dim", "attention_rnn_dim", "decoder_rnn_dim", "attention_dim",
        "attention_location_n_filters", "attention_location_kernel_size", "attention_window_size",
        "postnet_embedding_dim", "postnet_kernel_size", "postnet_n_convolutions")] + \
        [("gate_threshold", ctypes.c_float), ("bn_eps", ctypes.c_float)]


class TacoDecodeOpts(ctypes.Structure):
    """facppg_taco_decode_opts (include/facppg.h): the inputs, then the launch report the call fills in."""
    _fields_ = [("max_workgroups", ctypes.c_int32), ("frame_words_dev", ctypes.c_void_p), ("frame_words_frames", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("workgroups", ctypes.c_int32), ("streamed", ctypes.c_int32), ("step", ctypes.c_int32)]


class TacoLaunchReport(ctypes.Structure):
    """facppg_taco_launch_report (include/facppg.h): what facppg_taco_launch_plan says a call would launch."""
    _fields_ = [(n, ctypes.c_int32) for n in ("mode", "workgroups", "launches", "step", "nu", "first_utts", "last_utts")] + \
        [("first_u", ctypes.c_int32 * 2), ("last_u", ctypes.c_int32 * 2)] + \
        [(n, ctypes.c_int32) for n in ("regw", "q_res", "pause", "dbg_flags", "prof", "lds_bytes", "streamed_possible",
                                       "bilstm_kind", "bilstm_legacy")]


class TrainLaunchReport(ctypes.Structure):
    """facppg_train_launch_report (include/facppg.h): what facppg_train_bf16_launch_plan says the bf16 training calls would launch."""
    _fields_ = [(n, ctypes.c_int32) for n in ("tile_positions", "fused_fwd", "fused_bwd", "fused_workgroups")] + \
        [("gemm_cols", ctypes.c_int32 * 5), ("gemm_workgroups", ctypes.c_int32 * 5)] + \
        [(n, ctypes.c_int32) for n in ("dspect_bgemm", "dspect_cols", "dspect_workgroups", "dspect_lds_bytes")] + \
        [(n, ctypes.c_int32 * 3) for n in ("wgrad_tile", "wgrad_splits", "wgrad_workgroups", "wgrad_xcd_map")] + \
        [(n, ctypes.c_int32) for n in ("pack_per_step", "edge_nchunk", "edge_n_parts", "upsample_gemm", "fwd_lds_bytes", "bwd_lds_bytes",
                                       "wgrad_lds_bytes", "wgrad2_lds_bytes")]


class TacoAttentionBackwardArgs(ctypes.Structure):
    """facppg_taco_attention_backward_args (include/facppg.h): twelve inputs, four outputs, all device pointers."""
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "w_cat", "w_query", "v", "w_loc_dense", "w_loc_conv", "memory", "align", "tanh_s", "act_a", "c_a", "base_ctx", "base_ah",
        "dgates_a", "dctx", "ds", "de")]


class WnWeights(ctypes.Structure):
    """facppg_wn_weights (include/facppg.h)."""
    _fields_ = [("start_w", ctypes.c_void_p), ("start_b", ctypes.c_void_p),
                ("in_w", ctypes.c_void_p * 8), ("in_b", ctypes.c_void_p * 8),
                ("cond_w", ctypes.c_void_p * 8), ("cond_b", ctypes.c_void_p * 8),
                ("rs_w", ctypes.c_void_p * 8), ("rs_b", ctypes.c_void_p * 8),
                ("end_w", ctypes.c_void_p), ("end_b", ctypes.c_void_p)]


class WnGrads(ctypes.Structure):
    """facppg_wn_grads (include/facppg.h): fp32 gradient outputs, same shapes as WnWeights."""
    _fields_ = WnWeights._fields_


class WnBf16Offsets(ctypes.Structure):
    """facppg_wn_bf16_offsets (include/facppg.h): where facppg_wn_forward_bf16 / _backward_bf16 keep each stage in state and scratch."""
    _fields_ = [(n, ctypes.c_int32) for n in ("Lr", "Lp", "halo", "reserved")] + \
        [(n, ctypes.c_size_t) for n in ("h", "h_stride", "ts", "ts_stride", "acts", "acts_stride", "skip", "skip_bytes", "state_end",
                                        "dpre", "dpre_stride", "dh", "dh_stride", "dskip", "dskip_bytes", "grads_end", "scratch_end")]


class GlowBf16Sizes(ctypes.Structure):
    """facppg_glow_bf16_sizes (include/facppg.h)."""
    _fields_ = [("packed_bytes_per_flow", ctypes.c_size_t), ("state_bytes_per_flow", ctypes.c_size_t), ("work_bytes", ctypes.c_size_t),
                ("n_parts", ctypes.c_int), ("part_floats", ctypes.c_int)]


class GlowFlow(ctypes.Structure):
    """facppg_glow_flow (include/facppg.h): one flow of a group call of the bf16 training direction."""
    _fields_ = [("w", ctypes.POINTER(WnWeights)), ("g", ctypes.POINTER(WnGrads)),
                ("conv_w", ctypes.c_void_p), ("d_conv_w", ctypes.c_void_p), ("logdet", ctypes.c_void_p), ("g_logdet", ctypes.c_void_p),
                ("ld_scale", ctypes.c_float), ("c", ctypes.c_int), ("early", ctypes.c_int),
                ("early_io", ctypes.c_void_p), ("early_bs", ctypes.c_long),
                ("u", ctypes.c_void_p), ("z", ctypes.c_void_p), ("wn_out", ctypes.c_void_p), ("dzp", ctypes.c_void_p),
                ("dlog_s", ctypes.c_void_p), ("dls_b", ctypes.c_long), ("dls_j", ctypes.c_long), ("dls_n", ctypes.c_long),
                ("part", ctypes.c_void_p), ("packed", ctypes.c_void_p), ("state", ctypes.c_void_p)]


class TdnnLayer(ctypes.Structure):
    """facppg_tdnn_layer (include/facppg.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("out_dim", "in_dim", "taps", "dil", "first", "relu")] + [("renorm_target_rms", ctypes.c_float)]


class F0Config(ctypes.Structure):
    """facppg_f0_config (include/facppg.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "frame_shift", "window", "lag_min", "lag_max")] + \
        [(n, ctypes.c_float) for n in ("ballast", "voicing_cost", "freq_weight")]


class AlignConfig(ctypes.Structure):
    """facppg_align_config (include/facppg.h)."""
    _fields_ = [("floor", ctypes.c_float), ("switch_cost", ctypes.c_float)]


class SumSegment(ctypes.Structure):
    """facppg_sum_segment (include/facppg.h)."""
    _fields_ = [("data_dev", ctypes.c_void_p), ("outer_stride", ctypes.c_long), ("outer", ctypes.c_int), ("inner", ctypes.c_int),
                ("square", ctypes.c_int)]


def _declare(lib):
    c = ctypes
    vp, i32, u64, f32, sz = c.c_void_p, c.c_int32, c.c_uint64, c.c_float, c.c_size_t
    sigs = {
        "facppg_version": (c.c_int, []),
        "facppg_last_error": (c.c_char_p, []),
        "facppg_wg_weight_count": (sz, [c.POINTER(WgConfig)]),
        "facppg_wg_create": (c.c_int, [c.POINTER(WgConfig), vp, sz, c.c_int, vp, c.POINTER(vp)]),
        "facppg_wg_destroy": (None, [vp]),
        "facppg_wg_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_wg_infer": (c.c_int, [vp, vp, vp, vp, u64, f32, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_wg_create_f16": (c.c_int, [c.POINTER(WgConfig), vp, sz, c.c_int, vp, c.POINTER(vp)]),
        "facppg_wg_infer_f16": (c.c_int, [vp, vp, vp, vp, u64, f32, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_wg_log_s_count": (sz, [vp, c.c_int, c.c_int]),
        "facppg_wg_forward": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_wn_train_workspace_bytes": (sz, [c.c_int, c.c_int, c.c_int]),
        "facppg_wn_forward_save": (c.c_int, [c.POINTER(WnWeights), c.c_int, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp, vp, vp,
                                             vp, sz, vp]),
        "facppg_wn_backward_data": (c.c_int, [c.POINTER(WnWeights), c.c_int, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp, vp, vp,
                                              vp, vp, sz, vp]),
        "facppg_wn_weight_grads_workspace_bytes": (sz, [c.c_int]),
        "facppg_wn_weight_grads": (c.c_int, [c.c_int, c.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, c.c_int, c.c_int, c.POINTER(WnGrads),
                                             vp, sz, vp]),
        "facppg_conv1x1": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, vp]),
        "facppg_logdet": (c.c_int, [vp, c.c_int, vp, vp, vp]),
        "facppg_conv1x1_wgrad_workspace_bytes": (sz, [c.c_int]),
        "facppg_conv1x1_wgrad": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, vp, sz, vp]),
        "facppg_wn_bf16_padded_len": (c.c_int, [c.c_int]),
        "facppg_wn_bf16_state_bytes": (sz, [c.c_int, c.c_int, c.c_int]),
        "facppg_wn_bf16_scratch_bytes": (sz, [c.c_int, c.c_int, c.c_int]),
        "facppg_wn_bf16_launch_plan": (c.c_int, [c.c_int, c.c_int, c.c_int]),
        "facppg_wn_bf16_layout": (c.c_int, [c.c_int, c.c_int, c.c_int, c.POINTER(WnBf16Offsets)]),
        "facppg_train_bf16_launch_plan": (c.c_int, [c.c_int, c.c_int, c.c_int, c.POINTER(TrainLaunchReport)]),
        "facppg_spect_to_bf16": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp]),
        "facppg_posmajor_to_f32": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, vp, c.c_int, vp]),
        "facppg_wn_forward_bf16": (c.c_int, [c.POINTER(WnWeights), c.c_int, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp, sz, vp, sz, vp]),
        "facppg_wn_backward_bf16": (c.c_int, [c.POINTER(WnWeights), c.POINTER(WnGrads), c.c_int, c.c_int, vp, vp, vp, c.c_int, c.c_int,
                                              vp, sz, vp, vp, c.c_int, vp, sz, vp]),
        "facppg_glow_bf16_layout": (c.c_int, [c.c_int, c.c_int, c.c_int, c.POINTER(GlowBf16Sizes)]),
        "facppg_glow_bf16_begin": (c.c_int, [c.POINTER(WnWeights), c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp]),
        "facppg_glow_bf16_group_forward": (c.c_int, [c.POINTER(GlowFlow), c.c_int, c.c_int, vp, c.c_long, vp, c.c_long, vp, c.c_int, c.c_int, vp]),
        "facppg_glow_bf16_group_backward": (c.c_int, [c.POINTER(GlowFlow), c.c_int, c.c_int, vp, c.c_long, vp, c.c_long, vp, vp, c.c_int, vp,
                                                      c.c_int, c.c_int, vp]),
        "facppg_upsample_forward_workspace_bytes": (sz, [c.c_int] * 6),
        "facppg_upsample_regroup_bf16": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_upsample_backward_workspace_bytes": (sz, [c.c_int] * 6),
        "facppg_upsample_regroup_backward": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_weight_norm_forward": (c.c_int, [vp, c.c_int, c.c_long, vp]),
        "facppg_weight_norm_backward": (c.c_int, [vp, vp, c.c_int, c.c_long, vp]),
        "facppg_affine_forward": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, vp]),
        "facppg_segment_sums": (c.c_int, [c.POINTER(SumSegment), c.c_int, vp, sz, vp, vp]),
        "facppg_affine_backward": (c.c_int, [vp, vp, vp, vp, vp, c.c_int, c.c_int, c.c_int, vp]),
        "facppg_wg_set_profiling": (c.c_int, [vp, c.c_int]),
        "facppg_wg_last_layer_ms": (c.c_int, [vp, c.POINTER(f32), c.POINTER(c.c_int)]),
        "facppg_wg_last_launch_shape": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "facppg_wg_last_layer_schedule": (c.c_int, [vp, c.POINTER(c.c_int)]),
        "facppg_wg_seed_layout": (c.c_int, [vp, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(sz)]),
        "facppg_wg_cond_seed": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, sz, vp, c.c_int, vp, vp]),
        "facppg_wg_mel_pad": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_wg_infer_seeded": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_uint64, f32, vp, vp, sz, vp, vp]),
        "facppg_wg_infer_f16_order": (c.c_int, [vp, vp, vp, vp, u64, f32, c.c_int, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_wg_seed_layout_f16": (c.c_int, [vp, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(sz)]),
        "facppg_wg_mel_pad_f16": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp]),
        "facppg_wg_cond_seed_f16": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, sz, vp, c.c_int, vp, vp]),
        "facppg_wg_infer_seeded_f16": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_uint64, f32, vp, vp, sz, vp, vp]),
        "facppg_wg_split_create": (c.c_int, [c.POINTER(WgConfig), vp, sz, c.c_int, vp, c.POINTER(vp)]),
        "facppg_wg_split_destroy": (None, [vp]),
        "facppg_wg_split_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_wg_split_infer": (c.c_int, [vp, vp, vp, vp, u64, f32, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_wg_split_last_launch_shape": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "facppg_wg_split_seed_layout": (c.c_int, [vp, c.c_int, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(sz), c.POINTER(c.c_int)]),
        "facppg_wg_split_mel_pad": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp]),
        "facppg_wg_split_cond_seed": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, sz, vp, c.c_int, vp, vp]),
        "facppg_wg_split_infer_seeded": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, c.c_int, vp, c.c_uint64, f32, vp, vp, sz, vp, vp]),
        "facppg_stft_create": (c.c_int, [c.c_int, c.c_int, vp, vp, vp, vp, c.c_int, c.c_int, vp, c.POINTER(vp)]),
        "facppg_stft_destroy": (None, [vp]),
        "facppg_stft_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_stft_transform": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_stft_inverse": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_stft_mel": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_denoise": (c.c_int, [vp, vp, vp, vp, f32, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_stft_set_mel_pinv": (c.c_int, [vp, vp, vp]),
        "facppg_mel_to_magnitude": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_griffin_lim_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_griffin_lim": (c.c_int, [vp, vp, vp, vp, vp, c.c_int, f32, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_griffin_lim_draw_phase": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_taco_weight_count": (sz, [c.POINTER(TacoConfig)]),
        "facppg_taco_create": (c.c_int, [c.POINTER(TacoConfig), vp, sz, c.c_int, vp, c.POINTER(vp)]),
        "facppg_taco_destroy": (None, [vp]),
        "facppg_taco_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_taco_decode_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_taco_collect_frames": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, vp, c.c_int, vp, vp, vp]),
        "facppg_taco_postnet_stream_workspace_bytes": (sz, [vp, c.c_int]),
        "facppg_taco_postnet_range": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, c.c_int, vp, sz, c.c_int, vp, vp]),
        "facppg_taco_postnet_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_taco_encode": (c.c_int, [vp, vp, vp, vp, u64, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_taco_decode": (c.c_int, [vp, vp, vp, vp, vp, vp, u64, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, vp, sz,
                                         c.POINTER(TacoDecodeOpts), vp]),
        "facppg_taco_launch_plan": (c.c_int, [c.POINTER(TacoConfig), c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int,
                                              c.POINTER(TacoLaunchReport)]),
        "facppg_taco_coop_limit": (c.c_int, [vp]),
        "facppg_taco_draw_dropout": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, vp, vp, vp]),
        "facppg_taco_encode_padded": (c.c_int, [vp, vp, vp, vp, vp, u64, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_taco_decode_forced_workspace_bytes": (sz, [vp, c.c_int, c.c_int]),
        "facppg_taco_decode_forced": (c.c_int, [vp, vp, vp, vp, vp, vp, u64, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, sz,
                                                c.POINTER(TacoDecodeOpts), vp]),
        "facppg_taco_draw_dropout_forced": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_taco_decode_forced_state": (c.c_int, [vp, vp, sz, c.c_int, c.c_int, vp, vp, vp, vp]),
        "facppg_taco_encode_state": (c.c_int, [vp, vp, sz, c.c_int, c.c_int, vp, vp]),
        "facppg_lstm_cell_scan": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, vp]),
        "facppg_lstm_backward_workspace_bytes": (sz, [c.c_int, c.c_int]),
        "facppg_lstm_backward": (c.c_int, [vp, vp, vp, vp, vp, c.c_int, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_taco_attention_backward_workspace_bytes": (sz, [c.POINTER(TacoConfig), c.c_int, c.c_int]),
        "facppg_taco_attention_backward": (c.c_int, [c.POINTER(TacoConfig), c.POINTER(TacoAttentionBackwardArgs), c.c_int, c.c_int,
                                                     c.c_int, vp, sz, vp]),
        "facppg_wg_draw_noise": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_taco_postnet": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_mfcc_create": (c.c_int, [c.c_int, c.c_int, c.c_int, vp, vp, c.c_int, vp, c.c_int, c.c_int, vp, c.POINTER(vp)]),
        "facppg_mfcc_destroy": (None, [vp]),
        "facppg_mfcc_num_frames": (c.c_int, [vp, c.c_int]),
        "facppg_mfcc_workspace_bytes": (sz, [vp, c.c_int]),
        "facppg_mfcc_compute": (c.c_int, [vp, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_cmn_splice_transform": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, c.c_int, c.c_int, vp, vp, vp]),
        "facppg_mfcc_batch_workspace_bytes": (sz, [vp, c.c_int]),
        "facppg_mfcc_compute_batch": (c.c_int, [vp, vp, vp, vp, vp, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_cmn_splice_transform_batch": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, vp, c.c_int, c.c_int, vp, vp, vp]),
        "facppg_resample_num_samples": (c.c_int, [c.c_int, c.c_int, c.c_int]),
        "facppg_resample": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, vp, vp]),
        "facppg_reduce_ppg": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, vp, vp]),
        "facppg_adam_chunk_elems": (c.c_int, []),
        "facppg_adam_step": (c.c_int, [vp, c.c_int, vp, c.c_int, vp, f32, c.c_double, c.c_double, f32, f32, vp]),
        "facppg_tdnn_weight_count": (sz, [c.POINTER(TdnnLayer), c.c_int]),
        "facppg_tdnn_create": (c.c_int, [c.POINTER(TdnnLayer), c.c_int, c.c_int, vp, sz, c.c_int, vp, c.POINTER(vp)]),
        "facppg_tdnn_destroy": (None, [vp]),
        "facppg_tdnn_context": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_int)]),
        "facppg_tdnn_workspace_bytes": (sz, [vp, c.c_int]),
        "facppg_tdnn_forward": (c.c_int, [vp, vp, c.c_int, vp, vp, sz, vp]),
        "facppg_tdnn_batch_workspace_bytes": (sz, [vp, vp, c.c_int]),
        "facppg_tdnn_forward_batch": (c.c_int, [vp, vp, vp, vp, c.c_int, vp, vp, sz, vp]),
        "facppg_tdnn_forward_batch_reduced": (c.c_int, [vp, vp, vp, vp, c.c_int, vp, c.c_int, vp, vp, sz, vp]),
        "facppg_tdnn_forward_batch_padded": (c.c_int, [vp, vp, vp, vp, c.c_int, vp, c.c_int, c.c_int, vp, vp, sz, vp]),
        "facppg_attention_window_mask": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp]),
        "facppg_ppg_pause_flags": (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_int, vp, vp, c.c_int, f32, vp, vp]),
        "facppg_ppg_gather_segments": (c.c_int, [vp, c.c_int, c.c_int, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_join_segments": (c.c_int, [vp, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp]),
        "facppg_ppg_dtw_workspace_bytes": (sz, [c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]),
        "facppg_ppg_dtw": (c.c_int, [vp, vp, vp, c.c_int, vp, vp, vp, c.c_int, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, sz, vp]),
        "facppg_mel_dtw_workspace_bytes": (sz, [c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int]),
        "facppg_mel_dtw": (c.c_int, [vp, vp, vp, c.c_int, vp, vp, vp, c.c_int, c.c_int, c.c_int, vp, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_attention_path_workspace_bytes": (sz, [c.c_int, c.c_int, c.c_int]),
        "facppg_attention_path": (c.c_int, [vp, vp, vp, c.c_int, vp, vp, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_tdnn_forward_batch_padded_strided": (c.c_int, [vp, vp, vp, vp, c.c_int, vp, c.c_int, c.c_int, sz, vp, vp, sz, vp]),
        "facppg_f0_workspace_bytes": (sz, [c.POINTER(F0Config), c.c_int]),
        "facppg_f0_nccf_batch": (c.c_int, [c.POINTER(F0Config), vp, vp, vp, vp, vp, c.c_int, vp, vp]),
        "facppg_f0_track_batch": (c.c_int, [c.POINTER(F0Config), vp, vp, vp, c.c_int, vp, vp, vp, vp, sz, vp]),
        "facppg_f0_batch": (c.c_int, [c.POINTER(F0Config), vp, vp, vp, vp, vp, c.c_int, vp, vp, vp, vp, sz, vp]),
        "facppg_lf0_rows_padded": (c.c_int, [vp, vp, vp, c.c_int, c.c_int, sz, vp, vp]),
        "facppg_ppg_emissions": (c.c_int, [c.POINTER(AlignConfig), vp, c.c_int, c.c_int, c.c_int, vp, vp, vp, vp, vp, vp]),
        "facppg_ppg_decode_phones_workspace_bytes": (sz, [c.c_int, c.c_int]),
        "facppg_ppg_decode_phones": (c.c_int, [c.POINTER(AlignConfig), vp, vp, vp, c.c_int, c.c_int, vp, vp, vp, sz, vp]),
        "facppg_ppg_force_align_workspace_bytes": (sz, [c.c_int, c.c_int]),
        "facppg_ppg_force_align": (c.c_int, [vp, vp, vp, vp, vp, c.c_int, c.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    return sigs


def exported_symbols():
    """Names include/facppg.h declares and the binding uses (checked by the CPU tests)."""
    return sorted(_declare(load()))


def load():
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise FacppgError(
                "%s is not built. Build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
                "(or `make -C fac-via-ppg_amd/csrc`). There is no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        _declare(lib)
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        raise FacppgError("libfacppg_hip: error %d: %s" % (rc, load().facppg_last_error().decode()))


def require_cuda(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise FacppgError(
            "%s must be a GPU tensor: this build runs only on the HIP kernels of libfacppg_hip.so "
            "(MI355X / gfx950); there is no CPU path." % what)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def upload(values, dtype, device):
    """A small host list -> device tensor WITHOUT stalling the host behind the work already queued on the stream: a copy
    from pageable memory waits for the stream to reach it (with a WaveGlow.infer in front, > 100 ms during which nothing
    else gets enqueued); from a pinned staging tensor it is just another queued command."""
    return torch.tensor(values, dtype=dtype).pin_memory().to(device, non_blocking=True)


def host_offsets(lengths):
    """Lengths of a batch of utterances laid end to end -> their B + 1 offsets as a C int32 array (the host copy the batch
    entry points take); ``offsets_array(values)`` wraps offsets that are already cumulative."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return offsets_array(off)


def offsets_array(offsets):
    return (ctypes.c_int32 * len(offsets))(*[int(v) for v in offsets])


def current_stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class WeightIdentity(object):
    """What a packed-weight handle was built from, cheap to re-check on every call: the identity of every parameter, buffer
    AND submodule of ``module`` (re-assigning a Parameter, or replacing a submodule -- ``model.WN[k] = ...`` --, changes an
    id in its parent's dict), and per tensor its in-place version (optimizer steps, any in-place op) and its storage address
    (``p.data = other`` keeps both the id and the version: EMA swaps and the like).  The module tree is walked once; a check
    reads the live dicts' values, and the versions / addresses of the cached flat tensor list only while the ids still match."""

    def __init__(self, module):
        self.dicts = [d for m in module.modules() for d in (m._parameters, m._buffers, m._modules)]
        self.ids = self._ids()
        self.tensors = [v for d in self.dicts for v in d.values() if torch.is_tensor(v)]
        self.state = self._state()

    def _ids(self):
        return tuple(id(v) for d in self.dicts for v in d.values())

    def _state(self):
        return tuple(t._version for t in self.tensors), tuple(t.data_ptr() for t in self.tensors)

    def unchanged(self):
        return self._ids() == self.ids and self._state() == self.state

