"""ctypes binding of libserhip.so (the C ABI in include/ser_hip.h).

There is exactly one compute backend.  If the library cannot be loaded the
import of this module raises: the product never falls back to PyTorch ops or to
the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  -- FIRST: torch brings its own libamdhip64; libserhip must bind to that copy, not load a second
#                              HIP runtime beside it (with the library loaded first, launches fail with "no ROCm-capable device")

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SER_HIP_LIB") or os.path.join(_HERE, "lib", "libserhip.so")   # override: A/B builds (tools/)

MODE_BF16 = 1
MODE_FP32X = 2
MODE_FP16 = 3
MODE_FP16X = 4
MODE_FP16Q = 5
MODE_FP16M = 6
ACT_NONE = 0
ACT_GELU = 1
WS_LOGMEL = 1
WS_WAVE_FRAMES = 2
WS_GN_STATS = 3
GRU_ERR_TIMEOUT = 1             # SER_GRU_ERR_TIMEOUT: a cluster wait of ser_gru_v gave up
RESAMPLE_TILE = 1024            # SER_RESAMPLE_TILE: output samples per block of ser_resample_v
SELECT_ROWS_TILE = 8            # SER_SELECT_ROWS_TILE: rows per block tile of ser_select_rows_v
ABI_VERSION = 18

c_void_p, c_int, c_i64, c_float = C.c_void_p, C.c_int, C.c_int64, C.c_float


class GemmArgs(C.Structure):
    """Mirror of ``ser_gemm_args`` (include/ser_hip.h); field order is ABI."""
    _fields_ = [
        ("A", c_void_p), ("a_plane_stride", c_i64), ("a_rowoff", c_void_p), ("lda", c_i64),
        ("kc", C.c_int32), ("ldj", c_i64),
        ("W", c_void_p), ("w_plane_stride", c_i64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("groups", C.c_int32),
        ("a_group_stride", c_i64), ("w_group_stride", c_i64), ("c_group_stride", C.c_int32),
        ("mode", C.c_int32), ("bias", c_void_p), ("act", C.c_int32),
        ("residual", c_void_p), ("ldr", c_i64), ("res_row_mod", C.c_int32),
        ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("out_rowmap", c_void_p),
        ("ln_gamma", c_void_p), ("ln_beta", c_void_p), ("ln_eps", c_float), ("tile_cfg", C.c_int32),
        ("ln_stats_in", c_void_p), ("ln_groups", C.c_int32), ("ln_colsum", c_void_p),
        ("stat_out", c_void_p), ("stat_groups", C.c_int32), ("f32_col_begin", C.c_int32),
        ("col_scale", c_float), ("col_scale_end", C.c_int32),
        ("shift_in", c_void_p), ("shift_out", c_void_p), ("shift_const", c_float), ("out_mode", C.c_int32),
        ("ln_shift", c_void_p), ("mean_out", c_void_p), ("lnstat_out", c_void_p),
        ("a_scale", c_void_p), ("a_scale_ld", c_i64), ("w_scale", c_void_p), ("w_scale_ld", c_i64),
        ("out_scale", c_void_p), ("out_scale_ld", c_i64), ("range_flag", c_void_p),
        ("gn_scale", c_void_p), ("gn_shift", c_void_p), ("gn_row_offs", c_void_p), ("gn_B", C.c_int32), ("gn_ld", C.c_int32),
    ]


class AttentionArgs(C.Structure):
    """Mirror of ``ser_attention_args``."""
    _fields_ = [
        ("qkv", c_void_p), ("ld", c_i64), ("plane_stride", c_i64),
        ("q_col", C.c_int32), ("k_col", C.c_int32), ("v_col", C.c_int32), ("B", C.c_int32),
        ("frame_offs", c_void_p), ("table", c_void_p), ("gate", c_void_p),
        ("max_frames", C.c_int32), ("table_T", C.c_int32),
        ("out", c_void_p), ("ldo", c_i64), ("out_plane_stride", c_i64),
        ("H", C.c_int32), ("dh", C.c_int32), ("scale", c_float), ("mode", C.c_int32),
        ("gate_col", C.c_int32), ("out_mode", C.c_int32),
        ("gru_const", c_void_p), ("key_lens", c_void_p),
        ("bias2d", c_void_p), ("bias2d_ld", c_i64),
        ("gate_x", c_void_p), ("gate_x_ld", c_i64), ("gate_x_plane_stride", c_i64),
        ("gate_stat", c_void_p), ("gate_w", c_void_p), ("gate_cb", c_void_p),
        ("gate_x_planes", C.c_int32), ("reserved1", C.c_int32), ("gate_w_plane_stride", c_i64),
        ("out_scale", c_void_p), ("out_scale_ld", c_i64),
    ]


class LayerNormArgs(C.Structure):
    """Mirror of ``ser_layernorm_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("g", c_void_p), ("b", c_void_p), ("eps", c_float), ("gelu", C.c_int32),
        ("out_f32", c_void_p), ("ldo_f32", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32), ("reserved0", C.c_int32),
        ("range_flag", c_void_p),
    ]


class WaveFramesArgs(C.Structure):
    """Mirror of ``ser_wave_frames_args``."""
    _fields_ = [
        ("wav", c_void_p), ("sample_offs", c_void_p), ("frame_offs", c_void_p),
        ("B", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("mode", C.c_int32),
        ("out", c_void_p), ("out_plane_stride", c_i64), ("work", c_void_p),
        ("total_rows", C.c_int32), ("no_norm", C.c_int32),
        ("range_flag", c_void_p),
    ]


class GnStatsArgs(C.Structure):
    """Mirror of ``ser_gn_stats_args`` (ABI 15)."""
    _fields_ = [
        ("wav", c_void_p), ("sample_offs", c_void_p), ("frame_offs", c_void_p),
        ("w", c_void_p), ("bias", c_void_p), ("gamma", c_void_p), ("beta", c_void_p),
        ("wave_stats", c_void_p),
        ("scale", c_void_p), ("shift", c_void_p), ("stat_out", c_void_p), ("work", c_void_p),
        ("B", C.c_int32), ("C", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("ld", C.c_int32), ("no_norm", C.c_int32),
        ("eps", c_float), ("reserved0", C.c_int32),
    ]


class RowCenterArgs(C.Structure):
    """Mirror of ``ser_row_center_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("stats", c_void_p), ("shift", c_void_p),
        ("stat_groups", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32),
        ("out_scale", c_void_p), ("out_scale_ld", c_i64), ("range_flag", c_void_p),
    ]


class LogmelArgs(C.Structure):
    """Mirror of ``ser_logmel_args``."""
    _fields_ = [("wav", c_void_p), ("sample_offs", c_void_p), ("mel", c_void_p), ("out", c_void_p), ("work", c_void_p),
                ("B", C.c_int32), ("n_mels", C.c_int32)]


class PackActArgs(C.Structure):
    """Mirror of ``ser_pack_act_args``."""
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("ldo", c_i64), ("out_plane_stride", c_i64),
                ("B", C.c_int32), ("C", C.c_int32), ("T", C.c_int32), ("halo", C.c_int32), ("mode", C.c_int32), ("reserved0", C.c_int32),
                ("range_flag", c_void_p)]


class PosLnArgs(C.Structure):
    """Mirror of ``ser_pos_ln_args`` (ABI 16)."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("out_rowmap", c_void_p),
        ("residual", c_void_p), ("ldr", c_i64),
        ("g", c_void_p), ("b", c_void_p),
        ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("eps_pos", c_float), ("eps", c_float),
        ("last", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32),
        ("range_flag", c_void_p),
    ]


class ResampleArgs(C.Structure):
    """Mirror of ``ser_resample_args`` (ABI 18)."""
    _fields_ = [
        ("wav", c_void_p), ("in_offs", c_void_p), ("out_offs", c_void_p),
        ("up", c_void_p), ("down", c_void_p), ("half", c_void_p), ("bank_off", c_void_p),
        ("bank", c_void_p), ("out", c_void_p),
        ("total_in", c_i64), ("total_out", c_i64), ("max_out", c_i64),
        ("B", C.c_int32), ("reserved0", C.c_int32),
    ]


class AspPoolArgs(C.Structure):
    """Mirror of ``ser_asp_pool_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("hlin", c_void_p), ("ldh", c_i64), ("a", c_void_p), ("frame_offs", c_void_p),
        ("scores", c_void_p), ("out", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("D", C.c_int32), ("rows", C.c_int32), ("max_frames", C.c_int32),
    ]


class MlpHeadArgs(C.Structure):
    """Mirror of ``ser_mlp_head_args``."""
    _fields_ = [
        ("p", c_void_p), ("ldp", c_i64),
        ("W1", c_void_p), ("b1", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
        ("hidden", c_void_p), ("out", c_void_p),
        ("eps", c_float),
        ("B", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("n_out", C.c_int32), ("reserved0", C.c_int32),
    ]


class LayerPoolArgs(C.Structure):
    """Mirror of ``ser_layer_pool_args``."""
    _fields_ = [
        ("s", c_void_p), ("state_stride", c_i64), ("lds", c_i64), ("w", c_void_p),
        ("frame_offs", c_void_p), ("frame_offs_host", c_void_p),
        ("work", c_void_p), ("work_elems", c_i64), ("out", c_void_p), ("ldo", c_i64),
        ("n_states", C.c_int32), ("B", C.c_int32), ("D", C.c_int32), ("rows", C.c_int32), ("max_frames", C.c_int32), ("reserved0", C.c_int32),
    ]


class ClsTailArgs(C.Structure):
    """Mirror of ``ser_cls_tail_args``."""
    _fields_ = [
        ("pooled", c_void_p), ("ldp", c_i64), ("P", c_void_p), ("bp", c_void_p), ("C", c_void_p), ("bc", c_void_p),
        ("out", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("D", C.c_int32), ("proj", C.c_int32), ("n_labels", C.c_int32),
    ]


class LayerMixArgs(C.Structure):
    """Mirror of ``ser_layer_mix_args``."""
    _fields_ = [
        ("s", c_void_p), ("state_stride", c_i64), ("lds", c_i64), ("w", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("range_flag", c_void_p),
        ("n_states", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32),
    ]


class StatPoolArgs(C.Structure):
    """Mirror of ``ser_stat_pool_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("frame_offs", c_void_p), ("frame_offs_host", c_void_p),
        ("work", c_void_p), ("work_elems", c_i64), ("out", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("D", C.c_int32), ("rows", C.c_int32), ("max_frames", C.c_int32), ("relu", C.c_int32), ("reserved0", C.c_int32),
    ]


class XvecTailArgs(C.Structure):
    """Mirror of ``ser_xvec_tail_args``."""
    _fields_ = [
        ("stats", c_void_p), ("lds", c_i64), ("F", c_void_p), ("bf", c_void_p), ("C", c_void_p), ("bc", c_void_p),
        ("emb", c_void_p), ("lde", c_i64), ("logits", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("D", C.c_int32), ("dim", C.c_int32), ("n_labels", C.c_int32),
    ]


class CtcGreedyArgs(C.Structure):
    """Mirror of ``ser_ctc_greedy_args``."""
    _fields_ = [
        ("z", c_void_p), ("ldz", c_i64), ("frame_offs", c_void_p), ("work", c_void_p), ("work_elems", c_i64),
        ("ids", c_void_p), ("starts", c_void_p), ("ends", c_void_p), ("ld_tok", c_i64), ("counts", c_void_p),
        ("frame_ids", c_void_p), ("frame_margin", c_void_p), ("min_margin", c_void_p), ("err", c_void_p),
        ("B", C.c_int32), ("V", C.c_int32), ("rows", C.c_int32), ("blank", C.c_int32), ("max_frames", C.c_int32), ("reserved0", C.c_int32),
    ]


class CtcAlignArgs(C.Structure):
    """Mirror of ``ser_ctc_align_args``."""
    _fields_ = [
        ("z", c_void_p), ("ldz", c_i64), ("frame_offs", c_void_p), ("targets", c_void_p), ("tgt_offs", c_void_p),
        ("work", c_void_p), ("work_bytes", c_i64),
        ("starts", c_void_p), ("ends", c_void_p), ("tok_score", c_void_p), ("ld_tok", c_i64), ("status", c_void_p), ("path_logit", c_void_p),
        ("pos", c_void_p), ("frame_score", c_void_p),
        ("B", C.c_int32), ("V", C.c_int32), ("rows", C.c_int32), ("blank", C.c_int32), ("max_frames", C.c_int32), ("max_tokens", C.c_int32),
        ("n_targets", C.c_int32), ("reserved0", C.c_int32),
    ]


class DecKeepQArgs(C.Structure):
    """Mirror of ``ser_dec_keep_q_args``."""
    _fields_ = [
        ("q", c_void_p), ("ldq", c_i64), ("pos", c_void_p), ("keep", c_void_p), ("head", C.c_int32 * 16),
        ("n_heads", C.c_int32), ("slot0", C.c_int32), ("n_align", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("max_pos", C.c_int32),
    ]


class TsWeightsArgs(C.Structure):
    """Mirror of ``ser_ts_weights_args``."""
    _fields_ = [
        ("keep", c_void_p), ("cross", c_void_p), ("layer_stride", c_i64), ("batch_stride", c_i64), ("ldc", c_i64),
        ("n_rows", c_void_p), ("n_frames", c_void_p), ("w", c_void_p), ("ld_w", c_i64), ("scale", c_float),
        ("B", C.c_int32), ("n_align", C.c_int32), ("n_keys", C.c_int32), ("pos0", C.c_int32), ("max_rows", C.c_int32), ("max_pos", C.c_int32),
        ("n_layers", C.c_int32), ("H", C.c_int32), ("reserved0", C.c_int32),
        ("head_layer", C.c_int32 * 32), ("head_index", C.c_int32 * 32),
    ]


class TsMatrixArgs(C.Structure):
    """Mirror of ``ser_ts_matrix_args``."""
    _fields_ = [
        ("w", c_void_p), ("ld_w", c_i64), ("n_rows", c_void_p), ("n_frames", c_void_p), ("stats", c_void_p),
        ("matrix", c_void_p), ("ld_m", c_i64), ("status", c_void_p),
        ("B", C.c_int32), ("n_align", C.c_int32), ("max_rows", C.c_int32), ("max_frames", C.c_int32), ("width", C.c_int32), ("reserved0", C.c_int32),
    ]


class DtwArgs(C.Structure):
    """Mirror of ``ser_dtw_args``."""
    _fields_ = [
        ("matrix", c_void_p), ("ld_m", c_i64), ("n_rows", c_void_p), ("n_frames", c_void_p), ("work", c_void_p), ("work_bytes", c_i64),
        ("first_frame", c_void_p), ("ld_t", c_i64), ("status", c_void_p),
        ("path_text", c_void_p), ("path_time", c_void_p), ("path_len", c_void_p),
        ("B", C.c_int32), ("max_rows", C.c_int32), ("max_frames", C.c_int32), ("reserved0", C.c_int32),
    ]


class GruArgs(C.Structure):
    """Mirror of ``ser_gru_args``."""
    _fields_ = [
        ("gx", c_void_p), ("ldgx", c_i64), ("whh", c_void_p), ("whh_plane_stride", c_i64), ("bhh", c_void_p), ("frame_offs", c_void_p),
        ("out", c_void_p), ("ldo", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("work", c_void_p), ("work_bytes", c_i64), ("err", c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("rows", C.c_int32), ("max_frames", C.c_int32), ("mode", C.c_int32), ("cluster", C.c_int32),
        ("epoch", C.c_uint32), ("reserved0", C.c_int32),
    ]


class XattnArgs(C.Structure):
    """Mirror of ``ser_xattn_args``."""
    _fields_ = [
        ("q", c_void_p), ("ldq", c_i64), ("k", c_void_p), ("ldk", c_i64), ("v", c_void_p), ("ldv", c_i64),
        ("q_offs", c_void_p), ("k_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("range_flag", c_void_p), ("scale", c_float),
        ("B", C.c_int32), ("E", C.c_int32), ("q_rows", C.c_int32), ("k_rows", C.c_int32), ("max_q", C.c_int32), ("mode", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class XattnMhArgs(C.Structure):
    """Mirror of ``ser_xattn_mh_args``."""
    _fields_ = [
        ("q", c_void_p), ("ldq", c_i64), ("k", c_void_p), ("ldk", c_i64), ("v", c_void_p), ("ldv", c_i64),
        ("q_offs", c_void_p), ("k_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("range_flag", c_void_p), ("scale", c_float),
        ("B", C.c_int32), ("E", C.c_int32), ("heads", C.c_int32), ("q_rows", C.c_int32), ("k_rows", C.c_int32), ("max_q", C.c_int32),
        ("mode", C.c_int32),
    ]


class AttnPoolArgs(C.Structure):
    """Mirror of ``ser_attn_pool_args``."""
    _fields_ = [
        ("a", c_void_p), ("lda", c_i64), ("b", c_void_p), ("ldb", c_i64), ("w", c_void_p), ("frame_offs", c_void_p),
        ("scores", c_void_p), ("out", c_void_p), ("ldo", c_i64), ("bias", c_float),
        ("col0", C.c_int32), ("B", C.c_int32), ("E", C.c_int32), ("rows", C.c_int32), ("max_frames", C.c_int32), ("reserved0", C.c_int32),
    ]


class FusionClsArgs(C.Structure):
    """Mirror of ``ser_fusion_cls_args``."""
    _fields_ = [
        ("p", c_void_p), ("ldp", c_i64), ("gamma", c_void_p), ("beta", c_void_p),
        ("W1", c_void_p), ("b1", c_void_p), ("W2", c_void_p), ("b2", c_void_p),
        ("xn", c_void_p), ("hidden", c_void_p), ("out", c_void_p), ("eps", c_float),
        ("B", C.c_int32), ("K", C.c_int32), ("H1", C.c_int32), ("n_out", C.c_int32), ("reserved0", C.c_int32),
    ]


class SelectRowsArgs(C.Structure):
    """Mirror of ``ser_select_rows_args``."""
    _fields_ = [
        ("src", c_void_p * 4), ("ld_src", c_i64), ("src_offs", c_void_p), ("dst_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("out_f32", c_void_p), ("ldo_f32", c_i64),
        ("range_flag", c_void_p),
        ("n_src", C.c_int32), ("B", C.c_int32), ("D", C.c_int32), ("max_rows", C.c_int32), ("mode", C.c_int32), ("reserved0", C.c_int32),
    ]


class DecEmbedArgs(C.Structure):
    """Mirror of ``ser_dec_embed_args``."""
    _fields_ = [("ids", c_void_p), ("ld_ids", c_i64), ("pos", c_void_p), ("embed_tokens", c_void_p), ("embed_positions", c_void_p),
                ("out", c_void_p), ("ldo", c_i64), ("B", C.c_int32), ("D", C.c_int32), ("vocab", C.c_int32), ("max_pos", C.c_int32)]


class DecAttnArgs(C.Structure):
    """Mirror of ``ser_dec_attn_args``."""
    _fields_ = [
        ("q", c_void_p), ("ldq", c_i64), ("k_new", c_void_p), ("v_new", c_void_p), ("ld_new", c_i64),
        ("kcache", c_void_p), ("vcache", c_void_p), ("ldc", c_i64), ("batch_stride", c_i64),
        ("lens", c_void_p), ("lens_stride", C.c_int32), ("len_add", C.c_int32),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("range_flag", c_void_p), ("scale", c_float),
        ("B", C.c_int32), ("H", C.c_int32), ("dh", C.c_int32), ("max_len", C.c_int32), ("mode", C.c_int32),
    ]


class DecSelectArgs(C.Structure):
    """Mirror of ``ser_dec_select_args``."""
    _fields_ = [
        ("logits", c_void_p), ("ldl", c_i64), ("mask", c_void_p), ("ldm", c_i64), ("phase", c_void_p), ("forced", c_void_p),
        ("ids", c_void_p), ("ld_ids", c_i64), ("finished", c_void_p), ("margin", c_void_p), ("ld_margin", c_i64),
        ("pos", c_void_p), ("unfinished", c_void_p), ("work", c_void_p), ("err", c_void_p),
        ("B", C.c_int32), ("V", C.c_int32), ("eos", C.c_int32), ("pad", C.c_int32), ("max_pos", C.c_int32), ("reserved0", C.c_int32),
    ]


class DecAttnBeamArgs(C.Structure):
    """Mirror of ``ser_dec_attn_beam_args``."""
    _fields_ = [("base", DecAttnArgs), ("src", c_void_p), ("src_parity_stride", c_i64), ("ld_src", C.c_int32), ("row_div", C.c_int32)]


class BeamSelectArgs(C.Structure):
    """Mirror of ``ser_beam_select_args``."""
    _fields_ = [
        ("logits", c_void_p), ("ldl", c_i64), ("mask", c_void_p), ("ldm", c_i64), ("phase", c_void_p), ("lenpow", c_void_p),
        ("ids", c_void_p), ("ld_ids", c_i64), ("src", c_void_p), ("src_parity_stride", c_i64),
        ("run", c_void_p), ("fin_score", c_void_p), ("fin_handle", c_void_p), ("state", c_void_p),
        ("trace_run", c_void_p), ("trace_cand", c_void_p), ("cand_score", c_void_p), ("gaps", c_void_p),
        ("work", c_void_p), ("work_bytes", c_i64), ("pos", c_void_p), ("unfinished", c_void_p), ("ticket", c_void_p), ("err", c_void_p),
        ("B", C.c_int32), ("K", C.c_int32), ("V", C.c_int32), ("eos", C.c_int32), ("pad", C.c_int32), ("max_pos", C.c_int32),
        ("max_length", C.c_int32), ("prompt_len", C.c_int32), ("ld_src", C.c_int32), ("reserved0", C.c_int32),
    ]


class DecSelectTsArgs(C.Structure):
    """Mirror of ``ser_dec_select_ts_args``."""
    _fields_ = [("base", DecSelectArgs), ("ts_gap", c_void_p), ("ld_gap", c_i64),
                ("ts_begin", C.c_int32), ("no_ts", C.c_int32), ("begin_index", C.c_int32), ("max_initial", C.c_int32)]


class DecSelectScoreArgs(C.Structure):
    """Mirror of ``ser_dec_select_score_args``."""
    _fields_ = [("ts", DecSelectTsArgs), ("logprob", c_void_p), ("ld_logprob", c_i64), ("no_speech", c_void_p),
                ("no_speech_token", C.c_int32), ("rule", C.c_int32)]


class LogmelLongArgs(C.Structure):
    """Mirror of ``ser_logmel_long_args``."""
    _fields_ = [("wav", c_void_p), ("sample_offs", c_void_p), ("sample_offs_host", c_void_p), ("mel", c_void_p),
                ("out", c_void_p), ("bases", c_void_p), ("tiles", c_void_p), ("files", c_void_p), ("table", c_void_p), ("scratch", c_void_p),
                ("B", C.c_int32), ("n_mels", C.c_int32), ("n_tiles", C.c_int32), ("max_pitch", C.c_int32)]


class MelWindowArgs(C.Structure):
    """Mirror of ``ser_mel_window_args``."""
    _fields_ = [("src", c_void_p), ("rows", c_void_p), ("rows_host", c_void_p), ("out", c_void_p), ("B", C.c_int32), ("n_mels", C.c_int32)]


class ProsodyMelArgs(C.Structure):
    """Mirror of ``ser_prosody_mel_args``."""
    _fields_ = [
        ("wav", c_void_p), ("sample_offs", c_void_p), ("frame_offs", c_void_p),
        ("dft", c_void_p), ("mel", c_void_p), ("lin_w", c_void_p), ("lin_b", c_void_p),
        ("mel_out", c_void_p), ("out", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("max_frames", C.c_int32), ("n_bins", C.c_int32), ("n_mels", C.c_int32), ("D", C.c_int32), ("reserved0", C.c_int32),
    ]


class FvqArgs(C.Structure):
    """Mirror of ``ser_fvq_args``."""
    _fields_ = [
        ("z", c_void_p), ("ldz", c_i64), ("w_in", c_void_p), ("b_in", c_void_p), ("codes", c_void_p),
        ("table", c_void_p), ("ld_table", c_i64), ("idx", c_void_p), ("gap", c_void_p),
        ("out_f32", c_void_p), ("ldo_f32", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("range_flag", c_void_p), ("err", c_void_p),
        ("rows", C.c_int32), ("D", C.c_int32), ("n_codes", C.c_int32), ("code_dim", C.c_int32), ("mode", C.c_int32), ("reserved0", C.c_int32),
    ]


class ActRowsArgs(C.Structure):
    """Mirror of ``ser_act_rows_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64),
        ("out_rowmap", c_void_p), ("range_flag", c_void_p),
        ("relu", C.c_int32), ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32),
    ]


class CodecUnitArgs(C.Structure):
    """Mirror of ``ser_codec_unit_args``."""
    _fields_ = [
        ("x", c_void_p), ("y", c_void_p), ("row_offs", c_void_p), ("taps", c_void_p),
        ("ea1", c_void_p), ("ib1", c_void_p), ("w7", c_void_p), ("b7", c_void_p),
        ("ea2", c_void_p), ("ib2", c_void_p), ("w1", c_void_p), ("b1", c_void_p),
        ("B", C.c_int32), ("C", C.c_int32), ("k", C.c_int32), ("dilation", C.c_int32), ("max_rows", C.c_int32), ("rows", C.c_int32),
    ]


class CodecConvArgs(C.Structure):
    """Mirror of ``ser_codec_conv_args``."""
    _fields_ = [
        ("x", c_void_p), ("in_offs", c_void_p), ("out_offs", c_void_p),
        ("taps", c_void_p), ("ea", c_void_p), ("ib", c_void_p), ("w", c_void_p), ("bias", c_void_p),
        ("y", c_void_p), ("ldy", c_i64),
        ("B", C.c_int32), ("C_in", C.c_int32), ("C_out", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
        ("max_out_rows", C.c_int32), ("rows", C.c_int32),
    ]


class SnakeArgs(C.Structure):
    """Mirror of ``ser_snake_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("row_offs", c_void_p), ("taps", c_void_p), ("ea", c_void_p), ("ib", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("out_rowmap", c_void_p),
        ("out_f32", c_void_p), ("ldo_f32", c_i64), ("range_flag", c_void_p),
        ("B", C.c_int32), ("C", C.c_int32), ("max_rows", C.c_int32), ("rows", C.c_int32), ("mode", C.c_int32), ("reserved0", C.c_int32),
    ]


class FbankArgs(C.Structure):
    """Mirror of ``ser_fbank_args``."""
    _fields_ = [
        ("wav", c_void_p), ("sample_offs", c_void_p), ("mel_offs", c_void_p), ("frame_offs", c_void_p),
        ("dft", c_void_p), ("melw", c_void_p), ("mel_range", c_void_p), ("work", c_void_p), ("out", c_void_p), ("ldo", c_i64),
        ("B", C.c_int32), ("max_mel_frames", C.c_int32), ("n_mels", C.c_int32), ("stride", C.c_int32),
    ]


class RelkeyTableArgs(C.Structure):
    """Mirror of ``ser_relkey_table_args``."""
    _fields_ = [
        ("qkv", c_void_p), ("ld", c_i64), ("plane_stride", c_i64), ("E", c_void_p), ("qe", c_void_p), ("ld_qe", c_i64),
        ("q_col", C.c_int32), ("rows", C.c_int32), ("H", C.c_int32), ("dh", C.c_int32), ("P", C.c_int32), ("mode", C.c_int32),
    ]


class AttentionRkArgs(C.Structure):
    """Mirror of ``ser_attention_rk_args``."""
    _fields_ = [("base", AttentionArgs), ("qe", c_void_p), ("ld_qe", c_i64), ("left_max", C.c_int32), ("right_max", C.c_int32)]


class ConformerConvArgs(C.Structure):
    """Mirror of ``ser_conformer_conv_args``."""
    _fields_ = [
        ("y", c_void_p), ("ldy", c_i64), ("w", c_void_p), ("gamma", c_void_p), ("beta", c_void_p), ("frame_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("range_flag", c_void_p), ("eps", c_float),
        ("B", C.c_int32), ("D", C.c_int32), ("K", C.c_int32), ("max_frames", C.c_int32), ("rows", C.c_int32), ("mode", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class SwishRowsArgs(C.Structure):
    """Mirror of ``ser_swish_rows_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("range_flag", c_void_p),
        ("mode", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32), ("reserved0", C.c_int32),
    ]


class RopeRowsArgs(C.Structure):
    """Mirror of ``ser_rope_rows_args``."""
    _fields_ = [
        ("x", c_void_p), ("ldx", c_i64), ("cos_t", c_void_p), ("sin_t", c_void_p), ("frame_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("range_flag", c_void_p),
        ("B", C.c_int32), ("rows", C.c_int32), ("D", C.c_int32), ("dh", C.c_int32), ("table_T", C.c_int32), ("max_frames", C.c_int32),
        ("mode", C.c_int32), ("reserved0", C.c_int32),
    ]


class ConformerConvBnArgs(C.Structure):
    """Mirror of ``ser_conformer_conv_bn_args``."""
    _fields_ = [
        ("y", c_void_p), ("ldy", c_i64), ("w", c_void_p), ("scale", c_void_p), ("shift", c_void_p), ("frame_offs", c_void_p),
        ("out_act", c_void_p), ("ldo_act", c_i64), ("out_plane_stride", c_i64), ("range_flag", c_void_p),
        ("B", C.c_int32), ("D", C.c_int32), ("K", C.c_int32), ("max_frames", C.c_int32), ("rows", C.c_int32), ("mode", C.c_int32),
    ]


class RelposBiasArgs(C.Structure):
    """Mirror of ``ser_relpos_bias_args``."""
    _fields_ = [
        ("qkv", c_void_p), ("ld", c_i64), ("plane_stride", c_i64), ("P", c_void_p), ("ldp", c_i64), ("off", c_void_p),
        ("frame_offs", c_void_p), ("pb", c_void_p), ("ld_pb", c_i64),
        ("q_col", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("dh", C.c_int32), ("P_T", C.c_int32), ("max_frames", C.c_int32),
        ("rows", C.c_int32), ("mode", C.c_int32),
    ]


class AttentionRbArgs(C.Structure):
    """Mirror of ``ser_attention_rb_args``."""
    _fields_ = [("base", AttentionArgs), ("pb", c_void_p), ("ld_pb", c_i64)]


LAYER_POOL_FC = 32              # SER_LAYER_POOL_FC: frames per chunk of ser_layer_pool_v
CLS_TAIL_MAX = 2048             # widest projector / most labels of ser_cls_tail_v (and widest embedding / most labels of ser_xvec_tail_v)
STAT_POOL_FC = 32               # SER_STAT_POOL_FC: frames per chunk of ser_stat_pool_v
CCONV_TILE = 8                  # SER_CCONV_TILE: rows per block of ser_conformer_conv_v
CODEC_TILE = 128                # SER_CODEC_TILE: output rows per block of ser_codec_unit_v
FVQ_ERR_NONFINITE = 1           # ser_fvq_v *err bit 0: a row's projected latent was not finite
DEC_ERR_NONFINITE = 1           # ser_dec_select_v *err bit 0: a winning masked logit was not finite
DEC_ERR_POSITION = 4            # bit 2: the position left the ids buffer
BEAM_ERR_CANDIDATES = 8         # ser_beam_select_v *err bit 3: fewer than 2K finite candidates (bits 0 and 2 as ser_dec_select_v's)
BEAM_MAX_K = 8                  # SER_BEAM_MAX_K: the most beams
BEAM_CHUNK = 4096               # SER_BEAM_CHUNK: vocabulary columns per block of ser_beam_select_v's scan
CTC_CHUNK = 256                 # SER_CTC_CHUNK: frames per chunk of ser_ctc_greedy_v's collapse
CTC_ERR_NONFINITE = 1           # ser_ctc_greedy_v *err bit 0: a frame's winning logit was not finite
WAVE = 64                       # lanes of a wave: a ballot of ser_ctc_align_v packs the back pointers of 64 consecutive states
CTC_ALIGN_THREADS = 512         # SER_CTC_ALIGN_THREADS: threads of ser_ctc_align_v's block (state s on thread s % THREADS)
CTC_ALIGN_MAX_TOKENS = 1023     # SER_CTC_ALIGN_MAX_TOKENS: the longest target of ser_ctc_align_v
CTC_ALIGN_INFEASIBLE = 1        # ser_ctc_align_v status: too few frames for the target
CTC_ALIGN_NONFINITE = 2         # a NaN or +inf in a column the trellis reads, or a best score that is not finite
CTC_ALIGN_BAD_TARGET = 4        # a target id outside [0, V) or equal to the blank, or a target / utterance over the limits
TS_THREADS = 512                # SER_TS_THREADS: threads of ser_dtw_v's block = its most token rows
TS_BAND = 256                   # SER_TS_BAND: frames per band of ser_dtw_v's backtrack
TS_MAX_KEYS = 1536              # SER_TS_MAX_KEYS: the most cross keys ser_ts_weights_v takes (Whisper: 1500)
TS_MAX_HEADS = 32               # SER_TS_MAX_HEADS: the most alignment heads
TS_KEEP_HEADS = 16              # SER_TS_KEEP_HEADS: the most heads of one ser_dec_keep_q_v launch
TS_NONFINITE = 1                # ser_ts_matrix_v / ser_dtw_v status: a z-score, matrix entry or final cost that is not finite
TS_BAD_SHAPE = 2                # a row or frame count outside the buffers
TS_NO_FRAMES = 4                # token rows but no frame


class _CmdUnion(C.Union):
    _fields_ = [("gemm", GemmArgs), ("attention", AttentionArgs), ("layernorm", LayerNormArgs), ("wave_frames", WaveFramesArgs),
                ("row_center", RowCenterArgs), ("logmel", LogmelArgs), ("pack_act", PackActArgs), ("gn_stats", GnStatsArgs),
                ("pos_ln", PosLnArgs), ("dec_embed", DecEmbedArgs), ("dec_attn", DecAttnArgs), ("dec_select", DecSelectArgs),
                ("prosody_mel", ProsodyMelArgs), ("fvq", FvqArgs), ("act_rows", ActRowsArgs),
                ("codec_unit", CodecUnitArgs), ("codec_conv", CodecConvArgs), ("snake", SnakeArgs),
                ("fbank", FbankArgs), ("relkey_table", RelkeyTableArgs), ("attention_rk", AttentionRkArgs),
                ("conformer_conv", ConformerConvArgs), ("swish_rows", SwishRowsArgs), ("dec_keep_q", DecKeepQArgs),
                ("dec_attn_beam", DecAttnBeamArgs), ("beam_select", BeamSelectArgs),
                ("rope_rows", RopeRowsArgs), ("conformer_conv_bn", ConformerConvBnArgs), ("relpos_bias", RelposBiasArgs),
                ("attention_rb", AttentionRbArgs), ("dec_select_ts", DecSelectTsArgs),
                ("logmel_long", LogmelLongArgs), ("mel_window", MelWindowArgs), ("dec_select_score", DecSelectScoreArgs)]


class Cmd(C.Structure):
    """Mirror of ``ser_cmd``: one recorded launch of a command list (``ser_run``)."""
    _fields_ = [("op", C.c_int32), ("reserved0", C.c_int32), ("u", _CmdUnion)]


OP_GEMM, OP_ATTENTION, OP_LAYERNORM, OP_WAVE_FRAMES, OP_ROW_CENTER, OP_LOGMEL, OP_PACK_ACT, OP_GN_STATS, OP_POS_LN = 1, 2, 3, 4, 5, 6, 7, 8, 9
OP_DEC_EMBED, OP_DEC_ATTN, OP_DEC_SELECT = 10, 11, 12
OP_PROSODY_MEL, OP_FVQ, OP_ACT_ROWS = 13, 14, 15
OP_CODEC_UNIT, OP_CODEC_CONV, OP_SNAKE = 16, 17, 18
OP_FBANK, OP_RELKEY_TABLE, OP_ATTENTION_RK, OP_CONFORMER_CONV, OP_SWISH_ROWS = 19, 20, 21, 22, 23
OP_DEC_KEEP_Q = 24
OP_DEC_ATTN_BEAM, OP_BEAM_SELECT = 25, 26
OP_ROPE_ROWS, OP_CONFORMER_CONV_BN, OP_RELPOS_BIAS, OP_ATTENTION_RB = 27, 28, 29, 30
OP_DEC_SELECT_TS = 31
OP_LOGMEL_LONG, OP_MEL_WINDOW = 32, 33
OP_DEC_SELECT_SCORE = 34
STRUCT_MIRRORS = {"ser_gemm_args": GemmArgs, "ser_attention_args": AttentionArgs, "ser_layernorm_args": LayerNormArgs,
                  "ser_wave_frames_args": WaveFramesArgs, "ser_row_center_args": RowCenterArgs, "ser_logmel_args": LogmelArgs,
                  "ser_pack_act_args": PackActArgs, "ser_gn_stats_args": GnStatsArgs, "ser_pos_ln_args": PosLnArgs, "ser_resample_args": ResampleArgs, "ser_asp_pool_args": AspPoolArgs,
                  "ser_mlp_head_args": MlpHeadArgs, "ser_gru_args": GruArgs, "ser_xattn_args": XattnArgs, "ser_xattn_mh_args": XattnMhArgs, "ser_attn_pool_args": AttnPoolArgs,
                  "ser_fusion_cls_args": FusionClsArgs, "ser_select_rows_args": SelectRowsArgs, "ser_dec_embed_args": DecEmbedArgs, "ser_dec_attn_args": DecAttnArgs,
                  "ser_dec_select_args": DecSelectArgs, "ser_prosody_mel_args": ProsodyMelArgs, "ser_fvq_args": FvqArgs,
                  "ser_act_rows_args": ActRowsArgs, "ser_codec_unit_args": CodecUnitArgs, "ser_codec_conv_args": CodecConvArgs,
                  "ser_snake_args": SnakeArgs, "ser_fbank_args": FbankArgs, "ser_relkey_table_args": RelkeyTableArgs,
                  "ser_attention_rk_args": AttentionRkArgs, "ser_conformer_conv_args": ConformerConvArgs,
                  "ser_swish_rows_args": SwishRowsArgs, "ser_layer_pool_args": LayerPoolArgs, "ser_cls_tail_args": ClsTailArgs,
                  "ser_layer_mix_args": LayerMixArgs, "ser_stat_pool_args": StatPoolArgs, "ser_xvec_tail_args": XvecTailArgs,
                  "ser_ctc_greedy_args": CtcGreedyArgs, "ser_ctc_align_args": CtcAlignArgs,
                  "ser_dec_keep_q_args": DecKeepQArgs, "ser_ts_weights_args": TsWeightsArgs, "ser_ts_matrix_args": TsMatrixArgs,
                  "ser_dtw_args": DtwArgs, "ser_dec_attn_beam_args": DecAttnBeamArgs, "ser_beam_select_args": BeamSelectArgs,
                  "ser_rope_rows_args": RopeRowsArgs, "ser_conformer_conv_bn_args": ConformerConvBnArgs,
                  "ser_relpos_bias_args": RelposBiasArgs, "ser_attention_rb_args": AttentionRbArgs,
                  "ser_dec_select_ts_args": DecSelectTsArgs,
                  "ser_logmel_long_args": LogmelLongArgs, "ser_mel_window_args": MelWindowArgs,
                  "ser_dec_select_score_args": DecSelectScoreArgs,
                  "ser_cmd": Cmd}

_SIGNATURES = {
    "ser_version": (c_int, []),
    "ser_last_error": (C.c_char_p, []),
    "ser_wave_norm": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "ser_wave_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_i64, c_int, c_void_p,
                                c_int, c_void_p]),
    "ser_conv0_ln_gelu": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_i64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ser_gemm": (c_int, [C.POINTER(GemmArgs), c_void_p]),
    "ser_layernorm": (c_int, [c_void_p, c_i64, c_void_p, c_void_p, c_float, c_int, c_void_p, c_i64, c_void_p, c_i64,
                              c_i64, c_int, c_int, c_int, c_void_p]),
    "ser_row_center": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ser_row_center_v": (c_int, [c_void_p, c_void_p]),
    "ser_layernorm_v": (c_int, [c_void_p, c_void_p]),
    "ser_wave_frames_v": (c_int, [c_void_p, c_void_p]),
    "ser_pack_act_v": (c_int, [c_void_p, c_void_p]),
    "ser_gn_stats_v": (c_int, [c_void_p, c_void_p]),
    "ser_pos_ln_v": (c_int, [c_void_p, c_void_p]),
    "ser_resample_v": (c_int, [c_void_p, c_void_p]),
    "ser_asp_pool_v": (c_int, [c_void_p, c_void_p]),
    "ser_mlp_head_v": (c_int, [c_void_p, c_void_p]),
    "ser_layer_pool_v": (c_int, [c_void_p, c_void_p]),
    "ser_cls_tail_v": (c_int, [c_void_p, c_void_p]),
    "ser_layer_mix_v": (c_int, [c_void_p, c_void_p]),
    "ser_stat_pool_v": (c_int, [c_void_p, c_void_p]),
    "ser_xvec_tail_v": (c_int, [c_void_p, c_void_p]),
    "ser_ctc_greedy_v": (c_int, [c_void_p, c_void_p]),
    "ser_ctc_align_v": (c_int, [c_void_p, c_void_p]),
    "ser_ctc_align_work_bytes": (c_i64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ser_dec_keep_q_v": (c_int, [c_void_p, c_void_p]),
    "ser_ts_weights_v": (c_int, [c_void_p, c_void_p]),
    "ser_ts_matrix_v": (c_int, [c_void_p, c_void_p]),
    "ser_dtw_v": (c_int, [c_void_p, c_void_p]),
    "ser_dtw_work_bytes": (c_i64, [C.c_int32, C.c_int32, C.c_int32]),
    "ser_dec_attn_beam_v": (c_int, [c_void_p, c_void_p]),
    "ser_beam_select_v": (c_int, [c_void_p, c_void_p]),
    "ser_beam_work_bytes": (c_i64, [C.c_int32, C.c_int32, C.c_int32]),
    "ser_gru_v": (c_int, [c_void_p, c_void_p]),
    "ser_gru_work_bytes": (c_i64, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ser_xattn_v": (c_int, [c_void_p, c_void_p]),
    "ser_xattn_mh_v": (c_int, [c_void_p, c_void_p]),
    "ser_attn_pool_v": (c_int, [c_void_p, c_void_p]),
    "ser_fusion_cls_v": (c_int, [c_void_p, c_void_p]),
    "ser_select_rows_v": (c_int, [c_void_p, c_void_p]),
    "ser_dec_embed_v": (c_int, [c_void_p, c_void_p]),
    "ser_dec_attn_v": (c_int, [c_void_p, c_void_p]),
    "ser_dec_select_v": (c_int, [c_void_p, c_void_p]),
    "ser_prosody_mel_v": (c_int, [c_void_p, c_void_p]),
    "ser_fvq_v": (c_int, [c_void_p, c_void_p]),
    "ser_act_rows_v": (c_int, [c_void_p, c_void_p]),
    "ser_codec_unit_v": (c_int, [c_void_p, c_void_p]),
    "ser_codec_conv_v": (c_int, [c_void_p, c_void_p]),
    "ser_snake_v": (c_int, [c_void_p, c_void_p]),
    "ser_fbank_v": (c_int, [c_void_p, c_void_p]),
    "ser_relkey_table_v": (c_int, [c_void_p, c_void_p]),
    "ser_attention_rk_v": (c_int, [c_void_p, c_void_p]),
    "ser_conformer_conv_v": (c_int, [c_void_p, c_void_p]),
    "ser_swish_rows_v": (c_int, [c_void_p, c_void_p]),
    "ser_rope_rows_v": (c_int, [c_void_p, c_void_p]),
    "ser_conformer_conv_bn_v": (c_int, [c_void_p, c_void_p]),
    "ser_relpos_bias_v": (c_int, [c_void_p, c_void_p]),
    "ser_attention_rb_v": (c_int, [c_void_p, c_void_p]),
    "ser_dec_select_ts_v": (c_int, [c_void_p, c_void_p]),
    "ser_logmel_long_v": (c_int, [c_void_p, c_void_p]),
    "ser_mel_window_v": (c_int, [c_void_p, c_void_p]),
    "ser_dec_select_score_v": (c_int, [c_void_p, c_void_p]),
    "ser_pack_f16m": (c_int, [c_void_p, c_i64, c_int, c_int, c_void_p, c_i64, c_i64, c_void_p, c_i64, c_int, c_void_p, c_void_p]),
    "ser_wavlm_bias_table": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "ser_wavlm_gate": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                               c_int, c_void_p]),
    "ser_attention": (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_int,
                              c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "ser_attention_v": (c_int, [c_void_p, c_void_p]),
    "ser_embed_ln": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                             c_i64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ser_embed_ln_flagged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                     c_i64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ser_logmel_init": (c_int, [c_void_p, c_int, c_void_p]),
    "ser_logmel_whisper": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ser_pack_act": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_i64, c_int, c_void_p]),
    "ser_mean4": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p]),
    "ser_split_bf16": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_i64, c_void_p]),
    "ser_embed_ln_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_i64,
                                    c_int, c_int, c_int, c_int, c_void_p]),
    "ser_embed_ln_masked_flagged": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_i64,
                                            c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ser_deberta_attention": (c_int, [c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_void_p, c_void_p, c_i64, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "ser_pack_rows": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_i64, c_int, c_void_p]),
    "ser_pack_rows_flagged": (c_int, [c_void_p, c_i64, c_int, c_int, c_int, c_int, c_void_p, c_i64, c_i64, c_int, c_void_p, c_void_p]),
    "ser_zero_padded_rows": (c_int, [c_void_p, c_i64, c_void_p, c_i64, c_i64, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ser_deberta_bias": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_int, c_int, c_int,
                                 c_float, c_void_p]),
    "ser_run": (c_int, [c_void_p, C.c_int32, c_void_p, c_void_p]),
    "ser_ragged_index": (c_int, [c_void_p, c_void_p, c_int, c_i64, c_i64, c_i64, c_void_p, c_i64, c_void_p]),
    "ser_workspace_bytes": (C.c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "ser_wav_read_f32": (c_i64, [C.c_char_p, c_void_p, c_i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ser_pt_write_f32": (c_int, [C.c_char_p, c_void_p, c_i64, c_i64]),
    "ser_pt_write_f32_vec": (c_int, [C.c_char_p, c_void_p, c_i64]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


class SerHipError(RuntimeError):
    pass


def _load():
    if not os.path.isfile(LIB_PATH):
        raise SerHipError(
            f"{LIB_PATH} is missing: build it with `make -C interspeech_ser_amd/csrc` "
            "(or python -c 'import __graft_entry__ as g; g.build()').  There is no fallback backend.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    got = lib.ser_version()
    if got != ABI_VERSION:
        raise SerHipError(f"libserhip ABI version {got} != expected {ABI_VERSION}")
    return lib


lib = _load()


def check(rc: int, what: str = "") -> None:
    """Turn a non-zero launcher return into a Python exception; the drivers'
    per-utterance try/except then logs and skips (preprocess_speech.py:46,72-73)."""
    if rc != 0:
        msg = lib.ser_last_error()
        raise SerHipError(f"{what or 'libserhip'} failed (rc={rc}): {msg.decode() if msg else ''}")
