// C-ABI plumbing of libserhip: launch check, workspace sizing, command lists (version + error text: hosterr.hip).
#include "ser_common.h"
#include <stdarg.h>
#include <stdio.h>

int ser_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        return ser_fail((int)e, "%s: launch failed: %s", what, hipGetErrorString(e));
    }
    return 0;
}


extern "C" size_t ser_workspace_bytes(int op, int B, int T, int D, int H, int mode) {
    (void)T; (void)D; (void)H; (void)mode;
    switch (op) {
        case SER_WS_LOGMEL:
            // per-block partial maxima [B][256] floats + the fp64 twiddle table [400][208] x (cos, -sin) + the Hann window (ser_logmel_init)
            return (size_t)(B > 0 ? B : 1) * 1024 + (size_t)400 * 208 * 16 + 400 * 4;
        case SER_WS_GN_STATS:
            return (size_t)(B > 0 ? B : 1) * 32 * 65 * sizeof(double);     // [B][32 chunks][65 frame moments] (rowops.hip K2g)
        case SER_WS_WAVE_FRAMES:
            return (size_t)(B > 0 ? B : 1) * 64 * 2 * sizeof(double);      // [B][64] partial (sum, sum^2)
        default:
            return 0;
    }
}


// ---- command lists (see ser_hip.h): one foreign call per batch instead of one per kernel ------------------------
extern "C" int ser_run(const ser_cmd* cmds, int32_t n, int32_t* failed_at, void* stream) {
    if (!cmds || n < 0) return ser_fail(-1, "ser_run: bad command list");
    for (int32_t i = 0; i < n; ++i) {
        const ser_cmd& c = cmds[i];
        int rc;
        switch (c.op) {
            case SER_OP_GEMM:
                rc = ser_gemm(&c.u.gemm, stream);
                break;
            case SER_OP_ATTENTION: {
                rc = ser_attention_v(&c.u.attention, stream);
                break;
            }
            case SER_OP_LAYERNORM: {
                rc = ser_layernorm_v(&c.u.layernorm, stream);
                break;
            }
            case SER_OP_WAVE_FRAMES: {
                rc = ser_wave_frames_v(&c.u.wave_frames, stream);
                break;
            }
            case SER_OP_ROW_CENTER: {
                rc = ser_row_center_v(&c.u.row_center, stream);
                break;
            }
            case SER_OP_LOGMEL: {
                const ser_logmel_args& a = c.u.logmel;
                rc = ser_logmel_whisper(a.wav, a.sample_offs, a.B, a.mel, a.n_mels, a.out, a.work, stream);
                break;
            }
            case SER_OP_PACK_ACT: {
                rc = ser_pack_act_v(&c.u.pack_act, stream);
                break;
            }
            case SER_OP_GN_STATS: {
                rc = ser_gn_stats_v(&c.u.gn_stats, stream);
                break;
            }
            case SER_OP_POS_LN: {
                rc = ser_pos_ln_v(&c.u.pos_ln, stream);
                break;
            }
            case SER_OP_DEC_EMBED: {
                rc = ser_dec_embed_v(&c.u.dec_embed, stream);
                break;
            }
            case SER_OP_DEC_ATTN: {
                rc = ser_dec_attn_v(&c.u.dec_attn, stream);
                break;
            }
            case SER_OP_DEC_SELECT: {
                rc = ser_dec_select_v(&c.u.dec_select, stream);
                break;
            }
            case SER_OP_PROSODY_MEL: {
                rc = ser_prosody_mel_v(&c.u.prosody_mel, stream);
                break;
            }
            case SER_OP_FVQ: {
                rc = ser_fvq_v(&c.u.fvq, stream);
                break;
            }
            case SER_OP_ACT_ROWS: {
                rc = ser_act_rows_v(&c.u.act_rows, stream);
                break;
            }
            case SER_OP_CODEC_UNIT: {
                rc = ser_codec_unit_v(&c.u.codec_unit, stream);
                break;
            }
            case SER_OP_CODEC_CONV: {
                rc = ser_codec_conv_v(&c.u.codec_conv, stream);
                break;
            }
            case SER_OP_SNAKE: {
                rc = ser_snake_v(&c.u.snake, stream);
                break;
            }
            case SER_OP_FBANK: {
                rc = ser_fbank_v(&c.u.fbank, stream);
                break;
            }
            case SER_OP_RELKEY_TABLE: {
                rc = ser_relkey_table_v(&c.u.relkey_table, stream);
                break;
            }
            case SER_OP_ATTENTION_RK: {
                rc = ser_attention_rk_v(&c.u.attention_rk, stream);
                break;
            }
            case SER_OP_CONFORMER_CONV: {
                rc = ser_conformer_conv_v(&c.u.conformer_conv, stream);
                break;
            }
            case SER_OP_SWISH_ROWS: {
                rc = ser_swish_rows_v(&c.u.swish_rows, stream);
                break;
            }
            case SER_OP_DEC_KEEP_Q: {
                rc = ser_dec_keep_q_v(&c.u.dec_keep_q, stream);
                break;
            }
            case SER_OP_DEC_ATTN_BEAM: {
                rc = ser_dec_attn_beam_v(&c.u.dec_attn_beam, stream);
                break;
            }
            case SER_OP_BEAM_SELECT: {
                rc = ser_beam_select_v(&c.u.beam_select, stream);
                break;
            }
            case SER_OP_ROPE_ROWS: {
                rc = ser_rope_rows_v(&c.u.rope_rows, stream);
                break;
            }
            case SER_OP_CONFORMER_CONV_BN: {
                rc = ser_conformer_conv_bn_v(&c.u.conformer_conv_bn, stream);
                break;
            }
            case SER_OP_RELPOS_BIAS: {
                rc = ser_relpos_bias_v(&c.u.relpos_bias, stream);
                break;
            }
            case SER_OP_ATTENTION_RB: {
                rc = ser_attention_rb_v(&c.u.attention_rb, stream);
                break;
            }
            case SER_OP_DEC_SELECT_TS: {
                rc = ser_dec_select_ts_v(&c.u.dec_select_ts, stream);
                break;
            }
            case SER_OP_LOGMEL_LONG: {
                rc = ser_logmel_long_v(&c.u.logmel_long, stream);
                break;
            }
            case SER_OP_MEL_WINDOW: {
                rc = ser_mel_window_v(&c.u.mel_window, stream);
                break;
            }
            case SER_OP_DEC_SELECT_SCORE: {
                rc = ser_dec_select_score_v(&c.u.dec_select_score, stream);
                break;
            }
            default:
                rc = ser_fail(-2, "ser_run: command %d has unknown op %d", i, c.op);
        }
        if (rc != 0) {
            if (failed_at) *failed_at = i;
            return rc;
        }
    }
    return 0;
}
