/* ser_hip.h -- C ABI of libserhip.so: hand-written gfx950 (MI355X / CDNA4) kernels
 * for the SSL embedding-extraction hot path of AI-Unicamp/interspeech_ser.
 *
 * The reference has no FFI of its own on this path: preprocessing/
 * preprocess_speech.py:49-50,66-67 calls  model(**inputs, output_hidden_states=True)
 * and preprocessing/preprocess_whisper.py:57,71 calls model.encoder(input_features,
 * output_hidden_states=True); every device op below replaces one implicit
 * cuDNN/cuBLAS/ATen launch inside those two calls (SURVEY.md 2.3 rows K1..K15,
 * cited per entry point).  INTEGRATION.md shows the ctypes binding a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C, no C++/torch types; every pointer is a DEVICE pointer unless named host_*;
 *   - the caller owns all memory; launchers never allocate, free or synchronise;
 *   - every launcher enqueues on `stream` (a hipStream_t passed as void*) and returns
 *     0 on success, <0 for an argument/shape error, >0 = hipError_t of the launch;
 *     ser_last_error() gives the thread-local message of the last non-zero return;
 *   - launchers are re-entrant (the reference drives its model from 4 Python threads,
 *     preprocess_speech.py:120-122).
 *
 * Data layout (DESIGN.md "HBM layout")
 *   - utterances are PACKED, never padded: a ragged batch is one [rows, C] matrix
 *     whose utterance b owns rows frame_offs[b] .. frame_offs[b+1]-1;
 *   - "act" tensors feed matrix-core GEMMs: bf16, row-major, 1 plane (SER_MODE_BF16) or
 *     2 planes hi/lo with x ~= hi + lo (SER_MODE_FP32X, the 3-product split that gives
 *     fp32-grade results on the bf16 MFMA pipe), 1 plane of fp16 (SER_MODE_FP16) or 2 planes of fp16 (SER_MODE_FP16X);
 *     plane p lives at base + p*plane_stride;
 *   - the residual stream / hidden states are fp32 row-major [rows, D].
 */
#ifndef SER_HIP_H
#define SER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SER_ABI_VERSION 18

#define SER_MODE_BF16  1   /* act tensors have 1 plane; GEMMs do 1 bf16 MFMA product   */
#define SER_MODE_FP32X 2   /* act tensors have 2 planes; GEMMs do hi*hi + lo*hi + hi*lo */
#define SER_MODE_FP16  3   /* act tensors have 1 plane of IEEE fp16 (11 significand bits, saturated at +-65504);
                            * GEMMs do 1 f16 MFMA product -- same rate as bf16, 8x finer operand rounding.  The host
                            * runs the conv stem in FP32X and the encoder layers in FP16 ("f16" numerics mode) */
#define SER_MODE_FP16X 4   /* act tensors have 2 planes of IEEE fp16, x ~= hi + lo (22 significand bits; hi is exactly the FP16 copy, so
                            * a single-product FP16 launch may read plane 0 of an FP16X tensor); GEMMs and ser_attention do
                            * hi*hi + lo*hi + hi*lo on the f16 MFMA.  The host's "f16a" numerics mode runs the whole ATTENTION BLOCK of
                            * every encoder layer in it (packed projection, attention, output projection) and the feed-forward pair in
                            * FP16; "f16q" only the LOGIT path -- the q / k (+ WavLM gate) columns of the packed projection and, through
                            * SER_MODE_FP16Q, S = K Q^T: a softmax weight moves by (logit error) * ln 2, so the attention block is where
                            * single-product rounding is amplified (reference arithmetic is fp32: preprocess_speech.py:50,66) */
#define SER_MODE_FP16Q 5   /* ser_attention only: q and k are FP16X column blocks (3-product S = K Q^T), v is read from plane 0 and
                            * P V runs single fp16 products; the output is a single-plane FP16 tensor */

#define SER_MODE_FP16M 6   /* round 5, the "f16m" numerics mode: fp16 main product + block-scaled 8-bit cross terms on gfx950's
                            * v_mfma_scale_f32_16x16x128_f8f6f4 -- x W^T ~= x_hi w_hi + x_lo w_8 + x_8 w_lo, i.e. 1 + 1/2 + 1/2 = 2 fp16 product-
                            * equivalents per algorithmic FLOP instead of FP16X's 3 (the scaled e4m3 instruction runs at twice the fp16 rate).
                            * An FP16M tensor has
                            *   plane 0 (at base):                fp16 hi = fp16(x), [rows][ld], exactly the FP16 copy;
                            *   plane 1 (at base + plane_stride): the CROSS-TERM plane, same pitch in bytes: for every row and every 64-column tile t,
                            *       the 128 bytes at byte offset 2 * (row * ld + 64 t) hold [P: 64 e4m3 bytes, columns 64t .. 64t+63][Q: 64 e4m3 bytes];
                            *       activations: P = x - hi (the fp16 rounding residual), Q = x;   weights: P = w, Q = w - fp16(w);
                            *   scales (their own pointer): uint32 [ld / 64][scale_ld], word (t, row) = four E8M0 codes (value 2^(c - 127)), one per
                            *       32 consecutive elements: [P cols 0-31, P cols 32-63, Q cols 0-31, Q cols 32-63] of tile t -- the OCP MX block format,
                            *       the smallest power of two that brings the block's largest magnitude to <= 448.
                            * ser_gemm accumulates, per 64-deep K tile, two fp16 MFMA k-steps (hi x hi) and ONE scaled e4m3 MFMA whose 128-long K is
                            * [P | Q] of both operands: P_a P_w + Q_a Q_w = x_lo w_8 + x_8 w_lo.  The cross terms carry 2^-11 of the result, so their
                            * 4-bit significands leave an operand error of ~2^-15 (oracle/numerics_whatif_f16m.py).  Range: fp16's (saturation at
                            * +-65504, reported through range_flag).  Reference arithmetic is fp32 end to end (preprocess_speech.py:50,66). */

#define SER_ACT_NONE 0
#define SER_ACT_GELU 1     /* exact erf GELU (ACT2FN["gelu"]) */

int         ser_version(void);
const char* ser_last_error(void);

/* K1  zero_mean_unit_var_norm (HF feature_extraction_wav2vec2.py:77-97; call site
 * preprocess_speech.py:48).  wav/out: packed fp32 samples; sample_offs[B+1] (device). */
int ser_wave_norm(const float* wav, const int64_t* sample_offs, int B, float* out, void* stream);

/* K1 + framing for the matrix-core form of conv layer 0: normalise each utterance (as ser_wave_norm)
 * and write frame t as one act row [x_n[stride*t .. stride*t+k-1], 0, ...] of 64 elements, so that
 * Conv1d(1,C,k,stride)+LayerNorm+GELU (HF modeling_wavlm.py:696-720) is ser_gemm with K = 64 and the
 * LayerNorm epilogue.  out: act [total_rows, 64]; work: ser_workspace_bytes(SER_WS_WAVE_FRAMES, B, ...). */
int ser_wave_frames(const float* wav, const int64_t* sample_offs, const int32_t* frame_offs, int B,
                    int k, int stride, void* out, int64_t out_plane_stride, int mode, void* work,
                    int total_rows, void* stream);

/* K2  conv layer 0: Conv1d(1,C,k,stride) [+bias] -> LayerNorm(C) -> GELU
 * (HF modeling_wavlm.py:696-720).  One output row per frame.
 * w: [C,k] fp32; bias may be NULL; out: act [rows,C]. C multiple of 64, C <= 1024, k <= 16. */
int ser_conv0_ln_gelu(const float* wav_norm, const int64_t* sample_offs, const int32_t* frame_offs,
                      int B, const float* w, const float* bias, const float* ln_g, const float* ln_b,
                      void* out, int64_t out_plane_stride, int mode,
                      int C, int k, int stride, int total_rows, void* stream);

/* K3/K4/K5/K7/K10/K11/K12/K14  one matrix-core GEMM with an implicit-convolution
 * row map and a fused epilogue:   C[m,n] = sum_k A(m,k) * W[n,k]
 *   A(m,k)  = A[ a_row(m)*8 + (k / kc)*ldj + (k % kc) ]   (kc == 0: plain row-major, lda)
 *   a_row(m)= a_rowoff ? a_rowoff[m] : m*lda/8             (units of 8 elements = 16 bytes)
 * so that a strided Conv1d over a channels-last [frames, C] matrix (HF modeling_wavlm.py:
 * 696-720, modeling_whisper.py:618-619), the grouped positional conv (:48-90) and every
 * nn.Linear (:133-136, :288-294) are the same kernel.  Epilogue order:
 *   v = acc + bias[n];  v = act(v);  v += residual[(m % res_row_mod or m)*ldr + n];
 *   out_f32[m*ldo_f32 + n] = v;   out_act[out_row(m)*ldo_act + n] = split(v)
 * With ln_gamma != NULL the epilogue is  v = act(LayerNorm_row(acc + bias)) instead.
 * Requirements: K % 64 == 0, kc % 64 == 0, N % 8 == 0, all row starts 16-byte aligned. */
typedef struct ser_gemm_args {
    const void*    A;              /* act (bf16 planes) */
    int64_t        a_plane_stride; /* elements between hi and lo plane (FP32X) */
    const int32_t* a_rowoff;       /* [M] or NULL */
    int64_t        lda;            /* elements, used when a_rowoff == NULL */
    int32_t        kc;             /* K-chunk length of the conv map, 0 = none */
    int64_t        ldj;            /* element step between K-chunks (conv tap stride) */
    const void*    W;              /* bf16 [groups][N][K] (+ lo plane) */
    int64_t        w_plane_stride;
    int32_t        M, N, K;
    int32_t        groups;         /* blockIdx.y; 1 for dense */
    int64_t        a_group_stride; /* elements added to A per group (column offset) */
    int64_t        w_group_stride; /* elements per group in W */
    int32_t        c_group_stride; /* output columns per group */
    int32_t        mode;           /* SER_MODE_* */
    const float*   bias;           /* [groups*N] or NULL */
    int32_t        act;            /* SER_ACT_* */
    const float*   residual;       /* fp32 or NULL */
    int64_t        ldr;
    int32_t        res_row_mod;    /* 0: row m; >0: row m % res_row_mod (Whisper positions) */
    float*         out_f32;        /* may be NULL */
    int64_t        ldo_f32;
    void*          out_act;        /* may be NULL */
    int64_t        ldo_act;
    int64_t        out_plane_stride;
    const int32_t* out_rowmap;     /* [M] row index in out_act, or NULL (identity) */
    /* optional fused LayerNorm over the full output row (conv stack: Conv1d -> LayerNorm(C) -> GELU,
     * HF modeling_wavlm.py:712-719): v = LN(acc + bias) * gamma + beta, then act.  Needs N <= 512,
     * groups == 1, no residual. */
    const float*   ln_gamma;       /* [N] or NULL */
    const float*   ln_beta;        /* [N] */
    float          ln_eps;
    int32_t        tile_cfg;       /* 0 = auto; 1 = 128x128, 2 = 256x128, 3 = 256x256 block tile -- a request the mode families treat
                                    * differently.  BF16 / FP16: honoured, unless ln_gamma is set (the row count alone picks the LayerNorm
                                    * tile).  FP16M: 2 and 3 are honoured; 1 only switches the automatic choice off, which leaves 128x128.
                                    * FP32X / FP16X: ignored, the automatic choice stands.  Values outside 0..3 are refused (-13). */
    /* DEFERRED LayerNorm of the A operand (encoder layers: LN -> Linear, HF modeling_wavlm.py:357-358,
     * 366): the LayerNorm kernel and its HBM round trip disappear.  With W' = W * gamma (folded at load),
     *   LN(x) W^T + b = rstd_m * (x W'^T - mu_m * colsum(W')_n) + (beta W^T + b)_n
     * A holds the raw (un-normalised) rows; mu/rstd come from per-row partial sums (sum, sum of squares
     * per 64-column group) that the PRODUCER of x wrote through stat_out.  bias must hold beta W^T + b. */
    const float*   ln_stats_in;    /* [M][ln_groups][2] or NULL */
    int32_t        ln_groups;      /* even */
    const float*   ln_colsum;      /* [N] */
    float*         stat_out;       /* [M][stat_groups][2] row partials of the values written, or NULL */
    int32_t        stat_groups;    /* >= N/64 */
    int32_t        f32_col_begin;  /* out_f32 receives only columns >= f32_col_begin (stored at n - f32_col_begin) */
    /* columns n < col_scale_end are multiplied by col_scale after bias (before act): the packed QKV projection
     * scales q by dh^-0.5 (what HF does before the product, modeling_whisper.py:309) times log2(e), so the
     * attention kernel's softmax runs in the exp2 domain with no per-score multiply. */
    float          col_scale;
    int32_t        col_scale_end;  /* multiple of 4; 0 = no scaling */
    /* SHIFTED operand copy for the deferred LayerNorm.  Real checkpoints carry offsets in the residual stream (rows
     * whose mean is many standard deviations); rounding such a row to bf16 and then forming acc - mu*colsum loses the
     * signal.  With shift_out != NULL a PRODUCER launch takes, per row,
     *   c[m] = shift_const + (shift_in ? shift_in[m] : 0)
     * -- shift_in = the absolute row mean of its RESIDUAL input, shift_const = a load-time constant (mean of the bias) --
     * stores it in shift_out[m] and writes out_act and stat_out for v - c[m] (out_f32 keeps v).  LayerNorm is shift
     * invariant, so the CONSUMER only has to report the absolute mean for the next producer down the residual stream:
     * mean_out[m] = mu_m + (ln_shift ? ln_shift[m] : 0), where mu_m is the mean it derives from ln_stats_in (relative
     * to the shift ln_shift its A rows were stored with). */
    const float*   shift_in;       /* [M] absolute row mean of the residual rows, or NULL (0) */
    float*         shift_out;      /* [M] or NULL (no shifting) */
    float          shift_const;
    int32_t        out_mode;       /* format of out_act: 0 = mode; SER_MODE_FP16 with mode == SER_MODE_FP32X converts (one plane of
                                    * fp16 written from a 3-product GEMM: the stem -> layers boundary of the host's "f16" mode);
                                    * SER_MODE_FP16X with mode == SER_MODE_FP16 writes hi + lo fp16 planes from a single-product
                                    * GEMM (FC2 -> the next layer's packed projection in the "f16q" / "f16a" modes); SER_MODE_FP16 with
                                    * mode == SER_MODE_FP16X writes one plane from a 3-product GEMM (output projection -> FC1, "f16a") */
    const float*   ln_shift;       /* [M] shift of the A rows / their partials (consumer), or NULL */
    float*         mean_out;       /* [M] absolute row mean of the A rows (consumer), or NULL */
    float*         lnstat_out;     /* [M][2] (row mean relative to ln_shift, 1/sqrt(var + eps)) the consumer derived from ln_stats_in, or
                                    * NULL: what ser_attention's in-kernel WavLM gate (ser_attention_args.gate_x) applies to the same rows */
    /* SER_MODE_FP16M operands (ABI 13): block scales of A (row index m; needs a_rowoff == NULL, kc == 0, groups == 1) and of W (row index n),
     * and -- with out_mode == SER_MODE_FP16M -- of the out_act copy (row index out_row(m), tile index (output column) / 64; the first output
     * column of the launch must be a multiple of 64).  *_scale_ld = words between consecutive 64-column tiles. */
    const uint32_t* a_scale;  int64_t a_scale_ld;
    const uint32_t* w_scale;  int64_t w_scale_ld;
    uint32_t*       out_scale; int64_t out_scale_ld;
    /* fp16 range guard (ABI 13): when not NULL, the launch ORs into *range_flag bit 0 if any value it rounds to an fp16 operand plane
     * (out_act in the FP16 / FP16X / FP16M formats) exceeds 65504 in magnitude (or is a NaN or Inf) BEFORE the saturating conversion, bit 1 if
     * one exceeds half that (bit 0 never comes alone).  Only values the launch stores count, not the tail columns of a tile past N -- the host reads the word back with the batch's features and fails that batch's files instead of writing
     * clipped ones (preprocess_speech.py:46,72-73: a bad file is a printed failure, never silent garbage).  ser_layernorm_v,
     * ser_row_center_v, ser_wave_frames_v, ser_pack_act_v, ser_pos_ln_v and ser_pack_f16m take the same word. */
    uint32_t*       range_flag;
    /* GroupNorm-over-time stem (ABI 15; conv layer 0 of the *-base checkpoints, HF WavLMGroupNormConvLayer): with gn_scale != NULL the
     * epilogue applies, after the bias and before act,  v = v * gn_scale[u][n] + gn_shift[u][n]  where u is the utterance of row m
     * (gn_row_offs[u] <= m < gn_row_offs[u + 1], B + 1 entries): the per-(utterance, channel) affine ser_gn_stats_v computes.  A block
     * tile may straddle utterances.  Needs groups == 1, no LayerNorm epilogue, no deferred LayerNorm.  NULL (zero) = no affine. */
    const float*    gn_scale;       /* [gn_B][gn_ld] */
    const float*    gn_shift;       /* [gn_B][gn_ld] */
    const int32_t*  gn_row_offs;    /* [gn_B + 1] */
    int32_t         gn_B, gn_ld;
} ser_gemm_args;
int ser_gemm(const ser_gemm_args* args, void* stream);

/* K6  LayerNorm over the last dim (+ optional GELU), fp32 in
 * (HF modeling_wavlm.py:357,366,513; conv-stack LN :716-718).  Either output may be NULL. */
int ser_layernorm(const float* x, int64_t ldx, const float* g, const float* b, float eps, int gelu,
                  float* out_f32, int64_t ldo_f32, void* out_act, int64_t ldo_act, int64_t out_plane_stride,
                  int mode, int rows, int D, void* stream);

/* Centred operand copy of hidden_states[0] for the deferred LayerNorm of encoder layer 0 (the LayerNorm itself is
 * HF modeling_wavlm.py:357): out_act = split(x - mean_row), stats[m][0] = (sum, sum of squares) of the centred row
 * (remaining slots zero), shift[m] = mean_row.  See ser_gemm_args.shift_out. */
int ser_row_center(const float* x, int64_t ldx, void* out_act, int64_t ldo_act, int64_t out_plane_stride,
                   float* stats /*[rows][stat_groups][2]*/, int stat_groups, float* shift /*[rows]*/,
                   int mode, int rows, int D, void* stream);

/* K8a WavLM relative-position bias as a [H, 2*T-1] table: column (key-query)+(T-1)
 * (compute_bias + _relative_positions_bucket, HF modeling_wavlm.py:243-271). */
int ser_wavlm_bias_table(const float* rel_attn_embed /*[num_buckets,H]*/, float* table /*[H,2T-1]*/,
                         int T, int H, int num_buckets, int max_distance, void* stream);

/* K8b WavLM GRU gate (HF modeling_wavlm.py:167-180): gate[row,h] from the layer-normed act x. */
int ser_wavlm_gate(const void* x_ln, int64_t ldx, int64_t plane_stride, int mode,
                   const float* w8 /*[8,dh]*/, const float* b8 /*[8]*/, const float* gru_const /*[H]*/,
                   float* gate /*[rows,H]*/, int rows, int H, int dh, void* stream);

/* K9  fused attention over a packed ragged batch:
 *   out[q,:] = softmax_k( q.k * scale + gate[q,h] * table[h, k-q+table_T-1] ) v
 * q/k/v are column blocks of one act matrix [rows, ld] (packed QKV projection output);
 * utterance b owns rows frame_offs[b] .. frame_offs[b+1]-1 and attends only to itself
 * (batch-of-one semantics of preprocess_speech.py:76-81, so no key-padding mask exists).
 * WavLM: HF modeling_wavlm.py:188-241; wav2vec2/HuBERT: modeling_wav2vec2.py:438-548;
 * Whisper: modeling_whisper.py:284-357 (pass scale = dh^-0.5, identical in exact arithmetic).
 * scale <= 0 means q is PRE-SCALED by dh^-0.5 * log2(e) (ser_gemm col_scale): scores are used as exp2 exponents.
 * dh in {64, 80, 96, 120, 128}; table/gate NULL for plain attention.
 * The WavLM gate is given either as gate[rows,H] (from ser_wavlm_gate) or, fused, as its two
 * pre-activations per head stored in columns gate_col + 2h, +1 of the qkv matrix (extra output
 * columns of the packed projection GEMM) together with gru_const[H]. */
int ser_attention(const void* qkv, int64_t ld, int64_t plane_stride, int q_col, int k_col, int v_col,
                  const int32_t* frame_offs /*[B+1] device*/, int B, int max_frames,
                  const float* table, int table_T, const float* gate,
                  void* out, int64_t ldo, int64_t out_plane_stride,
                  int H, int dh, float scale, int mode,
                  int gate_col, const float* gru_const /*[H]*/,
                  const int32_t* key_lens /*[B] or NULL: keys >= key_lens[b] are padding (RoBERTa attention_mask)*/,
                  const float* bias2d /*[B][H][max_frames][bias2d_ld] fp32 dense additive bias in the exp2 domain, or NULL
                                        (DeBERTa, from ser_deberta_bias): uniform-length batches, q pre-scaled, dh <= 64, modes BF16 / FP32X / FP16X; padded
                                        query rows (q >= key_lens[b]) then come out as the uniform average of all value rows*/,
                  int64_t bias2d_ld,
                  void* stream);

/* next row 8f-1 (text side): RoBERTa embeddings word[id] + position[cumsum(non-pad)] + token_type[0] -> LayerNorm
 * (HF modeling_roberta.py:56-155; call site preprocessing/preprocess_roberta.py:47-57).  ids: [B,T] int32.
 * mode (here and in ser_embed_ln_masked / ser_pack_rows / ser_zero_padded_rows): the format of the operand copy, BF16 / FP32X / FP16X.
 * The *_flagged forms (here, of ser_embed_ln_masked and of ser_pack_rows; ABI 17) take range_flag just before stream: the fp16 range
 * guard of the values stored to out_act in FP16X (see ser_gemm_args.range_flag), may be NULL.  The unsuffixed forms keep their
 * arguments and run the same launch with range_flag = NULL. */
int ser_embed_ln(const int32_t* ids, const float* word_emb, const float* pos_emb, const float* type_emb,
                 const float* ln_g, const float* ln_b, float eps, float* out_f32, void* out_act,
                 int64_t out_plane_stride, int mode, int B, int T, int D, int pad_id, void* stream);
int ser_embed_ln_flagged(const int32_t* ids, const float* word_emb, const float* pos_emb, const float* type_emb,
                         const float* ln_g, const float* ln_b, float eps, float* out_f32, void* out_act,
                         int64_t out_plane_stride, int mode, int B, int T, int D, int pad_id, uint32_t* range_flag, void* stream);

/* K13 Whisper log-mel front end (HF feature_extraction_whisper.py:135-169): packed fp32
 * samples -> [B, n_mels, 3000] fp32 (zero-pad/truncate to 480000, reflect pad, Hann,
 * 400-pt DFT power, mel, log10, per-utterance max-8 floor, (x+4)/4).
 * mel: [201, n_mels] fp32.  work: ser_workspace_bytes(SER_WS_LOGMEL, B, ...) bytes, prepared ONCE per buffer by
 * ser_logmel_init (the DFT twiddle table lives there; the per-utterance maxima are per-block partials reduced by the
 * finishing pass: no atomics, nothing to reset between calls). */
int ser_logmel_init(void* work, int B, void* stream);
int ser_logmel_whisper(const float* wav, const int64_t* sample_offs, int B, const float* mel, int n_mels,
                       float* out, void* work, void* stream);

/* fp32 [rows, C] -> act (bf16 / hi+lo planes), optional transpose of a [B, C, T] input
 * into channels-last rows with `halo` zero rows before and after each utterance
 * (feeds the Whisper stem convs, HF modeling_whisper.py:618-619). */
int ser_pack_act(const float* x, int B, int C, int T, int halo, void* out, int64_t ldo,
                 int64_t out_plane_stride, int mode, void* stream);

/* DeBERTa-v2/v3 variant of the text side (preprocessing/preprocess_deroberta.py:106-107 builds it with AutoModel).
 * ser_embed_ln_masked: LayerNorm(word_emb[id]) with rows t >= key_lens[b] zeroed (HF modeling_deberta_v2.py
 * DebertaV2Embeddings in the v3 configuration: no absolute positions, no token types, embeddings * mask).
 * ser_deberta_attention: softmax((Qc Kc^T + c2p + p2c) / sqrt(3 dh)) V per (sequence, head)
 * (DisentangledSelfAttention.forward / disentangled_attention_bias).  c2p, p2c: [B*T, ldp] fp32, head h in columns
 * h*Nr .. h*Nr+Nr-1 = content queries / keys times the position keys / queries (shared q/k projections of the
 * LayerNorm-ed relative embeddings) restricted to the Nr relative-position rows a T-token sequence reaches;
 * c2p_col / p2c_col: [2T-1] int32, column inside that window for signed distance d at index d + T - 1
 * (c2p reads c2p[q][c2p_col[q-k]], p2c reads p2c[k][p2c_col[k-q]]; the log-bucket map is built by the host).
 * A (query, key) pair counts only if both are real tokens (t < key_lens[b]); a padded query row comes out as the
 * uniform average of all T value rows, as HF's masked_fill(finfo.min) + softmax gives.  T <= 128, dh <= 64.
 * (ser_deberta_attention is the one-thread-per-query statement of the op, kept as the kernel-level reference; the encoder
 * runs ser_deberta_bias + ser_attention(bias2d), which has no 128-token limit.) */
int ser_embed_ln_masked(const int32_t* ids, const float* word_emb, const float* ln_g, const float* ln_b, float eps,
                        const int32_t* key_lens, float* out_f32, void* out_act, int64_t out_plane_stride,
                        int mode, int B, int T, int D, void* stream);
int ser_embed_ln_masked_flagged(const int32_t* ids, const float* word_emb, const float* ln_g, const float* ln_b, float eps,
                                const int32_t* key_lens, float* out_f32, void* out_act, int64_t out_plane_stride,
                                int mode, int B, int T, int D, uint32_t* range_flag, void* stream);
/* ConvLayer of deberta-v2-xlarge / xxlarge (HF modeling_deberta_v2.py ConvLayer; the checkpoint the reference's README runs
 * preprocess_deroberta.py with, README.md:66): Conv1d(D, D, 3) over the token axis of the embedding output, activation, + layer
 * 0's output, LayerNorm, padded rows zero.  The conv is ser_gemm's implicit-conv map over the halo'd copy ser_pack_rows makes
 * (row b*(T+2*halo) + halo + t of `out` = split(x[b*T + t]); the halo rows are the caller's zeros); ser_zero_padded_rows zeroes
 * rows t >= key_lens[b] of an fp32 matrix and / or its act copy.  ser_embed_ln_masked's padded rows store zeros and do not count for
 * the range_flag of its _flagged form; ser_zero_padded_rows stores only zeros and has no such form. */
int ser_pack_rows(const float* x, int64_t ldx, int B, int T, int D, int halo, void* out, int64_t ldo, int64_t out_plane_stride,
                  int mode, void* stream);
int ser_pack_rows_flagged(const float* x, int64_t ldx, int B, int T, int D, int halo, void* out, int64_t ldo, int64_t out_plane_stride,
                          int mode, uint32_t* range_flag, void* stream);
int ser_zero_padded_rows(float* x, int64_t ldx, void* act, int64_t lda, int64_t plane_stride, int mode, const int32_t* key_lens,
                         int B, int T, int D, void* stream);

/* Dense disentangled-attention bias for ser_attention's bias2d argument (the matrix-core path the DeBERTa encoder uses):
 *   out[b][h][q][k] = c2p[q][c2p_col[q-k]] + p2c_scale * p2c[k][p2c_col[k-q]]   for q, k < key_lens[b], else 0;   row pitch ld.
 * c2p is expected from a q that already carries the score scale (ser_gemm col_scale), p2c from the plain k. */
int ser_deberta_bias(const float* c2p, const float* p2c, int64_t ldp, int Nr, const int32_t* c2p_col, const int32_t* p2c_col,
                     const int32_t* key_lens, float* out, int64_t ld, int B, int T, int H, float p2c_scale, void* stream);
int ser_deberta_attention(const void* qkv, int64_t ld, int64_t plane_stride, int q_col, int k_col, int v_col,
                          const float* c2p, const float* p2c, int64_t ldp, int Nr, const int32_t* c2p_col,
                          const int32_t* p2c_col, const int32_t* key_lens, void* out, int64_t ldo,
                          int64_t out_plane_stride, int B, int T, int H, int dh, int mode, void* stream);

/* K15 mean of 4 fp32 states (--use_average y; preprocess_speech.py:52-63). */
int ser_mean4(const float* s0, const float* s1, const float* s2, const float* s3, float* out,
              int64_t n, void* stream);

/* ser_select_rows_v: the device heads' ragged gather.  Utterance b's row t (t < dst_offs[b + 1] - dst_offs[b]) is read from source row
 * src_offs[b] + t and written to packed row dst_offs[b] + t: as the GEMM operand copy out_act (SER_MODE_BF16 / FP32X / FP16X; the planes
 * ser_pack_rows_flagged stores for the same fp32 values) and / or unsplit as out_f32 -- at least one of the two.  n_src == 1: the value of
 * src[0]; n_src == 4: (((s0 + s1) + s2) + s3) / 4, ser_mean4's order.  The sources are fp32 row matrices of one pitch ld_src (>= D, a
 * multiple of 4), 16-byte aligned; src_offs [B] in any order, dst_offs [B + 1] ascending from 0 with at least one row per utterance (int32,
 * device); max_rows = the longest count (it sizes the grid: SER_SELECT_ROWS_TILE rows per block, one grid row per utterance, B <= 65535).
 * In FP16X, range_flag (may be NULL) gets the fp16 range guard's bits over the SELECTED rows only: a source row no utterance selects
 * is never read.  The caller guarantees that every selected row lies inside the sources.  Additive export of ABI 18. */
#define SER_SELECT_ROWS_TILE 8
typedef struct ser_select_rows_args {
    const float* src[4]; int64_t ld_src;
    const int32_t* src_offs; const int32_t* dst_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    int32_t n_src, B, D, max_rows, mode, reserved0;
} ser_select_rows_args;
int ser_select_rows_v(const ser_select_rows_args* args, void* stream);

/* weights: fp32 -> bf16 hi (+ lo) planes, done once at load. */
int ser_split_bf16(const float* x, void* out, int64_t plane_stride, int mode, int64_t n, void* stream);

/* fp32 [rows][ldx] -> a SER_MODE_FP16M tensor (see the mode's comment): hi plane at out, cross-term plane at out + plane_stride (elements),
 * scale words at scales[t * scale_ld + row].  cols % 64 == 0, ldo % 64 == 0.  is_weight selects the plane roles (weights: P = w, Q = w - hi;
 * activations: P = x - hi, Q = x).  Used at load for the weights (HF modeling_wavlm.py:133-136,288-294 Linear weights) and by the kernel tests. */
int ser_pack_f16m(const float* x, int64_t ldx, int rows, int cols, void* out, int64_t ldo, int64_t plane_stride,
                  uint32_t* scales, int64_t scale_ld, int is_weight, uint32_t* range_flag, void* stream);

/* Row-index tables of a packed ragged batch, built on the device (no per-batch host tables to upload):
 *   out[m] = (base[b] + step * (m - row_offs[b])) * mult / div      for row_offs[b] <= m < row_offs[b+1]
 * row_offs: [B+1] int32 first output row of every utterance; base: [B] int64.  This is the implicit-conv row offset
 * table ser_gemm_args.a_rowoff of a strided Conv1d over packed utterances (base = first input row, step = stride,
 * mult = C_in, div = 8), the positional conv's halo map, and every other "utterance b starts here" table that
 * replaces the reference's padded [B, T] indexing (preprocess_speech.py:49 runs B = 1, so it never needs one). */
int ser_ragged_index(const int32_t* row_offs, const int64_t* base, int B, int64_t step, int64_t mult, int64_t div,
                     int32_t* out, int64_t total_rows, void* stream);

/* ---- command lists -----------------------------------------------------------------------------------------------
 * A forward over a packed ragged batch is ~150 launches whose POINTERS are fixed once the host has laid its buffers out
 * and whose only per-batch variables are a handful of row counts.  The host therefore records the launches once as an
 * array of ser_cmd, patches the row counts in place for every batch and replays the array with ONE call: the launching
 * thread leaves the interpreter once per batch instead of once per kernel (the reference pays one Python dispatch per
 * torch op, preprocess_speech.py:49).  Each ser_cmd carries the arguments of the launcher of the same name. */
typedef struct ser_attention_args {
    const void* qkv; int64_t ld; int64_t plane_stride; int32_t q_col, k_col, v_col, B;
    const int32_t* frame_offs; const float* table; const float* gate;
    int32_t max_frames, table_T;
    void* out; int64_t ldo; int64_t out_plane_stride;
    int32_t H, dh; float scale; int32_t mode; int32_t gate_col, out_mode;   /* out_mode: 0 = `mode`'s planes, SER_MODE_FP16M: see out_scale */
    const float* gru_const; const int32_t* key_lens;
    const float* bias2d; int64_t bias2d_ld;
    /* WavLM gate computed INSIDE the kernel (round 3; ser_attention_v only): the two pre-activations per (row, head) are linear in
     * LayerNorm1(x) restricted to the head's dh channels (HF modeling_wavlm.py:167-180), so instead of riding along as 2H extra output
     * columns of the packed projection (gate_col: a 13th 256-wide column tile for 32 columns at D = 1024) every query block multiplies
     * its rows' dh elements of the layer input's operand copy with the head's two folded weight rows on the matrix cores (one MFMA chain
     * shaped like S = K Q^T) and applies the deferred LayerNorm in closed form:
     *   pre_j = rstd * (sum_d x[d] * gate_w[h][j][d] - mean * gate_cb[h][j]) + gate_cb[h][2 + j],   j = 0, 1
     * gate_x = that copy (the A operand of the packed projection: element type and plane count of `mode`), gate_stat = the projection's
     * ser_gemm_args.lnstat_out, gate_w = gamma-folded summed weights as operand planes [planes][H][2][dh] in the same format (ser_split_bf16),
     * gate_cb = fp32 [H][4] (column sums of the fp32 fold | beta W^T + b).  Needs table and gru_const; gate and gate_col are ignored. */
    const void* gate_x; int64_t gate_x_ld; int64_t gate_x_plane_stride;
    const float* gate_stat; const void* gate_w; const float* gate_cb;
    int32_t gate_x_planes, reserved1;
    int64_t gate_w_plane_stride;
    /* ABI 14: context rows as SER_MODE_FP16M operands for an output projection in that format (out_mode = SER_MODE_FP16M; mode FP16X,
     * head dim 64 -- a head is one 64-column tile): plane 0 of `out` = the fp16 copy, plane 1 = [P | Q] e4m3 bytes, out_scale[D / 64][out_scale_ld]
     * = one word of four E8M0 codes per (head, row).  The reference has no counterpart (fp32 end to end, preprocess_speech.py:50). */
    uint32_t* out_scale; int64_t out_scale_ld;
} ser_attention_args;
/* ser_attention with its arguments in a struct (the form command lists carry); the only entry point that takes the gate_x fields. */
int ser_attention_v(const ser_attention_args* args, void* stream);

typedef struct ser_layernorm_args {
    const float* x; int64_t ldx; const float* g; const float* b; float eps; int32_t gelu;
    float* out_f32; int64_t ldo_f32; void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    int32_t mode, rows, D, reserved0;
    uint32_t* range_flag;                           /* fp16 range guard, may be NULL (ABI 13) */
} ser_layernorm_args;
int ser_layernorm_v(const ser_layernorm_args* args, void* stream);

typedef struct ser_row_center_args {
    const float* x; int64_t ldx; void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    float* stats; float* shift; int32_t stat_groups, mode, rows, D;
    uint32_t* out_scale; int64_t out_scale_ld;      /* mode == SER_MODE_FP16M: block scales of the copy (ABI 13) */
    uint32_t* range_flag;                           /* fp16 range guard, may be NULL (see ser_gemm_args.range_flag) */
} ser_row_center_args;
int ser_row_center_v(const ser_row_center_args* args, void* stream);

typedef struct ser_logmel_args {
    const float* wav; const int64_t* sample_offs; const float* mel; float* out; void* work; int32_t B, n_mels;
} ser_logmel_args;

typedef struct ser_pack_act_args {
    const float* x; void* out; int64_t ldo; int64_t out_plane_stride; int32_t B, C, T, halo, mode, reserved0;
    uint32_t* range_flag;                           /* fp16 range guard, may be NULL (ABI 13) */
} ser_pack_act_args;
int ser_pack_act_v(const ser_pack_act_args* args, void* stream);

typedef struct ser_wave_frames_args {
    const float* wav; const int64_t* sample_offs; const int32_t* frame_offs; int32_t B, k, stride, mode;
    void* out; int64_t out_plane_stride; void* work; int32_t total_rows;
    int32_t no_norm;                                /* ABI 15: 1 = frames of the raw samples (do_normalize=False checkpoints); 0 = normalise */
    uint32_t* range_flag;                           /* fp16 range guard, may be NULL (ABI 13) */
} ser_wave_frames_args;
int ser_wave_frames_v(const ser_wave_frames_args* args, void* stream);

/* a5r (ABI 18)  ser_resample: the resampling half of librosa.load(path, sr=16000) (preprocess_speech.py:47) for a ragged, MIXED-RATE
 * batch in one launch: a Kaiser (beta 14) polyphase FIR, the filter scipy.signal.resample_poly designs (parity with librosa's soxr_hq is
 * unpinned; pinned is the output length ceil(n * 16000 / sr)).  Per utterance b with g = gcd(sr, 16000), up = 16000 / g, down = sr / g,
 * R = max(up, down), half = 10 R and the float64 bank h[0 .. 2 half] at bank + bank_off[b]
 *   (h[k] = up w[k] / sum(w),  w[k] = sinc((k - half) / R) / R * kaiser_14(2 half + 1)[k]):
 *   y[m] = sum_j x[j] h[m down - j up + half]  over 0 <= j < n with 0 <= m down - j up + half <= 2 half,   m = 0 .. n_out - 1,
 * n = in_offs[b + 1] - in_offs[b], n_out = out_offs[b + 1] - out_offs[b] (the caller's (n up + down - 1) / down).  fp32 samples times
 * float64 coefficients, accumulated in float64 in ascending j, rounded to fp32 once at the store: the order is fixed per output sample, so
 * a result does not depend on the rest of the batch (no atomics).  up == down == 1 copies the utterance bit for bit (half, bank_off unused).
 * Device: wav / out packed fp32, in_offs / out_offs / bank_off int64, up / down / half int32, bank float64 (every distinct bank of the
 * batch, once).  Host: B, total_in / total_out (packed sample totals) and max_out (the longest n_out; sizes the grid) -- the only fields
 * validated before the launch (-1 null pointer, -2 sizes); the per-utterance arrays are the caller's contract. */
#define SER_RESAMPLE_TILE 1024                      /* output samples per block */
typedef struct ser_resample_args {
    const float* wav; const int64_t* in_offs; const int64_t* out_offs;
    const int32_t* up; const int32_t* down; const int32_t* half; const int64_t* bank_off;
    const double* bank; float* out;
    int64_t total_in, total_out, max_out;
    int32_t B, reserved0;
} ser_resample_args;
int ser_resample_v(const ser_resample_args* args, void* stream);

/* K2g (ABI 15)  GroupNorm-over-time statistics of conv layer 0 for the *-base checkpoints (Conv1d(1, C, k, stride) -> GroupNorm(C, C,
 * eps) -> GELU, HF WavLMGroupNormConvLayer; the reference runs one file at a time, preprocess_speech.py:76-81, so the statistics of an
 * utterance cover exactly its frames).  Channel c is linear in the k-sample frame, so per utterance  mean_c = w_c . m + b_c,
 * var_c = w_c^T S w_c  from the frame mean m and covariance S: one read of the waveform, fp64 moments over a fixed chunking (32 chunks
 * per utterance, fixed merge order, no atomics: independent of the batch).  The frames are those ser_wave_frames writes: normalised
 * with its statistics (wave_stats = its workspace, so it must run first on the stream) unless no_norm.  Writes per (utterance b, channel c)
 *   scale[b * ld + c] = gamma_c * rstd_c,   shift[b * ld + c] = beta_c - mean_c * scale,
 * the ser_gemm_args.gn_scale / gn_shift of the conv-0 GEMM, and optionally stat_out[(b * C + c) * 2 + {0, 1}] = (mean_c, rstd_c).
 * w: [C][k] fp32 (k <= 10); bias may be NULL; frame_offs: rows of conv layer 0 [B + 1]; work: ser_workspace_bytes(SER_WS_GN_STATS, B). */
typedef struct ser_gn_stats_args {
    const float* wav; const int64_t* sample_offs; const int32_t* frame_offs;
    const float* w; const float* bias; const float* gamma; const float* beta;
    const void* wave_stats;
    float* scale; float* shift; float* stat_out; void* work;
    int32_t B, C, k, stride, ld, no_norm;
    float eps; int32_t reserved0;
} ser_gn_stats_args;
int ser_gn_stats_v(const ser_gn_stats_args* args, void* stream);

/* K6p (ABI 16)  data2vec-audio's positional stack (HF Data2VecAudioPositionalConvLayer / Data2VecAudioEncoder.forward): each of the
 * num_conv_pos_embeddings layers is a grouped Conv1d (run as ser_gemm over the zero-halo'd operand copy, bias added, fp32 out) followed
 * by LayerNorm(D, no affine, eps_pos) and GELU.  The LayerNorm spans all groups of a row, so it is a row pass of its own: one wave per row,
 * two-pass fp32 mean / variance (rows of a conv output may have a large mean), exact-erf GELU.
 *   last == 0 (intermediate layer):  y = gelu(LN(x))  -> out_act row out_rowmap[m] in `mode` (the next conv's operand planes at the
 *             row's halo'd position; the halo rows are never written and stay zero).  out_rowmap NULL = row m.
 *   last == 1 (last layer):          t = gelu(LN(x)) + residual;  z = LN(t) * g + b (encoder.layer_norm, eps)  -> out_f32 row m
 *             (hidden_states[0]) and, when out_act is not NULL, its operand copy at row m (out_rowmap must be NULL).
 * Modes SER_MODE_BF16 / FP32X / FP16 / FP16X.  rows <= 2^31, D % 4 == 0, D <= 2048, pitches multiples of 4.  range_flag: fp16 range
 * guard of the out_act values (see ser_gemm_args.range_flag), may be NULL.  The reference has no counterpart (fp32 end to end). */
typedef struct ser_pos_ln_args {
    const float* x; int64_t ldx;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    const int32_t* out_rowmap;
    const float* residual; int64_t ldr;
    const float* g; const float* b;
    float* out_f32; int64_t ldo_f32;
    float eps_pos, eps;
    int32_t last, mode, rows, D;
    uint32_t* range_flag;
} ser_pos_ln_args;
int ser_pos_ln_v(const ser_pos_ln_args* args, void* stream);

/* a22 (added under ABI 18: new entry points only, nothing existing changed)  The utterance-level tail of the organiser baseline's inference scripts (benchmark/train_eval_files/eval_cat_ser.py:164-177,
 * eval_dim_ser.py): last_hidden_state -> AttentiveStatisticsPooling (benchmark/net/pooling.py) -> EmotionRegression (benchmark/net/ser.py).
 * Neither launcher is a command-list op: they run after the recorded forward.  Both accumulate every sum in float64, in an order fixed
 * by the utterance alone (never by what else is in the batch: no atomics), and round once to fp32 at each store.
 *
 * ser_asp_pool_v: attentive statistics pooling over a packed ragged batch.  Per utterance b with rows r = frame_offs[b] .. frame_offs[b+1]-1:
 *   s_r = sum_d tanhf(hlin[r, d]) * a[d]          (hlin = x W^T + b of sap_linear, the caller's ser_gemm; accurate tanhf)
 *   w_r = exp(s_r - max_r s) / sum_r exp(s_r - max_r s)
 *   mu_d = sum_r w_r x[r, d];   rh_d = sqrt(max(sum_r w_r x[r, d]^2 - mu_d^2, 1e-5f))
 *   out[b] = [mu | rh], 2 D wide.  One frame gives mu = x, rh = sqrt(1e-5f).
 * Two launches: the scores (one wave per row, into the caller's workspace `scores` [rows]), then one block per (utterance, 64-column
 * slab) that reads x once -- the two kernels of ser_attn_pool_v, here with the tanh term and with the second moment kept.
 * x [rows, ldx], hlin [rows, ldh], a [D]: fp32, 16-byte aligned, pitches multiples of 4; frame_offs int32
 * [B + 1] on the device (the caller's contract: ascending, inside [0, rows]); out fp32 [B, ldo], ldo >= 2 D.  D % 4 == 0.  max_frames
 * (the longest utterance) is checked against rows and changes no result.  Validated before the launch: -1 null pointer, -2 sizes. */
typedef struct ser_asp_pool_args {
    const float* x; int64_t ldx;
    const float* hlin; int64_t ldh;
    const float* a;
    const int32_t* frame_offs;
    float* scores;
    float* out; int64_t ldo;
    int32_t B, D, rows, max_frames;
} ser_asp_pool_args;
int ser_asp_pool_v(const ser_asp_pool_args* args, void* stream);

/* ser_mlp_head_v: Linear(K, H) -> LayerNorm(H, eps) -> ReLU -> Linear(H, n_out) on B rows (EmotionRegression with one hidden layer;
 * Dropout is the identity in eval).  p [B, ldp], W1 [H, K], b1 / gamma / beta [H], W2 [n_out, H], b2 [n_out], workspace hidden [B, H],
 * out [B, n_out], all fp32.  Two launches: one wave per hidden unit (its W1 row in registers, looping over the B rows), then one block
 * per row -- the two kernels of ser_fusion_cls_v, here without the ReLU at the hidden units and with LayerNorm + ReLU ahead of the outputs.
 * K % 4 == 0, K <= 4096, 1 <= n_out <= 8, p and W1 16-byte aligned, ldp a multiple of 4. */
typedef struct ser_mlp_head_args {
    const float* p; int64_t ldp;
    const float* W1; const float* b1; const float* gamma; const float* beta;
    const float* W2; const float* b2;
    float* hidden; float* out;
    float eps;
    int32_t B, K, H, n_out, reserved0;
} ser_mlp_head_args;
int ser_mlp_head_v(const ser_mlp_head_args* args, void* stream);

/* a29 (added under ABI 18: new entry points only)  The head the hub's audio-classification checkpoints share (HF
 * WavLMForSequenceClassification.forward and its wav2vec2 / HuBERT / data2vec-audio / w2v-BERT twins, WhisperForAudioClassification):
 *   x = sum_l softmax(layer_weights)[l] hs[l]  (use_weighted_layer_sum; else the last state)  ->  projector  ->  mean over the frames  ->  classifier.
 * Projector and mean are linear, so the mean is taken first: the [M, D] weighted sum and the M-row projection are never formed.
 * Neither launcher is a command-list op: they run after the recorded forward.  Both accumulate every sum in float64, in an order fixed by
 * the utterance alone (its frame count and the widths, never what else is in the batch: no atomics), and round once to fp32 at each store.
 *
 * ser_layer_pool_v: per utterance b with rows r0 = frame_offs[b] .. frame_offs[b+1]-1 (T_b of them):
 *   out[b, d] = (1 / T_b) sum_t sum_l w[l] s[l, r0 + t, d]
 * s: n_states fp32 planes [rows, lds], state l at s + l * state_stride (floats); n_states = 1 with w = {1.0} and s at the last state is
 * the form without the weighted sum.  w: float64 [n_states] on the device.  The frames are cut into chunks of SER_LAYER_POOL_FC counted
 * from the utterance's first row; two launches: one block per (256-column slab, chunk, utterance) adds its terms frame by frame, within
 * a frame in ascending state, into the float64 workspace work [B, ceil(max_frames / SER_LAYER_POOL_FC), D] (a chunk past the
 * utterance's end leaves at once), then one thread per (utterance, column) adds the chunk partials in ascending chunk, divides by T_b and
 * rounds.  s is read once, 16 bytes at a time.  frame_offs int32 [B + 1] on the device and the same numbers at frame_offs_host, which the
 * launcher validates.  out fp32 [B, ldo], ldo >= D; columns beyond D are not written.
 * Refused before the launch: -1 null pointer; -2 D % 4 != 0, n_states < 1, an empty utterance, offsets outside [0, rows] or descending,
 * an utterance longer than max_frames, max_frames > rows, B > 65535, lds / state_stride not multiples of 4, s not 16-byte aligned, a
 * workspace smaller than B * ceil(max_frames / SER_LAYER_POOL_FC) * D doubles. */
#define SER_LAYER_POOL_FC 32
typedef struct ser_layer_pool_args {
    const float* s; int64_t state_stride; int64_t lds;
    const double* w;
    const int32_t* frame_offs;
    const int32_t* frame_offs_host;
    double* work; int64_t work_elems;
    float* out; int64_t ldo;
    int32_t n_states, B, D, rows, max_frames, reserved0;
} ser_layer_pool_args;
int ser_layer_pool_v(const ser_layer_pool_args* args, void* stream);

/* ser_cls_tail_v: out[b] = C (P pooled[b] + bp) + bc on B rows: Linear(D, proj) then Linear(proj, n_labels), nothing between them (HF's
 * projector and classifier).  pooled [B, ldp], P [proj, D], bp [proj], C [n_labels, proj], bc [n_labels], out [B, ldo], all fp32.  One
 * block per row: a wave per projector unit (products added per lane in ascending column, then the butterfly; the unit is kept in
 * float64, not rounded), then a wave per label.  D % 4 == 0, 1 <= proj <= 2048, 1 <= n_labels <= 2048 (n_labels = 1: regression),
 * pooled and P 16-byte aligned, ldp a multiple of 4, ldo >= n_labels, B <= 65535. */
typedef struct ser_cls_tail_args {
    const float* pooled; int64_t ldp;
    const float* P; const float* bp; const float* C; const float* bc;
    float* out; int64_t ldo;
    int32_t B, D, proj, n_labels;
} ser_cls_tail_args;
int ser_cls_tail_v(const ser_cls_tail_args* args, void* stream);

/* a30 (added under ABI 18: new entry points only)  The x-vector head of the hub's speaker-verification checkpoints (HF
 * WavLMForXVector.forward; the wav2vec2 / data2vec-audio / w2v-BERT classes are the same text), one utterance of T frames:
 *   x = sum_l softmax(layer_weights)[l] hs[l]  (use_weighted_layer_sum; else the last state)                      [T, D]
 *   x = projector(x)                                                                                               [T, tdnn_dim[0]]
 *   TDNN layer i:  y[t] = ReLU(b + sum_{j < k_i} W_j x[t + j d_i]),  t < T_i = T_{i-1} - d_i (k_i - 1);  kernel.weight [out, k in], tap-major
 *   stats = cat(mean_t y, std_t y) over the T' rows of the last layer, std unbiased (divided by T' - 1)
 *   embeddings = feature_extractor(stats);  logits = classifier(embeddings)
 * A ReLU follows the projector's successors, so projector and mean do not commute: the [T, D] mix is formed.  The projector and every TDNN
 * layer are ser_gemm launches (a layer: kc = its padded input width, ldj = d_i * the operand pitch, a_rowoff from ser_ragged_index over
 * the per-layer offsets, so no window crosses an utterance; ser_act_rows_v(relu = 1) makes the next operand).  The three launchers below
 * are the rest.  None is a command-list op; none uses a float atomic; every sum runs in an order fixed by the utterance alone.
 *
 * ser_layer_mix_v: out[m, d] = sum_l w[l] s[l, m, d] over n_states fp32 planes [rows, lds] (state l at s + l * state_stride floats), each
 * element ONE float64 sum -- products rounded to float64, added in ascending l, no fused multiply-add -- rounded once to fp32; that fp32
 * value goes to the operand planes out_act in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X) and, when out_f32 is not NULL, to out_f32
 * [rows, ldo_f32].  w: float64 [n_states] on the device; n_states = 1 with w = {1.0} is the form without the weighted sum.  Wave per row;
 * D % 4 == 0, D <= 2048, pitches multiples of 4, s 16-byte aligned.  range_flag: the fp16 range guard, reported as ser_act_rows_v does;
 * may be NULL.  Refused: -1 null pointer, -2 sizes, -3 pitches / alignment, -4 mode. */
typedef struct ser_layer_mix_args {
    const float* s; int64_t state_stride; int64_t lds;
    const double* w;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    int32_t n_states, mode, rows, D;
} ser_layer_mix_args;
int ser_layer_mix_v(const ser_layer_mix_args* args, void* stream);

/* ser_stat_pool_v: statistics pooling.  Per utterance b with rows r0 = frame_offs[b] .. frame_offs[b+1]-1 (T_b >= 2 of them) of the fp32
 * rows x [rows, ldx], with relu == 1 read as max(x, 0):
 *   out[b, d] = mean_t x[r0 + t, d];   out[b, D + d] = sqrt( sum_t (x[r0 + t, d] - mean)^2 / (T_b - 1) )
 * in float64, one rounding at each store.  The frames are cut into chunks of SER_STAT_POOL_FC counted from the utterance's first row.  One
 * block per (256-column slab, chunk, utterance) takes the chunk's mean and then, in a second pass over the chunk, its CENTRED second
 * moment sum_t (x - chunk mean)^2 into work [B, chunks, 2, D]; one thread per (utterance, column) then merges the chunks in ascending
 * order (Chan et al.: M2 += M2_c + delta^2 n n_c / (n + n_c)).  No sum of raw squares is ever formed, so a column whose mean is 10^5
 * times its deviation keeps its std.  Columns beyond D of x (ldx > D: the zero padding of a GEMM's output width) are never read.
 * frame_offs int32 [B + 1] on the device and the same numbers at frame_offs_host, which the launcher validates.  out fp32 [B, ldo],
 * ldo >= 2 D.  Refused before the launch: -1 null pointer; -2 D % 4 != 0, relu not 0 / 1, an utterance with fewer than 2 rows (named by
 * its index), offsets outside [0, rows] or descending, an utterance longer than max_frames, max_frames > rows, B > 65535, ldx not a
 * multiple of 4 or < D, x not 16-byte aligned, a workspace smaller than B * ceil(max_frames / SER_STAT_POOL_FC) * 2 * D doubles. */
#define SER_STAT_POOL_FC 32
typedef struct ser_stat_pool_args {
    const float* x; int64_t ldx;
    const int32_t* frame_offs;
    const int32_t* frame_offs_host;
    double* work; int64_t work_elems;
    float* out; int64_t ldo;
    int32_t B, D, rows, max_frames, relu, reserved0;
} ser_stat_pool_args;
int ser_stat_pool_v(const ser_stat_pool_args* args, void* stream);

/* ser_xvec_tail_v: ser_cls_tail_v's kernel with the intermediate written too:
 *   emb[b] = fp32(F stats[b] + bf)   (HF's `embeddings`; rounded ONCE, and the classifier reads that fp32 value, as HF's does)
 *   logits[b] = C emb[b] + bc
 * stats [B, lds], F [dim, D], bf [dim], C [n_labels, dim], bc [n_labels], emb [B, lde], logits [B, ldo], all fp32; sums in float64 in
 * ser_cls_tail_v's order.  D % 4 == 0, 1 <= dim <= 2048, 1 <= n_labels <= 2048, stats and F 16-byte aligned, lds a multiple of 4 and
 * >= D, lde >= dim, ldo >= n_labels, B <= 65535. */
typedef struct ser_xvec_tail_args {
    const float* stats; int64_t lds;
    const float* F; const float* bf; const float* C; const float* bc;
    float* emb; int64_t lde;
    float* logits; int64_t ldo;
    int32_t B, D, dim, n_labels;
} ser_xvec_tail_args;
int ser_xvec_tail_v(const ser_xvec_tail_args* args, void* stream);

/* a31 (added under ABI 18: new entry points only)  Greedy CTC decoding behind the lm_head of the hub's CTC checkpoints (HF *ForCTC:
 * logits = lm_head(last_hidden_state); predicted_ids = argmax(logits, -1); Wav2Vec2CTCTokenizer.decode groups equal neighbours and drops
 * the blank).  The lm_head is a ser_gemm launch with fp32 output (its weight zero-padded to a multiple of 8 rows); ser_ctc_greedy_v is
 * the rest.  Not a command-list op.
 *
 * z: fp32 logits [rows, ldz], the packed ragged rows of a batch; the true width is V, and columns V .. ldz - 1 (the GEMM's padding) are
 * NEVER read, so nothing there can win.  Utterance b owns frames r0 = frame_offs[b] .. frame_offs[b + 1] - 1 (int32 [B + 1] on the
 * device).  Per frame t of it:
 *   tok[t]    = argmax_v z[r0 + t, v], v < V; on a tie the lowest index wins (torch.argmax; ser_dec_select_v's rule)
 *   margin[t] = top1 - top2, one fp32 subtraction (+inf when V == 1, or when every other column is -inf)
 *   t is KEPT when tok[t] != blank and (t == 0 or tok[t] != tok[t - 1]) -- the previous frame of the SAME utterance only
 * The kept tokens in order go to ids[b, 0 .. n_b - 1], counts[b] = n_b; starts[b, j] is the frame index (inside the utterance) of kept
 * token j and ends[b, j] one past the last frame of its run: HF's char_offsets in frames.  ids / starts / ends are int32 [B, ld_tok],
 * ld_tok >= max_frames; entries at j >= n_b are not written.  An utterance longer than max_frames is cut there (never a write past the
 * pitch).  Optional outputs, each skipped when NULL: frame_ids [rows] (HF's predicted_ids, before the collapse), frame_margin [rows],
 * min_margin [B] (the smallest margin of the utterance's frames; +inf for an utterance without frames).
 * err: a frame whose winning value is not finite -- all -inf, a +inf, or a NaN among its V columns (a NaN is read as +inf, so it wins) --
 * ORs SER_CTC_ERR_NONFINITE into *err, which the caller zeroes; the batch then fails like a range-guard hit.  This is
 * ser_dec_select_v's rule.  The other frames' and utterances' outputs are what they would be without that frame.
 * work: int32 words, work_elems >= 2 * rows of them (the per-frame tokens and margins between the two kernels).
 *
 * Two kernels.  Argmax: a grid over all rows; G lanes of a wave (8 .. 64, from V) take one frame with 16-byte loads and reduce
 * (top1, its index, top2) triples.  Collapse: one block per utterance walks its frames in chunks of SER_CTC_CHUNK, a block-wide exclusive
 * scan of the keep flags per chunk, the running count carried from chunk to chunk.
 * Determinism: there is no floating-point sum and no atomic on data.  max, the lowest index of the max and the second value are
 * functions of a row's multiset of (value, index) pairs, so the merge of two triples is associative and commutative and no split of V
 * over lanes, no lane count and no shuffle order can change a result; the margin is one subtraction of two such values; min_margin is
 * a min, exact in any order; the scan adds integers.  Every output is therefore a pure function of (the utterance's rows of z, blank) and
 * bit-identical whatever else shares the batch.
 * Refused before any launch: -1 null pointer (z, frame_offs, work, ids, starts, ends, counts, err); -2 sizes (B < 1 or > 65535, V < 1,
 * rows < 1, blank outside [0, V), max_frames < 1, work_elems < 2 * rows); -3 pitches / alignment (ldz < V or not a multiple of 4,
 * ld_tok < max_frames, z not 16-byte aligned). */
#define SER_CTC_CHUNK 256
#define SER_CTC_ERR_NONFINITE 1
typedef struct ser_ctc_greedy_args {
    const float* z; int64_t ldz;
    const int32_t* frame_offs;
    int32_t* work; int64_t work_elems;
    int32_t* ids; int32_t* starts; int32_t* ends; int64_t ld_tok;
    int32_t* counts;
    int32_t* frame_ids; float* frame_margin; float* min_margin;
    uint32_t* err;
    int32_t B, V, rows, blank, max_frames, reserved0;
} ser_ctc_greedy_args;
int ser_ctc_greedy_v(const ser_ctc_greedy_args* args, void* stream);

/* a32 (added under ABI 18: new entry points only)  CTC forced alignment: the single best CTC path that spells a GIVEN target, per
 * utterance of a packed ragged batch of a31's logits.  Not a command-list op.
 *
 * The rule, one utterance: fp32 logits z[T, V] (rows frame_offs[b] .. frame_offs[b + 1] - 1 of z), the blank id, a target y[0 .. L-1]
 * (targets[tgt_offs[b] .. tgt_offs[b + 1] - 1], int32 on the device), every y[j] in [0, V) and != blank.
 *   states     S = 2 L + 1; state s emits the blank when s is even and y[s / 2] when s is odd
 *   emission   e(t, s) = (double) z[t, label(s)]: RAW logits (a frame's log-sum-exp shifts every path alike and stays out)
 *   alpha      float64.  alpha[0][0] = e(0, 0), alpha[0][1] = e(0, 1), the rest -inf;
 *              alpha[t][s] = max(alpha[t-1][s], alpha[t-1][s-1], alpha[t-1][s-2]) + e(t, s), the third term only for odd s >= 3 with
 *              y[s/2] != y[s/2 - 1].  One max of exact values and one float64 addition per cell, every fp32 -> double conversion exact,
 *              nothing to contract: a numpy float64 loop reproduces every alpha bit for bit (tests/ctc_align_ref.py).
 *   ties       the smaller jump wins (stay, then step, then skip: a candidate replaces the current one only when strictly greater); the
 *              path ends in state S - 1 only when alpha[T-1][S-1] > alpha[T-1][S-2], else in S - 2.  L == 0: state 0, every frame blank.
 *   feasible   iff T >= 1 and T >= L + #{j : y[j] == y[j-1]}
 * Outputs per utterance: pos[t] (optional, [rows]) the target index whose state frame t is in, -1 for a blank frame; starts[b, j] /
 * ends[b, j] the first frame of token j and one past its last (contiguous by construction); path_logit[b] the final alpha (float64);
 * frame_score[t] (optional, [rows]) = fp32((double) z[t, c_t] - lse64[t]), c_t the emitted label and lse64[t] the float64 log-sum-exp of
 * row t's V columns (max subtracted first): the path's log-probability per frame; tok_score[b, j] = fp32 of the float64 mean of
 * frame_score over the token's frames, summed in frame order.  starts / ends / tok_score are [B, ld_tok], ld_tok >= max_tokens; entries
 * at j >= L_b are not written.  Columns V .. ldz - 1 are NEVER read.
 * status[b] (always written), 0 or ONE of, checked in this order:
 *   SER_CTC_ALIGN_BAD_TARGET  a target id outside [0, V) or equal to the blank, L_b > max_tokens (or > SER_CTC_ALIGN_MAX_TOKENS), more
 *                             than max_frames frames, or offsets that leave [0, rows] / [0, n_targets]
 *   SER_CTC_ALIGN_INFEASIBLE  too few frames (the feasibility rule above)
 *   SER_CTC_ALIGN_NONFINITE   a logit in a column of {blank} U y, at any of the utterance's frames, is NaN or +inf, or the best score
 *                             is not finite (-inf is a legal logit; a NaN in any OTHER column sets no status: that frame's lse64, and
 *                             with it frame_score and its token's tok_score, are then NaN)
 * A non-zero status leaves the utterance's other outputs unspecified (path_logit may be written); every other utterance's outputs are
 * exactly what they would be without it.
 * work: 8-byte aligned, work_bytes >= ser_ctc_align_work_bytes(rows, B, max_frames, max_tokens) = 16 rows (lse64, the path's states and
 * the frame scores) + B * max_frames * 16 * ceil((2 max_tokens + 1) / 64) (the back pointers); -1 for arguments ser_ctc_align_v refuses.
 *
 * Two kernels.  lse64: a grid over all rows on a31's lane-group split.  Alignment: ONE block of SER_CTC_ALIGN_THREADS threads per
 * utterance, state s on thread s % THREADS, frames the serial loop: three reads of the previous alpha row (two float64 rows in LDS, so one
 * barrier per frame), one max, one add, one write; the next frame's emissions are loaded before the barrier; the back pointers are two
 * bits per cell, packed by two wave ballots per 64 states.  The backtrack (T dependent reads, once) runs on one thread over chunks of
 * back pointers the block copies into LDS; pos, frame_score, the spans and the token means are parallel passes.
 * Determinism: no atomics; max and compare are exact; the lse's sum order is a function of V alone and a token's mean is one thread's
 * sum in frame order.  Every output is a pure function of (the utterance's rows of z, its target, blank), whatever shares the batch.
 * Refused before any launch: -1 null pointer (z, frame_offs, targets, tgt_offs, work, starts, ends, tok_score, status, path_logit);
 * -2 sizes (B < 1 or > 65535, V < 1, rows < 1, max_frames < 1, n_targets < 0, max_tokens outside [0, SER_CTC_ALIGN_MAX_TOKENS], blank
 * outside [0, V), work_bytes too small); -3 pitches / alignment (ldz < V, ld_tok < max_tokens, z not 4-byte, work or path_logit not
 * 8-byte aligned). */
#define SER_CTC_ALIGN_THREADS 512
#define SER_CTC_ALIGN_MAX_TOKENS 1023
#define SER_CTC_ALIGN_INFEASIBLE 1
#define SER_CTC_ALIGN_NONFINITE 2
#define SER_CTC_ALIGN_BAD_TARGET 4
typedef struct ser_ctc_align_args {
    const float* z; int64_t ldz;
    const int32_t* frame_offs;
    const int32_t* targets; const int32_t* tgt_offs;
    void* work; int64_t work_bytes;
    int32_t* starts; int32_t* ends; float* tok_score; int64_t ld_tok;
    int32_t* status; double* path_logit;
    int32_t* pos; float* frame_score;
    int32_t B, V, rows, blank, max_frames, max_tokens, n_targets, reserved0;
} ser_ctc_align_args;
int ser_ctc_align_v(const ser_ctc_align_args* args, void* stream);
int64_t ser_ctc_align_work_bytes(int32_t rows, int32_t B, int32_t max_frames, int32_t max_tokens);

/* a33 (added under ABI 18: new entry points, one ser_cmd member and one SER_OP code only)  Whisper token timestamps from the decoder's
 * cross-attention: HF's WhisperGenerationMixin._extract_token_timestamps for EVERY UTTERANCE ALONE (batch 1, greedy short-form generate,
 * return_token_timestamps=True, num_frames = len(samples) / 160), restated.  P = 4 prompt positions; an utterance whose generated tokens are
 * g_0 .. g_{n-1} (the last one eos, or the token at the length cap) has R = n - 1 token rows: the cross-attention of the steps that FEED
 * g_0 .. g_{n-2}, positions P .. P + n - 2.  F = (len / 160) / 2 frames.  What shares the batch changes nothing.
 *
 * The rule, one utterance, alignment heads (layer_k, head_k), k < A, in list order:
 *   weights  w_k[r][s] = softmax over ALL n_keys keys s of scale * <q_k[P + r], K_k[s]> (float64 dot and softmax over the fp32 queries and
 *            the fp32 cross cache, as HF's softmax runs over max_source_positions), rounded to fp32; frames s < F are kept
 *   z-score  per (k, f): mean and BIASED std over the utterance's R rows, float64, sums in ascending row order (two passes);
 *            z = (w - mean) / std
 *   median   per (k, r): the median of `width` (odd; 7) along the frames with reflect padding; F <= width / 2 leaves z as it is.  A
 *            selection: exact
 *   mean     over the heads, added in list order, divided by A; ONE rounding to fp32: matrix[R][F]
 *   DTW      HF's _dynamic_time_warping on -matrix.  cost is fp32 [R + 1][F + 1], +inf but cost[0][0] = 0.  Frames j ascending, rows i
 *            ascending: c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]; c = c0 (trace 0) if c0 < c1 and c0 < c2, else c1
 *            (trace 1) if c1 < c0 and c1 < c2, else c2 (trace 2); cost[i][j] = fp32(double(-matrix[i-1][j-1]) + double(c)).  One exact
 *            conversion each, one float64 add, one rounding: a numpy loop reproduces every cell bit for bit (tests/whisper_ts_ref.py).
 *            Backtrace from (R, F) while i > 0 or j > 0: emit (i - 1, j - 1); row 0 is forced left (trace 2), column 0 up (trace 1).
 *            first_frame[r] = the frame of the path's earliest cell in row r (HF's jump times / time_precision)
 *   times    token k < n - 1: first_frame[k] * 0.02 s; the last token repeats the one before it (HF has no cross-attention row for it)
 * Edge cases, settled against HF (tools/make_whisper_timestamps_golden.py):
 *   n = 1   R = 0: no rows, the time is 0; nothing is launched for the utterance's rows
 *   n = 2   R = 1: the std over one row is 0, the row is NaN, every comparison of the DTW is false and the path runs along row 0: time 0.
 *           ser_ts_matrix_v sets no status for R = 1; ser_dtw_v follows the rule through the NaNs (its status is SER_TS_NONFINITE, which
 *           the caller ignores for R = 1)
 *   F <= 3  (width 7) the median filter returns its input
 *   F = 0   with R >= 1: SER_TS_NO_FRAMES; the file fails alone
 *   any other non-finite matrix entry or z-score (a column whose std is 0 with R >= 2): SER_TS_NONFINITE for that utterance alone, never a
 *   silent time
 *
 * ser_dec_keep_q_v (SER_OP_DEC_KEEP_Q): the capture of one decode step and one layer: copies the layer's alignment heads' cross queries
 * q[b][head[h] * 64 .. + 64] (fp32, the output of the cross q projection, before the scale) to keep[*pos][b][slot0 + h][0 .. 64];
 * keep is [max_pos][B][n_align][64] fp32.  A position outside [0, max_pos) writes nothing.  One launch of n_heads x B waves.
 * ser_ts_weights_v: keep, the cross cache (K of layer l, utterance b, key s, head h at cross + l layer_stride + b batch_stride + s ldc +
 * 64 h), n_rows[b] = R_b and n_frames[b] = F_b on the device -> w [B][n_align][max_rows][ld_w] fp32; entries at r >= R_b or s >= F_b are
 * not written.  A block takes 4 token rows of one (utterance, head): each key is read once for the four.  The softmax sum: a thread adds
 * keys t, t + 256, .. in order, the lanes meet by xor shuffles, the four waves are added in wave order: a function of n_keys alone.
 * ser_ts_matrix_v: w -> matrix [B][max_rows][ld_m] fp32 and status[b] (always written: 0, SER_TS_BAD_SHAPE for R_b outside [0, max_rows]
 * or F_b outside [0, max_frames], SER_TS_NO_FRAMES, SER_TS_NONFINITE); stats is work of B * n_align * max_frames * 16 bytes.
 * ser_dtw_v: matrix -> first_frame [B][ld_t] int32 (entries r < R_b), status[b] (always written; SER_TS_NONFINITE when the final cost is not
 * finite -- the outputs still follow the rule), optionally the path in BACKTRACE order (path_text / path_time [B][max_rows + max_frames],
 * path_len[b]; all three or none).  One block of SER_TS_THREADS threads per utterance, thread = token row (max_rows <= SER_TS_THREADS),
 * anti-diagonal wavefront: three diagonals of fp32 costs in LDS, one barrier per diagonal (R + F - 1 of them); a thread reads its matrix
 * row a block of 8 diagonals ahead and packs its 2-bit back pointers 32 to a 64-bit word of work (work_bytes >= ser_dtw_work_bytes(B, max_rows,
 * max_frames) = 8 B max_rows ceil(max_frames / 32); -1 for sizes ser_dtw_v refuses).  The backtrack runs on one thread over bands of
 * SER_TS_BAND frames the block stages in LDS.
 * Determinism: no atomics on data; every output of an utterance is a pure function of its own queries, keys, R and F.
 * Refused before any launch: -1 null pointer, -2 sizes, -3 pitches / alignment, each naming the argument. */
#define SER_TS_THREADS 512
#define SER_TS_BAND 256
#define SER_TS_MAX_KEYS 1536
#define SER_TS_MAX_HEADS 32
#define SER_TS_KEEP_HEADS 16
#define SER_TS_NONFINITE 1
#define SER_TS_BAD_SHAPE 2
#define SER_TS_NO_FRAMES 4
typedef struct ser_dec_keep_q_args {
    const float* q; int64_t ldq;
    const int32_t* pos;
    float* keep;
    int32_t head[SER_TS_KEEP_HEADS];
    int32_t n_heads, slot0, n_align, B, H, max_pos;
} ser_dec_keep_q_args;
int ser_dec_keep_q_v(const ser_dec_keep_q_args* args, void* stream);
typedef struct ser_ts_weights_args {
    const float* keep;
    const float* cross; int64_t layer_stride; int64_t batch_stride; int64_t ldc;
    const int32_t* n_rows; const int32_t* n_frames;
    float* w; int64_t ld_w;
    float scale;
    int32_t B, n_align, n_keys, pos0, max_rows, max_pos, n_layers, H, reserved0;
    int32_t head_layer[SER_TS_MAX_HEADS];
    int32_t head_index[SER_TS_MAX_HEADS];
} ser_ts_weights_args;
int ser_ts_weights_v(const ser_ts_weights_args* args, void* stream);
typedef struct ser_ts_matrix_args {
    const float* w; int64_t ld_w;
    const int32_t* n_rows; const int32_t* n_frames;
    double* stats;
    float* matrix; int64_t ld_m;
    int32_t* status;
    int32_t B, n_align, max_rows, max_frames, width, reserved0;
} ser_ts_matrix_args;
int ser_ts_matrix_v(const ser_ts_matrix_args* args, void* stream);
typedef struct ser_dtw_args {
    const float* matrix; int64_t ld_m;
    const int32_t* n_rows; const int32_t* n_frames;
    void* work; int64_t work_bytes;
    int32_t* first_frame; int64_t ld_t;
    int32_t* status;
    int32_t* path_text; int32_t* path_time; int32_t* path_len;
    int32_t B, max_rows, max_frames, reserved0;
} ser_dtw_args;
int ser_dtw_v(const ser_dtw_args* args, void* stream);
int64_t ser_dtw_work_bytes(int32_t B, int32_t max_rows, int32_t max_frames);

/* a23 (added under ABI 18: new entry points only)  The reference's bimodal fusion head (bin/train_cat_bimodal_lazy_1head.py:236-334,
 * MultiModalEmotionClassifier) on packed ragged batches: every utterance alone, as the reference's evaluation runs it (batch_size = 1,
 * bin/eval_cat_bimodal_lazy_1head.py:292) -- no pad frame enters the recurrence, the attention or a pooling softmax.  None of the four is a
 * command-list op.  No atomics on float data; an utterance's result does not depend on what else is in the batch.
 *
 * ser_gru_v: the recurrence of nn.GRU(H, H, bidirectional=True), torch's convention (gates r, z, n; h_0 = 0):
 *   r = sigmoid(gx_r + W_hr h + b_hr);  z likewise;  n = tanh(gx_n + r (W_hn h + b_hn));  h' = (1 - z) n + z h
 * gx [rows, ldgx >= 6 H] fp32 = x W_ih^T + b_ih of BOTH directions (forward gates in columns 0 .. 3H-1, backward in 3H .. 6H-1: one ser_gemm
 * over the stacked weight_ih matrices).  whh: fp16 hi + lo planes of the stacked [weight_hh_l0 ; weight_hh_l0_reverse] = [6 H, H]
 * (ser_split_bf16 in SER_MODE_FP16X; whh_plane_stride in elements); bhh [6 H] fp32, stacked alike.  The backward direction runs from each
 * utterance's own last row to its first.  out [rows, ldo >= 2 H] fp32: forward h in columns 0 .. H-1, backward in H .. 2H-1; out_act (may be
 * NULL): the same rows as GEMM operand planes in `mode` (SER_MODE_BF16, FP32X or FP16X).
 * Precision: W_hh h is always the 3-product split on v_mfma_f32_16x16x32_f16 (hi hi + lo hi + hi lo), h re-split into fp16 hi + lo every
 * step (|h| < 1: no range guard); the gates are fp32 with accurate expf / tanhf.  Up to 16 utterances ride the MFMA's N dimension.
 * Forms: a cluster of R blocks serves each (group of <= 16 utterances, direction); a block owns H / R hidden units x 3 gates, its W_hh slice
 * resident in LDS when it fits, and the blocks exchange the new h every step through `work` as tagged 8-byte granules (double-buffered
 * by step parity, tag = (epoch mod 4096) << 20 | step + 1; the workspace is also zeroed ahead of every launch, and a tag is never zero).
 * cluster = 0 chooses R (the smallest whose slice fits LDS: 1 at H = 64, 32 at H = 512); an explicit value forces it and must divide H / 16.
 * R = 1 is block-local (h through LDS, no global wait; weights streamed from L2 when they do not fit).  The order of every sum is the same
 * for every R: results are bit-identical across cluster sizes.  At most 256 blocks per launch; the launcher loops over further groups.
 * Every cluster wait is bounded (one second): on give-up the block stores SER_GRU_ERR_TIMEOUT to *err and the launch drains without
 * waiting again; the caller zeroes *err, reads it back with the results and fails the batch when it is set.
 * H % 64 == 0, H <= 512; max_frames < 2^20.  R > 1 needs work (16-byte aligned, work_bytes >= ser_gru_work_bytes) and err.
 * ser_gru_work_bytes: the workspace bytes for (H, cluster), 0 for R = 1, -1 for a bad pair; *R_out (may be NULL) receives R. */
#define SER_GRU_ERR_TIMEOUT 1
typedef struct ser_gru_args {
    const float* gx; int64_t ldgx;
    const void* whh; int64_t whh_plane_stride;
    const float* bhh;
    const int32_t* frame_offs;
    float* out; int64_t ldo;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    void* work; int64_t work_bytes;
    uint32_t* err;
    int32_t B, H, rows, max_frames, mode, cluster;
    uint32_t epoch; int32_t reserved0;
} ser_gru_args;
int ser_gru_v(const ser_gru_args* args, void* stream);
int64_t ser_gru_work_bytes(int32_t H, int32_t cluster, int32_t* R_out);

/* ser_xattn_v: ser_xattn_mh_v with heads = 1 (one validation and launch routine serves both; messages carry the entry point's own name):
 * nn.MultiheadAttention(E, 1) between its in- and out-projection, over ragged pairs: utterance b's queries are rows
 * q_offs[b] .. q_offs[b+1]-1 of q, its keys / values rows k_offs[b] .. k_offs[b+1]-1 of k / v (fp32, from ser_gemm; no mask):
 *   ctx[r] = sum_j softmax_j(scale q[r] . k[j]) v[j]
 * fp32 FMAs, online softmax in base 2 (logits pre-scaled by scale log2 e), one block per (utterance, 16 queries), keys in tiles of 16 from
 * the utterance's first key: tiles never cross utterances.  out_act: ctx as GEMM operand planes in `mode` (BF16 / FP32X / FP16X; FP16X
 * reports into range_flag, may be NULL); out_f32: ctx in fp32.  Either may be NULL, not both.  E % 64 == 0, E <= 1024; B <= 65535;
 * q / k / v / out_f32 16-byte aligned, pitches multiples of 4.  max_q (the longest query side) sizes the grid. */
typedef struct ser_xattn_args {
    const float* q; int64_t ldq;
    const float* k; int64_t ldk;
    const float* v; int64_t ldv;
    const int32_t* q_offs; const int32_t* k_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    float scale;
    int32_t B, E, q_rows, k_rows, max_q, mode, reserved0;
} ser_xattn_args;
int ser_xattn_v(const ser_xattn_args* args, void* stream);

/* ser_xattn_mh_v: nn.MultiheadAttention(E, heads) between its in- and out-projection, over the same ragged pairs: ser_xattn_v's contract
 * plus `heads`.  With dh = E / heads, head h is columns h dh .. (h+1) dh - 1 of q, k, v and of the context:
 *   ctx[r, head h] = sum_j softmax_j(scale q_h[r] . k_h[j]) v_h[j]      over the utterance's own keys
 * `scale` comes from the caller (dh^-0.5 for torch's module).  The same kernel as ser_xattn_v with the head as a grid dimension: one block per
 * (16 queries, head, utterance) stages its head's dh columns only (LDS grows with dh, not E); heads == 1 is bit-identical to ser_xattn_v.
 * No atomics on float data; an utterance's result does not depend on the batch around it.  heads >= 1, E % heads == 0, dh % 64 == 0,
 * E <= 1024, B <= 65535; alignment, pitches, out_act / out_f32, `mode` and the FP16X report into range_flag as for ser_xattn_v. */
typedef struct ser_xattn_mh_args {
    const float* q; int64_t ldq;
    const float* k; int64_t ldk;
    const float* v; int64_t ldv;
    const int32_t* q_offs; const int32_t* k_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    float scale;
    int32_t B, E, heads, q_rows, k_rows, max_q, mode;
} ser_xattn_mh_args;
int ser_xattn_mh_v(const ser_xattn_mh_args* args, void* stream);

/* ser_attn_pool_v: the head's attention pooling.  With x = a + b (a: the GRU output, b: the attention out-projection's fp32 output):
 *   s_r = x[r] . w + bias;   out[u, col0 .. col0 + E - 1] = sum_r softmax_r(s) x[r]   over utterance u's rows.
 * The two kernels of ser_asp_pool_v, here with the (a + b) . w term and source and the first moment only: scores by one wave per row into
 * the workspace `scores` [rows], then one block per (64-column slab, utterance);
 * float64 accumulation in ascending frame order, fixed-order merges, one rounding at the store.  One frame gives a + b exactly.
 * E % 4 == 0; a / b / w 16-byte aligned, pitches multiples of 4; ldo >= col0 + E. */
typedef struct ser_attn_pool_args {
    const float* a; int64_t lda;
    const float* b; int64_t ldb;
    const float* w;
    const int32_t* frame_offs;
    float* scores;
    float* out; int64_t ldo;
    float bias;
    int32_t col0, B, E, rows, max_frames, reserved0;
} ser_attn_pool_args;
int ser_attn_pool_v(const ser_attn_pool_args* args, void* stream);

/* ser_fusion_cls_v: LayerNorm(K, eps) -> Linear(K, H1) -> ReLU -> Linear(H1, n_out) on B rows (layer_norm and classifier of the head;
 * Dropout is the identity in eval).  A LayerNorm kernel of its own, then the two kernels of ser_mlp_head_v (hidden units with the ReLU at
 * their store, outputs without a LayerNorm): p [B, ldp], gamma / beta [K], W1 [H1, K],
 * b1 [H1], W2 [n_out, H1], b2 [n_out], workspaces xn [B, K] and hidden [B, H1], out [B, n_out], all fp32; float64 accumulation.
 * K % 4 == 0, K <= 4096, 1 <= n_out <= 8, xn and W1 16-byte aligned. */
typedef struct ser_fusion_cls_args {
    const float* p; int64_t ldp;
    const float* gamma; const float* beta;
    const float* W1; const float* b1; const float* W2; const float* b2;
    float* xn; float* hidden; float* out;
    float eps;
    int32_t B, K, H1, n_out, reserved0;
} ser_fusion_cls_args;
int ser_fusion_cls_v(const ser_fusion_cls_args* args, void* stream);

/* a25 (added under ABI 18: new entry points, ser_cmd members and SER_OP codes only; nothing existing changed)  The Whisper decoder's step
 * (HF modeling_whisper.py WhisperDecoder; the reference's transcripts: test/Whisper transcriptions.ipynb): the three kernels of a decode
 * step that are neither a GEMM nor a LayerNorm.  All sequences of a batch stand at the same position, which lives in device memory
 * (`pos`, int32 [1]): a step takes ids[:, pos] to ids[:, pos + 1] with no host decision and no pointer that changes between steps, so its
 * launches are command-list ops and a recorded step is replayed as it is.  No atomics on float data; a sequence's result does not depend on
 * the batch around it.
 *
 * ser_dec_embed_v: out[b] = embed_tokens[ids[b, *pos]] + embed_positions[*pos], fp32 rows (one exact fp32 add per element).  ids int32
 * [B, ld_ids >= max_pos]; tables fp32 [vocab, D] / [max_pos, D], 16-byte aligned; D % 4 == 0.  An id or position outside its table reads
 * the nearest valid row (never out of bounds; ser_dec_select_v is what reports a position that left the buffer). */
typedef struct ser_dec_embed_args {
    const int32_t* ids; int64_t ld_ids;
    const int32_t* pos;
    const float* embed_tokens; const float* embed_positions;
    float* out; int64_t ldo;
    int32_t B, D, vocab, max_pos;
} ser_dec_embed_args;
int ser_dec_embed_v(const ser_dec_embed_args* args, void* stream);

/* ser_dec_attn_v: one query per (sequence, head) over the first len[b] rows of that sequence's K / V cache:
 *   ctx[b, h] = sum_j softmax_j(scale q_h . K_h[j]) V_h[j],   j < len[b] = len_add + (lens ? lens[b * lens_stride] : 0), clamped to [1, max_len]
 * q [B, ldq], the caches (row j of sequence b at cache + b * batch_stride + j * ldc) and all arithmetic are fp32; online softmax in base 2;
 * head h is columns 64 h .. 64 h + 63 (dh == 64, the head dim of every Whisper size).  Rows at or beyond len[b] are never read.
 *   self-attention:  lens = the position word, lens_stride = 0, len_add = 1; k_new / v_new [B, ld_new] = this step's k and v rows (columns of
 *     the packed projection's fp32 output).  The block of (b, h) stores its own 64 columns of both at row len[b] - 1 -- the append -- and
 *     reads them from k_new / v_new, not back from the cache; no other block touches those columns.
 *   cross-attention: lens = NULL, len_add = the encoder's row count, k_new = v_new = NULL (nothing is appended).
 * One block per (head, sequence): 16 groups of 16 lanes, group g takes keys g, g + 16, ..., a lane owns 4 columns (16-byte loads, K / V straight
 * to registers); the 16 partial results are merged in ascending group order.  The order of every sum is a function of len[b] alone.
 * out_act: ctx [B, ldo_act] as GEMM operand planes in `mode` (SER_MODE_BF16, FP32X or FP16X; FP16X reports into range_flag, may be NULL).
 * q, k_new, v_new and the caches 16-byte aligned, pitches and batch_stride multiples of 4, batch_stride >= max_len * ldc when B > 1. */
typedef struct ser_dec_attn_args {
    const float* q; int64_t ldq;
    const float* k_new; const float* v_new; int64_t ld_new;
    float* kcache; float* vcache; int64_t ldc; int64_t batch_stride;
    const int32_t* lens; int32_t lens_stride, len_add;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag;
    float scale;
    int32_t B, H, dh, max_len, mode;
} ser_dec_attn_args;
int ser_dec_attn_v(const ser_dec_attn_args* args, void* stream);

/* ser_dec_select_v: the greedy choice of a step and its bookkeeping.  With p = *pos, per row b (one block per row, wave reductions):
 *   finished[b]            -> token = pad
 *   forced[p] >= 0         -> token = forced[p]                                    (logits are not read: the host may skip their launches)
 *   else                   -> token = argmax_{v < V} (logits[b, v] + mask[phase[p], v]), the lowest index on a tie (torch.argmax)
 * mask fp32 [3, ldm]: rows 0 steady, 1 first generated position, 2 language set (0 or -inf); columns >= V of logits (the padded
 * vocabulary) are never read.  Writes ids[b, p + 1] = token, margin[b, p] = the top-1 minus top-2 masked logit (+inf where nothing was
 * decided: forced or finished rows, or a single unmasked token); token == eos sets finished[b].  The block that finishes last stores the count
 * of unfinished rows to *unfinished and advances *pos (integer tickets in `work`, int32 [2], zero before the first launch and left zero).
 * *err (ORed): bit 0 = a winning masked logit was not finite (a NaN counts as the winner) -- the batch fails, as with the range guard,
 * never a silent token; bit 2 = p + 1 >= max_pos (nothing is written).  ids int32 [B, ld_ids >= max_pos], margin [B, ld_margin >= max_pos - 1],
 * phase / forced int32 [max_pos]. */
typedef struct ser_dec_select_args {
    const float* logits; int64_t ldl;
    const float* mask; int64_t ldm;
    const int32_t* phase; const int32_t* forced;
    int32_t* ids; int64_t ld_ids;
    int32_t* finished;
    float* margin; int64_t ld_margin;
    int32_t* pos; int32_t* unfinished; int32_t* work;
    uint32_t* err;
    int32_t B, V, eos, pad, max_pos, reserved0;
} ser_dec_select_args;
int ser_dec_select_v(const ser_dec_select_args* args, void* stream);

/* a26 (added under ABI 18: new entry points, ser_cmd members and SER_OP codes only; nothing existing changed)  The prosody stream: the
 * NaturalSpeech 3 / FACodec feature the reference's three-stream heads read as their third input (preprocessing/preprocess_ns3_prosody.py;
 * src/ns3/facodec.py get_prosody_feature / get_processed_style_embedding).  Of that model only a 20-bin log-mel, melspec_linear, the four
 * pre-LayerNorm layers of melspec_encoder and the first quantizer reach the saved tensor.  Three kernels are its own; the layers run on
 * ser_layernorm_v, ser_gemm and ser_attention_v.
 *
 * ser_prosody_mel_v: packed ragged waveforms -> log-mel rows and layer 0's input rows.  Utterance b (n = sample_offs[b + 1] - sample_offs[b]
 * samples, n >= 400: the CALLER's check) has T = n / 200 + 1 = frame_offs[b + 1] - frame_offs[b] frames: the reference zero-pads to 200 T
 * samples, reflect-pads 412 each side and runs torch.stft(n_fft 1024, hop 200, win 800, center=False), so frame t is the 800 samples
 * 200 t - 300 .. 200 t + 499 of the zero-padded wave, mirrored at 0 and at 200 T - 1, under the periodic Hann window.  Per frame:
 *   X[k] = sum_j x[j] dft[j][k]     dft [800][n_bins] pairs of float64 (w[j] cos, -w[j] sin)(2 pi k (j + 112) / 1024), built by the host
 *   mel[m] = log(max(sum_k melw[m][k] sqrt(re^2 + im^2 + 1e-9), 1e-5))       melw fp32 [n_mels][n_bins]: rows of the Slaney basis over its
 *                                                                             non-zero bins (n_bins <= 64, n_mels <= 32)
 * all in float64 with ascending j / k, rounded to fp32 once -> mel_out [rows][n_mels] (may be NULL).  With out != NULL also
 *   out[row][d] = lin_b[d] + sum_m lin_w[d][m] * mel[m]   (fp32 FMAs on the rounded log-mel, ascending m; lin_b carries the position-0
 *   encoding the reference adds to every frame).  max_frames (the longest T) sizes the grid; B <= 65535.  A frame's result depends on its
 *   own utterance alone. */
typedef struct ser_prosody_mel_args {
    const float* wav; const int64_t* sample_offs; const int32_t* frame_offs;
    const double* dft; const float* mel;
    const float* lin_w; const float* lin_b;
    float* mel_out;
    float* out; int64_t ldo;
    int32_t B, max_frames, n_bins, n_mels, D, reserved0;
} ser_prosody_mel_args;
int ser_prosody_mel_v(const ser_prosody_mel_args* args, void* stream);

/* ser_fvq_v: one factorized quantizer's lookup (src/ns3/quantize/fvq.py decode_latents + out_proj) on fp32 rows z [rows][ldz]:
 *   z_e = w_in z + b_in (w_in fp32 [8][D], weight norm folded);  e = z_e / max(|z_e|, 1e-12);
 *   idx = argmin_n |e|^2 - 2 e . codes[n] + |codes[n]|^2      codes fp32 [n_codes][8], L2-normalised by the host; the lowest n on a tie;
 *   gap = second smallest distance - smallest (fp32; +inf with one code);  out row = table[idx]   table fp32 [n_codes][ld_table] =
 *   out_proj of the RAW code, built once at load.
 * One wave per row, float64 products and sums.  Writes idx (int32 [rows]), gap ([rows], may be NULL), the row as out_f32 and / or as
 * operand planes out_act in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X; the fp16 formats report into range_flag, may be NULL).  A row
 * whose z_e is not finite ORs bit 0 into *err (may be NULL) and takes code 0: the batch fails, as with ser_dec_select_v's error word.
 * D % 4 == 0, D <= 2048, code_dim == 8, pitches multiples of 4, everything 16-byte aligned. */
typedef struct ser_fvq_args {
    const float* z; int64_t ldz;
    const float* w_in; const float* b_in;
    const float* codes;
    const float* table; int64_t ld_table;
    int32_t* idx; float* gap;
    float* out_f32; int64_t ldo_f32;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag; uint32_t* err;
    int32_t rows, D, n_codes, code_dim, mode, reserved0;
} ser_fvq_args;
int ser_fvq_v(const ser_fvq_args* args, void* stream);

/* ser_act_rows_v: fp32 rows x [rows][ldx] -> GEMM operand planes in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X) at row out_rowmap[m]
 * (NULL: m), with relu == 1 as max(x, 0): the ReLU between the prosody encoder's FC1 (a k = 5 convolution, run as an implicit ser_gemm)
 * and FC2 (src/ns3/transformer.py TransformerFFNLayer), and LayerNorm 2's rows into that convolution's zero-halo'd operand copy.  Wave
 * per row; D % 4 == 0, D <= 2048, pitches multiples of 4.  range_flag: the fp16 range guard, may be NULL. */
typedef struct ser_act_rows_args {
    const float* x; int64_t ldx;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    const int32_t* out_rowmap;
    uint32_t* range_flag;
    int32_t relu, mode, rows, D;
} ser_act_rows_args;
int ser_act_rows_v(const ser_act_rows_args* args, void* stream);

/* a27 (added under ABI 18: new entry points, ser_cmd members and SER_OP codes only; nothing existing changed)  The speaker half of the
 * reference's 512-wide third stream (preprocessing/preprocess_ns3_prosody_speaker.py:41-60 saves cat(prosody rows, timbre rows)):
 * FACodecEncoderV2.block (src/ns3/facodec.py), the waveform-rate stack conv_in -> four EncoderBlocks (three ResidualUnits of dilation 1, 3, 9,
 * an activation, a strided convolution C -> 2 C) -> activation -> k = 3 convolution, every convolution weight-normed with zero padding, every
 * activation an alias-free SnakeBeta (src/ns3/alias_free_torch Activation1d).  On rows x[0 .. T-1] of one utterance, per channel c, with the
 * 12 Kaiser-sinc taps f (`taps`, fp32 [12]), ea = e^alpha_c and ib = 1 / (e^beta_c + 1e-9) folded by the host:
 *   u[m] = 2 sum_i xp[i] f[m + 15 - 2 i]                  xp = x replicate-padded by 5 a side, m = 0 .. 2 T - 1
 *   s[m] = u[m] + sin(u[m] ea)^2 ib                       accurate sinf
 *   Act(x)[t] = sum_k sp[2 t + k] f[k]                    sp = s replicate-padded by (5, 6), t = 0 .. T - 1
 * Both clamps act at every utterance's own ends; Act(x)[t] reaches x[t - 6 .. t + 6].  Layout: channels-last fp32 rows of a packed ragged
 * batch, utterance b = rows offs[b] .. offs[b + 1] - 1 (offsets on the device).  All three kernels use fp32 FMAs in a fixed order --
 * ascending tap, then ascending input channel -- whatever the numerics mode, and tile each utterance from its own first row, so a batched
 * run is bit-equal to a batch of one.  Routing is by input channels: a convolution with C_in % 64 == 0 is ser_snake_v + ser_gemm (its
 * operand copy in a zero-halo'd layout supplies the padding), every narrower one (C_in 1, 8, 16, 32) goes through the two narrow kernels.
 * Narrow weights are K-MAJOR: w[(tap * C_in + c) * C_out + n] -- the transpose of ser_gemm's [N][K] -- so that the 4 output channels a
 * thread owns are one 16-byte load.
 *
 * ser_codec_unit_v: one whole ResidualUnit per launch,  y = x + W1 Act2(conv_k_d(Act1(x)) + b7) + b1,  C = 8, 16, 24 or 32, k odd <= 7,
 * dilation d <= 9 (padding (k / 2) d).  A block takes SER_CODEC_TILE rows of one utterance; Act1(x), the convolution's output and
 * Act2 of it exist only in LDS, on a halo of (k / 2) d + 12 rows a side: nothing between x and y goes to HBM.  y must not alias x.
 * max_rows = the longest utterance (sizes the grid); rows = the row count of x and y (only validated: 0 <= max_rows <= rows). */
#define SER_CODEC_TILE 128
typedef struct ser_codec_unit_args {
    const float* x; float* y;
    const int32_t* row_offs;
    const float* taps;
    const float* ea1; const float* ib1;
    const float* w7; const float* b7;
    const float* ea2; const float* ib2;
    const float* w1; const float* b1;
    int32_t B, C, k, dilation, max_rows, rows;
} ser_codec_unit_args;
int ser_codec_unit_v(const ser_codec_unit_args* args, void* stream);

/* ser_codec_conv_v: the narrow strided convolution, with Activation1d fused on its input when ea != NULL:
 *   y[t][n] = bias[n] + sum_tap sum_c w[(tap C_in + c) C_out + n] v[t stride - pad + tap][c],   v = Act(x) or x, zero outside [0, L)
 * for t < T_out = out_offs[b + 1] - out_offs[b] (the caller's count; the codec's levels divide exactly), where L = in_offs[b + 1] -
 * in_offs[b] is the utterance's input length: the activation's clamps act at 0 and L - 1.  int64 input offsets: conv_in (no activation,
 * C_in = 1) reads the packed, UNPADDED waveform and writes the padded length's rows -- the zeros the reference pads the wave with are the
 * zeros beyond L.
 * C_in 1, 8, 16 or 32; C_out % 8 == 0; k <= 16; stride <= 8.  A block takes SER_CODEC_TILE / stride output rows.  y fp32 [rows][ldy]. */
typedef struct ser_codec_conv_args {
    const float* x;
    const int64_t* in_offs; const int32_t* out_offs;
    const float* taps; const float* ea; const float* ib;
    const float* w; const float* bias;
    float* y; int64_t ldy;
    int32_t B, C_in, C_out, k, stride, pad, max_out_rows, rows;
} ser_codec_conv_args;
int ser_codec_conv_v(const ser_codec_conv_args* args, void* stream);

/* ser_snake_v: Activation1d for the wide levels (C % 64 == 0), as the producer of ser_gemm's operand copy: Act(x) of fp32 rows x [rows][ldx]
 * -> operand planes out_act in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X) at row out_rowmap[m] (NULL: m) -- a zero-halo'd layout whose
 * rows between utterances are the caller's zeros and are never written -- and / or the fp32 value out_f32 at row m.  The fp16 formats
 * report every value they round into range_flag (may be NULL; see ser_gemm_args.range_flag). */
typedef struct ser_snake_args {
    const float* x; int64_t ldx;
    const int32_t* row_offs;
    const float* taps; const float* ea; const float* ib;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    const int32_t* out_rowmap;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    int32_t B, C, max_rows, rows, mode, reserved0;
} ser_snake_args;
int ser_snake_v(const ser_snake_args* args, void* stream);

/* a28 (added under ABI 18: new entry points, ser_cmd members and SER_OP codes only; nothing existing changed)  w2v-BERT 2.0
 * (HF Wav2Vec2BertModel behind SeamlessM4TFeatureExtractor), an encoder the reference does not ship but its heads take like any other
 * [T, D] stream: a Kaldi fbank front end, conformer layers, a relative-key attention bias.  Five kernels are its own; everything else runs on
 * ser_layernorm_v and ser_gemm.  Every kernel is a plain grid (no inter-block waits, no atomics on float data), every sum runs in an order
 * fixed by the utterance alone (a batched run is bit-equal to a batch of one), every fp16 operand plane reports into range_flag.
 *
 * ser_fbank_v: packed ragged waveforms -> normalised, stacked fp32 rows.  Utterance b (n = sample_offs[b + 1] - sample_offs[b] >= 400
 * samples: the CALLER's check) has F = 1 + (n - 400) / 160 = mel_offs[b + 1] - mel_offs[b] frames (400 samples, hop 160, no centring) and
 * T = F / stride = frame_offs[b + 1] - frame_offs[b] rows.  Per frame, with x = 2^15 wav:
 *   y[j] = x[j] - mean(x);   z[j] = y[j] - 0.97 y[j - 1],  z[0] = (1 - 0.97) y[0];
 *   X[k] = sum_j z[j] dft[j][k]       dft [400][257] pairs of float64 (w[j] cos, -w[j] sin)(2 pi k j / 512), w = the Povey window (host)
 *   mel[m] = log(max(sum_k melw[m][k] |X[k]|^2, 1.192092955078125e-07))   melw float64 [n_mels][257], summed over k in mel_range[m][0 .. 1)
 * all in float64 with ascending j / k, rounded to fp32 once -> work [total frames][n_mels].  A second launch takes, per utterance and mel
 * bin, the mean and the unbiased variance over ALL F frames (float64, a fixed order) and writes
 *   out[row][s n_mels + m] = (mel[stride row + s][m] - mean_m) / sqrt(var_m + 1e-7),     s < stride, row < T
 * (an odd last frame counts for the statistics and has no row).  n_mels <= 128, 1 <= stride <= 4, ldo >= stride n_mels; B <= 65535;
 * max_mel_frames (the longest F) sizes the grids. */
typedef struct ser_fbank_args {
    const float* wav; const int64_t* sample_offs; const int32_t* mel_offs; const int32_t* frame_offs;
    const double* dft; const double* melw; const int32_t* mel_range;
    float* work;
    float* out; int64_t ldo;
    int32_t B, max_mel_frames, n_mels, stride;
} ser_fbank_args;
int ser_fbank_v(const ser_fbank_args* args, void* stream);

/* ser_relkey_table_v: the query side of the relative-key bias (HF Wav2Vec2BertSelfAttention, position_embeddings_type "relative_key"):
 *   qe[(m H + h) ld_qe + p] = sum_d q_h[m][d] E[p][d],    p < P = left_max + right_max + 1
 * in fp32 FMAs with ascending d, q read where the packed projection left it (column block q_col of the operand planes qkv in `mode`:
 * hi, or hi + lo, as fp32) -- so qe carries the dh^-0.5 log2 e the projection's epilogue gave q.  E fp32 [P][dh]: distance_embedding, shared
 * by all heads.  Modes SER_MODE_BF16 / FP32X / FP16X; dh % 8 == 0, dh <= 128, P <= 128, H dh <= 2048, ld_qe >= P. */
typedef struct ser_relkey_table_args {
    const void* qkv; int64_t ld; int64_t plane_stride;
    const float* E;
    float* qe; int64_t ld_qe;
    int32_t q_col, rows, H, dh, P, mode;
} ser_relkey_table_args;
int ser_relkey_table_v(const ser_relkey_table_args* args, void* stream);

/* ser_attention_rk_v: ser_attention_v's tiled attention with the relative-key bias added to every logit,
 *   out[q, :] = softmax_k( q.k + qe[(q H + h) ld_qe + clamp(k - q, -left_max, right_max) + left_max] ) v,
 * as further instantiations of the same kernel: `base` is an ser_attention_args with a pre-scaled q (scale <= 0), head dim 64, no table,
 * gate, key_lens, bias2d or FP16M output; modes SER_MODE_BF16 / FP32X / FP16X.  The S accumulators start at the bias instead of at zero,
 * so with E = 0 the result is bit-equal to ser_attention_v's low-occupancy form on the same operands.  A key tile wholly left of q - left_max
 * or wholly right of q + right_max for all 32 queries of a wave adds one constant per query; only tiles that cross the band gather. */
typedef struct ser_attention_rk_args {
    ser_attention_args base;
    const float* qe; int64_t ld_qe;
    int32_t left_max, right_max;
} ser_attention_rk_args;
int ser_attention_rk_v(const ser_attention_rk_args* args, void* stream);

/* ser_conformer_conv_v: the middle of the conformer convolution module (HF Wav2Vec2BertConvModule) between its two pointwise GEMMs:
 *   g[t][c] = y[t][c] sigmoid(y[t][D + c])                                  GLU of pointwise-1's fp32 output y [rows][ldy >= 2 D]
 *   u[t][c] = sum_k w[k][c] g[t - (K - 1) + k][c]                           causal depthwise convolution: rows before the utterance's
 *                                                                           first (frame_offs) are zeros, never the previous utterance's
 *   out[t]  = swish(LayerNorm_D(u[t]) gamma + beta)                         -> operand planes of pointwise-2's input, in `mode`
 * fp32 FMAs in ascending k, accurate expf, two-pass LayerNorm statistics in a fixed order.  w fp32 [K][D] (the checkpoint's [D][1][K]
 * transposed by the host).  A block takes SER_CCONV_TILE rows of one utterance and computes the GLU of each input row once.
 * D % 4 == 0, D <= 2048, K odd <= 31; pitches multiples of 4.  Modes SER_MODE_BF16 / FP32X / FP16 / FP16X. */
#define SER_CCONV_TILE 8
typedef struct ser_conformer_conv_args {
    const float* y; int64_t ldy;
    const float* w; const float* gamma; const float* beta;
    const int32_t* frame_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag;
    float eps;
    int32_t B, D, K, max_frames, rows, mode, reserved0;
} ser_conformer_conv_args;
int ser_conformer_conv_v(const ser_conformer_conv_args* args, void* stream);

/* ser_swish_rows_v: fp32 rows x [rows][ldx] -> x sigmoid(x) as GEMM operand planes in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X): the
 * activation between the two GEMMs of a conformer feed-forward block, ser_act_rows_v's counterpart.  Wave per row; D % 4 == 0, D <= 2048 per
 * 2048-column slab (wider rows take further slabs: D <= 8192), pitches multiples of 4.  range_flag: the fp16 range guard, may be NULL. */
typedef struct ser_swish_rows_args {
    const float* x; int64_t ldx;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag;
    int32_t mode, rows, D, reserved0;
} ser_swish_rows_args;
int ser_swish_rows_v(const ser_swish_rows_args* args, void* stream);

/* a34 (added under ABI 18: new entry points, two ser_cmd members and two SER_OP codes only; ser_dec_attn_v, ser_dec_select_v and every
 * existing layout are unchanged)  Whisper beam search: HF's GenerationMixin._beam_search for do_sample = False, early_stopping = False,
 * num_return_sequences = 1 and one eos token, restated with masks (tests/whisper_beam_ref.py is the float64 statement).  K beams of B
 * utterances are the B K rows of one decode step; row b K + k is beam k of utterance b.
 *
 * ser_dec_attn_beam_v (SER_OP_DEC_ATTN_BEAM): ser_dec_attn_v's arithmetic, statement for statement, with the cache row of a key found
 * through a table or a divisor.  `base` is read as by ser_dec_attn_v except that kcache / vcache + r * batch_stride is PHYSICAL row r:
 *   src != NULL  (self-attention) key j < len - 1 of logical row b lies in physical row src[parity][b][j], parity = (len - 1) & 1; int32
 *                [2][B][ld_src >= max_len], the halves src_parity_stride words apart; an entry outside [0, B) is clamped.  Row b appends
 *                its step's k / v at ITS OWN physical row b, position len - 1, and reads them from k_new / v_new.  With the identity table
 *                the result equals ser_dec_attn_v's bit for bit.
 *   src == NULL  (cross-attention) row b reads physical row b / row_div: K beams share their utterance's cross cache; nothing is appended.
 * Keys and values never move: what a step reorders is the table (ser_beam_select_v), B K p small integers.
 *
 * ser_beam_select_v (SER_OP_BEAM_SELECT): one step of the rule for every utterance.  With p = *pos, cur = p + 1 tokens per row:
 *   scores   logp = z - logsumexp(z) over the RAW logits z (fp32) of a row, float64: suppressed tokens count in the normaliser.  Then the
 *            mask row mask[phase[p]] (0 / -inf, as ser_dec_select_v's); then + run[b][k], the running score (-inf: a dead beam; the first
 *            step starts from [0, -inf, ...], HF's [0, -1e9, ...]).
 *   top 2K   of the K V scores; the larger first, on a tie the lower flat index k V + token.  parent = index / V, token = index % V.
 *   hit      token == eos, or cur + 1 >= max_length.
 *   running  the best K candidates that did not hit, in rank order; missing ones are dead rows (parent = own index, token = pad).
 *   finished only candidates of rank < K that hit, and only while the flag is up: score / lenpow[cur + 1 - prompt_len], merged into the
 *            K best kept in descending order (an older entry wins a tie); handle = (p, rank) into the trace.
 *   flag     sticky AND: with K finished, run'[0] / lenpow[cur + 1 - prompt_len] > the worst finished score; untouched before that.
 *   done     the flag dropped, or every candidate hit.  A done utterance is frozen: its rows keep stepping with identity parents and pad.
 * lenpow [max_pos + 1] float64: n ^ length_penalty, tabulated by the host so that the device divides by the very number numpy does.
 * State (device, across steps; the host zeroes it and sets run and flag = 1): run, fin_score [B][K] float64, fin_handle [B][K][2],
 * state [B][4] = (n finished, flag, done, the position at which done was set).  Per step, indexed by p: trace_run [max_pos][B][K][2]
 * (parent, token) of the new running rows (parent -1 where the utterance was frozen), trace_cand [max_pos][B][2K][2] and cand_score
 * [max_pos][B][2K] of the candidates (-1 where there was none), gaps [max_pos][B] float64: the smallest gap of a comparison that decided
 * the step (the cut at rank 2K, the cut behind the K-th candidate that did not hit, rank K - 1 against K when either hit, the finished
 * merge against the worst kept, both sides of the flag's comparison; +inf where none applied).  Also writes ids[b K + r][p + 1], the
 * ancestor table's other half (src'[r][j] = src[parent(r)][j] for j < p, src'[r][p] = parent(r); src may be NULL), *unfinished = the count
 * of utterances not done, and advances *pos last (ser_dec_select_v's tickets; `ticket` int32 [2], zero before the first launch).
 * *err (ORed): bit 0 a winning score that is not finite (a NaN logit wins), bit 2 p + 1 >= max_pos (nothing is written), bit 3 fewer
 * than 2K finite candidates.  After an error bit only the error word is specified: the batch fails.
 * Two launches.  Scan, blocks (chunk, beam, utterance) over SER_BEAM_CHUNK columns: the chunk's (max, sum exp) in float64 and its top 2K + 1
 * masked logits (inside a row the order of the logits is the order of the scores).  Merge, one block per utterance: log-sum-exp from the
 * partials in chunk order, the best 2K + 1 scores, the bookkeeping on one thread, the table copy on all.  Every order of a sum is a
 * function of V alone; no atomics on data: an utterance's bits do not depend on B or on what shares the batch.  Every index read from
 * device memory is clamped before use and every loop is bounded by a launch argument.  work: ser_beam_work_bytes(B, K, V) bytes, 8-byte
 * aligned (-1 for sizes ser_beam_select_v refuses: K outside 2..SER_BEAM_MAX_K, V < 2 K or beyond SER_BEAM_MAX_CHUNKS chunks). */
#define SER_BEAM_MAX_K 8
#define SER_BEAM_MAX_CAND 17
#define SER_BEAM_CHUNK 4096
#define SER_BEAM_MAX_CHUNKS 13
#define SER_BEAM_ERR_NONFINITE 1
#define SER_BEAM_ERR_POSITION 4
#define SER_BEAM_ERR_CANDIDATES 8
typedef struct ser_dec_attn_beam_args {
    ser_dec_attn_args base;
    const int32_t* src; int64_t src_parity_stride;
    int32_t ld_src, row_div;
} ser_dec_attn_beam_args;
int ser_dec_attn_beam_v(const ser_dec_attn_beam_args* args, void* stream);
typedef struct ser_beam_select_args {
    const float* logits; int64_t ldl;
    const float* mask; int64_t ldm;
    const int32_t* phase;
    const double* lenpow;
    int32_t* ids; int64_t ld_ids;
    int32_t* src; int64_t src_parity_stride;
    double* run; double* fin_score; int32_t* fin_handle; int32_t* state;
    int32_t* trace_run; int32_t* trace_cand; double* cand_score; double* gaps;
    void* work; int64_t work_bytes;
    int32_t* pos; int32_t* unfinished; int32_t* ticket;
    uint32_t* err;
    int32_t B, K, V, eos, pad, max_pos, max_length, prompt_len, ld_src, reserved0;
} ser_beam_select_args;
int ser_beam_select_v(const ser_beam_select_args* args, void* stream);
int64_t ser_beam_work_bytes(int32_t B, int32_t K, int32_t V);

/* a35 (added under ABI 18: new entry points, four ser_cmd members and four SER_OP codes only; every existing layout and kernel is
 * unchanged)  The wav2vec2-conformer encoders (HF Wav2Vec2ConformerModel: facebook/wav2vec2-conformer-{rope,rel-pos}-large): wav2vec2's
 * convolutional stem and feature projection, then conformer layers
 *   x += FFN1(LN x) / 2;  x += Attn(LN x);  x += Conv(x);  x += FFN2(LN x) / 2;  x = LN x
 * with hidden_states[i < L] = the input of layer i and hidden_states[L] = encoder.layer_norm of the last layer's output; no positional
 * convolution.  Two position schemes and a convolution module of their own; the rest runs on a28's kernels, ser_layernorm_v, ser_gemm and
 * ser_attention_v.  Every kernel is a plain grid, every sum runs in an order fixed by the utterance alone (a batched run is bit-equal to a
 * batch of one), every fp16 operand plane reports into range_flag.  tests/w2vconf_ref.py is the float64 statement.
 *
 * Rotary ("rotary").  The layer-normed rows are rotated BEFORE linear_q and linear_k; linear_v reads the un-rotated rows.  With t = the
 * row's frame index INSIDE its utterance, dh the head dim and c a channel of a head,
 *   x'[c] = x[c] cos[t][c] + (c < dh / 2 ? -x[c + dh / 2] : x[c - dh / 2]) sin[t][c]
 *   cos[t][c] = cos(t inv_freq[c mod dh / 2]),  inv_freq[i] = 1 / base^(2 i / dh) held in fp32 (HF's buffer)
 * The tables are built by the HOST: float64 products of t with the fp32 inv_freq, cos / sin in float64, rounded once to fp32.
 * ser_rope_rows_v: fp32 rows x [rows][ldx] -- the OUTPUT of ser_layernorm_v, which also writes the plain operand planes linear_v reads; the
 * kernel applies no norm -- to the rotated rows as operand planes in `mode` (SER_MODE_BF16 / FP32X / FP16 / FP16X).  One product, one FMA
 * per element: x' = fma(x_pair, sin, x cos).  Wave per row; the row's utterance b is found by bisection of frame_offs [B + 1], the
 * position is row - frame_offs[b] < table_T (a position beyond the table is an argument error of the caller: max_frames <= table_T is
 * checked, and the kernel clamps).  D % dh == 0, dh % 8 == 0, D % 4 == 0, D <= 2048; pitches multiples of 4. */
typedef struct ser_rope_rows_args {
    const float* x; int64_t ldx;
    const float* cos_t; const float* sin_t;
    const int32_t* frame_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag;
    int32_t B, rows, D, dh, table_T, max_frames, mode, reserved0;
} ser_rope_rows_args;
int ser_rope_rows_v(const ser_rope_rows_args* args, void* stream);

/* ser_conformer_conv_bn_v: the middle of this family's convolution module (HF Wav2Vec2ConformerConvolutionModule) between its two
 * pointwise GEMMs -- ser_conformer_conv_v's block shape with a CENTRED window and BatchNorm1d in eval in LayerNorm's place:
 *   g[t][c] = y[t][c] sigmoid(y[t][D + c])                                  GLU of pointwise-1's fp32 output y [rows][ldy >= 2 D]
 *   u[t][c] = sum_k w[k][c] g[t - (K - 1) / 2 + k][c]                       rows outside the utterance (frame_offs) are zeros on BOTH
 *                                                                           sides, never a neighbouring utterance's
 *   out[t]  = swish(fma(u[t][c], scale[c], shift[c]))                       -> operand planes of pointwise-2's input, in `mode`
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean scale: folded by the host in float64, rounded once.  fp32 FMAs in
 * ascending k, accurate expf.  w fp32 [K][D].  D % 4 == 0, D <= 2048, K odd <= 31; pitches multiples of 4.  Modes BF16 / FP32X / FP16 / FP16X. */
typedef struct ser_conformer_conv_bn_args {
    const float* y; int64_t ldy;
    const float* w; const float* scale; const float* shift;
    const int32_t* frame_offs;
    void* out_act; int64_t ldo_act; int64_t out_plane_stride;
    uint32_t* range_flag;
    int32_t B, D, K, max_frames, rows, mode;
} ser_conformer_conv_bn_args;
int ser_conformer_conv_bn_v(const ser_conformer_conv_bn_args* args, void* stream);

/* Relative ("relative", Transformer-XL).  With i, j the frame indices of query and key inside their utterance,
 *   scores[i][j] = ((q_i + u_h) . k_j + (q_i + v_h) . P_h(i - j)) / sqrt(dh),     P(r) = linear_pos(pe(r)) (no bias),
 *   pe(r)[0::2] = sin(r div), pe(r)[1::2] = cos(r div), div = exp(arange(0, D, 2) (-ln 10000 / D));   r > 0: the key is to the left
 * (HF's zero-pad / view / slice "shift" is exactly this index).  P depends on the distance alone.  The host folds u into linear_q's bias
 * (the projection emits q + u, scaled by dh^-0.5 log2 e through ser_gemm's col_scale) and passes off_h = (v_h - u_h) dh^-0.5 log2 e.
 * ser_relpos_bias_v: for every row m of utterance b (i = m - frame_offs[b], T = the utterance's frames) and head h
 *   pb[(m H + h) ld_pb + j] = sum_d (q_h[m][d] + off_h[d]) P[(P_T + i - j) ldp + h dh + d]       j < T;      0 for T <= j < 64 ceil(T / 64)
 * fp32 in the exp2 domain (q carries the scale), q read from the packed projection's planes as fp32 (hi, or hi + lo: ser_relkey_table_v's
 * arithmetic), one rounding of q + off, fp32 FMAs in ascending d.  P fp32 [2 P_T][ldp], row P_T + r = P(r) for -P_T <= r < P_T;
 * max_frames <= P_T.  A block takes 32 query rows x 64 keys of one (utterance, head) and stages the 95 rows of P_h they need in LDS.
 * dh == 64, B H <= 65535, ld_pb % 64 == 0 and >= 64 ceil(max_frames / 64).  Modes SER_MODE_BF16 / FP32X / FP16X. */
typedef struct ser_relpos_bias_args {
    const void* qkv; int64_t ld; int64_t plane_stride;
    const float* P; int64_t ldp;
    const float* off;
    const int32_t* frame_offs;
    float* pb; int64_t ld_pb;
    int32_t q_col, B, H, dh, P_T, max_frames, rows, mode;
} ser_relpos_bias_args;
int ser_relpos_bias_v(const ser_relpos_bias_args* args, void* stream);

/* ser_attention_rb_v: ser_attention_rk_v's kernel with a per-(query row, head) bias ROW indexed by the key's index in its utterance,
 *   out[q, :] = softmax_k( q.k + pb[(q H + h) ld_pb + k] ) v,
 * a further instantiation of the same kernel behind `base` (as ser_attention_rk_v reads it: pre-scaled q, head dim 64, no table, gate,
 * key_lens, bias2d or FP16M output; modes BF16 / FP32X / FP16X).  The S accumulators start at the bias, so with pb = 0 the result is
 * bit-equal to ser_attention_v's low-occupancy form.  pb 16-byte aligned, ld_pb % 64 == 0 and >= 64 ceil(max_frames / 64); a row is read
 * up to 64 ceil(T / 64) entries, which ser_relpos_bias_v leaves finite. */
typedef struct ser_attention_rb_args {
    ser_attention_args base;
    const float* pb; int64_t ld_pb;
} ser_attention_rb_args;
int ser_attention_rb_v(const ser_attention_rb_args* args, void* stream);

/* a36 (added under ABI 18: one new entry point, one ser_cmd member and one SER_OP code only; ser_dec_select_v and every struct above are
 * what they were)  Whisper segment timestamps: the model's own <|0.00|> text <|6.44|> tokens, HF's generate(return_timestamps=True).
 *
 * ser_dec_select_ts_v (SER_OP_DEC_SELECT_TS): ser_dec_select_v with HF's WhisperTimeStampLogitsProcessor between the static mask and
 * the argmax -- HF's order is begin-suppress, suppress, then the timestamp processor.  One block per row; finished and forced rows, ids,
 * margin, finished, the tickets in `work`, *unfinished, *pos and the error bits are ser_dec_select_v's.  With p = *pos and
 * n = p + 1 - begin_index generated tokens (n < 0, a prompt step such as the language step: ser_dec_select_v's choice, no rule), per row b:
 *   1. x[v] = logits[b, v] + mask[phase[p], v];  x[no_ts] = -inf
 *   2. last = ids[b, p] (n >= 1), pen = ids[b, p - 1] (n >= 2);  last_ts = n >= 1 and last >= ts_begin;  pen_ts = n < 2 or pen >= ts_begin
 *      last_ts and pen_ts      -> x[ts_begin:] = -inf         (a closed pair: text follows)
 *      last_ts and not pen_ts  -> x[:eos] = -inf              (text, then a timestamp: its pair or eos follows)
 *   3. t = the LAST id >= ts_begin among ids[b, begin_index .. p] (not the largest: a teacher-forced row need not be monotone); if there is
 *      one, x[ts_begin:bound] = -inf with bound = t when last_ts and not pen_ts, else t + 1
 *   4. n == 0 -> x[:ts_begin] = -inf, and with max_initial >= 0 also x[ts_begin + max_initial + 1:] = -inf
 *   5. L = log sum_{v >= ts_begin} exp(x[v]) in float64, M = max_{v < ts_begin} x[v];  L > M -> x[:ts_begin] = -inf  (L == M keeps the text).
 *      HF compares the two log-softmax values; their difference is L - M, so the normaliser is not computed.
 *      ts_gap[b, p] = |L - M|, +inf when either side is not finite or nothing was decided
 *   6. token = argmax x, the lowest index on a tie; margin[b, p] = top-1 minus top-2 of the final x
 * The float64 sum runs over a fixed tree of (thread, wave) slots, a function of V and ts_begin alone; a row's result does not depend on
 * what shares its batch, bit for bit.  Columns >= V are never read.  *err bit 0: the winner is not finite (an all-masked row), or the row
 * holds a NaN in a column < V, live or masked (a NaN counts as +inf where it is live); bit 2 as ser_dec_select_v's.
 * 0 < ts_begin < V, 0 <= no_ts, eos < V, 1 <= begin_index < max_pos, max_initial >= -1 (-1: none); ts_gap float64 [B, ld_gap >= max_pos - 1]. */
typedef struct ser_dec_select_ts_args {
    ser_dec_select_args base;
    double* ts_gap; int64_t ld_gap;
    int32_t ts_begin, no_ts, begin_index, max_initial;
} ser_dec_select_ts_args;
int ser_dec_select_ts_v(const ser_dec_select_ts_args* args, void* stream);

/* a37 (added under ABI 18: two new entry points, two ser_cmd members and two SER_OP codes only; ser_logmel_whisper and every struct above are
 * what they were)  Whisper long-form features: HF's generate() on input longer than 30 s reads features of the WHOLE file
 * (WhisperFeatureExtractor(truncation=False)), and a window of its seek loop is a slice of them.
 *
 * ser_logmel_long_v (SER_OP_LOGMEL_LONG): B ragged files, packed fp32 samples wav with sample_offs [B + 1] (int64, device; the host's copy
 * sample_offs_host is what the launcher validates on).  With len_b the file's samples, F_b = len_b / 160 frames (the STFT has 1 + len_b / 160;
 * the last is dropped) and pitch_b = F_b rounded up to 4:
 *   p[i]      = x[reflect(i - 200)] about the file's OWN first and last sample
 *   raw[m, t] = log10(max(sum_k mel[k, m] |DFT_400(p[160 t .. 160 t + 399] hann)[k]|^2, 1e-10)),  t < F_b     (the guard's logarithm is the
 *               constant -10, as in ser_logmel_whisper: silence is exactly -1.5 after the scaling)
 *   out[bases[b] + m pitch_b + t] = (max(raw[m, t], max_{m, t < F_b} raw - 8) + 4) / 4
 * fp32 [n_mels][pitch_b] at the float offset bases[b] (int64, device, a multiple of 4) of `out` (16-byte aligned).  Columns F_b .. pitch_b - 1
 * are written too (a finite value: the image of a zero frame) and are in no maximum; nothing outside [n_mels][pitch_b] is written.
 * ser_logmel_whisper's fp64-MFMA DFT tile over 32 frames; the grid is the tile table `tiles` [n_tiles][2] (int32, device) of (file, first frame),
 * every file's tiles contiguous and ascending; `files` [B][4] (int32, device) = F_b, pitch_b, the file's first tile, its tile count.  A tile
 * writes its maximum into its own slot of `scratch` (fp32 [n_tiles + B]: no atomics, no reset), a second kernel reduces a file's slots, a third
 * scales in place: a file gives the same bits alone and in any batch.  `table`: a buffer ser_logmel_init has filled (twiddles and Hann).
 * Refused before any launch: a null pointer, B <= 0, n_mels <= 0, a file under 201 samples (numpy's reflect pad is undefined there), n_tiles or
 * max_pitch that are not what the host's offsets give. */
typedef struct ser_logmel_long_args {
    const float* wav; const int64_t* sample_offs; const int64_t* sample_offs_host;
    const float* mel;
    float* out; const int64_t* bases;
    const int32_t* tiles; const int32_t* files;
    const void* table; float* scratch;
    int32_t B, n_mels, n_tiles, max_pitch;
} ser_logmel_long_args;
int ser_logmel_long_v(const ser_logmel_long_args* args, void* stream);

/* ser_mel_window_v (SER_OP_MEL_WINDOW): the [B, n_mels, 3000] input features of B windows, gathered from ser_logmel_long_v's output `src`.
 * rows [B][5] (int64, device; rows_host: the host's copy, validated by the launcher) = base, pitch, F, seek, nf of each row:
 *   out[b, m, t] = src[base + m pitch + seek + t]   t < nf;      +0.0f   nf <= t < 3000          (HF's _get_input_segment)
 * Bit copies; seek need not be a multiple of 4.  Refused before any launch: nf outside 1 .. 3000, seek < 0, seek + nf > F, pitch < F. */
typedef struct ser_mel_window_args {
    const float* src;
    const int64_t* rows; const int64_t* rows_host;
    float* out;
    int32_t B, n_mels;
} ser_mel_window_args;
int ser_mel_window_v(const ser_mel_window_args* args, void* stream);

/* a38 (added under ABI 18: one new entry point, one ser_cmd member and one SER_OP code only; ser_dec_select_v, ser_dec_select_ts_v and every
 * struct above are what they were)  Whisper transcript scores: the log-probability of every generated token and the no-speech
 * probability, what HF's generate() thresholds (logprob_threshold, no_speech_threshold) read.
 *
 * ser_dec_select_score_v (SER_OP_DEC_SELECT_SCORE): rule == 0: ser_dec_select_v's choice and bookkeeping (ts.base alone is read);
 * rule == 1: ser_dec_select_ts_v's (all of ts).  Token, margin, ts_gap, ids, finished, the tickets in `work`, *unfinished and *pos are
 * bit for bit those of the unscored launcher on the same inputs.  One block per row.  With p = *pos, per row b also:
 *   logprob[b, p]  = x[token] - log sum_{v < V} exp(x[v]) in float64, x the PROCESSED row the choice was made from (HF's `scores`):
 *                    logits + mask[phase[p]], and under the rule also its -inf columns, step 5's among them -- when the timestamps
 *                    together outweigh the best text token the sum runs over the live timestamp columns only.  Computed around the
 *                    winner w = max x as (x[token] - w) - log sum exp(x[v] - w), whose first term is 0.  +inf where nothing was decided
 *                    (forced or finished rows), as margin.
 *   no_speech[b]   = softmax_{v < V}(logits[b, :])[no_speech_token] in float64, written by the step at p == 0 only, from the RAW row: no
 *                    mask, no rule, whether the step's token is forced or chosen (HF's WhisperNoSpeechDetection reads the unprocessed
 *                    logits of the first decoder position).  So the logits of that step must have been computed even when its token is forced.
 * The float64 sums run over a fixed tree of (thread, wave) slots, a function of V and ts_begin alone; a row's result does not depend on
 * what shares its batch, bit for bit.  Columns >= V are never read.  *err bit 0 is also set when the row at position 0 holds a NaN or an
 * infinity (no_speech is then NaN), or when a decided row's normaliser is not finite; otherwise the bits are the unscored launcher's.
 * logprob float64 [B, ld_logprob >= max_pos - 1], no_speech float64 [B], 0 <= no_speech_token < V; rule == 0 ignores ts.ts_gap (may be
 * NULL) and the four token fields of ts. */
typedef struct ser_dec_select_score_args {
    ser_dec_select_ts_args ts;
    double* logprob; int64_t ld_logprob;
    double* no_speech;
    int32_t no_speech_token, rule;
} ser_dec_select_score_args;
int ser_dec_select_score_v(const ser_dec_select_score_args* args, void* stream);

#define SER_OP_GEMM 1
#define SER_OP_ATTENTION 2
#define SER_OP_LAYERNORM 3
#define SER_OP_WAVE_FRAMES 4
#define SER_OP_ROW_CENTER 5
#define SER_OP_LOGMEL 6
#define SER_OP_PACK_ACT 7
#define SER_OP_GN_STATS 8
#define SER_OP_POS_LN 9
#define SER_OP_DEC_EMBED 10
#define SER_OP_DEC_ATTN 11
#define SER_OP_DEC_SELECT 12
#define SER_OP_PROSODY_MEL 13
#define SER_OP_FVQ 14
#define SER_OP_ACT_ROWS 15
#define SER_OP_CODEC_UNIT 16
#define SER_OP_CODEC_CONV 17
#define SER_OP_SNAKE 18
#define SER_OP_FBANK 19
#define SER_OP_RELKEY_TABLE 20
#define SER_OP_ATTENTION_RK 21
#define SER_OP_CONFORMER_CONV 22
#define SER_OP_SWISH_ROWS 23
#define SER_OP_DEC_KEEP_Q 24
#define SER_OP_DEC_ATTN_BEAM 25
#define SER_OP_BEAM_SELECT 26
#define SER_OP_ROPE_ROWS 27
#define SER_OP_CONFORMER_CONV_BN 28
#define SER_OP_RELPOS_BIAS 29
#define SER_OP_ATTENTION_RB 30
#define SER_OP_DEC_SELECT_TS 31
#define SER_OP_LOGMEL_LONG 32
#define SER_OP_MEL_WINDOW 33
#define SER_OP_DEC_SELECT_SCORE 34
typedef struct ser_cmd {
    int32_t op, reserved0;
    union {
        ser_gemm_args        gemm;
        ser_attention_args   attention;
        ser_layernorm_args   layernorm;
        ser_wave_frames_args wave_frames;
        ser_row_center_args  row_center;
        ser_logmel_args      logmel;
        ser_pack_act_args    pack_act;
        ser_gn_stats_args    gn_stats;
        ser_pos_ln_args      pos_ln;
        ser_dec_embed_args   dec_embed;
        ser_dec_attn_args    dec_attn;
        ser_dec_select_args  dec_select;
        ser_prosody_mel_args prosody_mel;
        ser_fvq_args         fvq;
        ser_act_rows_args    act_rows;
        ser_codec_unit_args  codec_unit;
        ser_codec_conv_args  codec_conv;
        ser_snake_args       snake;
        ser_fbank_args       fbank;
        ser_relkey_table_args relkey_table;
        ser_attention_rk_args attention_rk;
        ser_conformer_conv_args conformer_conv;
        ser_swish_rows_args  swish_rows;
        ser_dec_keep_q_args  dec_keep_q;
        ser_dec_attn_beam_args dec_attn_beam;
        ser_beam_select_args beam_select;
        ser_rope_rows_args   rope_rows;
        ser_conformer_conv_bn_args conformer_conv_bn;
        ser_relpos_bias_args relpos_bias;
        ser_attention_rb_args attention_rb;
        ser_dec_select_ts_args dec_select_ts;
        ser_logmel_long_args logmel_long;
        ser_mel_window_args  mel_window;
        ser_dec_select_score_args dec_select_score;
    } u;
} ser_cmd;

/* Enqueue cmds[0..n) in order on `stream`.  Stops at the first launcher that fails and returns its code
 * (ser_last_error() names it); *failed_at, if not NULL, receives the index. */
int ser_run(const ser_cmd* cmds, int32_t n, int32_t* failed_at, void* stream);

/* ---- host-side file I/O (HOST pointers, no stream; plain C, re-entrant, entered without the Python GIL) --------------
 * a5  ser_wav_read_f32: what librosa.load(path, sr=16000) -> soundfile yields for a RIFF/WAVE file
 *     (preprocessing/preprocess_speech.py:47) before any resampling: mono float32 in [-1, 1], integer PCM / 2^(bits-1),
 *     channels averaged.  Returns the number of frames, or < 0; with host_dst == NULL only the header is read.
 * a21 ser_pt_write_f32: the file torch.save(feats, "<name>.pt") leaves for the heads (preprocess_speech.py:69-71;
 *     consumer torch.load(path), bin/train_cat_bimodal_lazy_1head.py:227): a bare [rows, cols] float32 CPU tensor in
 *     torch's zip archive format. */
int64_t ser_wav_read_f32(const char* path, float* host_dst, int64_t capacity, int32_t* sample_rate, int32_t* channels);
int     ser_pt_write_f32(const char* path, const float* host_data, int64_t rows, int64_t cols);
/* ser_pt_write_f32_vec (added under ABI 18: a new entry point only): the same archive through the same writer for a 1-D [n] float32 tensor,
 * what torch.save(embeddings[0], "<utt>.pt") leaves of one utterance's x-vector (a30). */
int     ser_pt_write_f32_vec(const char* path, const float* host_data, int64_t n);

#define SER_WS_LOGMEL 1
#define SER_WS_WAVE_FRAMES 2
#define SER_WS_GN_STATS 3
size_t ser_workspace_bytes(int op, int B, int T, int D, int H, int mode);

#ifdef __cplusplus
}
#endif
#endif /* SER_HIP_H */
