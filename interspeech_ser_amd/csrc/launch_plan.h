// Launch plans of ser_gemm and ser_attention_v as plain data: argument checks, tile / kernel-form selection, grid and LDS bytes.
// Host-only C++17 without a HIP type: gemm.hip and attention.hip dispatch from what these functions return, and launch_plan_check.cc
// (plain g++, `make plan_check`; tests/test_launch_plan_host.py) pins the same functions against tests/golden/launch_plans.txt.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/ser_hip.h"

int ser_fail(int code, const char* fmt, ...);      // hosterr.hip

// Tile-selection thresholds are constants in the product build; `make EXPERIMENTS=1` turns them back into the environment knobs the
// A/B scripts under tools/ set (SER_GEMM_T256_MIN, SER_GEMM_FORCE, ...).
#ifdef SER_EXPERIMENTS
static inline long ser_knob(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
#else
constexpr long ser_knob(const char*, long dflt) { return dflt; }
#endif

// ---- ser_gemm --------------------------------------------------------------------------------------------------------------------------
// WM x WN waves, each TM x TN MFMA tiles of 16x16; BK = K tile; ST = ring stages; LNEPI = row-complete LayerNorm epilogue;
// two_plane = the tile serves FP32X / FP16X (both planes of a K tile per stage), otherwise BF16 / FP16 / FP16M.
struct gemm_tile {
    const char* name;
    int WM, WN, TM, TN, BK, ST;
    bool LNEPI, two_plane;
    constexpr int BM() const { return WM * TM * 16; }
    constexpr int BN() const { return WN * TN * 16; }
    constexpr int threads() const { return 64 * WM * WN; }
    constexpr bool dense() const { return !LNEPI && BN() >= 128; }
};
enum gemm_tile_id {
    GEMM_128x128, GEMM_256x128, GEMM_256x256,          // tile_cfg 1, 2, 3 and SER_GEMM_FORCE's 0, 1, 2 are these three, in this order
    GEMM_128x64, GEMM_LN512, GEMM_LN512_M64, GEMM_LN512_M32,
    GEMM_X_128x128x64, GEMM_X_256x128x32, GEMM_X_256x256x32, GEMM_X_128x64x32, GEMM_X_LN128x512x32,
    GEMM_TILES
};
constexpr gemm_tile GEMM_TILE[GEMM_TILES] = {
    {"128x128",         2, 2, 4, 4, 64, 2, false, false},     // 4 waves, 2 blocks/CU: small grids
    {"256x128",         4, 2, 4, 4, 64, 3, false, false},     // 8 waves of 64x64 on a three-stage ring
    {"256x256",         2, 4, 8, 4, 64, 2, false, false},     // 8 waves of 128x64: half the L2 -> LDS bytes per FLOP
    {"128x64",          4, 1, 2, 4, 64, 2, false, false},     // 4 waves of 32x64: a wave owns a whole 64-column stat group
    {"LN512",           2, 4, 4, 8, 64, 2, true,  false},     // 128 x 512: 160 KiB ring, one barrier per 64-deep K tile
    {"LN512_M64",       1, 8, 4, 4, 64, 2, true,  false},     // 64 x 512 tile, 8 waves of 64x64
    {"LN512_M32",       1, 4, 2, 8, 64, 2, true,  false},     // 32 x 512 tile, 4 waves of 32x128
    {"X_128x128x64",    4, 2, 2, 4, 64, 2, false, true},      // 8 waves (32x64 each): 2 waves/SIMD hide the LDS reads
    {"X_256x128x32",    4, 2, 4, 4, 32, 3, false, true},      // 64x64 wave tiles on a 32-deep, 3-stage ring (144 KiB)
    {"X_256x256x32",    4, 2, 4, 8, 32, 2, false, true},      // 64x128 wave tiles, 2 stages (128 KiB)
    {"X_128x64x32",     4, 1, 2, 4, 32, 2, false, true},      // grouped positional conv, like the single-plane 128x64
    {"X_LN128x512x32",  2, 4, 4, 8, 32, 2, true,  true},      // the two-plane ring doubles: the LayerNorm tile that still fits 160 KiB
};

// (mode of the operands, format of the out_act copy): the kernels that exist.  om == mode is a launch that does not convert.
struct gemm_pair { int mode, om; };
constexpr gemm_pair GEMM_PAIR[] = {
    {SER_MODE_BF16, SER_MODE_BF16},
    {SER_MODE_FP16, SER_MODE_FP16},
    {SER_MODE_FP16, SER_MODE_FP16X},      // FC2 of the "f16q" mode: the next layer's q / k projection reads hi + lo planes
    {SER_MODE_FP16M, SER_MODE_FP16M},
    {SER_MODE_FP16M, SER_MODE_FP16X},     // packed projection of "f16m": q, k, v leave as fp16 hi + lo planes for ser_attention
    {SER_MODE_FP32X, SER_MODE_FP32X},
    {SER_MODE_FP32X, SER_MODE_FP16},      // stem -> layers boundary of the "f16" numerics mode
    {SER_MODE_FP16X, SER_MODE_FP16X},     // attention block ("f16a") / logit path ("f16q") / conv stack of the f16 modes: 3 products on the f16 MFMA
    {SER_MODE_FP16X, SER_MODE_FP16},      // output projection of "f16a": 3 products, one-plane copy for FC1
    {SER_MODE_FP16X, SER_MODE_FP16M},     // output projection of "f16m": 3 products on the attention kernel's hi + lo context rows, FP16M copy for FC1
};
constexpr int GEMM_PAIRS = (int)(sizeof(GEMM_PAIR) / sizeof(GEMM_PAIR[0]));
constexpr int gemm_pair_index(int mode, int om) {          // -1: no such kernel
    for (int i = 0; i < GEMM_PAIRS; ++i)
        if (GEMM_PAIR[i].mode == mode && GEMM_PAIR[i].om == om) return i;
    return -1;
}
constexpr bool gemm_two_plane(int mode) { return mode == SER_MODE_FP32X || mode == SER_MODE_FP16X; }
// Which (tile, pair) kernels are built.  The LayerNorm tiles take no conversion; a converting pair needs a dense tile (no LayerNorm
// epilogue, BN >= 128), except that every two-plane tile without the LayerNorm epilogue also writes the one-plane fp16 copy
// (FP32X / FP16X -> FP16); FP16M needs a dense tile with BK = 64 whatever it writes.
constexpr bool gemm_tile_serves(const gemm_tile& t, gemm_pair p) {
    if (t.two_plane != gemm_two_plane(p.mode)) return false;
    if (p.mode == SER_MODE_FP16M) return t.dense() && t.BK == 64;
    if (p.om == p.mode) return true;
    if (t.two_plane && p.om == SER_MODE_FP16) return !t.LNEPI;
    return t.dense();
}

// Every threshold of gemm_pick_tile, read once (experiment builds: from the environment).
struct gemm_knobs {
    int ln_bm, n64, deepk;
    long t256_min, x32_256_min, x32_sq_min, m16_sq_min, m16_256_min;
};
static inline const gemm_knobs& gemm_knobs_get() {
    static const gemm_knobs k = {
        (int)ser_knob("SER_GEMM_LN_BM", 0), (int)ser_knob("SER_GEMM_N64", 1), (int)ser_knob("SER_GEMM_DEEPK_256x128", 1),
        ser_knob("SER_GEMM_T256_MIN", 150),       // 200 before the ping-pong schedule; XLS-R-2B's QKV (184 tiles at 4 x 10 s): +3.2 % on its step
        ser_knob("SER_GEMM_X32_256_MIN", 100),    // 100: M = 3992 out-proj / FC2 (128 tiles) gain, M = 1996 ones (64 tiles) lose
        ser_knob("SER_GEMM_X32_SQ_MIN", 150), ser_knob("SER_GEMM_M16_SQ_MIN", 100), ser_knob("SER_GEMM_M16_256_MIN", 100)};
    return k;
}

#ifdef SER_EXPERIMENTS
// experiments: SER_GEMM_FORCE="N:K:cfg[,N:K:cfg...]" pins the tile config of matching single-plane launches (tools/); -1 = no rule
static inline int gemm_forced_tile(const ser_gemm_args* a) {
    struct Rule { int n, k, cfg; };
    static Rule rules[8];
    static const int nrules = [] {
        const char* e = getenv("SER_GEMM_FORCE");
        int n = 0;
        while (e && *e && n < 8) {
            int a0, a1, a2, used = 0;
            if (sscanf(e, "%d:%d:%d%n", &a0, &a1, &a2, &used) != 3) break;
            rules[n++] = {a0, a1, a2};
            e += used;
            if (*e == ',') ++e;
        }
        return n;
    }();
    for (int i = 0; i < nrules; ++i)
        if (rules[i].n == a->N && rules[i].k == a->K && rules[i].cfg >= 0 && rules[i].cfg <= GEMM_256x256) return rules[i].cfg;
    return -1;
}
#endif

// The tile of a launch whose arguments passed gemm_plan's checks.  tile_cfg (1 = 128x128, 2 = 256x128, 3 = 256x256) is honoured
//   BF16 / FP16:    always, unless the LayerNorm epilogue is on (ln_gamma: the row count alone picks the tile);
//   FP16M:          2 and 3; 1 is not a request -- with it the launch takes 128x128 without looking at the auto rules, as it does for 0
//                   when they pick nothing larger;
//   FP32X / FP16X:  never.
static inline int gemm_pick_tile(const ser_gemm_args* a) {
    const gemm_knobs& kn = gemm_knobs_get();
    const long rt256 = (a->M + 255) / 256;
    const long t256sq = rt256 * ((a->N + 255) / 256) * a->groups;         // 256x256 tiles (FP16M: groups == 1)
    const long t256x128 = rt256 * ((a->N + 127) / 128) * a->groups;
    if (gemm_two_plane(a->mode)) {
        // both planes share a stage: the ring doubles, so FP32X uses the configurations that still fit 160 KiB
        if (a->ln_gamma) return GEMM_X_LN128x512x32;
        // grouped positional conv (<= 64 output channels per group): 128x64 tiles of 32x64 wave tiles, like the bf16 path's -- the
        // 128x128 tile below computes 64 dead columns per group (fp32x pos-conv: 360 us against 100 us in bf16)
        if (kn.n64 && a->N <= 64) return GEMM_X_128x64x32;
        // Large grids: 256x128 tiles of 64x64 wave tiles on a 32-deep, 3-stage ring (144 KiB): 16 fragments feed 48 MFMAs per
        // k-step (0.33 LDS fragment reads per MFMA against 0.5 for the 32x64 wave tile below), one ping-pong phase per K tile
        // Largest grids (round 3): 256x256 tiles of 64x128 wave tiles, both planes of a 32-deep K tile per stage, 2 stages (128 KiB):
        // 24 fragments feed 96 MFMAs per K tile (0.25 LDS fragment reads per MFMA, half the L2 -> LDS bytes per product of the
        // 256x128 tile), the weight fragments taken in two halves like the LayerNorm tile's (PPW).  From SER_GEMM_X32_SQ_MIN tiles.
        // Measured on the step (two A/B pairs, one box): the packed QKV projection on it f16a 1 110 / 1 114 -> 1 134 / 1 130 utt/s; FC1 too
        // (its GELU epilogue on 128 accumulators + 64 spilled bias / column-sum registers) gives the gain back: fp32x 848 -> 846.
        // Hence only launches without an activation take it.
        // ... and only grids whose last round of 256 blocks is mostly full (round 4): WavLM-large's packed projection has 384 such tiles = 1.5 rounds
        // (efficiency 0.75) and is 0.5 % faster on the f16x step as 768 tiles of 256x128 = 3 full rounds (XLS-R-2B at 8 x 10 s, 368 tiles: + 0.2 %), while
        // HuBERT-xlarge's 480 (0.94) and Whisper's 705 (0.92) lose 2.7 % / 4.7 % of their steps without the square tile (same-box pairs, experiments build).
        const long sq_rounds = (t256sq + 255) / 256;
        const bool sq_full = t256sq * 100 >= sq_rounds * 256 * 85;
        if (kn.x32_sq_min > 0 && a->N >= 256 && t256sq >= kn.x32_sq_min && sq_full && a->act == SER_ACT_NONE) return GEMM_X_256x256x32;
        if (kn.x32_256_min > 0 && a->N >= 128 && t256x128 >= kn.x32_256_min) return GEMM_X_256x128x32;
        return GEMM_X_128x128x64;
    }
    if (a->mode == SER_MODE_FP16M) {
        // the single-plane tiles walked twice per K tile (H unit, E unit): 256x256 from 100 tiles up, 256x128 on a three-stage ring, 128x128 on four
        // waves for small M.  Alone, one launch at a time, the 256x256 form is the SLOWER one at M = 7 984 (packed projection 139 us against 122 on
        // 256x128, FC2 -- 128 tiles, half the chip -- 206 against 130: profiles/r05_gemm_f16m_bench.txt); on the step it is the FASTER one: 928 ->
        // 973 utt/s with the packed projection and FC1 on it, 990 with FC2 and the output projection too (profiles/r05_f16m_tile_choice_step_ab.txt).
        // The step runs at the board's power cap (profiles/r05_power_sample_bf16_step.txt): what counts is energy per FLOP, and the square tile
        // moves 2/3 of the L2 -> LDS bytes per FLOP.  (The same threshold on the bf16 tiles LOSES 1.3 %: T256_MIN stays 150.)
        if (a->tile_cfg == 3 || (!a->tile_cfg && a->N >= 256 && t256sq >= kn.m16_sq_min)) return GEMM_256x256;
        if (a->tile_cfg == 2 || (!a->tile_cfg && a->N >= 128 && t256x128 >= kn.m16_256_min)) return GEMM_256x128;
        return GEMM_128x128;
    }
    if (a->ln_gamma) {
        // Row-complete LayerNorm tiles are BM x 512.  The last conv layers have few rows (M = 16k / 8k / 4k for eight
        // 10 s utterances): 128-row tiles would leave half to 7/8 of the CUs idle, so the tile gets shorter until
        // the grid covers the chip (measured per layer with tools/gemm_by_layer.py).
        const int bm = kn.ln_bm ? kn.ln_bm : (a->M >= 200 * 128 ? 128 : (a->M >= 200 * 64 ? 64 : 32));
        return bm == 128 ? GEMM_LN512 : (bm == 64 ? GEMM_LN512_M64 : GEMM_LN512_M32);
    }
    if (a->tile_cfg > 0) return a->tile_cfg - 1;
    // Measured on MI355X (tools/gemm_sweep.py, M = 7984): the simple ring keeps the 128x128 tile
    // (2 blocks/CU) ahead of 256x128 on every N <= 3072 shape; 256x256 wins once it has >= ~2 full
    // rounds of blocks (N = 4096, conv layers) because it halves the L2->LDS bytes per FLOP.
    // In the real step (two utterance groups in flight) 256x256 already pays from ~200 tiles (QKV and FC1
    // at M = 3992): 9.6 -> 9.1 ms per step, A/B on one device.
#ifdef SER_EXPERIMENTS
    if (const int forced = gemm_forced_tile(a); forced >= 0) return forced;
#endif
    if (a->N >= 256 && t256sq >= kn.t256_min) return GEMM_256x256;
    // grouped positional conv: 64 output channels per group -> a 128x64 tile wastes no MFMA columns
    if (kn.n64 && a->N <= 64) return GEMM_128x64;
    // Deep-K, narrow-N GEMMs (FC2: N = D, K = 4D) that are too small for the 256x256 tile: 256x128 tiles are SLOWER
    // in isolation (52 -> 64 us at M = 3992: only 128 blocks) but +1.5 % on the real step in five A/B pairs -- the
    // launch then occupies half the CUs for its whole (long) K loop and the other utterance group's kernels own the
    // other half, instead of both time-slicing every CU.  The shallow out-projection (K = D) loses with it.
    if (kn.deepk && a->groups == 1 && a->K >= 2048 && a->N >= 128 && a->M >= 512) return GEMM_256x128;
    return GEMM_128x128;
}

// Epilogue class of the dense (non-LayerNorm) epilogue: which of its optional features a kernel is COMPILED with.  The features a class
// names as absent are not tested per element, they are not in the code.
//   LN_ACT   deferred-LayerNorm transform, optional column scale, optional GELU, out_act only: the packed projection and FC1;
//   RESID    residual + fp32 output, optional operand copy (shifted or not) with row partials, no activation: output projection and FC2;
//   GENERIC  every feature behind its run-time test: all other launches.
enum gemm_epi_id { GEMM_EPI_GENERIC, GEMM_EPI_LN_ACT, GEMM_EPI_RESID, GEMM_EPIS };
constexpr const char* GEMM_EPI_NAME[GEMM_EPIS] = {"GENERIC", "LN_ACT", "RESID"};
// Which (tile, pair) kernels exist in a specialised class: the three single-plane hot tiles of the encoder layers, and per class the pairs
// the layers launch it with -- LN_ACT: the packed projection and FC1 (BF16, FP16, FP16M, FP16M -> FP16X); RESID: the output projection and
// FC2 (the same and FP16 -> FP16X).  (The positional conv's 128x64 tile -- GELU + residual, one launch per forward -- and the two-plane
// tiles stay on GENERIC: every further kernel is compile time of gemm.hip.)
constexpr bool gemm_epi_built(int tile, gemm_pair p, int epi) {
    if (epi == GEMM_EPI_GENERIC) return gemm_tile_serves(GEMM_TILE[tile], p);
    if (tile != GEMM_128x128 && tile != GEMM_256x128 && tile != GEMM_256x256) return false;
    if (!gemm_tile_serves(GEMM_TILE[tile], p) || gemm_two_plane(p.mode)) return false;
    return epi == GEMM_EPI_RESID || !(p.mode == SER_MODE_FP16 && p.om == SER_MODE_FP16X);
}
// The class of a launch that passed gemm_plan's checks: exact predicates on the fields the kernel's epilogue tests.
static inline int gemm_pick_epi(const ser_gemm_args* a, int tile, int pair) {
    int epi = GEMM_EPI_GENERIC;
    if (a->gn_scale) return epi;
    if (a->ln_stats_in && a->out_act && !a->residual && !a->out_f32 && !a->shift_out && !a->stat_out) epi = GEMM_EPI_LN_ACT;
    else if (a->residual && a->out_f32 && !a->f32_col_begin && a->col_scale_end <= 0 && !a->ln_stats_in && a->act != SER_ACT_GELU) epi = GEMM_EPI_RESID;
    return gemm_epi_built(tile, GEMM_PAIR[pair], epi) ? epi : GEMM_EPI_GENERIC;
}

struct gemm_launch {
    int tile, pair;                    // indices into GEMM_TILE / GEMM_PAIR
    unsigned grid_x, grid_y;           // (row tiles x column tiles, groups)
    int block, lds;
    int epi;                           // gemm_epi_id
};

// Checks the arguments (codes and texts of ser_gemm) and plans the launch.  0, or the code ser_fail was given.
static inline int gemm_plan(const ser_gemm_args* a, gemm_launch* out) {
    if (!a || !a->A || !a->W) return ser_fail(-1, "ser_gemm: null operand");
    if (a->M <= 0 || a->N <= 0 || a->K <= 0) return ser_fail(-2, "ser_gemm: bad shape M=%d N=%d K=%d", a->M, a->N, a->K);
    if (a->K % 64) return ser_fail(-3, "ser_gemm: K=%d must be a multiple of 64", a->K);
    if (a->kc && (a->kc % 64 || a->K % a->kc)) return ser_fail(-4, "ser_gemm: kc=%d must divide K and be a multiple of 64", a->kc);
    if (a->N % 8) return ser_fail(-5, "ser_gemm: N=%d must be a multiple of 8", a->N);
    if (gemm_pair_index(a->mode, a->mode) < 0) return ser_fail(-6, "ser_gemm: bad mode %d", a->mode);
    if (a->mode == SER_MODE_FP16M) {
        if (!a->a_scale || !a->w_scale || a->a_scale_ld < a->M || a->w_scale_ld < a->N)
            return ser_fail(-23, "ser_gemm: FP16M needs a_scale / w_scale with *_scale_ld >= the row count");
        if (a->a_rowoff || a->kc || a->groups != 1 || a->ln_gamma || (a->lda % 64))
            return ser_fail(-23, "ser_gemm: FP16M takes plain row-major operands (no row map / conv chunks / groups / LayerNorm epilogue), lda %% 64 == 0");
    }
    if (a->out_mode == SER_MODE_FP16M || (a->mode == SER_MODE_FP16M && !a->out_mode && a->out_act)) {
        if (!a->out_scale || (a->N % 64) || (a->ldo_act % 64) || a->groups != 1 || a->ln_gamma)
            return ser_fail(-24, "ser_gemm: an FP16M out_act needs out_scale, N %% 64 == 0, ldo_act %% 64 == 0, groups == 1, no LayerNorm epilogue");
    }
    if (!a->a_rowoff && (a->lda % 8)) return ser_fail(-7, "ser_gemm: lda must be a multiple of 8");
    if (a->groups < 1) return ser_fail(-8, "ser_gemm: groups=%d", a->groups);
    if (!a->out_f32 && !a->out_act) return ser_fail(-9, "ser_gemm: no output");
    if ((a->ldo_f32 % 4) || (a->ldo_act % 4) || (a->ldr % 4) || (a->c_group_stride % 4))
        return ser_fail(-10, "ser_gemm: output/residual pitches must be multiples of 4");
    if (a->ln_gamma) {
        if (!a->ln_beta) return ser_fail(-11, "ser_gemm: ln_gamma without ln_beta");
        if (a->N > 512 || a->groups != 1 || a->residual)
            return ser_fail(-12, "ser_gemm: the LayerNorm epilogue needs N <= 512, groups == 1, no residual");
    }
    if (a->ln_stats_in) {
        if (!a->ln_colsum || a->ln_groups < 2 || a->ln_groups > 32 || (a->ln_groups & 1) || a->ln_gamma)
            return ser_fail(-14, "ser_gemm: deferred LayerNorm needs ln_colsum, an even ln_groups in [2,32] and no fused-LN epilogue");
    }
    if (a->stat_out && (a->ln_gamma || a->stat_groups < a->groups * ((a->N + 63) / 64)))
        return ser_fail(-15, "ser_gemm: stat_out needs stat_groups >= groups*ceil(N/64) and no fused-LN epilogue");
    if (a->shift_out && (!a->stat_out || a->ln_gamma)) return ser_fail(-19, "ser_gemm: shift_out needs stat_out and no fused-LN epilogue");
    if (a->mean_out && !a->ln_stats_in) return ser_fail(-20, "ser_gemm: mean_out needs ln_stats_in");
    if (a->lnstat_out && !a->ln_stats_in) return ser_fail(-20, "ser_gemm: lnstat_out needs ln_stats_in");
    const int om = a->out_mode ? a->out_mode : a->mode;
    const int pair = gemm_pair_index(a->mode, om);
    if (om != a->mode && !a->ln_gamma && pair < 0)
        return ser_fail(-21, "ser_gemm: out_mode %d with mode %d (FP32X -> FP16, FP16 <-> FP16X, FP16X <-> FP16M convert)", a->out_mode, a->mode);
    if (om != a->mode && a->ln_gamma) return ser_fail(-21, "ser_gemm: out_mode %d with the LayerNorm epilogue", a->out_mode);
    if (a->col_scale_end % 4) return ser_fail(-17, "ser_gemm: col_scale_end must be a multiple of 4");
    if (a->gn_scale && (!a->gn_shift || !a->gn_row_offs || a->gn_B < 1 || a->gn_ld < a->N || (a->gn_ld % 4) || a->groups != 1 ||
                        a->ln_gamma || a->ln_stats_in))
        return ser_fail(-25, "ser_gemm: gn_scale needs gn_shift, gn_row_offs, gn_B >= 1, gn_ld >= N (multiple of 4), groups == 1, "
                             "no LayerNorm epilogue and no deferred LayerNorm");
    if ((a->ldo_act % 8) || (a->c_group_stride % 8)) return ser_fail(-18, "ser_gemm: act pitch / group stride must be multiples of 8");
    if (a->f32_col_begin < 0 || (a->f32_col_begin % 8)) return ser_fail(-16, "ser_gemm: f32_col_begin must be a non-negative multiple of 8");
    if (a->tile_cfg < 0 || a->tile_cfg > 3) return ser_fail(-13, "ser_gemm: tile_cfg=%d (0 auto, 1..3)", a->tile_cfg);

    const int tile = gemm_pick_tile(a);
    const gemm_tile& t = GEMM_TILE[tile];
    if (!gemm_tile_serves(t, GEMM_PAIR[pair])) {
        if (a->mode == SER_MODE_FP16M) return ser_fail(-22, "ser_gemm: FP16M needs a dense tile (N > 64, no LayerNorm epilogue)");
        if (a->mode == SER_MODE_FP16X) return ser_fail(-22, "ser_gemm: FP16X -> FP16M output needs a dense tile (N > 64)");
        return ser_fail(-22, "ser_gemm: FP16 -> FP16X output needs a dense tile (N > 64, no LayerNorm epilogue)");
    }
    const int BM = t.BM(), BN = t.BN();
    out->tile = tile;
    out->pair = pair;
    out->epi = gemm_pick_epi(a, tile, pair);
    out->grid_x = (unsigned)(((a->M + BM - 1) / BM) * ((a->N + BN - 1) / BN));
    out->grid_y = (unsigned)a->groups;
    out->block = t.threads();
    out->lds = (gemm_two_plane(a->mode) ? 2 : 1) * t.ST * (BM + BN) * t.BK * 2 + (t.LNEPI ? 0 : BM * 8)    // ring (+ [BM][2] row statistics)
             + (a->mode == SER_MODE_FP16M ? t.ST * (BM + BN) * 4 : 0);                                       // FP16M: + the block-scale words of every stage
    return 0;
}

// ---- ser_attention_v -------------------------------------------------------------------------------------------------------------------
constexpr int ATTN_BKV = 64;       // keys per tile
constexpr int ATTN_NWV = 4;        // waves per block, 32 query rows each

// The form of the kernel and the launch: attention_kernel<dhp, mode, pre, tbl, ATTN_NWV, b2d, gb, occ> on `grid` blocks with `lds` bytes.
struct attn_launch {
    int dhp, mode;
    bool pre, tbl, b2d, gb, occ;
    int nbuf, bias_stride;
    size_t lds;
    int nq;
    unsigned grid;
};
constexpr int attn_qk_planes(int mode) { return (mode == SER_MODE_FP32X || mode == SER_MODE_FP16X || mode == SER_MODE_FP16Q) ? 2 : 1; }
constexpr int attn_v_planes(int mode) { return (mode == SER_MODE_FP32X || mode == SER_MODE_FP16X) ? 2 : 1; }
// Which forms are built: bias2d and the global-memory bias table only 64 wide with a pre-scaled q (bias2d not in FP16 / FP16Q), the
// high-occupancy form for single-plane 64-wide launches, FP16X / FP16Q only with a pre-scaled q.
constexpr bool attn_form_built(int dhp, int mode, bool pre, bool tbl, bool b2d, bool gb, bool occ) {
    if (b2d) return dhp == 64 && pre && !tbl && !gb && !occ && (mode == SER_MODE_BF16 || mode == SER_MODE_FP32X || mode == SER_MODE_FP16X);
    if (gb) return dhp == 64 && pre && tbl && !occ;
    if (occ) return dhp == 64 && attn_qk_planes(mode) == 1;
    return pre || (mode != SER_MODE_FP16X && mode != SER_MODE_FP16Q);
}

// Checks the arguments (codes and texts of ser_attention_v) and plans the launch.  0, or the code ser_fail was given.
static inline int attn_plan(const ser_attention_args* a, attn_launch* out) {
    if (!a) return ser_fail(-1, "ser_attention: null pointer");
    if (!a->qkv || !a->frame_offs || !a->out) return ser_fail(-1, "ser_attention: null pointer");
    const int np = attn_qk_planes(a->mode), npv = attn_v_planes(a->mode);      // planes of q / k, of v
    if (a->gate_x) {
        if (!a->table || !a->gru_const || a->gate || !a->gate_stat || !a->gate_w || !a->gate_cb)
            return ser_fail(-13, "ser_attention: gate_x needs table, gru_const, gate_stat, gate_w, gate_cb and no gate[]");
        if ((a->gate_x_ld % 8) || (a->gate_x_plane_stride % 8) || (a->gate_w_plane_stride % 8) || a->gate_x_planes != np || (a->dh % 8))
            return ser_fail(-13, "ser_attention: gate_x / gate_w pitch, or gate_x_planes != the planes of mode %d", a->mode);
    }
    if (a->out_mode && a->out_mode != SER_MODE_FP16M) return ser_fail(-14, "ser_attention: out_mode %d (0 or SER_MODE_FP16M)", a->out_mode);
    if (a->out_mode == SER_MODE_FP16M &&
        (a->mode != SER_MODE_FP16X || a->dh != 64 || !a->out_scale || (a->ldo % 64) || a->bias2d || a->out_scale_ld <= 0))
        return ser_fail(-14, "ser_attention: SER_MODE_FP16M context rows need mode FP16X, head dim 64, out_scale, ldo %% 64 == 0 and no bias2d");
    if (a->B <= 0 || a->H <= 0 || a->max_frames <= 0) return ser_fail(-2, "ser_attention: bad B/H/max_frames");
    if (a->dh % 8 || a->dh < 8 || a->dh > 128) return ser_fail(-3, "ser_attention: head dim %d unsupported (multiple of 8, <= 128)", a->dh);
    if ((a->ld % 8) || (a->ldo % 4) || (a->q_col % 8) || (a->k_col % 8) || (a->v_col % 8)) return ser_fail(-4, "ser_attention: misaligned pitches/columns");
    if (a->mode < SER_MODE_BF16 || a->mode > SER_MODE_FP16Q) return ser_fail(-5, "ser_attention: bad mode %d", a->mode);
    if ((a->table != nullptr) != (a->gate != nullptr || a->gru_const != nullptr))
        return ser_fail(-6, "ser_attention: the bias table needs a gate (gate[] or gate_col + gru_const) and vice versa");
    if (a->gate && a->gru_const) return ser_fail(-9, "ser_attention: give gate[] or gru_const, not both");
    if (a->gru_const && !a->gate_x && (a->gate_col < 0 || (a->gate_col % 2))) return ser_fail(-10, "ser_attention: bad gate_col %d", a->gate_col);
    if (a->table && a->table_T < a->max_frames) return ser_fail(-7, "ser_attention: bias table built for T=%d < max_frames=%d", a->table_T, a->max_frames);
    const bool pre = a->scale <= 0.f;
    if (a->bias2d) {
        if (a->table || !a->key_lens || !pre || a->dh > 64 || a->mode == SER_MODE_FP16 || a->mode == SER_MODE_FP16Q)
            return ser_fail(-11, "ser_attention: bias2d needs key_lens, a pre-scaled q (scale <= 0), dh <= 64, no table, bf16 / fp32x / fp16x");
        if (a->bias2d_ld < a->max_frames || (a->bias2d_ld % ATTN_BKV))
            return ser_fail(-12, "ser_attention: bias2d_ld=%lld must be a multiple of %d and >= max_frames", (long long)a->bias2d_ld, ATTN_BKV);
    }
    // padded head dim of the LDS images and MFMA loops: 64, 96 (head dims 72 .. 96: HuBERT-xlarge's 80 runs 6 + 6 k-steps and 3 output column
    // blocks instead of the 8 + 8 and 4 of the 128-wide form it used through round 3) or 128
    const int dhp = a->dh <= 64 ? 64 : (a->dh <= 96 ? 96 : 128);
    const int nch = ATTN_BKV * (dhp / 8) / (64 * ATTN_NWV);
    const int nq = (a->max_frames + 32 * ATTN_NWV - 1) / (32 * ATTN_NWV);
    const unsigned nblocks = (unsigned)(((a->H * a->B + 7) / 8) * 8 * nq);
    // K / V tiles: two buffers while a wave's DMA pieces stay within 8 per tile (and never in the high-occupancy form); + 4 shifted copies of
    // the bias window.  copy stride == 16 (mod 64) floats: the 4 shifted copies x the 4 query phases of a ds_read_b128
    // lane group then land on 16 distinct 4-bank slots (a multiple of 64 made them 2-way conflicts)
    int bias_stride = 0;
    if (a->table) {
        bias_stride = ((a->max_frames + 32 * ATTN_NWV + 2 * ATTN_BKV + 3 + 4) / 4) * 4;   // window of one query block (+ the 0..3 alignment slots), not all 2T-1 distances
        bias_stride += (16 - (bias_stride & 63) + 64) & 63;
    }
    const auto nbuf_of = [&](bool occ_) { return (!occ_ && nch * (np + npv) <= 8) ? 2 : 1; };
    const auto lds_of = [&](int nbuf_) { return (size_t)nbuf_ * (np + npv) * ATTN_BKV * dhp * 2 + (size_t)4 * bias_stride * 4; };
    // high-occupancy form (see the kernel): single-plane 64-wide launches with more than two blocks per CU to place that fit ONE round at
    // four per CU (measured: 16 x 16 heads x 300 / 499 frames and the ragged mix gain 8 - 11 %; Whisper's 1 920-block launches run several
    // rounds either way and LOSE 1 - 3 % on their step with it: left on the low-occupancy form)
    bool occ = dhp == 64 && np == 1 && !a->bias2d && nblocks > 2u * 256u && nblocks <= 4u * 256u;
    int nbuf = nbuf_of(occ);
    size_t lds = lds_of(nbuf);
    // ... and only while four blocks' LDS fit a CU: a long utterance's bias window (B = 1, ~8 000 frames: 1 008 blocks, 133 KiB of window) would
    // otherwise take the single-buffer 128-register form at ONE block per CU, the slow combination
    if (occ && lds > 40 * 1024) {
        occ = false;
        nbuf = nbuf_of(occ);
        lds = lds_of(nbuf);
    }
    // a bias window that does not fit (utterances beyond ~2 min; ~1.5 min in the two-plane modes): the table is read from global
    // memory instead (GB forms: pre-scaled q, head dim <= 64 -- what the WavLM encoders use)
    const bool gb = a->table && lds > 160 * 1024 && pre && dhp == 64 && ATTN_NWV == 4;
    if (gb) {                                                     // (the GB forms have no high-occupancy instantiation: double buffer)
        occ = false;
        nbuf = nbuf_of(occ);
        bias_stride = 0;
        lds = lds_of(nbuf);
    }
    if (lds > 160 * 1024) return ser_fail(-8, "ser_attention: LDS need %zu > 160 KiB (max_frames=%d)", lds, a->max_frames);
    // "f16a" / "f16q": the host always pre-scales q; only the PRE forms are built
    if ((a->mode == SER_MODE_FP16X || a->mode == SER_MODE_FP16Q) && !pre)
        return ser_fail(-13, "ser_attention: FP16X / FP16Q need a pre-scaled q (scale <= 0)");
    *out = attn_launch{dhp, a->mode, pre, a->table != nullptr, a->bias2d != nullptr, gb, occ, nbuf, bias_stride, lds, nq, nblocks};
    return 0;
}
