// Matrix-core GEMM with implicit-convolution row map and fused epilogues (ser_gemm).
//
//   C[m,n] = sum_k A(m,k) * W[n,k]     A: act bf16 (1 or 2 planes), W: bf16 [N][K] (1 or 2 planes)
//
// gfx950 design
//   * One kernel template, twelve tile configurations (launch_plan.h: the table GEMM_TILE, and gemm_pick_tile chooses per shape):
//     single-plane modes (BF16 / FP16 / FP16M), BM x BN x BK:
//       128x128x64, 4 waves, 2-stage ring, 2 blocks/CU   -- small grids (N = 1024 projections)
//       256x128x64, 8 waves, 3-stage ring                -- deep-K launches too small for the square tile
//       256x256x64, 8 waves, 2-stage ring                -- largest grids (half the L2->LDS bytes per FLOP)
//       128x64x64,  4 waves, 2-stage ring                -- grouped positional conv (<= 64 output channels per group)
//       128x512x64 (8 waves), 64x512x64 (8 waves), 32x512x64 (4 waves), 2-stage ring -- LayerNorm+GELU epilogue over the full 512-wide
//                                                           row; the fewer the rows, the shorter the tile
//     two-plane modes (FP32X / FP16X: both planes of a K tile per stage), 8 waves but for the 4 of 128x64x32:
//       128x128x64 2-stage, 256x128x32 3-stage, 256x256x32 2-stage, 128x64x32 2-stage, and the LayerNorm tile 128x512x32 2-stage
//   * v_mfma_f32_16x16x32_bf16 with the WEIGHT tile as the MFMA A operand and the activation
//     tile as the B operand: the accumulator then holds 4 consecutive output columns per register
//     quad, and by permuting which weight row sits in which LDS row each lane ends up owning
//     TN*4 CONSECUTIVE output columns of one row -> 16-byte epilogue loads/stores.
//   * global -> LDS by global_load_lds_dwordx4 (16 B/lane, no VGPR round trip).  The LDS image is
//     [row][BK bf16] with the 16-B chunk index XOR f(row): the DMA destination stays lane-linear,
//     the swizzle is applied to the per-lane SOURCE address and to the ds_read_b128 address (both
//     sides or neither).  f = row & 7 (BK=64) / (row >> 1) & 3 (BK=32): conflict-free for all four
//     16-lane groups of ds_read_b128 (checked by enumeration).
//   * S-stage LDS ring with COUNTED s_waitcnt vmcnt(N) and a raw s_barrier: loads of the next S-1
//     K tiles stay in flight across the barrier (a __syncthreads() would drain them), one barrier
//     per K tile, s_setprio around the MFMA cluster.
//   * FP32X mode runs the same loop over 3 K-segments (hi*hi, lo*hi, hi*lo) into one accumulator.
//   * FP16M mode (round 5): the ring carries TWO units per 64-deep K tile -- the fp16 hi planes (two f16 MFMA k-steps) and the e4m3 cross-term
//     planes + their block scales (ONE v_mfma_scale_f32_16x16x128_f8f6f4 per fragment pair): 2 product-equivalents instead of FP16X's 3.
//   * blockIdx.x -> tile through a bijective XCD swizzle so each of the 8 L2s sees a contiguous run
//     of tiles that share activation panels.
#include "ser_common.h"
#include "launch_plan.h"
#ifndef SER_GEMM_PP
#define SER_GEMM_PP 27        // ping-pong schedule, bit mask: 1 = 256x256, 2 = 256x128 / 64x512 (64x64 wave tiles), 4 = 128x512 LayerNorm tile, 8 = the FP32X 128x128 tile, 16 = the FP32X 128x512 LayerNorm tile; 0 = plain ring (A/B builds)
#endif
#include <stdlib.h>
#include <stdio.h>
#include <utility>
#ifdef SER_GEMM_DBG
// diagnostic build only (tools/gemm_clock.py): wave 0 of every block stamps s_memtime / s_memrealtime around its K loop
extern "C" { void* ser_gemm_dbg_ptr = nullptr; }
__device__ unsigned long long* ser_gemm_dbg_dev = nullptr;
#endif

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// One LDS-DMA wave instruction in its scalar-base form: 64 lanes x BYTES from (uniform base + the lane's 32-bit offset) to LDS bytes
// [lds_addr, lds_addr + 64 * BYTES), lane-linear.  M0 carries the LDS address; nothing else in this library uses M0.
// a pointer the compiler may hold in VGPRs although every lane has the same value -> SGPR pair (the "s" asm constraint is not enforced
// for 64-bit operands: without this the -DSER_GEMM_DBG build handed the instruction a VGPR pair)
__device__ __forceinline__ const char* uniform_ptr(const void* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (const char*)(((uint64_t)hi << 32) | lo);
}
template <int BYTES>
__device__ __forceinline__ void dma_lds(const void* ubase, uint32_t voff, uint32_t lds_addr) {
    static_assert(BYTES == 16 || BYTES == 4, "dwordx4 or dword");
    if constexpr (BYTES == 16)
        asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(ubase), "s"(lds_addr) : "memory");
    else
        asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dword %0, %1" :: "v"(voff), "s"(ubase), "s"(lds_addr) : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else static_assert(N < 0, "add a case");
}

// acc += (block-scaled e4m3 A) x (block-scaled e4m3 B), 16 x 16 x 128.  Issued from inline asm with the accumulator TIED: hipcc (ROCm 7.2) gives the
// builtin's result a fresh register quad (its destination is early-clobber, never coalesced with the C input), so the 128 accumulators of the
// 256x256 tile rotate through the file and 50 - 120 registers spill, some inside the K loop.  Hazards the compiler no longer sees: every call site
// sits behind an s_barrier + LDS waits after the last writer of its operands, consecutive calls target different accumulators, and the K loop ends
// in mfma_scale_drain() before anything else reads the accumulators.
__device__ __forceinline__ void mfma_scale8(f32x4& acc, const i32x8& a, const i32x8& b, int sa, int sb) {
    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]" : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb));
}
__device__ __forceinline__ void mfma_scale_drain() {
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 7" ::: "memory");          // > the 8 passes of the last scaled MFMA
}

// WM x WN waves, each TM x TN MFMA tiles of 16x16; BK = K tile; ST = ring stages.
// OM: format of the out_act copy (== MODE unless the launch converts, e.g. an FP32X stem GEMM feeding FP16 layers).
// EPI: epilogue class of the dense epilogue (launch_plan.h: gemm_epi_id), which optional epilogue features are compiled in.
// (Round 3's persistent form -- only the resident blocks are launched and each walks several tiles -- measured -8 % on the step and was
// removed from the kernel in round 4; DESIGN.md section 10 keeps the record.)
template <int WM, int WN, int TM, int TN, int BK, int ST, int MODE, bool LNEPI, int OM = MODE, int EPI = GEMM_EPI_GENERIC>
__global__ __launch_bounds__(64 * WM * WN, 2)
void ser_gemm_kernel(const ser_gemm_args p) {
    constexpr int NW = WM * WN, NT = 64 * NW;
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    constexpr int CH = BK / 8;                    // 16-byte chunks per LDS row
    constexpr int ROWB = BK * 2;                  // bytes per LDS row
    constexpr int RPP = 1024 / ROWB;              // rows per 1-KiB DMA piece (one wave instruction)
    // FP32X: both planes (hi, lo) of the A and W tiles of a K tile sit in one stage, fetched ONCE, and every
    // fragment pair feeds 3 MFMAs (hi*hi, lo*hi, hi*lo): 2x the L2->LDS bytes of bf16 for 3x the products,
    // instead of three full passes over K
    // FP16M: a stage holds ONE unit of a K tile -- its fp16 hi planes (even units) or its e4m3 cross-term planes (odd units), both
    // [rows][128 bytes] images with the same swizzle -- so the ring is the single-plane one walked twice per K tile
    constexpr bool M16 = (MODE == SER_MODE_FP16M);
    constexpr int NPL = M16 ? 1 : mode_traits<MODE>::planes;     // FP32X (bf16 hi/lo) and FP16X (fp16 hi/lo)
    constexpr int A_BYTES = BM * ROWB, W_BYTES = BN * ROWB, STAGE = NPL * (A_BYTES + W_BYTES);
    static_assert(!M16 || (BK == 64 && !LNEPI && (BM + BN) % 64 == 0), "FP16M: 64-deep K tiles, dense epilogue");
    static_assert(EPI == GEMM_EPI_GENERIC || !LNEPI, "epilogue classes: dense epilogue only");
    constexpr int SCW = BM + BN;                  // FP16M: scale words per unit (one per A row and W row of the tile)
    constexpr int LA = BM / RPP / NW, LW = BN / RPP / NW;       // DMA pieces per wave per K tile
    constexpr int LPT = NPL * (LA + LW);
    constexpr int KS = BK / 32;                   // MFMA k-steps per K tile
    static_assert(BM % (RPP * NW) == 0 && BN % (RPP * NW) == 0, "tile/wave mismatch");
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
#ifdef SER_GEMM_DBG
    const unsigned long long dbg_e0 = __builtin_amdgcn_s_memtime();
#endif

    const int ntn = (p.N + BN - 1) / BN;
    const int ntm = (p.M + BM - 1) / BM;
    int bid = blockIdx.x;
    {   // bijective XCD remap: blocks with equal (bid & 7) share an L2
        const int nwg = ntm * ntn;
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        bid = base + (bid >> 3);
    }
    // row-major tile order inside an XCD's run (the 4 x 8 super-tile order moved the step by nothing: DEADENDS.md)
    const int mt = bid / ntn;
    const int nt = bid - mt * ntn;
    const int g = blockIdx.y;
    const int m0 = mt * BM, n0 = nt * BN;

    const unsigned short* Abase = (const unsigned short*)p.A + (int64_t)g * p.a_group_stride;
    const unsigned short* Wbase = (const unsigned short*)p.W + (int64_t)g * p.w_group_stride;

    // ---- per-lane DMA sources: a 32-bit byte offset from a UNIFORM tile base ---------------------
    // (round 5) global_load_lds is issued in its scalar-base form -- global_load_lds_dwordx4 v_offset, s[base:base+1] -- from inline asm:
    // the K offset of a tile, the plane and the group go into the 64-bit SGPR base with scalar adds, the lane contributes the 32-bit
    // offset of its row / chunk inside the block's tile and there is NO vector instruction in front of a DMA.  With the builtin hipcc
    // keeps 64-bit VGPR pointers and emits two v_lshl_add_u64 per DMA (it never selects the scalar-base form); those vector instructions
    // compete for the SIMD's issue slots with the partner wave's MFMAs -- the DMA-issuing phase of one wave and the MFMA phase of the other
    // were not overlapping (FP16M FC2 at M = 7 984: MFMAs alone 82 us, DMA + reads alone 79 us, together 127 us; what-if builds, DEADENDS.md).
    // Offsets are relative to the tile's first row (a_rowoff maps must be non-decreasing in m -- every map the hosts build is), so they
    // stay far below 2^32 whatever the tensor size.
    const int prow = lane / CH, ppos = lane % CH;
    uint32_t aoff[LA], woff[LW];
    const int m0c = m0 < p.M ? m0 : p.M - 1;
    const int64_t arow0 = p.a_rowoff ? (int64_t)p.a_rowoff[m0c] * 8 : (int64_t)m0c * p.lda;      // uniform
    const char* const Atile = uniform_ptr(Abase + arow0);
    const char* const Wtile = uniform_ptr(Wbase + (int64_t)n0 * p.K);
#pragma unroll
    for (int q = 0; q < LA; ++q) {
        const int R = (q * NW + wave) * RPP + prow;                               // LDS row this lane fills
        const int f = (BK == 64) ? (R & 7) : ((R >> 1) & 3);
        const int c = ppos ^ f;                                                   // logical chunk to fetch
        int m = m0 + R;
        m = m < p.M ? m : p.M - 1;
        const int64_t arow = p.a_rowoff ? (int64_t)p.a_rowoff[m] * 8 : (int64_t)m * p.lda;
        aoff[q] = (uint32_t)((arow - arow0 + c * 8) * 2);
    }
#pragma unroll
    for (int q = 0; q < LW; ++q) {
        const int R = (q * NW + wave) * RPP + prow;
        const int f = (BK == 64) ? (R & 7) : ((R >> 1) & 3);
        const int c = ppos ^ f;
        int n = n0 + R;
        n = n < p.N ? n : p.N - 1;
        woff[q] = (uint32_t)(((int64_t)(n - n0) * p.K + c * 8) * 2);
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)lds);

    const int nk = p.K / BK;
    const int total = M16 ? 2 * nk : nk;          // FP16M: two ring units per K tile
    const int tpc = p.kc ? p.kc / BK : 0x7fffffff;                                // K tiles per conv chunk

    // FP16M: block scales of the tile's rows, one word per (row, K tile), fetched with the cross-term unit: wave w brings 64 of the
    // BM + BN words (A rows first), 4 bytes per lane; with more waves than 64-row chunks the surplus waves repeat a chunk (same bytes,
    // same place), so every wave issues the same number of DMAs and the counted waits stay uniform
    unsigned char* const scl = (unsigned char*)(lds + ST * STAGE + (LNEPI ? 0 : BM * 8));     // [ST][SCW] words, behind the row statistics
    const int sc_chunk = M16 ? (wave % (SCW / 64)) : 0;
    const bool sc_is_a = sc_chunk * 64 < BM;                                     // wave-uniform: this wave's 64 words are A rows / W rows
    const char* const sc_base = uniform_ptr(sc_is_a ? p.a_scale : p.w_scale);
    const int64_t sc_step = (sc_is_a ? p.a_scale_ld : p.w_scale_ld) * 4;       // bytes between K tiles
    uint32_t sc_off = 0;
    if constexpr (M16) {
        const int r = sc_chunk * 64 + lane;
        int i = sc_is_a ? m0 + r : n0 + r - BM;
        const int lim = sc_is_a ? p.M : p.N;
        i = i < lim ? i : lim - 1;
        sc_off = (uint32_t)i * 4u;
    }
    int i_kk = 0, i_cc = 0, i_cj = 0, i_stage = 0;                               // issue-side scalar state
    // one ring unit = LPT DMA pieces per wave, sent back to back by issue().  The begin / piece / end split is kept from the removed 4-wave
    // software pipeline (DEADENDS.md): folding it back moves hipcc's scalar register allocation in several kernels.
    const char* is_ua = nullptr; const char* is_uw = nullptr;
    uint32_t is_dstA = 0, is_dstW = 0;
    auto issue_begin = [&]() {
        int64_t koffA = (int64_t)i_cj * p.ldj + (int64_t)i_cc * BK;
        int64_t koffW = (int64_t)i_kk * BK;
        if constexpr (M16) {                                     // unit i_kk: K tile i_kk / 2, plane i_kk & 1 (same byte offsets in both planes)
            koffA = (int64_t)(i_kk >> 1) * BK + (i_kk & 1) * p.a_plane_stride;
            koffW = (int64_t)(i_kk >> 1) * BK + (i_kk & 1) * p.w_plane_stride;
            if (i_kk & 1) dma_lds<4>(sc_base + (int64_t)(i_kk >> 1) * sc_step, sc_off, lds0 + (uint32_t)(ST * STAGE + (LNEPI ? 0 : BM * 8) + (i_stage * SCW + sc_chunk * 64) * 4));
        }
        is_dstA = lds0 + i_stage * STAGE + wave * 1024;          // stage = [A hi][A lo][W hi][W lo]
        is_dstW = is_dstA + NPL * A_BYTES;
        is_ua = Atile + koffA * 2;
        is_uw = Wtile + koffW * 2;
    };
    auto issue_piece = [&](int j) {                              // j in [0, LPT): plane-major, A pieces then W pieces (compile-time j)
        const int pl = j / (LA + LW), q = j % (LA + LW);
        if (q < LA) dma_lds<16>(is_ua + (int64_t)pl * p.a_plane_stride * 2, aoff[q < LA ? q : 0], is_dstA + pl * A_BYTES + q * NW * 1024);
        else dma_lds<16>(is_uw + (int64_t)pl * p.w_plane_stride * 2, woff[q >= LA ? q - LA : 0], is_dstW + pl * W_BYTES + (q - LA) * NW * 1024);
    };
    auto issue_end = [&]() {
        ++i_kk; ++i_cc;
        if (i_cc == tpc) { i_cc = 0; ++i_cj; }
        i_stage = (i_stage + 1 == ST) ? 0 : i_stage + 1;
    };
    auto issue = [&]() {
        issue_begin();
#pragma unroll
        for (int j = 0; j < LPT; ++j) issue_piece(j);
        issue_end();
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // per-lane fragment read offsets; f(row) depends only on the lane because tile bases are multiples of 16
    const int frow = lane & 15, fq = lane >> 4;
    const int fsw = (BK == 64) ? (lane & 7) : ((frow >> 1) & 3);
    int offA[KS], offW[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int phys = ((s * 4 + fq) ^ fsw) << 4;
        offA[s] = (wm * TM * 16 + frow) * ROWB + phys;
        offW[s] = NPL * A_BYTES + (wn * TN * 16 + frow) * ROWB + phys;
    }

    // Natural MFMA accumulator layout: acc[ni][mi][r] is row (mi*16 + frow), column (ni*16 + fq*4 + r) of the
    // wave tile, so the four lanes of a row cover 16 consecutive columns: fp32 stores / residual loads are 64
    // contiguous bytes per row, and the bf16 stores reach the same after one cross-row register swap.
    constexpr int CPL = TN * 4;
    const int ncol0 = n0 + wn * (TN * 16) + fq * 4;                   // column of acc[0][.][0] within the group
    const int64_t gcol = (int64_t)g * p.c_group_stride + ncol0;       // in the output matrices
    // per-column epilogue constants (bias, deferred-LayerNorm column sums): 2 * TN * 4 registers.  The FP16M tiles request them AFTER the
    // K loop -- beside the 128 accumulators and the 64 + 8 registers of a cross-term phase they would spill (86 - 116 registers, some
    // inside the loop, on the 256x256 tile); everybody else keeps them across the loop (the loads fly beside the first DMA tiles)
    float bias[CPL], csum[CPL];
    auto load_cols = [&]() {
#pragma unroll
        for (int j = 0; j < CPL; ++j) { bias[j] = 0.f; csum[j] = 0.f; }
        if (p.bias) {
#pragma unroll
            for (int j4 = 0; j4 < TN; ++j4)
                if (ncol0 + j4 * 16 < p.N) {
                    const f32x4 b = *(const f32x4*)(p.bias + (int64_t)g * p.N + ncol0 + j4 * 16);
                    bias[j4 * 4 + 0] = b[0]; bias[j4 * 4 + 1] = b[1]; bias[j4 * 4 + 2] = b[2]; bias[j4 * 4 + 3] = b[3];
                }
        }
        // deferred LayerNorm (see ser_hip.h): per-column sum of the gamma-folded weights
        if (p.ln_colsum) {
#pragma unroll
            for (int j4 = 0; j4 < TN; ++j4)
                if (ncol0 + j4 * 16 < p.N) {
                    const f32x4 b = *(const f32x4*)(p.ln_colsum + ncol0 + j4 * 16);
                    csum[j4 * 4 + 0] = b[0]; csum[j4 * 4 + 1] = b[1]; csum[j4 * 4 + 2] = b[2]; csum[j4 * 4 + 3] = b[3];
                }
        }
    };
    constexpr bool LATE_COLS = M16;
    if constexpr (!LATE_COLS) load_cols();

#pragma unroll
    for (int t = 0; t < ST - 1; ++t)
        if (t < total) issue();

    // deferred LayerNorm: row mean / rstd of the A rows from the producer's partial sums, into the
    // LDS words behind the ring (one row per thread; the loads fly beside the first DMA tiles.  Requesting them BEFORE
    // the tiles -- so that they land first -- was measured and changes nothing: the reduction is short, what the block
    // waits for is one memory round trip either way)
    float* lnst = (float*)(lds + ST * STAGE);                         // [BM][2]
    if (p.ln_stats_in) {
        for (int r = tid; r < BM; r += NT) {
            int m = m0 + r;
            m = m < p.M ? m : p.M - 1;
            const float* ps = p.ln_stats_in + (int64_t)m * p.ln_groups * 2;
            // all partials are requested before any is consumed (up to 32 groups = 16 loads in flight)
            f32x4 pv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                pv[u] = (2 * u < p.ln_groups) ? *(const f32x4*)(ps + 4 * u) : (f32x4){0.f, 0.f, 0.f, 0.f};
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int u = 0; u < 16; ++u) { s1 += pv[u][0] + pv[u][2]; s2 += pv[u][1] + pv[u][3]; }
            const float invK = 1.0f / (float)p.K;
            const float mu = s1 * invK;
            const float var = fmaxf(s2 * invK - mu * mu, 0.f);
            lnst[2 * r] = mu;
            lnst[2 * r + 1] = rsqrtf(var + p.ln_eps);
            // absolute row mean of the A rows (their partials are relative to ln_shift): the next producer's shift
            if (p.mean_out && nt == 0 && g == 0 && m0 + r < p.M) p.mean_out[m] = mu + (p.ln_shift ? p.ln_shift[m] : 0.f);
            // (relative mean, rstd) of the rows for ser_attention's in-kernel WavLM gate, which normalises the same operand copy
            if (p.lnstat_out && nt == 0 && g == 0 && m0 + r < p.M) *(f32x2*)(p.lnstat_out + 2 * (int64_t)m) = (f32x2){mu, lnst[2 * r + 1]};
        }
        __syncthreads();
    }

    // Ping-pong schedule of the 8-wave tiles (two waves per SIMD: wave w and w + 4).  Left alone, both waves of a SIMD leave
    // the per-tile barrier together, read their fragments together and then compete for the matrix pipe together.  Here
    // waves 4..7 run ONE PHASE behind waves 0..3: a phase is either a batch of LDS reads (the fragments of one k-step for
    // the 128x64 / 64x128 wave tiles, of the whole K tile for 64x64 ones, plus this wave's share of the next DMA) or the 32
    // MFMAs that consume them; every phase ends in a barrier, so while one wave of a SIMD owns the matrix pipe the other one
    // owns the LDS port.  With PH read phases per K tile, the early half reads batch (kt, s) in global phase 2 (PH kt + s) and
    // multiplies in the next one; the late half does the same one phase later.  The stage of tile kt - 1 is last read in
    // phase 2 PH kt - 1 (late half), so both halves may refill it from their first read phase of tile kt on, and both make
    // sure tile kt + 1 has landed at the end of phase 2 PH (kt + 1) - 1, before the early half reads it.  Barrier counts match:
    // the late half has one extra up front and skips the one after its last MFMA phase -- which overlaps the early half's
    // epilogue.  Same arithmetic, same accumulation order: results are bit-identical to the plain ring.
#ifdef SER_GEMM_DBG
    const unsigned long long dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    constexpr int PP_BIT = NPL == 2 ? (LNEPI ? 16 : 8) : (LNEPI ? 4 : (TM * TN >= 32 ? 1 : 2));
    constexpr bool PP = !M16 && (SER_GEMM_PP & PP_BIT) && NW == 8 && (KS == 2 || NPL == 2);
    constexpr int PH = (NPL == 1 && TM * TN >= 32) ? KS : 1;          // read phases per K tile (FP32X: 12 fragments + 24 MFMAs per k-step, one phase)
    constexpr int SPP = KS / PH;                                      // k-steps per phase
    // FP32X tiles with 64x128 wave tiles (the LayerNorm tile: one k-step per 32-deep K tile, 24 fragments, 96 MFMAs): the two read
    // phases of a K tile are the two halves of the weight fragments (the activation fragments stay in registers across them), so
    // 64 fragment registers are live beside the 128 accumulators instead of 96
    constexpr bool PPW = PP && NPL == 2 && KS == 1 && TN >= 8;
    if constexpr (PPW) {
        constexpr int TNH = TN / 2;
        const int late = wave >> 2;
        if (total >= ST - 1) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (late) __builtin_amdgcn_s_barrier();
        int stage = 0;
        for (int kt = 0; kt < total; ++kt) {
            const bool more = kt + ST - 1 < total;
            if (more) issue();
            const char* sb = lds + stage * STAGE;
            stage = (stage + 1 == ST) ? 0 : stage + 1;
            const bool last = kt + 1 == total;
            bf16x8 ah[TM], al[TM];
#pragma unroll
            for (int ph = 0; ph < 2; ++ph) {
                bf16x8 wh[TNH], wl[TNH];
                if (ph == 0) {
#pragma unroll
                    for (int x = 0; x < TM; ++x) {
                        ah[x] = *(const bf16x8*)(sb + offA[0] + x * 16 * ROWB);
                        al[x] = *(const bf16x8*)(sb + offA[0] + A_BYTES + x * 16 * ROWB);
                    }
                }
#pragma unroll
                for (int x = 0; x < TNH; ++x) {
                    wh[x] = *(const bf16x8*)(sb + offW[0] + (ph * TNH + x) * 16 * ROWB);
                    wl[x] = *(const bf16x8*)(sb + offW[0] + W_BYTES + (ph * TNH + x) * 16 * ROWB);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (ph == 1 && late) { if (more) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>(); }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int nj = 0; nj < TNH; ++nj)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) {
                        const int ni = ph * TNH + nj;
                        acc[ni][mi] = mfma16<MODE>(wl[nj], ah[mi], acc[ni][mi]);
                        acc[ni][mi] = mfma16<MODE>(wh[nj], al[mi], acc[ni][mi]);
                        acc[ni][mi] = mfma16<MODE>(wh[nj], ah[mi], acc[ni][mi]);
                    }
                __builtin_amdgcn_s_setprio(0);
                if (ph == 1 && !late) { if (more) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>(); }
                __builtin_amdgcn_sched_barrier(0);
                if (!(ph == 1 && last && late)) __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (PP && !PPW) {
        const int late = wave >> 2;
        if (total >= ST - 1) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>();    // fewer tiles in flight when K is short
        __builtin_amdgcn_s_barrier();                                 // tile 0 is visible to every wave
        __builtin_amdgcn_sched_barrier(0);
        if (late) __builtin_amdgcn_s_barrier();
        int stage = 0;
        for (int kt = 0; kt < total; ++kt) {
            const bool more = kt + ST - 1 < total;
            if (more) issue();
            const char* sb = lds + stage * STAGE;
            stage = (stage + 1 == ST) ? 0 : stage + 1;
            const bool last = kt + 1 == total;
#pragma unroll
            for (int ph = 0; ph < PH; ++ph) {
                bf16x8 af[SPP][TM], wf[SPP][TN];
                bf16x8 al[NPL == 2 ? SPP : 1][NPL == 2 ? TM : 1], wl[NPL == 2 ? SPP : 1][NPL == 2 ? TN : 1];   // FP32X: the lo planes
#pragma unroll
                for (int u = 0; u < SPP; ++u) {
#pragma unroll
                    for (int x = 0; x < TM; ++x) {
                        af[u][x] = *(const bf16x8*)(sb + offA[ph * SPP + u] + x * 16 * ROWB);
                        if constexpr (NPL == 2) al[u][x] = *(const bf16x8*)(sb + offA[ph * SPP + u] + A_BYTES + x * 16 * ROWB);
                    }
#pragma unroll
                    for (int x = 0; x < TN; ++x) {
                        wf[u][x] = *(const bf16x8*)(sb + offW[ph * SPP + u] + x * 16 * ROWB);
                        if constexpr (NPL == 2) wl[u][x] = *(const bf16x8*)(sb + offW[ph * SPP + u] + W_BYTES + x * 16 * ROWB);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (ph == PH - 1 && late) { if (more) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>(); }
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int u = 0; u < SPP; ++u)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                        for (int mi = 0; mi < TM; ++mi) {
                            if constexpr (NPL == 2) {                     // same product order as the plain ring: lo*hi, hi*lo, hi*hi
                                acc[ni][mi] = mfma16<MODE>(wl[u][ni], af[u][mi], acc[ni][mi]);
                                acc[ni][mi] = mfma16<MODE>(wf[u][ni], al[u][mi], acc[ni][mi]);
                                acc[ni][mi] = mfma16<MODE>(wf[u][ni], af[u][mi], acc[ni][mi]);
                            } else {
                                acc[ni][mi] = mfma16<MODE>(wf[u][ni], af[u][mi], acc[ni][mi]);
                            }
                        }
                __builtin_amdgcn_s_setprio(0);
                if (ph == PH - 1 && !late) { if (more) wait_vmcnt<LPT * (ST - 2)>(); else wait_vmcnt<0>(); }
                __builtin_amdgcn_sched_barrier(0);
                if (!(ph == PH - 1 && last && late)) __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    // ---- FP16M: per 64-deep K tile one H unit (fp16 hi planes: the two f16 k-steps of the single-plane loop) and one E unit (e4m3
    // cross-term planes: each lane's 32 operand bytes are chunks fq and fq + 4 of its row -- the addresses of the two k-steps -- and
    // its scale byte is byte fq of the row's scale word; the instruction pairs chunk c of the weights with chunk c of the activations
    // and applies the scale of lane group b to chunks 2b, 2b + 1: [P cols 0-31, P cols 32-63, Q cols 0-31, Q cols 32-63], tools/mxprobe.hip).
    // Same ring, same ping-pong phases as the single-plane tiles; an E phase of the 256x128 / 128x128 tiles is TM x TN = 16 scaled MFMAs = the
    // matrix-pipe time of the 32 f16 MFMAs of its H phase.
    if constexpr (M16) {
        constexpr int LPTH = LPT, LPTE = LPT + 1;
        constexpr bool PPM = (NW == 8);
        constexpr int PHM = (TM * TN >= 32) ? 2 : 1;                  // phases per unit (256x256: two, like its bf16 form)
        constexpr int SPM = KS / PHM;                                 // H unit: k-steps per phase
        // E unit: phases and activation row fragments per phase
        constexpr int PHE = PHM;
        constexpr int TMP = TM / PHE;
        // unit kt has landed once at most the youngest unit (kt + ST - 1 ... only ST = 2, 3 exist) is still in flight
        auto wait_landed = [&](bool more, int young) {
            if (!more || ST == 2) wait_vmcnt<0>();
            else if (young & 1) wait_vmcnt<LPTE * (ST - 2)>();
            else wait_vmcnt<LPTH * (ST - 2)>();
        };
        auto h_phase_reads = [&](const char* sb, int ph, auto& af, auto& wf) {
#pragma unroll
            for (int u = 0; u < SPM; ++u) {
#pragma unroll
                for (int x = 0; x < TM; ++x) af[u][x] = *(const bf16x8*)(sb + offA[ph * SPM + u] + x * 16 * ROWB);
#pragma unroll
                for (int x = 0; x < TN; ++x) wf[u][x] = *(const bf16x8*)(sb + offW[ph * SPM + u] + x * 16 * ROWB);
            }
        };
        auto h_phase_mfma = [&](auto& af, auto& wf) {
#pragma unroll
            for (int u = 0; u < SPM; ++u)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) acc[ni][mi] = mfma16<SER_MODE_FP16>(wf[u][ni], af[u][mi], acc[ni][mi]);
        };
        auto e_phase_reads = [&](const char* sb, const unsigned char* scb, int ph, auto& a8, auto& w8, auto& sa, auto& sw) {
#pragma unroll
            for (int x = 0; x < TMP; ++x) {
                const int mi = ph * TMP + x;
                const u32x4 c0 = *(const u32x4*)(sb + offA[0] + mi * 16 * ROWB), c1 = *(const u32x4*)(sb + offA[1] + mi * 16 * ROWB);
                a8[x] = (i32x8){(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
                sa[x] = scb[(wm * TM * 16 + mi * 16 + frow) * 4 + fq];
            }
#pragma unroll
            for (int x = 0; x < TN; ++x) {
                const u32x4 c0 = *(const u32x4*)(sb + offW[0] + x * 16 * ROWB), c1 = *(const u32x4*)(sb + offW[1] + x * 16 * ROWB);
                w8[x] = (i32x8){(int)c0[0], (int)c0[1], (int)c0[2], (int)c0[3], (int)c1[0], (int)c1[1], (int)c1[2], (int)c1[3]};
                sw[x] = scb[(BM + wn * TN * 16 + x * 16 + frow) * 4 + fq];
            }
        };
        auto e_phase_mfma = [&](int ph, auto& a8, auto& w8, auto& sa, auto& sw) {
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int x = 0; x < TMP; ++x)
                    mfma_scale8(acc[ni][ph * TMP + x], w8[ni], a8[x], sw[ni], sa[x]);
        };
        // (the two kinds of unit are separate instantiations of one lambda, called alternately: with a run-time parity branch around the
        // phase bodies hipcc kept both fragment sets live and spilled 160 - 540 registers)
        if constexpr (PPM) {
            const int late = wave >> 2;
            wait_landed(total >= ST - 1, ST - 2);                         // units 0 .. ST-2 are in flight; unit 0 has landed
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if (late) __builtin_amdgcn_s_barrier();
            int stage = 0;
            auto unit = [&](int kt, auto etag) {
                constexpr bool EU = decltype(etag)::value;
                const bool more = kt + ST - 1 < total;
#ifdef SER_GEMM_DBG
                unsigned long long stp[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // phase stamps of units 8 .. 15 of one block (tools/gemm_m16_phases.py)
                const bool stamp = ser_gemm_dbg_dev && blockIdx.x == 40 && lane == 0 && kt >= 8 && kt < 16;
#define SER_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (stamp) stp[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
                SER_STAMP(0);
#else
#define SER_STAMP(i) do { } while (0)
#endif
                SER_STAMP(1);                                      // DMAs of unit kt + ST - 1 issued
                const char* sb = lds + stage * STAGE;
                const unsigned char* scb = scl + stage * SCW * 4;
                stage = (stage + 1 == ST) ? 0 : stage + 1;
                const bool last = kt + 1 == total;
                constexpr int NPH = EU ? PHE : PHM;
#pragma unroll
                for (int ph = 0; ph < NPH; ++ph) {
                    bf16x8 af[EU ? 1 : SPM][EU ? 1 : TM], wf[EU ? 1 : SPM][EU ? 1 : TN];
                    i32x8 a8[EU ? TMP : 1], w8[EU ? TN : 1];
                    int sa[EU ? TMP : 1], sw[EU ? TN : 1];
                    if constexpr (!EU) h_phase_reads(sb, ph, af, wf);
                    else e_phase_reads(sb, scb, ph, a8, w8, sa, sw);
                    // the DMAs of unit kt + ST - 1 go out BEHIND the fragment reads of the unit's first phase: the LDS latency of those reads
                    // passes under the ~350 cycles the DMA issue holds the wave (the stage they refill was last read one unit ago)
                    if (ph == 0 && more) { __builtin_amdgcn_sched_barrier(0); issue(); }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (ph == 0) SER_STAMP(2);                      // fragments in registers
                    if (ph == NPH - 1 && late) wait_landed(more, kt + ST - 1);
                    if (ph == 0) SER_STAMP(3);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    if (ph == 0) SER_STAMP(4);                      // past the barrier in front of the MFMA phase
                    __builtin_amdgcn_s_setprio(1);
                    if constexpr (!EU) h_phase_mfma(af, wf);
                    else e_phase_mfma(ph, a8, w8, sa, sw);
                    __builtin_amdgcn_s_setprio(0);
                    if (ph == 0) SER_STAMP(5);                      // MFMAs issued
                    if (ph == NPH - 1 && !late) wait_landed(more, kt + ST - 1);
                    if (ph == 0) SER_STAMP(6);
                    __builtin_amdgcn_sched_barrier(0);
                    if (!(ph == NPH - 1 && last && late)) __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    if (ph == 0) SER_STAMP(7);
                }
#ifdef SER_GEMM_DBG
                if (stamp) for (int i = 0; i < 8; ++i) ser_gemm_dbg_dev[262144 + ((wave * 8 + (kt - 8)) * 8 + i)] = stp[i];
#endif
            };
            for (int kt = 0; kt < total; kt += 2) {
                unit(kt, std::false_type{});
                unit(kt + 1, std::true_type{});
            }
        } else {
            int stage = 0;
            auto unit = [&](int kt, auto etag) {
                constexpr bool EU = decltype(etag)::value;
                wait_landed(kt + (ST - 2) < total, kt + ST - 2);
                __builtin_amdgcn_s_barrier();
                if (kt + ST - 1 < total) issue();
                const char* sb = lds + stage * STAGE;
                const unsigned char* scb = scl + stage * SCW * 4;
                stage = (stage + 1 == ST) ? 0 : stage + 1;
#pragma unroll
                for (int ph = 0; ph < (EU ? PHE : PHM); ++ph) {
                    if constexpr (!EU) {
                        bf16x8 af[SPM][TM], wf[SPM][TN];
                        h_phase_reads(sb, ph, af, wf);
                        __builtin_amdgcn_s_setprio(1);
                        h_phase_mfma(af, wf);
                        __builtin_amdgcn_s_setprio(0);
                    } else {
                        i32x8 a8[TMP], w8[TN];
                        int sa[TMP], sw[TN];
                        e_phase_reads(sb, scb, ph, a8, w8, sa, sw);
                        __builtin_amdgcn_s_setprio(1);
                        e_phase_mfma(ph, a8, w8, sa, sw);
                        __builtin_amdgcn_s_setprio(0);
                    }
                }
            };
            for (int kt = 0; kt < total; kt += 2) {
                unit(kt, std::false_type{});
                unit(kt + 1, std::true_type{});
            }
        }
    }
    // (the 256x256 tile on four waves with a hand-placed software pipeline, and the same pipeline on the 8-wave tiles: DEADENDS.md)
    if constexpr (M16) mfma_scale_drain();
    int c_stage = 0;
    for (int kt = 0; kt < ((PP || M16) ? 0 : total); ++kt) {
        // tile kt has landed once at most (ST-2) younger tiles are still in flight
        if (kt + (ST - 2) < total) wait_vmcnt<LPT * (ST - 2)>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (kt + ST - 1 < total) issue();           // refills the stage every wave finished reading before the barrier
        const char* sb = lds + c_stage * STAGE;
        c_stage = (c_stage + 1 == ST) ? 0 : c_stage + 1;
        if constexpr (NPL == 1) {
            // all k-steps' fragments are requested up front: the LDS reads of step s+1 complete under the
            // MFMAs of step s (the compiler places counted lgkmcnt waits between the clusters)
            // (PIPE; the 128x64-per-wave configuration has no registers to spare and loads per step)
            constexpr bool PIPE = (TM * TN * 4 + KS * (TM + TN) * 4) <= 208;
            bf16x8 af[KS][TM], wf[KS][TN];
            if constexpr (PIPE) {
#pragma unroll
                for (int s = 0; s < KS; ++s) {
#pragma unroll
                    for (int x = 0; x < TM; ++x) af[s][x] = *(const bf16x8*)(sb + offA[s] + x * 16 * ROWB);
#pragma unroll
                    for (int x = 0; x < TN; ++x) wf[s][x] = *(const bf16x8*)(sb + offW[s] + x * 16 * ROWB);
                }
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if constexpr (!PIPE) {
#pragma unroll
                    for (int x = 0; x < TM; ++x) af[s][x] = *(const bf16x8*)(sb + offA[s] + x * 16 * ROWB);
#pragma unroll
                    for (int x = 0; x < TN; ++x) wf[s][x] = *(const bf16x8*)(sb + offW[s] + x * 16 * ROWB);
                }
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi)
                        acc[ni][mi] = mfma16<MODE>(wf[s][ni], af[s][mi], acc[ni][mi]);
                __builtin_amdgcn_s_setprio(0);
            }
        } else {
            // FP32X: 4 fragment sets per k-step, 3 products per (weight, activation) sub-tile pair
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                bf16x8 ah[TM], al[TM], wh[TN], wl[TN];
#pragma unroll
                for (int x = 0; x < TM; ++x) {
                    ah[x] = *(const bf16x8*)(sb + offA[s] + x * 16 * ROWB);
                    al[x] = *(const bf16x8*)(sb + offA[s] + A_BYTES + x * 16 * ROWB);
                }
#pragma unroll
                for (int x = 0; x < TN; ++x) {
                    wh[x] = *(const bf16x8*)(sb + offW[s] + x * 16 * ROWB);
                    wl[x] = *(const bf16x8*)(sb + offW[s] + W_BYTES + x * 16 * ROWB);
                }
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) {
                        acc[ni][mi] = mfma16<MODE>(wl[ni], ah[mi], acc[ni][mi]);
                        acc[ni][mi] = mfma16<MODE>(wh[ni], al[mi], acc[ni][mi]);
                        acc[ni][mi] = mfma16<MODE>(wh[ni], ah[mi], acc[ni][mi]);
                    }
                __builtin_amdgcn_s_setprio(0);
            }
        }
    }

#ifdef SER_GEMM_DBG
    {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        unsigned long long* d = ser_gemm_dbg_dev;
        if (d && wave == 0 && lane == 0 && blockIdx.y == 0) {
            d[blockIdx.x * 2] = t1 - dbg_t0; d[blockIdx.x * 2 + 1] = r1 - dbg_r0;
            d[131072 + blockIdx.x * 4] = dbg_t0 - dbg_e0; d[131072 + blockIdx.x * 4 + 1] = t1;
        }
    }
#endif
    if constexpr (LATE_COLS) load_cols();
    // ---- epilogue: lane owns row m (per mi) and TN*4 consecutive columns ----------------------
    float ramax = 0.f;                            // largest |value| this lane rounded to an fp16 operand plane (range guard)
    if constexpr (LNEPI) {
        // LayerNorm over the full row (N <= BN, one N tile) + GELU, two-pass statistics.
        // Row partials cross the WN waves of a block row through LDS (the ring is idle now).
        __syncthreads();
        float* red = (float*)lds;                                     // [BM][WN][2]
        const float invN = 1.0f / (float)p.N;
        float mean[TM], rstd[TM], nmr[TM];
        // one exchange: per-row (sum, sum of squares) partials of the WN waves of a block row.
        // (fp32 accumulators, |mean| << std for conv outputs: E[x^2]-mean^2 is safe here)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float x = acc[ni][mi][r] + bias[ni * 4 + r];
                    acc[ni][mi][r] = x;
                    if (ncol0 + ni * 16 < p.N) { s1 += x; s2 += x * x; }
                }
            s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (fq == 0) {
                red[((wm * TM * 16 + mi * 16 + frow) * WN + wn) * 2] = s1;
                red[((wm * TM * 16 + mi * 16 + frow) * WN + wn) * 2 + 1] = s2;
            }
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < WN; ++w) {
                s1 += red[((wm * TM * 16 + mi * 16 + frow) * WN + w) * 2];
                s2 += red[((wm * TM * 16 + mi * 16 + frow) * WN + w) * 2 + 1];
            }
            mean[mi] = s1 * invN;
            rstd[mi] = rsqrtf(fmaxf(s2 * invN - mean[mi] * mean[mi], 0.f) + p.ln_eps);
            nmr[mi] = -mean[mi] * rstd[mi];                            // (x - mean) * rstd = fma(x, rstd, nmr)
        }
        float lg[CPL], lb[CPL];
#pragma unroll
        for (int j4 = 0; j4 < TN; ++j4) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (ncol0 + j4 * 16 < p.N) {
                a = *(const f32x4*)(p.ln_gamma + ncol0 + j4 * 16);
                b = *(const f32x4*)(p.ln_beta + ncol0 + j4 * 16);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) { lg[j4 * 4 + r] = a[r]; lb[j4 * 4 + r] = b[r]; }
        }
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            const int m = m0 + wm * TM * 16 + mi * 16 + frow;
            if (m >= p.M) continue;
            const int64_t orow = p.out_rowmap ? (int64_t)p.out_rowmap[m] : (int64_t)m;
#pragma unroll
            for (int ni = 0; ni < TN; ni += 2) {                      // fragment column blocks ni, ni+1: 4 + 4 columns
                const bool ok0 = ncol0 + ni * 16 < p.N, ok1 = ncol0 + ni * 16 + 16 < p.N;
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int nj = ni + (r >> 2), rr = r & 3;
                    v[r] = fmaf(fmaf(acc[nj][mi][rr], rstd[mi], nmr[mi]), lg[nj * 4 + rr], lb[nj * 4 + rr]);   // 2 FMAs
                }
                if (p.act == SER_ACT_GELU) {
#pragma unroll
                    for (int r = 0; r < 8; r += 2) {
                        const f32x2 y = gelu2<MODE == SER_MODE_BF16>((f32x2){v[r], v[r + 1]});
                        v[r] = y[0]; v[r + 1] = y[1];
                    }
                }
                if (p.out_f32) {
                    f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
                    if (ok0) *(f32x4*)(p.out_f32 + (int64_t)m * p.ldo_f32 + gcol + ni * 16) = o0;
                    if (ok1) *(f32x4*)(p.out_f32 + (int64_t)m * p.ldo_f32 + gcol + ni * 16 + 16) = o1;
                }
                if (p.out_act) {
                    const int c8 = ni * 16 + ((fq & 1) ? 12 : 0);     // after the swap this lane holds columns c8..c8+7
                    store_act8_swap<MODE>((unsigned short*)p.out_act + orow * p.ldo_act + gcol + c8, p.out_plane_stride,
                                          ncol0 + c8 < p.N, v);
                    if constexpr (mode_traits<MODE>::f16) {           // fp16 range guard (ser_hip.h range_flag): stored columns only
                        if (p.range_flag) range_fold8(ramax, v, ok0, ok1);
                    }
                }
            }
        }
    } else if constexpr (EPI == GEMM_EPI_GENERIC) {
        // wave-uniform feature flags: the column scale and the row partial sums cost 2 VALU each per element, and
        // most launches use neither (the epilogue is VALU-bound where it carries a GELU)
        const bool do_scale = p.col_scale_end > 0;
        const bool do_stat = p.stat_out != nullptr;
        // SHIFTED operand copy (ser_hip.h): c[m] = absolute row mean of the residual input + a load-time constant.  The
        // act copy and the row partials written below hold v - c[m], so rows whose mean is many standard deviations
        // (offsets living in the residual stream) still round to bf16 relative to their spread, and the consumer's
        // E[x^2] - mean^2 does not cancel.  LayerNorm is shift invariant: the consumer needs no change.
        float cs[TM];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            cs[mi] = 0.f;
            if (p.shift_out) {
                int m = m0 + wm * TM * 16 + mi * 16 + frow;
                m = m < p.M ? m : p.M - 1;
                cs[mi] = p.shift_const + (p.shift_in ? p.shift_in[m] : 0.f);
            }
        }
        // The residual tile is requested a batch of 4 fragment rows at a time, BEFORE that batch's first store: the
        // residual may be the output buffer itself (next state, written in place), so the compiler cannot move a row's
        // loads above the previous row's stores, and the epilogue used to pay the load latency (HBM / Infinity Cache:
        // 1-2 us) once per fragment row -- four to eight times per block.  The fragment registers of the K loop are dead
        // here, so the 64 registers of a batch cost no occupancy.  (A lane reads and writes only its own elements: moving
        // its loads ahead of its stores to OTHER rows cannot change what it reads.)
        constexpr int RB = (TM * TN > 16) ? 2 : (TM < 4 ? TM : 4);          // 256x256 tile (128 accumulators): 32 registers per batch
        f32x4 rres[RB][TN];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            if (mi % RB == 0 && p.residual) {
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    int mr = m0 + wm * TM * 16 + (mi + u) * 16 + frow;
                    mr = mr < p.M ? mr : p.M - 1;
                    const int rr_ = p.res_row_mod ? (mr % p.res_row_mod) : mr;
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        f32x4 r = {0.f, 0.f, 0.f, 0.f};
                        if (ncol0 + ni * 16 < p.N) r = *(const f32x4*)(p.residual + (int64_t)rr_ * p.ldr + gcol + ni * 16);
                        rres[u][ni] = r;
                    }
                }
            }
            const int m = m0 + wm * TM * 16 + mi * 16 + frow;
            if (m >= p.M) continue;
            const int64_t orow = p.out_rowmap ? (int64_t)p.out_rowmap[m] : (int64_t)m;
            float mu = 0.f, rs = 1.f;
            if (p.ln_stats_in) {
                mu = lnst[2 * (wm * TM * 16 + mi * 16 + frow)];
                rs = lnst[2 * (wm * TM * 16 + mi * 16 + frow) + 1];
            }
            const float cshift = cs[mi];
            if (p.shift_out && nt == 0 && g == 0 && wn == 0 && fq == 0) p.shift_out[m] = cshift;
            // GroupNorm-over-time stem (ABI 15): per-(utterance, column) affine of the row's utterance; a tile may straddle utterances, so
            // each row finds its own (binary search of gn_row_offs, wave-uniform flag: launches without it pay one branch)
            const float* gsc = nullptr;
            const float* gsh = nullptr;
            if (p.gn_scale) {
                int lo = 0, hi = p.gn_B;                              // largest u with gn_row_offs[u] <= m
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.gn_row_offs[mid] <= m) lo = mid; else hi = mid; }
                gsc = p.gn_scale + (int64_t)lo * p.gn_ld + ncol0;
                gsh = p.gn_shift + (int64_t)lo * p.gn_ld + ncol0;
            }
            float st1 = 0.f, st2 = 0.f;
            unsigned mcode[2] = {0u, 0u};                             // FP16M out copy: (P, Q) codes of the two blocks of a 64-column tile
#pragma unroll
            for (int ni = 0; ni < TN; ni += 2) {                      // fragment column blocks ni, ni+1: 4 + 4 columns
                const bool ok0 = ncol0 + ni * 16 < p.N, ok1 = ncol0 + ni * 16 + 16 < p.N;
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int nj = ni + (r >> 2), rr = r & 3;
                    // LN(x) W^T = rstd * (x W'^T - mu * colsum(W')) + (beta W^T + b)
                    float x = fmaf(rs, acc[nj][mi][rr] - mu * csum[nj * 4 + rr], bias[nj * 4 + rr]);
                    if (gsc && ncol0 + nj * 16 < p.N) x = fmaf(x, gsc[nj * 16 + rr], gsh[nj * 16 + rr]);   // GroupNorm: (acc + b) * gamma*rstd + (beta - mean*gamma*rstd)
                    if (do_scale && ncol0 + nj * 16 < p.col_scale_end) x *= p.col_scale;   // e.g. q *= dh^-0.5 * log2(e)
                    v[r] = x;
                }
                if (p.act == SER_ACT_GELU) {
#pragma unroll
                    for (int r = 0; r < 8; r += 2) {
                        const f32x2 y = gelu2<MODE == SER_MODE_BF16>((f32x2){v[r], v[r + 1]});
                        v[r] = y[0]; v[r + 1] = y[1];
                    }
                }
                if (p.residual) {
                    const f32x4 r0 = rres[mi % RB][ni], r1 = rres[mi % RB][ni + 1];
                    v[0] += r0[0]; v[1] += r0[1]; v[2] += r0[2]; v[3] += r0[3];
                    v[4] += r1[0]; v[5] += r1[1]; v[6] += r1[2]; v[7] += r1[3];
                }
                if (p.out_f32) {
                    float* op = p.out_f32 + (int64_t)m * p.ldo_f32 + gcol + ni * 16 - p.f32_col_begin;
                    f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
                    if (ok0 && ncol0 + ni * 16 >= p.f32_col_begin) *(f32x4*)op = o0;
                    if (ok1 && ncol0 + ni * 16 + 16 >= p.f32_col_begin) *(f32x4*)(op + 16) = o1;
                }
                if (p.shift_out) {                                    // wave-uniform; the fp32 output above stays unshifted
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[r] -= cshift;
                }
                if (do_stat && ok0) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { st1 += v[r]; st2 += v[r] * v[r]; }
                }
                if (do_stat && ok1) {
#pragma unroll
                    for (int r = 4; r < 8; ++r) { st1 += v[r]; st2 += v[r] * v[r]; }
                }
                if (p.out_act) {
                    const int c8 = ni * 16 + ((fq & 1) ? 12 : 0);     // after the swap this lane holds columns c8..c8+7
                    if constexpr (OM == SER_MODE_FP16M) {
                        // hi plane = the fp16 copy; cross-term plane: P = v - hi, Q = v as e4m3 with one power-of-two scale per 32 columns
                        // (this fragment pair = one block: the four lanes of the row hold 8 of its columns each)
                        store_act8_swap<SER_MODE_FP16>((unsigned short*)p.out_act + orow * p.ldo_act + gcol + c8, 0, ncol0 + c8 < p.N, v);
                        float lo[8], ax = 0.f, al = 0.f;
#pragma unroll
                        for (int r = 0; r < 8; r += 2) {
                            const unsigned h2 = pack_h2(v[r], v[r + 1]);
                            lo[r] = v[r] - h2f((unsigned short)(h2 & 0xffffu));
                            lo[r + 1] = v[r + 1] - h2f((unsigned short)(h2 >> 16));
                            ax = fmaxf(ax, fmaxf(fabsf(v[r]), fabsf(v[r + 1])));
                            al = fmaxf(al, fmaxf(fabsf(lo[r]), fabsf(lo[r + 1])));
                        }
                        // range guard: stored columns only (N % 64 == 0: a block is stored whole or not at all, so its scales see no tail)
                        if (p.range_flag) range_fold8(ramax, v, ok0, ok1);
                        ax = max_rowquad(ax); al = max_rowquad(al);
                        const unsigned cx = mx_code(ax), cl = mx_code(al);
                        const float ix = mx_inv(cx), il = mx_inv(cl);
                        unsigned q4[4] = {mx_pack4(lo[0] * il, lo[1] * il, lo[2] * il, lo[3] * il), mx_pack4(lo[4] * il, lo[5] * il, lo[6] * il, lo[7] * il),
                                          mx_pack4(v[0] * ix, v[1] * ix, v[2] * ix, v[3] * ix), mx_pack4(v[4] * ix, v[5] * ix, v[6] * ix, v[7] * ix)};
                        transpose_rowquad(q4);        // lane group fq now holds 16 consecutive bytes: P cols 0-15 | P 16-31 | Q 0-15 | Q 16-31 of the block
                        const int64_t bcol = gcol - fq * 4 + ni * 16;                    // the block's first output column
                        unsigned char* seg = (unsigned char*)((unsigned short*)p.out_act + p.out_plane_stride) + (orow * p.ldo_act + (bcol & ~(int64_t)63)) * 2;
                        if (ok0) *(u32x4*)(seg + (fq >> 1) * 64 + (bcol & 63) + (fq & 1) * 16) = (u32x4){q4[0], q4[1], q4[2], q4[3]};
                        mcode[(ni >> 1) & 1] = cl | (cx << 16);
                        if (((ni >> 1) & 1) && fq == 0 && ok0)                            // second block of a 64-column tile: its scale word
                            p.out_scale[(bcol >> 6) * p.out_scale_ld + orow] = (mcode[0] & 0xffu) | ((mcode[1] & 0xffu) << 8) | (mcode[0] & 0xff0000u) | ((mcode[1] & 0xff0000u) << 8);
                    } else {
                        store_act8_swap<OM>((unsigned short*)p.out_act + orow * p.ldo_act + gcol + c8, p.out_plane_stride,
                                            ncol0 + c8 < p.N, v);
                        if constexpr (mode_traits<OM>::f16) {             // fp16 range guard (ser_hip.h range_flag): stored columns only
                            if (p.range_flag) range_fold8(ramax, v, ok0, ok1);
                        }
                    }
                }
            }
            if (p.stat_out) {
                // row partials over this wave's columns (deterministic: one slot per 64-column group).  A 128-column wave tile (the
                // 3-product 256x256 tile) puts its partials in the first of its two slots and ZEROES in the second: every slot of the
                // columns a launch covers is written.  When it left the second slot alone, a buffer whose rows another launch shape had
                // filled before (the output projection's partials of "f16mf" with SER_F16M_OUT_M=1: FP16X layers, then FP16M layers,
                // then the next forward's FP16X layers) fed those stale values to the consumer's LayerNorm.
                st1 += __shfl_xor(st1, 16, 64); st2 += __shfl_xor(st2, 16, 64);
                st1 += __shfl_xor(st1, 32, 64); st2 += __shfl_xor(st2, 32, 64);
                const int cstart = n0 + wn * (TN * 16);
                const int grp = g * ((p.N + 63) >> 6) + (cstart >> 6);
                if (fq == 0 && cstart < p.N && grp < p.stat_groups) {
                    float* d = p.stat_out + ((int64_t)m * p.stat_groups + grp) * 2;
                    d[0] = st1; d[1] = st2;
                    if constexpr (TN * 16 > 64) {
                        if (cstart + 64 < p.N) { d[2] = 0.f; d[3] = 0.f; }     // (a second half past N: a padding slot, never written)
                    }
                }
            }
        }
    } else {
        // The specialised epilogue classes (launch_plan.h, gemm_pick_epi): the GENERIC body above with the features a class never has taken
        // out at compile time and the ones it always has without their test.  Left as run-time tests, hipcc turns the cheap features into
        // unconditional instructions + v_cndmask per element and wraps the lane-dependent ones in exec-mask branches that cut the GELU chains
        // into 8-element scheduling regions -- in every launch, also those (FC1, the packed projection) that use none of them.  What a taken
        // path computes per element is the GENERIC body's arithmetic in the same order: results are bit-identical
        // (tests/test_gpu_gemm_epilogue_classes.py).
        //   LN_ACT: deferred-LayerNorm transform, column scale / GELU decided per block, operand copy only;
        //   RESID:  acc + bias (the transform with mu = 0, rstd = 1, exactly), residual, fp32 output at column 0; the operand copy, its
        //           shift and the row partials stay wave-uniform run-time tests.
        constexpr bool LNA = EPI == GEMM_EPI_LN_ACT, RES = EPI == GEMM_EPI_RESID;
        static_assert(LNA || RES, "epilogue class");
        // the 64-bit output column is formed here, behind the K loop: at 256 registers (256x256 tile) hipcc otherwise spills it across the loop
        int ncol_e = ncol0;
        asm volatile("" : "+v"(ncol_e));
        const int64_t gcol = (int64_t)g * p.c_group_stride + ncol_e;
        const bool do_scale = p.col_scale_end > 0;
        const bool f_copy = LNA || p.out_act;
        const bool f_shift = RES && p.shift_out;
        const bool do_stat = RES && p.stat_out != nullptr;
        float cs[TM];
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
            cs[mi] = 0.f;
            if (f_shift) {
                int m = m0 + wm * TM * 16 + mi * 16 + frow;
                m = m < p.M ? m : p.M - 1;
                cs[mi] = p.shift_const + (p.shift_in ? p.shift_in[m] : 0.f);
            }
        }
        constexpr int RB = (TM * TN > 16) ? 2 : (TM < 4 ? TM : 4);          // the batched residual request, as above
        // The rows of the tile.  ACT (GELU) and SCL (column scale) are 0 = off, 1 = on for every element, 2 = the GENERIC body's run-time
        // test per fragment / per lane: both are decided ONCE per block, below, and the variant without the test runs.
        auto rows = [&](auto act_tag, auto scl_tag) {
            constexpr int ACT = decltype(act_tag)::value, SCL = decltype(scl_tag)::value;
            f32x4 rres[RB][TN];
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
                if (RES && mi % RB == 0) {
#pragma unroll
                    for (int u = 0; u < RB; ++u) {
                        int mr = m0 + wm * TM * 16 + (mi + u) * 16 + frow;
                        mr = mr < p.M ? mr : p.M - 1;
                        const int rr_ = p.res_row_mod ? (mr % p.res_row_mod) : mr;
#pragma unroll
                        for (int ni = 0; ni < TN; ++ni) {
                            f32x4 r = {0.f, 0.f, 0.f, 0.f};
                            if (ncol0 + ni * 16 < p.N) r = *(const f32x4*)(p.residual + (int64_t)rr_ * p.ldr + gcol + ni * 16);
                            rres[u][ni] = r;
                        }
                    }
                }
                const int m = m0 + wm * TM * 16 + mi * 16 + frow;
                if (m >= p.M) continue;
                const int64_t orow = p.out_rowmap ? (int64_t)p.out_rowmap[m] : (int64_t)m;
                float mu = 0.f, rs = 1.f;
                if (LNA) {
                    mu = lnst[2 * (wm * TM * 16 + mi * 16 + frow)];
                    rs = lnst[2 * (wm * TM * 16 + mi * 16 + frow) + 1];
                }
                const float cshift = cs[mi];
                if (f_shift && nt == 0 && g == 0 && wn == 0 && fq == 0) p.shift_out[m] = cshift;
                // the row's output addresses, once per fragment row
                float* const f32row = RES ? p.out_f32 + (int64_t)m * p.ldo_f32 + gcol : nullptr;
                unsigned short* const actrow = f_copy ? (unsigned short*)p.out_act + orow * p.ldo_act + gcol : nullptr;
                float st1 = 0.f, st2 = 0.f;
                unsigned mcode[2] = {0u, 0u};                             // FP16M out copy: (P, Q) codes of the two blocks of a 64-column tile
#pragma unroll
                for (int ni = 0; ni < TN; ni += 2) {                      // fragment column blocks ni, ni+1: 4 + 4 columns
                    const bool ok0 = ncol0 + ni * 16 < p.N, ok1 = ncol0 + ni * 16 + 16 < p.N;
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int nj = ni + (r >> 2), rr = r & 3;
                        // LN(x) W^T = rstd * (x W'^T - mu * colsum(W')) + (beta W^T + b)
                        float x = RES ? acc[nj][mi][rr] + bias[nj * 4 + rr] : fmaf(rs, acc[nj][mi][rr] - mu * csum[nj * 4 + rr], bias[nj * 4 + rr]);
                        if (SCL == 2 && do_scale && ncol0 + nj * 16 < p.col_scale_end) x *= p.col_scale;   // e.g. q *= dh^-0.5 * log2(e)
                        if constexpr (SCL == 1) {
                            // the ROUNDED product, as the conditional form above gives it: left visible, hipcc fuses this multiply into the
                            // v - hi of the two-plane / FP16M copies (one rounding instead of two: another lo plane than GENERIC's)
                            x *= p.col_scale;
                            asm("" : "+v"(x));
                        }
                        v[r] = x;
                    }
                    if (ACT == 1 || (ACT == 2 && p.act == SER_ACT_GELU)) {
#pragma unroll
                        for (int r = 0; r < 8; r += 2) {
                            const f32x2 y = gelu2<MODE == SER_MODE_BF16>((f32x2){v[r], v[r + 1]});
                            v[r] = y[0]; v[r + 1] = y[1];
                        }
                    }
                    if constexpr (RES) {
                        const f32x4 r0 = rres[mi % RB][ni], r1 = rres[mi % RB][ni + 1];
                        v[0] += r0[0]; v[1] += r0[1]; v[2] += r0[2]; v[3] += r0[3];
                        v[4] += r1[0]; v[5] += r1[1]; v[6] += r1[2]; v[7] += r1[3];
                    }
                    if constexpr (RES) {
                        float* op = f32row + ni * 16;
                        f32x4 o0 = {v[0], v[1], v[2], v[3]}, o1 = {v[4], v[5], v[6], v[7]};
                        if (ok0) *(f32x4*)op = o0;
                        if (ok1) *(f32x4*)(op + 16) = o1;
                    }
                    if (f_shift) {                                        // wave-uniform; the fp32 output above stays unshifted
#pragma unroll
                        for (int r = 0; r < 8; ++r) v[r] -= cshift;
                    }
                    if (do_stat && ok0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) { st1 += v[r]; st2 += v[r] * v[r]; }
                    }
                    if (do_stat && ok1) {
#pragma unroll
                        for (int r = 4; r < 8; ++r) { st1 += v[r]; st2 += v[r] * v[r]; }
                    }
                    if (f_copy) {
                        const int c8 = ni * 16 + ((fq & 1) ? 12 : 0);     // after the swap this lane holds columns c8..c8+7
                        if constexpr (OM == SER_MODE_FP16M) {
                            // hi plane = the fp16 copy; cross-term plane: P = v - hi, Q = v as e4m3 with one power-of-two scale per 32 columns
                            // (this fragment pair = one block: the four lanes of the row hold 8 of its columns each)
                            store_act8_swap<SER_MODE_FP16>(actrow + c8, 0, ncol0 + c8 < p.N, v);
                            float lo[8], ax = 0.f, al = 0.f;
#pragma unroll
                            for (int r = 0; r < 8; r += 2) {
                                const unsigned h2 = pack_h2(v[r], v[r + 1]);
                                lo[r] = v[r] - h2f((unsigned short)(h2 & 0xffffu));
                                lo[r + 1] = v[r + 1] - h2f((unsigned short)(h2 >> 16));
                                ax = fmaxf(ax, fmaxf(fabsf(v[r]), fabsf(v[r + 1])));
                                al = fmaxf(al, fmaxf(fabsf(lo[r]), fabsf(lo[r + 1])));
                            }
                            // range guard: stored columns only (N % 64 == 0: a block is stored whole or not at all, so its scales see no tail)
                            if (p.range_flag) range_fold8(ramax, v, ok0, ok1);
                            ax = max_rowquad(ax); al = max_rowquad(al);
                            const unsigned cx = mx_code(ax), cl = mx_code(al);
                            const float ix = mx_inv(cx), il = mx_inv(cl);
                            unsigned q4[4] = {mx_pack4(lo[0] * il, lo[1] * il, lo[2] * il, lo[3] * il), mx_pack4(lo[4] * il, lo[5] * il, lo[6] * il, lo[7] * il),
                                              mx_pack4(v[0] * ix, v[1] * ix, v[2] * ix, v[3] * ix), mx_pack4(v[4] * ix, v[5] * ix, v[6] * ix, v[7] * ix)};
                            transpose_rowquad(q4);        // lane group fq now holds 16 consecutive bytes: P cols 0-15 | P 16-31 | Q 0-15 | Q 16-31 of the block
                            const int64_t bcol = gcol - fq * 4 + ni * 16;                    // the block's first output column
                            unsigned char* seg = (unsigned char*)((unsigned short*)p.out_act + p.out_plane_stride) + (orow * p.ldo_act + (bcol & ~(int64_t)63)) * 2;
                            if (ok0) *(u32x4*)(seg + (fq >> 1) * 64 + (bcol & 63) + (fq & 1) * 16) = (u32x4){q4[0], q4[1], q4[2], q4[3]};
                            mcode[(ni >> 1) & 1] = cl | (cx << 16);
                            if (((ni >> 1) & 1) && fq == 0 && ok0)                            // second block of a 64-column tile: its scale word
                                p.out_scale[(bcol >> 6) * p.out_scale_ld + orow] = (mcode[0] & 0xffu) | ((mcode[1] & 0xffu) << 8) | (mcode[0] & 0xff0000u) | ((mcode[1] & 0xff0000u) << 8);
                        } else {
                            store_act8_swap<OM>(actrow + c8, p.out_plane_stride, ncol0 + c8 < p.N, v);
                            if constexpr (mode_traits<OM>::f16) {             // fp16 range guard (ser_hip.h range_flag): stored columns only
                                if (p.range_flag) range_fold8(ramax, v, ok0, ok1);
                            }
                        }
                    }
                }
                if (do_stat) {
                    // row partials over this wave's columns (deterministic: one slot per 64-column group).  A 128-column wave tile (the
                    // 3-product 256x256 tile) puts its partials in the first of its two slots and ZEROES in the second: every slot of the
                    // columns a launch covers is written.  When it left the second slot alone, a buffer whose rows another launch shape had
                    // filled before (the output projection's partials of "f16mf" with SER_F16M_OUT_M=1: FP16X layers, then FP16M layers,
                    // then the next forward's FP16X layers) fed those stale values to the consumer's LayerNorm.
                    st1 += __shfl_xor(st1, 16, 64); st2 += __shfl_xor(st2, 16, 64);
                    st1 += __shfl_xor(st1, 32, 64); st2 += __shfl_xor(st2, 32, 64);
                    const int cstart = n0 + wn * (TN * 16);
                    const int grp = g * ((p.N + 63) >> 6) + (cstart >> 6);
                    if (fq == 0 && cstart < p.N && grp < p.stat_groups) {
                        float* d = p.stat_out + ((int64_t)m * p.stat_groups + grp) * 2;
                        d[0] = st1; d[1] = st2;
                        if constexpr (TN * 16 > 64) {
                            if (cstart + 64 < p.N) { d[2] = 0.f; d[3] = 0.f; }     // (a second half past N: a padding slot, never written)
                        }
                    }
                }
            }
        };
        using std::integral_constant;
        if constexpr (LNA) {
            // block-uniform: GELU or not, and the tile wholly inside / outside the scaled columns [0, col_scale_end) -- a 256-wide tile of
            // the 3 x 1024-wide packed projection always is; a tile that straddles the boundary keeps the per-lane test
            const bool gelu = p.act == SER_ACT_GELU;
            const bool scl_all = n0 + BN <= p.col_scale_end, scl_none = p.col_scale_end <= n0;
            if (gelu && scl_none) rows(integral_constant<int, 1>{}, integral_constant<int, 0>{});             // FC1
            else if (!gelu && scl_all) rows(integral_constant<int, 0>{}, integral_constant<int, 1>{});        // q columns
            else if (!gelu && scl_none) rows(integral_constant<int, 0>{}, integral_constant<int, 0>{});       // k, v (, gate) columns
            else rows(integral_constant<int, 2>{}, integral_constant<int, 2>{});
        } else {
            rows(integral_constant<int, 0>{}, integral_constant<int, 0>{});
        }
    }
    if constexpr (mode_traits<OM>::f16) range_report(p.range_flag, ramax);
#ifdef SER_GEMM_DBG
    {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t2 = __builtin_amdgcn_s_memtime();
        unsigned long long* d = ser_gemm_dbg_dev;
        if (d && wave == 0 && lane == 0 && blockIdx.y == 0) d[131072 + blockIdx.x * 4 + 2] = t2;
    }
#endif
}

// ------------------------------------------------------------------------------------------------
// Host side: launch_plan.h checks the arguments and plans the launch (tile, (MODE, OM) pair, grid, LDS bytes); here the plan meets the
// kernel template.  gemm_epi_built guards the instantiation: exactly the (tile, pair, epilogue class) kernels it names are built.
template <int... I, class F>
static bool with_index(int i, std::integer_sequence<int, I...>, F&& f) { return ser_with_mode<I...>(i, f); }

template <int TILE, int PAIR, int EPI>
static int launch_planned(const ser_gemm_args* a, const gemm_launch& pl, hipStream_t s) {
    constexpr gemm_tile t = GEMM_TILE[TILE];
    constexpr gemm_pair pr = GEMM_PAIR[PAIR];
    auto k = ser_gemm_kernel<t.WM, t.WN, t.TM, t.TN, t.BK, t.ST, pr.mode, t.LNEPI, pr.om, EPI>;
    static std::atomic<bool> ready{false};          // per instantiation
    if (pl.lds > 65536)
        if (hipError_t e = ser_lds_optin(k, pl.lds, ready)) return ser_fail((int)e, "ser_gemm: cannot raise dynamic LDS to %d", pl.lds);
    hipLaunchKernelGGL(k, dim3(pl.grid_x, pl.grid_y, 1), dim3((unsigned)pl.block, 1, 1), pl.lds, s, *a);
    return ser_check_launch("ser_gemm");
}

extern "C" int ser_gemm(const ser_gemm_args* a, void* stream) {
    gemm_launch pl;
    if (int rc = gemm_plan(a, &pl)) return rc;
    hipStream_t s = (hipStream_t)stream;
#ifdef SER_GEMM_DBG
    {
        static void* planted = nullptr;
        if (planted != ser_gemm_dbg_ptr) {
            planted = ser_gemm_dbg_ptr;
            (void)hipMemcpyToSymbol(HIP_SYMBOL(ser_gemm_dbg_dev), &planted, sizeof(void*));
        }
    }
#endif
    int rc = -22;                                   // (never returned: gemm_plan refuses the (tile, pair) combinations that are not built)
    with_index(pl.tile, std::make_integer_sequence<int, GEMM_TILES>{}, [&](auto T) {
        with_index(pl.pair, std::make_integer_sequence<int, GEMM_PAIRS>{}, [&](auto P) {
            constexpr int tile = decltype(T)::value, pair = decltype(P)::value;
            with_index(pl.epi, std::make_integer_sequence<int, GEMM_EPIS>{}, [&](auto E) {
                constexpr int epi = decltype(E)::value;
                if constexpr (gemm_epi_built(tile, GEMM_PAIR[pair], epi)) rc = launch_planned<tile, pair, epi>(a, pl, s);
            });
        });
    });
    return rc;
}
