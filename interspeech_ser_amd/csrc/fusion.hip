// The reference's bimodal fusion head (bin/train_cat_bimodal_lazy_1head.py:236-334, MultiModalEmotionClassifier) behind the encoders:
//   ser_gru_v         bidirectional GRU recurrence over a packed ragged batch (the input products gx come from ser_gemm)
//   ser_xattn_mh_v    cross-attention over ragged (query, key) utterance pairs, fp32 FMA, online softmax; the head is a grid dimension: a
//                     block works on its head's E / heads columns
//   ser_xattn_v       ser_xattn_mh_v with heads = 1
// The pooling and the classifier behind them (ser_attn_pool_v, ser_fusion_cls_v) share pool.hip's kernels.  ser_hip.h states the arithmetic.  No atomics on float data; every sum runs in an order fixed by the utterance alone.
#include "ser_common.h"

// ================================================================================================ ser_gru_v
// One block serves (group of <= 16 utterances, direction, cluster rank): it owns U = H / R hidden units (x 3 gates), i.e. 3 U rows of W_hh,
// as fp16 hi + lo planes resident in LDS when they fit.  Per step and 16-unit tile: G[48, 16] = W[48, H] h[H, 16] on v_mfma_f32_16x16x32_f16,
// three products per k-step (hi hi + lo hi + hi lo); the utterances ride the MFMA's N dimension.  Wave w takes the k-steps w, w + 4, ...
// (a split that depends on H alone), the four partial tiles meet in LDS and are added as (p0 + p1) + (p2 + p3): the order of every
// output element's sum is the same for every R, so results are bit-identical across cluster sizes.
// Thread (u = tid / 16, n = tid % 16) then owns unit u of the tile for utterance n: gates in fp32 (accurate expf / tanhf), h kept in fp32.
// R == 1: the next step's operand (h split into fp16 hi + lo) goes to the other of two LDS buffers.
// R  > 1: it is published to the cluster as one 8-byte {tag, hi | lo << 16} granule per (unit, utterance), double-buffered by step parity,
//         tag = (epoch << 20) | (step + 1); every block then sweeps all H x 16 granules of the step into its LDS operand.  Waits are bounded:
//         on give-up the block writes SER_GRU_ERR_TIMEOUT to the error word and leaves; a block that fails a sweep pass and finds the
//         word set leaves too.
#define GRU_THREADS 256
#define GRU_NB 16
#define GRU_PAD 8                     // fp16 elements of row padding in LDS (16 bytes: keeps 16-byte reads aligned, spreads the banks)
#define GRU_MAX_BLOCKS 256
#define GRU_SPIN_TICKS 100000000LL    // wall_clock64 runs at 100 MHz: one second
#define GRU_SPIN_PASSES (1u << 22)
#define GRU_LDS_LIMIT (160 * 1024 - 256)

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((address_space(1))) unsigned int gu32;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct gru_params {
    const float* gx; int64_t ldgx;
    const unsigned short* whh; int64_t wplane;
    const float* bhh;
    const int32_t* offs;
    float* out; int64_t ldo;
    unsigned short* out_act; int64_t ldo_act; int64_t oplane;
    unsigned long long* xchg;
    uint32_t* err;
    int B, H, R, rows, group0, mode, wres;
    unsigned tagbase;
};

// explicit roundings: no contraction, so every instantiation rounds alike
__device__ __forceinline__ float gru_sigmoid(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }
__device__ __forceinline__ float gru_cell(float sr, float sz, float sn, float xr, float xz, float xn, float br, float bz, float bn, float h) {
    const float r = gru_sigmoid(__fadd_rn(__fadd_rn(xr, sr), br));
    const float z = gru_sigmoid(__fadd_rn(__fadd_rn(xz, sz), bz));
    const float n = tanhf(__fadd_rn(xn, __fmul_rn(r, __fadd_rn(sn, bn))));
    return __fadd_rn(__fmul_rn(__fsub_rn(1.0f, z), n), __fmul_rn(z, h));
}

template <bool CL>
__global__ __launch_bounds__(GRU_THREADS) void gru_kernel(gru_params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_abort;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = p.H, R = CL ? p.R : 1, U = H / R, tiles = U / 16, LDH = H + GRU_PAD;
    const int rank = blockIdx.x % R, cl = blockIdx.x / R, dir = cl & 1, grp = p.group0 + (cl >> 1);
    const int hB_elems = 2 * GRU_NB * LDH;
    unsigned short* hB = (unsigned short*)smem;                            // [CL ? 1 : 2][plane][utterance][LDH]
    float* part = (float*)(hB + (CL ? 1 : 2) * hB_elems);                  // [wave][gate][unit * 16 + utterance]
    float* hprev = part + 4 * 3 * 256;                                     // [tile][unit * 16 + utterance]
    unsigned short* Wl = (unsigned short*)(hprev + U * GRU_NB);            // [plane][gate * U + unit][LDH], when resident

    // the group's columns: utterance n of the group, its rows and length (the offsets are the caller's contract; never read outside [0, rows))
    int steps = 0;
    for (int n = 0; n < GRU_NB; ++n) {
        const int b = grp * GRU_NB + n;
        if (b < p.B) {
            int a0 = p.offs[b], a1 = p.offs[b + 1];
            if (a0 < 0) a0 = 0;
            if (a1 > p.rows) a1 = p.rows;
            steps = max(steps, a1 - a0);
        }
    }
    const int n = tid & 15, u = tid >> 4;
    int r0 = 0, len = 0;
    {
        const int b = grp * GRU_NB + n;
        if (b < p.B) {
            r0 = p.offs[b];
            int a1 = p.offs[b + 1];
            if (r0 < 0) r0 = 0;
            if (a1 > p.rows) a1 = p.rows;
            len = max(a1 - r0, 0);
        }
    }
    if (tid == 0) s_abort = 0;
    for (int i = tid; i < (CL ? 1 : 2) * hB_elems / 2; i += GRU_THREADS) ((unsigned*)hB)[i] = 0u;      // h_0 = 0 (and the padding)
    for (int i = tid; i < U * GRU_NB; i += GRU_THREADS) hprev[i] = 0.f;
    if (p.wres) {
        const int chunks = H / 8;
        for (int i = tid; i < 2 * 3 * U * chunks; i += GRU_THREADS) {
            const int c = i % chunks, row = (i / chunks) % (3 * U), pl = i / (chunks * 3 * U);
            const int g = row / U, lu = row % U;
            const unsigned short* src = p.whh + (int64_t)pl * p.wplane + ((int64_t)dir * 3 * H + (int64_t)g * H + rank * U + lu) * H + c * 8;
            *(u32x4*)(Wl + ((int64_t)pl * 3 * U + row) * LDH + c * 8) = *(const u32x4*)src;
        }
    }
    __syncthreads();

    const float* bh = p.bhh + (int64_t)dir * 3 * H;
    const int ksteps = H / 32;
    for (int s = 0; s < steps; ++s) {
        const unsigned short* hcur = hB + (CL ? 0 : (s & 1) * hB_elems);
        unsigned short* hnext = hB + (CL ? 0 : ((s + 1) & 1) * hB_elems);
        const bool live = s < len;
        const int64_t row = (int64_t)r0 + (dir ? len - 1 - s : s);
        for (int j = 0; j < tiles; ++j) {
            const int hu = rank * U + j * 16 + u;                          // this thread's hidden unit in the gate phase
            float xr = 0.f, xz = 0.f, xn = 0.f;
            if (live) {
                const float* g = p.gx + row * p.ldgx + (int64_t)dir * 3 * H + hu;
                xr = g[0]; xz = g[H]; xn = g[2 * H];
            }
            f32x4 acc[3];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int ks = wv; ks < ksteps; ks += 4) {
                const int kofs = ks * 32 + (lane >> 4) * 8;
                const f16x8 bhi = *(const f16x8*)(hcur + (lane & 15) * LDH + kofs);
                const f16x8 blo = *(const f16x8*)(hcur + (GRU_NB + (lane & 15)) * LDH + kofs);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    f16x8 ahi, alo;
                    if (p.wres) {
                        const unsigned short* w = Wl + (int64_t)(g * U + j * 16 + (lane & 15)) * LDH + kofs;
                        ahi = *(const f16x8*)w;
                        alo = *(const f16x8*)(w + (int64_t)3 * U * LDH);
                    } else {
                        const unsigned short* w = p.whh + ((int64_t)dir * 3 * H + (int64_t)g * H + rank * U + j * 16 + (lane & 15)) * H + kofs;
                        ahi = *(const f16x8*)w;
                        alo = *(const f16x8*)(w + p.wplane);
                    }
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, bhi, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(alo, bhi, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ahi, blo, acc[g], 0, 0, 0);
                }
            }
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int i = 0; i < 4; ++i) part[(wv * 3 + g) * 256 + ((lane >> 4) * 4 + i) * 16 + (lane & 15)] = acc[g][i];
            __syncthreads();
            float sg[3];
#pragma unroll
            for (int g = 0; g < 3; ++g)
                sg[g] = __fadd_rn(__fadd_rn(part[(0 * 3 + g) * 256 + tid], part[(1 * 3 + g) * 256 + tid]),
                                  __fadd_rn(part[(2 * 3 + g) * 256 + tid], part[(3 * 3 + g) * 256 + tid]));
            float hn = 0.f;                                                // a finished (or absent) column carries zeros from here on
            if (live) {
                hn = gru_cell(sg[0], sg[1], sg[2], xr, xz, xn, bh[hu], bh[H + hu], bh[2 * H + hu], hprev[j * 256 + tid]);
                p.out[row * p.ldo + dir * H + hu] = hn;
            }
            hprev[j * 256 + tid] = hn;
            unsigned short hi, lo;
            split_h(hn, hi, lo);
            if (live && p.out_act) {
                unsigned short* o = p.out_act + row * p.ldo_act + dir * H + hu;
                if (p.mode == SER_MODE_BF16) o[0] = f2bf(hn);
                else if (p.mode == SER_MODE_FP32X) { unsigned short bhi_, blo_; split_bf(hn, bhi_, blo_); o[0] = bhi_; o[p.oplane] = blo_; }
                else { o[0] = hi; o[p.oplane] = lo; }
            }
            if (CL) {
                if (s + 1 < steps) {
                    gu64* g = (gu64*)(p.xchg + ((int64_t)(cl * 2 + (s & 1)) * H + hu) * GRU_NB + n);
                    const unsigned long long v = ((unsigned long long)(p.tagbase | (unsigned)(s + 1)) << 32) | ((unsigned)hi | ((unsigned)lo << 16));
                    __hip_atomic_store(g, v, RLX_AGENT);                   // ONE aligned 8-byte store: value and tag arrive together
                }
            } else {
                hnext[n * LDH + hu] = hi;
                hnext[(GRU_NB + n) * LDH + hu] = lo;
            }
            if (j + 1 < tiles) __syncthreads();                            // the partial tiles are written again
        }
        if (CL && s + 1 < steps) {
            // sweep the step's H x 16 granules (this block's own among them) into the LDS operand; thread t owns granules t, t + 256, ...
            gu64* base = (gu64*)(p.xchg + (int64_t)(cl * 2 + (s & 1)) * H * GRU_NB);
            const unsigned tag = p.tagbase | (unsigned)(s + 1);
            const int ng = H * GRU_NB / GRU_THREADS;
            unsigned spins = 0;
            long long t0 = 0;
            for (;;) {
                bool ok = true;
                for (int k0 = 0; k0 < ng; k0 += 8) {                       // eight loads in flight, then their checks
                    unsigned long long x[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        x[i] = k0 + i < ng ? __hip_atomic_load(base + (k0 + i) * GRU_THREADS + tid, RLX_AGENT) : 0ull;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (k0 + i >= ng) continue;
                        const int idx = (k0 + i) * GRU_THREADS + tid;
                        if ((unsigned)(x[i] >> 32) == tag) {
                            unsigned short* d = hB + (idx & 15) * LDH + (idx >> 4);
                            d[0] = (unsigned short)(x[i] & 0xffffu);
                            d[GRU_NB * LDH] = (unsigned short)((x[i] >> 16) & 0xffffu);
                        } else ok = false;
                    }
                }
                if (ok) break;
                if (spins == 0) t0 = wall_clock64();
                ++spins;
                if (__hip_atomic_load((gu32*)p.err, RLX_AGENT) != 0u) { s_abort = 1; break; }       // another block gave up: drain
                if (spins > GRU_SPIN_PASSES || wall_clock64() - t0 > GRU_SPIN_TICKS) {
                    __hip_atomic_store((gu32*)p.err, (unsigned)SER_GRU_ERR_TIMEOUT, RLX_AGENT);
                    s_abort = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        __syncthreads();
        if (CL && *(volatile int*)&s_abort) return;
    }
}

// R for `cluster` (0 = choose), whether the weight slice stays in LDS, and the LDS bytes of a block
static size_t gru_lds_bytes(int H, int R, bool resident) {
    const size_t LDH = H + GRU_PAD, U = H / R;
    return (R > 1 ? 1 : 2) * 2 * GRU_NB * LDH * 2 + 4 * 3 * 256 * 4 + U * GRU_NB * 4 + (resident ? 2 * 3 * U * LDH * 2 : 0);
}
static int gru_plan(int H, int cluster, int* R, int* wres, size_t* lds) {
    if (H <= 0 || (H % 64) || H > 512) return -1;
    const int T = H / 16;
    int r = cluster;
    if (r == 0) {
        for (r = 1; r <= T; ++r)
            if (T % r == 0 && gru_lds_bytes(H, r, true) <= GRU_LDS_LIMIT) break;
    }
    if (r < 1 || r > T || (T % r)) return -2;
    *R = r;
    *wres = gru_lds_bytes(H, r, true) <= GRU_LDS_LIMIT;
    *lds = gru_lds_bytes(H, r, *wres != 0);
    return 0;
}
static int gru_groups_per_launch(int R) { return GRU_MAX_BLOCKS / (2 * R); }

extern "C" int64_t ser_gru_work_bytes(int32_t H, int32_t cluster, int32_t* R_out) {
    int R, wres;
    size_t lds;
    if (gru_plan(H, cluster, &R, &wres, &lds) != 0) return -1;
    if (R_out) *R_out = R;
    if (R == 1) return 0;
    return (int64_t)gru_groups_per_launch(R) * 2 * 2 * H * GRU_NB * 8;    // [cluster of the launch][parity][unit][utterance] granules
}

extern "C" int ser_gru_v(const ser_gru_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_gru: null pointer");
    if (!a->gx || !a->whh || !a->bhh || !a->frame_offs || !a->out) return ser_fail(-1, "ser_gru: null pointer");
    if (a->B <= 0 || a->rows <= 0 || a->max_frames <= 0 || a->max_frames > a->rows || a->max_frames >= (1 << 20))
        return ser_fail(-2, "ser_gru: bad B=%d rows=%d max_frames=%d (1 .. min(rows, 2^20 - 1))", a->B, a->rows, a->max_frames);
    if (a->H <= 0 || (a->H % 64) || a->H > 512) return ser_fail(-2, "ser_gru: H=%d must be a multiple of 64, at most 512", a->H);
    int R, wres;
    size_t lds;
    if (gru_plan(a->H, a->cluster, &R, &wres, &lds) != 0)
        return ser_fail(-2, "ser_gru: cluster=%d must divide H / 16 = %d (0 = choose)", a->cluster, a->H / 16);
    if (a->ldgx < 6 * (int64_t)a->H || a->ldo < 2 * (int64_t)a->H || a->whh_plane_stride < 6 * (int64_t)a->H * a->H)
        return ser_fail(-2, "ser_gru: bad pitches ldgx=%lld (>= 6 H) ldo=%lld (>= 2 H) whh_plane_stride=%lld (>= 6 H^2)", (long long)a->ldgx,
                        (long long)a->ldo, (long long)a->whh_plane_stride);
    if (((uintptr_t)a->whh & 15) || (a->whh_plane_stride % 8)) return ser_fail(-2, "ser_gru: whh must be 16-byte aligned, its plane stride a multiple of 8");
    if (a->out_act) {
        if (a->mode != SER_MODE_BF16 && a->mode != SER_MODE_FP32X && a->mode != SER_MODE_FP16X)
            return ser_fail(-2, "ser_gru: mode %d of the operand copy (BF16, FP32X or FP16X)", a->mode);
        if (a->ldo_act < 2 * (int64_t)a->H) return ser_fail(-2, "ser_gru: ldo_act=%lld (>= 2 H)", (long long)a->ldo_act);
    }
    const int gpl = gru_groups_per_launch(R);
    if (R > 1) {
        if (!a->work || !a->err) return ser_fail(-1, "ser_gru: the cluster form needs its workspace and the error word");
        if (((uintptr_t)a->work & 15) || a->work_bytes < (int64_t)gpl * 2 * 2 * a->H * GRU_NB * 8)
            return ser_fail(-2, "ser_gru: workspace of %lld bytes, 16-byte aligned (ser_gru_work_bytes), got %lld", (long long)gpl * 4 * a->H * GRU_NB * 8,
                            (long long)a->work_bytes);
    }
    hipStream_t s = (hipStream_t)stream;
    auto k = R > 1 ? gru_kernel<true> : gru_kernel<false>;
    static std::atomic<bool> ready[2] = {{false}, {false}};
    if (hipError_t e = ser_lds_optin(k, 160 * 1024 - 256, ready[R > 1])) return ser_fail((int)e, "ser_gru: hipFuncSetAttribute: %s", hipGetErrorString(e));
    gru_params p;
    p.gx = a->gx; p.ldgx = a->ldgx; p.whh = (const unsigned short*)a->whh; p.wplane = a->whh_plane_stride; p.bhh = a->bhh;
    p.offs = a->frame_offs; p.out = a->out; p.ldo = a->ldo;
    p.out_act = (unsigned short*)a->out_act; p.ldo_act = a->ldo_act; p.oplane = a->out_plane_stride;
    p.xchg = (unsigned long long*)a->work; p.err = a->err;
    p.B = a->B; p.H = a->H; p.R = R; p.rows = a->rows; p.mode = a->mode; p.wres = wres;
    const int groups = (a->B + GRU_NB - 1) / GRU_NB;
    int li = 0;
    for (int g0 = 0; g0 < groups; g0 += gpl, ++li) {
        const int ng = groups - g0 < gpl ? groups - g0 : gpl;
        p.group0 = g0;
        p.tagbase = ((a->epoch + (unsigned)li) & 0xfffu) << 20;
        if (R > 1) {
            // every polled word starts a launch at zero, and a tag is never zero: what an earlier launch left cannot match
            hipError_t e = hipMemsetAsync(a->work, 0, (size_t)ng * 2 * 2 * a->H * GRU_NB * 8, s);
            if (e != hipSuccess) return ser_fail((int)e, "ser_gru: hipMemsetAsync: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(k, dim3((unsigned)(ng * 2 * R)), dim3(GRU_THREADS), lds, s, p);
    }
    return ser_check_launch("ser_gru");
}

// ================================================================================================ ser_xattn_v, ser_xattn_mh_v
// Block (query tile of 16, utterance, head); thread (qi = tid / 16, c = tid % 16).  A block sees a window of W columns of q, k, v and the
// context, starting at column head * W: W = E and one head for ser_xattn_v, W = E / heads for ser_xattn_mh_v.  LDS holds W columns only.
// Per key tile of 16: K rows through LDS, thread (qi, c) owns the logit of query qi and key c (four fp32 FMA chains over W, added as
// (s0 + s1) + (s2 + s3)), the 16 lanes of a query share the tile's max and sum by butterflies; then V rows through the same LDS buffer,
// thread (qi, c) owns the context columns 4 c + 64 i of the window.  Online softmax in base 2, logits pre-scaled by scale log2(e).
// Tiles start at the utterance's first row and never cross utterances: a result depends on its own pair alone.
#define XA_QT 16
#define XA_KT 16
#define XA_EV 16                      // 64-column steps of a context row: W <= 1024

struct xattn_params {
    const float* q; int64_t ldq; const float* k; int64_t ldk; const float* v; int64_t ldv;
    const int32_t* qo; const int32_t* ko;
    unsigned short* out_act; int64_t ldo_act; int64_t oplane;
    float* out_f32; int64_t ldo_f32;
    uint32_t* range_flag;
    float scale2;
    int W, q_rows, k_rows;
};

template <int MODE>
__global__ __launch_bounds__(256) void xattn_kernel(xattn_params p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int E = p.W, LD = E + 4, w0 = blockIdx.z * p.W;   // E: the window's width from here on; w0: its first column
    float* qs = (float*)smem;                    // [16][LD]
    float* kv = qs + XA_QT * LD;                 // [16][LD]
    float* ps = kv + XA_KT * LD;                 // [16][17]
    const int b = blockIdx.y, tid = threadIdx.x, qi = tid >> 4, c = tid & 15;
    int q0 = p.qo[b], q1 = p.qo[b + 1], k0 = p.ko[b], k1 = p.ko[b + 1];
    if (q0 < 0) q0 = 0;
    if (k0 < 0) k0 = 0;
    if (q1 > p.q_rows) q1 = p.q_rows;
    if (k1 > p.k_rows) k1 = p.k_rows;
    const int Tq = q1 - q0, Tk = k1 - k0, qt0 = blockIdx.x * XA_QT;
    if (qt0 >= Tq || Tk <= 0) return;
    const int ev = E / 4;                        // 16-byte chunks of a row
    for (int i = tid; i < XA_QT * ev; i += 256) {
        const int r = i / ev, ch = i % ev;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (qt0 + r < Tq) v = *(const f32x4*)(p.q + (int64_t)(q0 + qt0 + r) * p.ldq + w0 + ch * 4);
        *(f32x4*)(qs + r * LD + ch * 4) = v;
    }
    f32x4 acc[XA_EV];
#pragma unroll
    for (int i = 0; i < XA_EV; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    for (int kt0 = 0; kt0 < Tk; kt0 += XA_KT) {
        __syncthreads();                                               // the V rows of the previous tile are read (first pass: nothing)
        for (int i = tid; i < XA_KT * ev; i += 256) {
            const int r = i / ev, ch = i % ev;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kt0 + r < Tk) v = *(const f32x4*)(p.k + (int64_t)(k0 + kt0 + r) * p.ldk + w0 + ch * 4);
            *(f32x4*)(kv + r * LD + ch * 4) = v;
        }
        __syncthreads();
        float sc = 0.f;
        {
            const float* qr = qs + qi * LD;
            const float* kr = kv + c * LD;
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f};                            // four chains of E / 4 products, then (s0 + s1) + (s2 + s3)
            for (int e = 0; e < E; e += 4) {
                const f32x4 a = *(const f32x4*)(qr + e), w = *(const f32x4*)(kr + e);
#pragma unroll
                for (int t = 0; t < 4; ++t) s4[t] = fmaf(a[t], w[t], s4[t]);
            }
            sc = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        }
        const bool valid = kt0 + c < Tk;
        sc = valid ? sc * p.scale2 : -INFINITY;
        float mx = sc;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float mnew = fmaxf(m, mx);                               // finite: key kt0 of the tile is valid
        const float pj = valid ? exp2f(sc - mnew) : 0.f;
        float rs = pj;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) rs += __shfl_xor(rs, o, 64);
        const float alpha = exp2f(m - mnew);                           // first tile: exp2(-inf) = 0
        l = fmaf(l, alpha, rs);
        m = mnew;
        ps[qi * 17 + c] = pj;
        __syncthreads();                                               // every logit is taken: the K rows may go
        for (int i = tid; i < XA_KT * ev; i += 256) {
            const int r = i / ev, ch = i % ev;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kt0 + r < Tk) v = *(const f32x4*)(p.v + (int64_t)(k0 + kt0 + r) * p.ldv + w0 + ch * 4);
            *(f32x4*)(kv + r * LD + ch * 4) = v;
        }
        __syncthreads();
        float pr[XA_KT];
#pragma unroll
        for (int j = 0; j < XA_KT; ++j) pr[j] = ps[qi * 17 + j];
#pragma unroll
        for (int i = 0; i < XA_EV; ++i) {
            if (i * 64 < E) {
                f32x4 t = acc[i] * alpha;
#pragma unroll
                for (int j = 0; j < XA_KT; ++j) {
                    const f32x4 w = *(const f32x4*)(kv + j * LD + i * 64 + c * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = fmaf(pr[j], w[e], t[e]);
                }
                acc[i] = t;
            }
        }
    }
    float amax = 0.f;
    if (qt0 + qi < Tq) {
        const float inv = 1.0f / l;
        const int64_t row = (int64_t)q0 + qt0 + qi;
#pragma unroll
        for (int i = 0; i < XA_EV; ++i) {
            if (i * 64 < E) {
                const f32x4 o = acc[i] * inv;
                const int col = w0 + i * 64 + c * 4;
                if (p.out_f32) *(f32x4*)(p.out_f32 + row * p.ldo_f32 + col) = o;
                if (p.out_act) {
                    store_act4<MODE>(p.out_act + row * p.ldo_act + col, p.oplane, o[0], o[1], o[2], o[3]);
#pragma unroll
                    for (int e = 0; e < 4; ++e) amax = range_fold(amax, o[e]);
                }
            }
        }
    }
    if (MODE == SER_MODE_FP16X) range_report(p.range_flag, amax);
}

// Both entry points: validation, then grid (query tiles, utterances, heads) and LDS for a window of E / heads columns.  `who` prefixes the messages.
static int xattn_run(const ser_xattn_mh_args* a, void* stream, const char* who) {
    if (!a) return ser_fail(-1, "%s: null pointer", who);
    if (!a->q || !a->k || !a->v || !a->q_offs || !a->k_offs || (!a->out_act && !a->out_f32)) return ser_fail(-1, "%s: null pointer", who);
    if (a->B <= 0 || a->B > 65535 || a->E <= 0 || (a->E % 64) || a->E > 1024 || a->q_rows <= 0 || a->k_rows <= 0 || a->max_q <= 0 || a->max_q > a->q_rows)
        return ser_fail(-2, "%s: bad B=%d E=%d (multiple of 64, <= 1024) q_rows=%d k_rows=%d max_q=%d", who, a->B, a->E, a->q_rows, a->k_rows, a->max_q);
    if (a->heads < 1 || (a->E % a->heads) || ((a->E / a->heads) % 64))                             // never with ser_xattn_v's heads = 1
        return ser_fail(-2, "%s: bad heads=%d for E=%d (heads >= 1, E %% heads == 0, (E / heads) %% 64 == 0)", who, a->heads, a->E);
    if (a->ldq < a->E || a->ldk < a->E || a->ldv < a->E || (a->ldq % 4) || (a->ldk % 4) || (a->ldv % 4))
        return ser_fail(-2, "%s: bad pitches ldq=%lld ldk=%lld ldv=%lld (>= E, multiples of 4)", who, (long long)a->ldq, (long long)a->ldk, (long long)a->ldv);
    if ((((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out_f32) & 15) || ((uintptr_t)a->out_act & 7))
        return ser_fail(-2, "%s: q, k, v and out_f32 must be 16-byte aligned, out_act 8-byte aligned", who);
    if (a->out_act && (a->ldo_act < a->E || (a->ldo_act % 4) || (a->out_plane_stride % 4)))
        return ser_fail(-2, "%s: bad ldo_act=%lld (>= E, multiple of 4) out_plane_stride=%lld", who, (long long)a->ldo_act, (long long)a->out_plane_stride);
    if (a->out_f32 && (a->ldo_f32 < a->E || (a->ldo_f32 % 4))) return ser_fail(-2, "%s: bad ldo_f32=%lld (>= E, multiple of 4)", who, (long long)a->ldo_f32);
    if (a->out_act && a->mode != SER_MODE_BF16 && a->mode != SER_MODE_FP32X && a->mode != SER_MODE_FP16X)
        return ser_fail(-2, "%s: mode %d of the operand copy (BF16, FP32X or FP16X)", who, a->mode);
    xattn_params p;
    p.q = a->q; p.ldq = a->ldq; p.k = a->k; p.ldk = a->ldk; p.v = a->v; p.ldv = a->ldv; p.qo = a->q_offs; p.ko = a->k_offs;
    p.out_act = (unsigned short*)a->out_act; p.ldo_act = a->ldo_act; p.oplane = a->out_plane_stride;
    p.out_f32 = a->out_f32; p.ldo_f32 = a->ldo_f32; p.range_flag = a->range_flag;
    p.scale2 = a->scale * 1.44269504088896340736f;
    p.W = a->E / a->heads; p.q_rows = a->q_rows; p.k_rows = a->k_rows;
    const int lds = (XA_QT + XA_KT) * (p.W + 4) * 4 + XA_QT * 17 * 4;
    const dim3 grid((unsigned)((a->max_q + XA_QT - 1) / XA_QT), (unsigned)a->B, (unsigned)a->heads);
    hipStream_t s = (hipStream_t)stream;
    static std::atomic<bool> ready[3] = {{false}, {false}, {false}};
    const auto launch = [&](auto kern, std::atomic<bool>& rdy) {
        const hipError_t e = ser_lds_optin(kern, 136 * 1024, rdy);
        if (e == hipSuccess) hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, p);
        return e;
    };
    const hipError_t e = a->mode == SER_MODE_BF16 ? launch(xattn_kernel<SER_MODE_BF16>, ready[0])
                       : a->mode == SER_MODE_FP32X ? launch(xattn_kernel<SER_MODE_FP32X>, ready[1]) : launch(xattn_kernel<SER_MODE_FP16X>, ready[2]);
    if (e != hipSuccess) return ser_fail((int)e, "%s: hipFuncSetAttribute: %s", who, hipGetErrorString(e));
    return ser_check_launch(who);
}

extern "C" int ser_xattn_mh_v(const ser_xattn_mh_args* a, void* stream) { return xattn_run(a, stream, "ser_xattn_mh"); }

// the single-head form: the same arguments without `heads`
extern "C" int ser_xattn_v(const ser_xattn_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_xattn: null pointer");
    ser_xattn_mh_args m;
    m.q = a->q; m.ldq = a->ldq; m.k = a->k; m.ldk = a->ldk; m.v = a->v; m.ldv = a->ldv; m.q_offs = a->q_offs; m.k_offs = a->k_offs;
    m.out_act = a->out_act; m.ldo_act = a->ldo_act; m.out_plane_stride = a->out_plane_stride; m.out_f32 = a->out_f32; m.ldo_f32 = a->ldo_f32;
    m.range_flag = a->range_flag; m.scale = a->scale;
    m.B = a->B; m.E = a->E; m.heads = 1; m.q_rows = a->q_rows; m.k_rows = a->k_rows; m.max_q = a->max_q; m.mode = a->mode;
    return xattn_run(&m, stream, "ser_xattn");
}
