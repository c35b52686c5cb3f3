// The conformer layer's own kernels (ser_hip.h a28, a35; HF modeling_wav2vec2_bert.py, modeling_wav2vec2_conformer.py): the middle of the
// convolution module between its two pointwise GEMMs, one body for both families (ser_conformer_conv_v: causal window and LayerNorm;
// ser_conformer_conv_bn_v: centred window and BatchNorm in eval), the swish between a feed-forward block's GEMMs (ser_swish_rows_v) and the
// query side of w2v-BERT's relative-key attention bias (ser_relkey_table_v).  The wav2vec2-conformer family's position kernels are in
// w2v_conformer.hip, the sigmoid in row_common.h.  The reference ships no conformer encoder; its heads take any [T, D] stream
// (bin/train_cat_bimodal_lazy_1head.py:220-228).  Plain grids, fixed summation orders, no atomics on float data.
#include "row_common.h"
#include <type_traits>

// ------------------------------------------------------------------------------------------------------------- convolution module
// One body for both families' convolution modules (ser_conformer_conv_v: causal window, LayerNorm; ser_conformer_conv_bn_v: centred window,
// BatchNorm in eval folded to an affine).  Block = SER_CCONV_TILE rows of one utterance, thread = 4 columns of every 1024-column slab.  The
// block walks the input rows t0 - lead .. t0 + TILE - 1 + trail that exist in the utterance once, takes the GLU of a row once and adds it to
// every output row whose window holds it: output row r sees its taps in ascending k.  Then the norm per output row, swish, operand planes.
// The kernel takes the entry point's own argument struct, as each family's kernel did (a repacked parameter block measured 0.7 - 1.4 %
// slower in the BatchNorm form: profiles/conformer_layer.txt); the window follows from K and the form.
#define CC_SLABS 2
typedef float cconv_stat[2];                    // of an output row: the mean, 1 / sqrt(var + eps)

// LayerNorm statistics of the block's R rows over D (two passes, wave sums merged in wave order).  Only the LayerNorm instantiations call
// this, so only they have LDS and barriers.
__device__ __forceinline__ const cconv_stat* cconv_ln_stats(const f32x4 (&acc)[CC_SLABS][SER_CCONV_TILE], int D, float eps) {
    constexpr int R = SER_CCONV_TILE;
    __shared__ float red[4][R];
    __shared__ float stat[R][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float ps[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < CC_SLABS; ++i)
            if (i * 1024 + tid * 4 < D) s += (acc[i][r][0] + acc[i][r][1]) + (acc[i][r][2] + acc[i][r][3]);
        ps[r] = wave_sum(s);
    }
    if (lane == 0)
#pragma unroll
        for (int r = 0; r < R; ++r) red[wave][r] = ps[r];
    __syncthreads();
    if (tid < R) stat[tid][0] = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) / (float)D;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float mu = stat[r][0];
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < CC_SLABS; ++i)
            if (i * 1024 + tid * 4 < D) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float d = acc[i][r][j] - mu; q = fmaf(d, d, q); }
            }
        ps[r] = wave_sum(q);
    }
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int r = 0; r < R; ++r) red[wave][r] = ps[r];
    __syncthreads();
    if (tid < R) stat[tid][1] = rsqrtf((((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) / (float)D + eps);
    __syncthreads();
    return stat;
}

template <int MODE, bool BN>
__global__ __launch_bounds__(256) void conformer_conv_kernel(std::conditional_t<BN, ser_conformer_conv_bn_args, ser_conformer_conv_args> a) {
    constexpr int R = SER_CCONV_TILE;
    const int b = blockIdx.y, t0 = blockIdx.x * R, tid = threadIdx.x;
    const int row0 = a.frame_offs[b], T = a.frame_offs[b + 1] - row0;
    if (t0 >= T) return;                                                   // block-uniform
    const int D = a.D, K = a.K;
    const int lead = BN ? (K - 1) >> 1 : K - 1, trail = BN ? lead : 0;     // output row t's window: t - lead .. t + trail (centred, or causal)
    f32x4 acc[CC_SLABS][R];
#pragma unroll
    for (int i = 0; i < CC_SLABS; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[i][r] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int s_begin = t0 - lead > 0 ? t0 - lead : 0;                     // never before the utterance's own first row
    const int s_end = t0 + R + trail < T ? t0 + R + trail : T;             // ... nor past its last
    for (int s = s_begin; s < s_end; ++s) {
        const float* yr = a.y + (int64_t)(row0 + s) * a.ldy;
#pragma unroll
        for (int i = 0; i < CC_SLABS; ++i) {
            const int c = i * 1024 + tid * 4;
            if (c < D) {
                const f32x4 va = *(const f32x4*)(yr + c), vb = *(const f32x4*)(yr + D + c);
                f32x4 g;
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = va[j] * sigmoid_f(vb[j]);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int k = s - (t0 + r) + lead;                     // tap of input row s in output row t0 + r's window
                    if (k >= 0 && k < K) {
                        const f32x4 w = *(const f32x4*)(a.w + (int64_t)k * D + c);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][r][j] = fmaf(w[j], g[j], acc[i][r][j]);
                    }
                }
            }
        }
    }
    const cconv_stat* stat = nullptr;
    const float *n0, *n1;                                                  // gamma, beta of the LayerNorm, or the BatchNorm's folded scale, shift
    if constexpr (BN) { n0 = a.scale; n1 = a.shift; }
    else { n0 = a.gamma; n1 = a.beta; stat = cconv_ln_stats(acc, D, a.eps); }
    float ramax = 0.f;
#pragma unroll
    for (int i = 0; i < CC_SLABS; ++i) {
        const int c = i * 1024 + tid * 4;
        if (c < D) {
            const f32x4 p0 = *(const f32x4*)(n0 + c), p1 = *(const f32x4*)(n1 + c);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (t0 + r < T) {
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float t;
                        if constexpr (BN) t = fmaf(acc[i][r][j], p0[j], p1[j]);
                        else t = (acc[i][r][j] - stat[r][0]) * stat[r][1] * p0[j] + p1[j];
                        v[j] = t * sigmoid_f(t);
                    }
                    unsigned short* orow = (unsigned short*)a.out_act + (int64_t)(row0 + t0 + r) * a.ldo_act;
                    store_act4<MODE>(orow + c, a.out_plane_stride, v[0], v[1], v[2], v[3]);
                    if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
                }
            }
        }
    }
    if constexpr (mode_traits<MODE>::f16) range_report(a.range_flag, ramax);
}

// The two entry points' argument checks and grid; `who` names the entry point in every message.  ARGS is ser_conformer_conv_args or
// ser_conformer_conv_bn_args (the same fields but for the norm's), p0 / p1 its norm's two vectors.
template <bool BN, class ARGS>
static int launch_conformer_conv(const char* who, const ARGS* a, const float* p0, const float* p1, void* stream) {
    if (!a->y || !a->w || !p0 || !p1 || !a->frame_offs || !a->out_act) return ser_fail(-1, "%s: null pointer", who);
    if (a->D % 4 || a->D <= 0 || a->D > 1024 * CC_SLABS || a->K < 1 || a->K > 31 || !(a->K & 1))
        return ser_fail(-2, "%s: D=%d (multiple of 4, <= %d) / K=%d (odd, <= 31) unsupported", who, a->D, 1024 * CC_SLABS, a->K);
    if (a->B <= 0 || a->B > 65535 || a->max_frames <= 0 || a->rows < a->max_frames)
        return ser_fail(-2, "%s: bad B=%d / max_frames=%d / rows=%d", who, a->B, a->max_frames, a->rows);
    if ((a->ldy % 4) || a->ldy < 2 * (int64_t)a->D || (a->ldo_act % 4) || a->ldo_act < a->D)
        return ser_fail(-3, "%s: pitches must be multiples of 4, ldy >= 2 D, ldo_act >= D", who);
    dim3 grid((a->max_frames + SER_CCONV_TILE - 1) / SER_CCONV_TILE, a->B), block(256);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL((conformer_conv_kernel<M(), BN>), grid, block, 0, (hipStream_t)stream, *a);
        }))
        return ser_fail(-4, "%s: bad mode %d", who, a->mode);
    return ser_check_launch(who);
}

extern "C" int ser_conformer_conv_v(const ser_conformer_conv_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_conformer_conv: null pointer");
    return launch_conformer_conv<false>("ser_conformer_conv", a, a->gamma, a->beta, stream);
}

extern "C" int ser_conformer_conv_bn_v(const ser_conformer_conv_bn_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_conformer_conv_bn: null pointer");
    return launch_conformer_conv<true>("ser_conformer_conv_bn", a, a->scale, a->shift, stream);
}

// ------------------------------------------------------------------------------------------------------- swish rows -> operand planes
// Wave per (row, 2048-column slab) on the row skeleton: x sigmoid(x) to the operand planes, with the range guard.
template <int MODE>
__global__ __launch_bounds__(256) void swish_rows_kernel(const float* __restrict__ x, int64_t ldx, unsigned short* __restrict__ oa, int64_t ldoa,
                                                         int64_t plane, int rows, int D, uint32_t* __restrict__ rflag) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int col0 = blockIdx.y * 2048, Ds = D - col0 < 2048 ? D - col0 : 2048;
    const float* xr = x + (int64_t)row * ldx + col0;
    unsigned short* orow = oa + (int64_t)row * ldoa + col0;
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < Ds) {
            f32x4 v = *(const f32x4*)(xr + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] * sigmoid_f(v[j]);
            store_act4<MODE>(orow + c, plane, v[0], v[1], v[2], v[3]);
            if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
        }
    });
    if constexpr (mode_traits<MODE>::f16) range_report(rflag, ramax);
}

extern "C" int ser_swish_rows_v(const ser_swish_rows_args* a, void* stream) {
    if (!a || !a->x || !a->out_act) return ser_fail(-1, "ser_swish_rows: null pointer");
    if (a->D % 4 || a->D > 8192 || a->D <= 0 || a->rows <= 0) return ser_fail(-2, "ser_swish_rows: D=%d rows=%d unsupported", a->D, a->rows);
    if ((a->ldx % 4) || (a->ldo_act % 4)) return ser_fail(-3, "ser_swish_rows: pitches must be multiples of 4");
    dim3 grid((a->rows + 3) / 4, (a->D + 2047) / 2048), block(256);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(swish_rows_kernel<M()>, grid, block, 0, (hipStream_t)stream, a->x, a->ldx, (unsigned short*)a->out_act, a->ldo_act,
                               a->out_plane_stride, a->rows, a->D, a->range_flag);
        }))
        return ser_fail(-4, "ser_swish_rows: bad mode %d", a->mode);
    return ser_check_launch("ser_swish_rows");
}

// --------------------------------------------------------------------------------------------------------------- relative-key table
// Block = one row: q of all heads as fp32 in LDS (hi + lo where the mode has two planes), E in LDS with an odd row pitch; thread (h, p)
// takes its dot product in ascending d.
#define RK_MAX_P 128
#define RK_MAX_DH 128
template <int MODE>
__global__ __launch_bounds__(256) void relkey_table_kernel(ser_relkey_table_args a) {
    extern __shared__ float rk_smem[];
    const int dh = a.dh, P = a.P, H = a.H, pitch = dh + 1;
    float* es = rk_smem;                       // [P][dh + 1]
    float* qs = rk_smem + P * pitch;           // [H dh]
    const int tid = threadIdx.x, m = blockIdx.x;
    for (int i = tid; i < P * dh; i += 256) { const int p = i / dh, d = i - p * dh; es[p * pitch + d] = a.E[i]; }
    const unsigned short* qr = (const unsigned short*)a.qkv + (int64_t)m * a.ld + a.q_col;
    for (int i = tid; i < H * dh; i += 256) {
        float v = elem2f<MODE>(qr[i]);
        if (mode_traits<MODE>::planes == 2) v += elem2f<MODE>(qr[a.plane_stride + i]);
        qs[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < H * P; i += 256) {
        const int h = i / P, p = i - h * P;
        const float* q = qs + h * dh;
        const float* e = es + p * pitch;
        float s = 0.f;
        for (int d = 0; d < dh; ++d) s = fmaf(q[d], e[d], s);
        a.qe[((int64_t)m * H + h) * a.ld_qe + p] = s;
    }
}

extern "C" int ser_relkey_table_v(const ser_relkey_table_args* a, void* stream) {
    if (!a || !a->qkv || !a->E || !a->qe) return ser_fail(-1, "ser_relkey_table: null pointer");
    if (a->rows <= 0 || a->H <= 0 || a->dh % 8 || a->dh <= 0 || a->dh > RK_MAX_DH || a->P < 1 || a->P > RK_MAX_P || (int64_t)a->H * a->dh > 2048 ||
        a->ld_qe < a->P || a->q_col < 0)
        return ser_fail(-2, "ser_relkey_table: rows=%d H=%d dh=%d P=%d ld_qe=%lld unsupported", a->rows, a->H, a->dh, a->P, (long long)a->ld_qe);
    const size_t lds = ((size_t)a->P * (a->dh + 1) + (size_t)a->H * a->dh) * sizeof(float);
    if (lds > 64 * 1024) return ser_fail(-2, "ser_relkey_table: P=%d x dh=%d does not fit LDS", a->P, a->dh);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(relkey_table_kernel<M()>, dim3(a->rows), dim3(256), lds, (hipStream_t)stream, *a);
        }))
        return ser_fail(-4, "ser_relkey_table: bad mode %d", a->mode);
    return ser_check_launch("ser_relkey_table");
}
