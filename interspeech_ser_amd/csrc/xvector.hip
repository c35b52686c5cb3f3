// The x-vector head of the hub's speaker-verification checkpoints (HF *ForXVector), the parts no other kernel here does:
//   ser_layer_mix_v   softmax-weighted sum of the hidden states, row by row, into the projector's GEMM operand planes
//   ser_stat_pool_v   statistics pooling: mean and unbiased std over an utterance's rows
//   ser_xvec_tail_v   feature_extractor and classifier on the pooled rows (ser_cls_tail_v's kernel, the embedding written too)
// The projector and the TDNN layers between them are ser_gemm launches.  ser_hip.h states the arithmetic.  Every sum accumulates in
// float64 in an order that depends on the utterance alone, never on the batch; one rounding to fp32 at each store.  No atomics but the
// range guard's rare OR.
#include "row_common.h"
#include "tail_common.h"

// ------------------------------------------------------------------------------- layer mix
// Wave per row on the row skeleton.  An element is ((w0 x0 + w1 x1) + w2 x2) + ...: every product and every sum rounded to float64 on its
// own (__dmul_rn / __dadd_rn keep the compiler from fusing them), so the fp32 result is the rounded float64 statement exactly.
template <int MODE>
__global__ __launch_bounds__(256) void layer_mix_kernel(const float* __restrict__ s, int64_t state_stride, int64_t lds,
                                                        const double* __restrict__ w, unsigned short* __restrict__ oa, int64_t ldoa,
                                                        int64_t plane, float* __restrict__ of, int64_t ldof, int n_states, int rows, int D,
                                                        uint32_t* __restrict__ rflag) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = s + (int64_t)row * lds;
    unsigned short* orow = oa + (int64_t)row * ldoa;
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            double acc[4];
            {
                const f32x4 v = *(const f32x4*)(xr + c);
                const double w0 = w[0];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __dmul_rn(w0, (double)v[j]);
            }
            for (int l = 1; l < n_states; ++l) {
                const f32x4 v = *(const f32x4*)(xr + (int64_t)l * state_stride + c);
                const double wl = w[l];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __dadd_rn(acc[j], __dmul_rn(wl, (double)v[j]));
            }
            const f32x4 y = {(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
            if (of) *(f32x4*)(of + (int64_t)row * ldof + c) = y;
            store_act4<MODE>(orow + c, plane, y[0], y[1], y[2], y[3]);
            if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, y[j]); }
        }
    });
    if constexpr (mode_traits<MODE>::f16) range_report(rflag, ramax);
}

extern "C" int ser_layer_mix_v(const ser_layer_mix_args* a, void* stream) {
    if (!a || !a->s || !a->w || !a->out_act) return ser_fail(-1, "ser_layer_mix: null pointer");
    if (a->n_states < 1) return ser_fail(-2, "ser_layer_mix: n_states=%d (at least 1)", a->n_states);
    if (a->D % 4 || a->D > 2048 || a->D <= 0 || a->rows <= 0) return ser_fail(-2, "ser_layer_mix: D=%d rows=%d unsupported (D %% 4 == 0, D <= 2048)", a->D, a->rows);
    if (a->lds < a->D || (a->lds % 4) || (a->state_stride % 4) || (a->n_states > 1 && a->state_stride <= 0) || a->ldo_act < a->D || (a->ldo_act % 4) ||
        (a->out_f32 && (a->ldo_f32 < a->D || (a->ldo_f32 % 4))))
        return ser_fail(-3, "ser_layer_mix: bad pitches lds=%lld state_stride=%lld ldo_act=%lld ldo_f32=%lld (>= D, multiples of 4)", (long long)a->lds,
                        (long long)a->state_stride, (long long)a->ldo_act, (long long)a->ldo_f32);
    if ((((uintptr_t)a->s | (uintptr_t)a->out_f32) & 15) != 0 || (((uintptr_t)a->w | (uintptr_t)a->out_act) & 7) != 0)
        return ser_fail(-3, "ser_layer_mix: s and out_f32 must be 16-byte aligned, w and out_act 8-byte aligned");
    dim3 grid((unsigned)((a->rows + 3) / 4)), block(256);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(layer_mix_kernel<M()>, grid, block, 0, (hipStream_t)stream, a->s, a->state_stride, a->lds, a->w,
                               (unsigned short*)a->out_act, a->ldo_act, a->out_plane_stride, a->out_f32, a->ldo_f32, a->n_states, a->rows, a->D,
                               a->range_flag);
        }))
        return ser_fail(-4, "ser_layer_mix: bad mode %d", a->mode);
    return ser_check_launch("ser_layer_mix");
}

// ------------------------------------------------------------------------------- statistics pooling
// Block (256-column slab, chunk, utterance): wave g owns the chunk's frames g, g + 4, ... and lane q the columns 4 q .. 4 q + 3 of the
// slab (one 1 KiB row segment per wave and load).  Pass 1: a thread adds its frames in ascending order, the four waves are merged in
// ascending g: the chunk's sum, and from it the chunk's mean.  Pass 2 reads the chunk again (it is in L2) and adds (x - mean)^2 the same
// way.  work[b, chunk, 0, :] = the chunk mean, work[b, chunk, 1, :] = its centred second moment.  A chunk past the utterance's last frame
// leaves at once.
__device__ __forceinline__ f32x4 stat_load(const float* p, int relu) {
    f32x4 v = *(const f32x4*)p;
    if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];          // (a NaN stays a NaN)
    }
    return v;
}

__global__ __launch_bounds__(256) void stat_pool_chunk_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ frame_offs,
                                                              double* __restrict__ work, int D, int rows, int n_chunks, int relu) {
    __shared__ double red[4][256];
    __shared__ double mean_s[256];
    const int b = blockIdx.z, chunk = blockIdx.y, tid = threadIdx.x;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;                                           // the launcher checked the host copy; never read outside [0, rows)
    if (r1 > rows) r1 = rows;
    const int t0 = chunk * SER_STAT_POOL_FC;
    if (t0 >= r1 - r0) return;                                    // block-uniform
    const int t1 = min(t0 + SER_STAT_POOL_FC, r1 - r0);
    const double n = (double)(t1 - t0);
    const int g = tid >> 6, q = tid & 63;
    const int col = blockIdx.x * 256 + q * 4;
    const bool live = col < D;                                    // D % 4 == 0: a quad is inside or outside as a whole
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
        for (int t = t0 + g; t < t1; t += 4) {
            const f32x4 v = stat_load(x + (int64_t)(r0 + t) * ldx + col, relu);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += (double)v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[g][q * 4 + j] = acc[j];
    __syncthreads();
    mean_s[tid] = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) / n;
    __syncthreads();
    if (live) {
        double m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { m[j] = mean_s[q * 4 + j]; acc[j] = 0.0; }
        for (int t = t0 + g; t < t1; t += 4) {
            const f32x4 v = stat_load(x + (int64_t)(r0 + t) * ldx + col, relu);
#pragma unroll
            for (int j = 0; j < 4; ++j) { const double d = (double)v[j] - m[j]; acc[j] = fma(d, d, acc[j]); }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[g][q * 4 + j] = acc[j];       // (every thread read red before the second barrier above)
    __syncthreads();
    const int c = blockIdx.x * 256 + tid;                         // one thread per column of the slab
    if (c < D) {
        double* wk = work + ((int64_t)b * n_chunks + chunk) * 2 * D;
        wk[c] = mean_s[tid];
        wk[D + c] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// One thread per (utterance, column): the chunks merged in ascending order, the division by T - 1, the root, one rounding each.
__global__ __launch_bounds__(256) void stat_pool_finish_kernel(const double* __restrict__ work, const int32_t* __restrict__ frame_offs,
                                                               float* __restrict__ out, int64_t ldo, int D, int rows, int n_chunks) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > rows) r1 = rows;
    const int T = r1 - r0;
    float* o = out + (int64_t)b * ldo;
    if (T < 2) {                                                  // (the launcher refuses these; never divide by zero)
        const float qnan = __uint_as_float(0x7fc00000u);
        o[c] = qnan;
        o[D + c] = qnan;
        return;
    }
    const int used = min((T + SER_STAT_POOL_FC - 1) / SER_STAT_POOL_FC, n_chunks);
    const double* p = work + (int64_t)b * n_chunks * 2 * D + c;
    double cnt = 0.0, mean = 0.0, m2 = 0.0;
    for (int k = 0; k < used; ++k) {
        const double nc = (double)min(SER_STAT_POOL_FC, T - k * SER_STAT_POOL_FC);
        const double mc = p[(int64_t)k * 2 * D], qc = p[(int64_t)k * 2 * D + D];
        const double tot = cnt + nc, delta = mc - mean;
        mean += delta * (nc / tot);
        m2 += qc + delta * delta * (cnt * nc / tot);
        cnt = tot;
    }
    o[c] = (float)mean;
    o[D + c] = (float)sqrt(m2 / (double)(T - 1));
}

extern "C" int ser_stat_pool_v(const ser_stat_pool_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_stat_pool: null pointer");
    if (!a->x || !a->frame_offs || !a->frame_offs_host || !a->work || !a->out) return ser_fail(-1, "ser_stat_pool: null pointer");
    if (a->relu != 0 && a->relu != 1) return ser_fail(-2, "ser_stat_pool: relu=%d must be 0 or 1", a->relu);
    if (a->B <= 0 || a->B > 65535 || a->D <= 0 || (a->D % 4) || a->rows <= 0 || a->max_frames <= 0 || a->max_frames > a->rows)
        return ser_fail(-2, "ser_stat_pool: bad B=%d (1..65535) D=%d (D %% 4 == 0) rows=%d max_frames=%d (<= rows)", a->B, a->D, a->rows,
                        a->max_frames);
    const int64_t n_chunks = ((int64_t)a->max_frames + SER_STAT_POOL_FC - 1) / SER_STAT_POOL_FC;
    if (n_chunks > 65535) return ser_fail(-2, "ser_stat_pool: max_frames=%d is beyond %d chunks of %d frames", a->max_frames, 65535, SER_STAT_POOL_FC);
    if (a->ldx < a->D || (a->ldx % 4) || a->ldo < 2 * (int64_t)a->D)
        return ser_fail(-2, "ser_stat_pool: bad pitches ldx=%lld (>= D, multiple of 4) ldo=%lld (>= 2 D)", (long long)a->ldx, (long long)a->ldo);
    if ((((uintptr_t)a->x) & 15) != 0 || (((uintptr_t)a->work) & 7) != 0)
        return ser_fail(-2, "ser_stat_pool: x must be 16-byte aligned, work 8-byte aligned");
    if (a->work_elems < (int64_t)a->B * n_chunks * 2 * a->D)
        return ser_fail(-2, "ser_stat_pool: work holds %lld doubles, B * ceil(max_frames / %d) * 2 * D = %lld are needed", (long long)a->work_elems,
                        SER_STAT_POOL_FC, (long long)((int64_t)a->B * n_chunks * 2 * a->D));
    for (int b = 0; b < a->B; ++b) {                              // the host copy of the offsets: what the grid and the reads rely on
        const int64_t r0 = a->frame_offs_host[b], r1 = a->frame_offs_host[b + 1];
        if (r0 < 0 || r1 > a->rows || r1 < r0) return ser_fail(-2, "ser_stat_pool: utterance %d owns rows %lld..%lld outside [0, %d]", b, (long long)r0, (long long)r1, a->rows);
        if (r1 - r0 < 2) return ser_fail(-2, "ser_stat_pool: utterance %d has %lld rows (the unbiased std needs at least 2)", b, (long long)(r1 - r0));
        if (r1 - r0 > a->max_frames) return ser_fail(-2, "ser_stat_pool: utterance %d has %lld rows, max_frames=%d", b, (long long)(r1 - r0), a->max_frames);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned slabs = (unsigned)((a->D + 255) / 256);
    hipLaunchKernelGGL(stat_pool_chunk_kernel, dim3(slabs, (unsigned)n_chunks, (unsigned)a->B), dim3(256), 0, st, a->x, a->ldx, a->frame_offs, a->work,
                       a->D, a->rows, (int)n_chunks, a->relu);
    hipLaunchKernelGGL(stat_pool_finish_kernel, dim3(slabs, (unsigned)a->B), dim3(256), 0, st, a->work, a->frame_offs, a->out, a->ldo, a->D, a->rows,
                       (int)n_chunks);
    return ser_check_launch("ser_stat_pool");
}

// ------------------------------------------------------------------------------- feature_extractor and classifier on the pooled rows
extern "C" int ser_xvec_tail_v(const ser_xvec_tail_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_xvec_tail: null pointer");
    if (!a->stats || !a->F || !a->bf || !a->C || !a->bc || !a->emb || !a->logits) return ser_fail(-1, "ser_xvec_tail: null pointer");
    if (a->dim < 1 || a->dim > CLS_TAIL_MAX || a->n_labels < 1 || a->n_labels > CLS_TAIL_MAX)
        return ser_fail(-2, "ser_xvec_tail: dim=%d n_labels=%d (1..%d each)", a->dim, a->n_labels, CLS_TAIL_MAX);
    if (a->B <= 0 || a->B > 65535 || a->D <= 0 || (a->D % 4) || a->lds < a->D || (a->lds % 4) || a->lde < a->dim || a->ldo < a->n_labels)
        return ser_fail(-2, "ser_xvec_tail: bad B=%d D=%d (D %% 4 == 0) lds=%lld (>= D, multiple of 4) lde=%lld (>= dim) ldo=%lld (>= n_labels)", a->B,
                        a->D, (long long)a->lds, (long long)a->lde, (long long)a->ldo);
    if ((((uintptr_t)a->stats | (uintptr_t)a->F) & 15) != 0) return ser_fail(-2, "ser_xvec_tail: stats and F must be 16-byte aligned");
    hipLaunchKernelGGL(cls_tail_kernel<true>, dim3((unsigned)a->B), dim3(1024), 0, (hipStream_t)stream, a->stats, a->lds, a->F, a->bf, a->C, a->bc,
                       a->logits, a->ldo, a->D, a->dim, a->n_labels, a->emb, a->lde);
    return ser_check_launch("ser_xvec_tail");
}
