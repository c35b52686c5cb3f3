// The organiser baseline's utterance-level tail (benchmark/train_eval_files/eval_cat_ser.py:164-177, eval_dim_ser.py): attentive
// statistics pooling over a packed ragged batch (benchmark/net/pooling.py AttentiveStatisticsPooling.forward) and the 2D -> H -> n_out
// head (benchmark/net/ser.py EmotionRegression).  ser_hip.h states the arithmetic.  Every sum accumulates in float64 in an order that
// depends on the utterance alone (its frame count, D, K, H), never on the batch; one rounding to fp32 at each store.  No atomics.
#include "ser_common.h"

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over the 4 waves of a 256-thread block, fixed order; every thread gets the result.  red: 4 doubles of LDS per call site in flight.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();                                              // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------- attention scores
// One wave per row: scores[m] = sum_d tanhf(hlin[m, d]) * a[d].  Lane l owns columns 4 l + 256 i (16-byte loads), adds its products in
// ascending i, then the wave butterfly.  tanhf is the library's (no fast-math in this build): <= 2 ulp.
__global__ __launch_bounds__(256) void asp_scores_kernel(const float* __restrict__ hlin, int64_t ldh, const float* __restrict__ a,
                                                         float* __restrict__ scores, int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;                                        // whole waves leave: the shuffles below stay wave-uniform
    const float* h = hlin + m * ldh;
    double acc = 0.0;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *(const f32x4*)(h + c);
        const f32x4 w = *(const f32x4*)(a + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)tanhf(v[j]) * (double)w[j];
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) scores[m] = (float)acc;
}

// ------------------------------------------------------------------------------- weighted moments
// Block (column slab of 64, utterance).  Thread (rg = tid / 16, cq = tid % 16) owns columns 4 cq .. 4 cq + 3 of the slab and the frames
// t = rg, rg + 16, ...: w_t = exp(s_t - max_t s) in float64, sums of w, w x, w x^2 in ascending t; the 16 row groups are merged in
// ascending rg.  x is read once (every element by exactly one thread, 16 bytes at a time); the scores are re-read per slab (4 bytes a row).
#define ASP_SLAB 64
#define ASP_RG 16
__global__ __launch_bounds__(256) void asp_pool_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ scores,
                                                       const int32_t* __restrict__ frame_offs, float* __restrict__ out, int64_t ldo,
                                                       int D, int rows) {
    __shared__ float smax[4];
    __shared__ double red[ASP_RG][16][9];                         // [row group][column quad][sum w | sum w x [4] | sum w x^2 [4]]
    const int b = blockIdx.y, tid = threadIdx.x;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;                                           // the offsets are the caller's contract; never read outside [0, rows)
    if (r1 > rows) r1 = rows;
    const int T = r1 - r0;
    const int col0 = blockIdx.x * ASP_SLAB;
    float* o = out + (int64_t)b * ldo;
    if (T <= 0) {                                                 // an empty utterance: no frames to weigh
        if (tid < ASP_SLAB && col0 + tid < D) { o[col0 + tid] = 0.f; o[D + col0 + tid] = (float)sqrt((double)1e-5f); }
        return;
    }
    const float* s = scores + r0;
    float mx = -INFINITY;
    for (int t = tid; t < T; t += 256) mx = fmaxf(mx, s[t]);
    mx = wave_max(mx);
    if ((tid & 63) == 0) smax[tid >> 6] = mx;
    __syncthreads();
    const double smx = (double)fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    const int rg = tid >> 4, cq = tid & 15;
    const int col = col0 + cq * 4;
    const bool live = col < D;                                    // D % 4 == 0: a quad is inside or outside as a whole
    double sw = 0.0, s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    const float* xp = x + (int64_t)r0 * ldx + col;
    for (int t = rg; t < T; t += ASP_RG) {
        const double w = exp((double)s[t] - smx);
        sw += w;
        if (live) {
            const f32x4 v = *(const f32x4*)(xp + (int64_t)t * ldx);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double xv = (double)v[j];
                s1[j] = fma(w, xv, s1[j]);
                s2[j] = fma(w, xv * xv, s2[j]);
            }
        }
    }
    red[rg][cq][0] = sw;
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[rg][cq][1 + j] = s1[j]; red[rg][cq][5 + j] = s2[j]; }
    __syncthreads();
    if (tid < ASP_SLAB && col0 + tid < D) {                       // one thread per column of the slab
        const int q = tid >> 2, j = tid & 3;
        double w = 0.0, m1 = 0.0, m2 = 0.0;
        for (int g = 0; g < ASP_RG; ++g) { w += red[g][q][0]; m1 += red[g][q][1 + j]; m2 += red[g][q][5 + j]; }
        const double mu = m1 / w;
        double var = m2 / w - mu * mu;
        if (!(var >= (double)1e-5f)) var = (double)1e-5f;         // .clamp(min=1e-5) (pooling.py:56)
        o[col0 + tid] = (float)mu;
        o[D + col0 + tid] = (float)sqrt(var);
    }
}

extern "C" int ser_asp_pool_v(const ser_asp_pool_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_asp_pool: null pointer");
    if (!a->x || !a->hlin || !a->a || !a->frame_offs || !a->scores || !a->out) return ser_fail(-1, "ser_asp_pool: null pointer");
    if (a->B <= 0 || a->B > 65535 || a->D <= 0 || (a->D % 4) || a->rows <= 0 || a->max_frames <= 0 || a->max_frames > a->rows)
        return ser_fail(-2, "ser_asp_pool: bad B=%d D=%d (D %% 4 == 0) rows=%d max_frames=%d", a->B, a->D, a->rows, a->max_frames);
    if (a->ldx < a->D || a->ldh < a->D || (a->ldx % 4) || (a->ldh % 4) || a->ldo < 2 * (int64_t)a->D)
        return ser_fail(-2, "ser_asp_pool: bad pitches ldx=%lld ldh=%lld (>= D, multiples of 4) ldo=%lld (>= 2 D)", (long long)a->ldx,
                        (long long)a->ldh, (long long)a->ldo);
    if ((((uintptr_t)a->x | (uintptr_t)a->hlin | (uintptr_t)a->a) & 15) != 0) return ser_fail(-2, "ser_asp_pool: x, hlin and a must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(asp_scores_kernel, dim3((unsigned)((a->rows + 3) / 4)), dim3(256), 0, s, a->hlin, a->ldh, a->a, a->scores, a->rows, a->D);
    hipLaunchKernelGGL(asp_pool_kernel, dim3((unsigned)((a->D + ASP_SLAB - 1) / ASP_SLAB), a->B), dim3(256), 0, s, a->x, a->ldx, a->scores,
                       a->frame_offs, a->out, a->ldo, a->D, a->rows);
    return ser_check_launch("ser_asp_pool");
}

// ------------------------------------------------------------------------------- head, first Linear
// One wave per hidden unit j: its W1 row sits in registers (KV 16-byte chunks per lane, lane l owns columns 4 l + 256 i), and the wave
// walks the B utterances: hidden[b, j] = fp32(sum_k p[b, k] W1[j, k] + b1[j]), products added per lane in ascending column, then the butterfly.
template <int KV>
__global__ __launch_bounds__(256) void mlp_hidden_kernel(const float* __restrict__ p, int64_t ldp, const float* __restrict__ W1,
                                                         const float* __restrict__ b1, float* __restrict__ hidden, int B, int K, int H) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= H) return;
    f32x4 w[KV];
#pragma unroll
    for (int i = 0; i < KV; ++i) {
        const int c = lane * 4 + 256 * i;
        w[i] = c < K ? *(const f32x4*)(W1 + (int64_t)j * K + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const double bias = (double)b1[j];
    for (int b = 0; b < B; ++b) {
        const float* pr = p + (int64_t)b * ldp;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < KV; ++i) {
            const int c = lane * 4 + 256 * i;
            if (c < K) {
                const f32x4 v = *(const f32x4*)(pr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = fma((double)v[e], (double)w[i][e], acc);
            }
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) hidden[(int64_t)b * H + j] = (float)(acc + bias);
    }
}

// ------------------------------------------------------------------------------- head, LayerNorm -> ReLU -> second Linear
// One block per utterance.  LayerNorm(H) two-pass (mean, then the centred squares; biased variance, eps inside the root), thread t owns
// units t, t + 256, ...; its n_out partial dot products run over the same units in ascending order.
#define MLP_NOUT_MAX 8
__global__ __launch_bounds__(256) void mlp_out_kernel(const float* __restrict__ hidden, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, const float* __restrict__ W2,
                                                      const float* __restrict__ b2, float* __restrict__ out, int H, int n_out) {
    __shared__ double red[4];
    __shared__ double redo[4][MLP_NOUT_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* h = hidden + (int64_t)b * H;
    double s = 0.0;
    for (int k = tid; k < H; k += 256) s += (double)h[k];
    const double mean = block_sum_f64(s, red) / (double)H;
    double q = 0.0;
    for (int k = tid; k < H; k += 256) { const double d = (double)h[k] - mean; q = fma(d, d, q); }
    const double rstd = 1.0 / sqrt(block_sum_f64(q, red) / (double)H + (double)eps);
    double acc[MLP_NOUT_MAX];
#pragma unroll
    for (int o = 0; o < MLP_NOUT_MAX; ++o) acc[o] = 0.0;
    for (int k = tid; k < H; k += 256) {
        double y = ((double)h[k] - mean) * rstd * (double)gamma[k] + (double)beta[k];
        y = y > 0.0 ? y : 0.0;
#pragma unroll
        for (int o = 0; o < MLP_NOUT_MAX; ++o)
            if (o < n_out) acc[o] = fma(y, (double)W2[(int64_t)o * H + k], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < MLP_NOUT_MAX; ++o) {
        const double v = wave_sum_f64(acc[o]);
        if ((tid & 63) == 0) redo[tid >> 6][o] = v;
    }
    __syncthreads();
    if (tid < n_out) out[(int64_t)b * n_out + tid] = (float)(((redo[0][tid] + redo[1][tid]) + (redo[2][tid] + redo[3][tid])) + (double)b2[tid]);
}

extern "C" int ser_mlp_head_v(const ser_mlp_head_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_mlp_head: null pointer");
    if (!a->p || !a->W1 || !a->b1 || !a->gamma || !a->beta || !a->W2 || !a->b2 || !a->hidden || !a->out)
        return ser_fail(-1, "ser_mlp_head: null pointer");
    if (a->n_out < 1 || a->n_out > MLP_NOUT_MAX) return ser_fail(-2, "ser_mlp_head: n_out=%d (1..%d)", a->n_out, MLP_NOUT_MAX);
    if (a->B <= 0 || a->H <= 0 || a->K <= 0 || (a->K % 4) || a->K > 4096 || a->ldp < a->K || (a->ldp % 4))
        return ser_fail(-2, "ser_mlp_head: bad B=%d H=%d K=%d (K %% 4 == 0, K <= 4096) ldp=%lld (>= K, multiple of 4)", a->B, a->H, a->K,
                        (long long)a->ldp);
    if ((((uintptr_t)a->p | (uintptr_t)a->W1) & 15) != 0) return ser_fail(-2, "ser_mlp_head: p and W1 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((a->H + 3) / 4)), block(256);
#define MLP_HIDDEN(KV) hipLaunchKernelGGL(mlp_hidden_kernel<KV>, grid, block, 0, s, a->p, a->ldp, a->W1, a->b1, a->hidden, a->B, a->K, a->H)
    if (a->K <= 256) MLP_HIDDEN(1);
    else if (a->K <= 512) MLP_HIDDEN(2);
    else if (a->K <= 1024) MLP_HIDDEN(4);
    else if (a->K <= 2048) MLP_HIDDEN(8);
    else MLP_HIDDEN(16);
#undef MLP_HIDDEN
    hipLaunchKernelGGL(mlp_out_kernel, dim3(a->B), dim3(256), 0, s, a->hidden, a->gamma, a->beta, a->eps, a->W2, a->b2, a->out, a->H, a->n_out);
    return ser_check_launch("ser_mlp_head");
}
