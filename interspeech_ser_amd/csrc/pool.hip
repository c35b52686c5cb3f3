// The utterance-level tails of the three device heads, one kernel per pattern:
//   ser_asp_pool_v    organiser baseline (benchmark/train_eval_files/eval_cat_ser.py:164-177, eval_dim_ser.py): attentive statistics pooling
//                     over a packed ragged batch (benchmark/net/pooling.py AttentiveStatisticsPooling.forward)
//   ser_mlp_head_v    its 2D -> H -> n_out head (benchmark/net/ser.py EmotionRegression)
//   ser_attn_pool_v   fusion heads (bin/train_cat_bimodal_lazy_1head.py MultiModalEmotionClassifier): softmax attention pooling of (a + b)
//   ser_fusion_cls_v  their LayerNorm -> Linear -> ReLU -> Linear on the pooled rows
//   ser_layer_pool_v  hub audio-classification heads (HF *ForSequenceClassification / WhisperForAudioClassification): softmax-weighted
//                     sum of the hidden states and the mean over an utterance's frames, in one pass over the states
//   ser_cls_tail_v    their projector and classifier on the pooled rows
// ser_hip.h states the arithmetic.  Every sum accumulates in float64 in an order that depends on the utterance alone (its frame count and
// the widths), never on the batch; one rounding to fp32 at each store.  No atomics.
#include "tail_common.h"

// sum over the 4 waves of a 256-thread block, fixed order; every thread gets the result.  red: 4 doubles of LDS per call site in flight.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();                                              // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// LayerNorm statistics of one row per block, two-pass (mean, then the centred squares; biased variance, eps inside the root); thread t
// owns elements t, t + 256, ...
__device__ __forceinline__ void row_stats_f64(const float* x, int n, float eps, double* red, double& mean, double& rstd) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += (double)x[k];
    mean = block_sum_f64(s, red) / (double)n;
    double q = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) { const double d = (double)x[k] - mean; q = fma(d, d, q); }
    rstd = 1.0 / sqrt(block_sum_f64(q, red) / (double)n + (double)eps);
}

// ------------------------------------------------------------------------------- attention scores
// One wave per row: lane l owns columns 4 l + 256 i (16-byte loads) and adds its terms in ascending i, then the wave butterfly; lane 0
// stores.  TERM::add puts the four terms of row m at columns c .. c + 3 on the lane's sum; TERM::finish makes the stored score.
struct asp_term {                                                 // ser_asp_pool_v: sum_d tanhf(hlin[m, d]) a[d]; tanhf is the library's
    const float* hlin; int64_t ldh; const float* a;               // (no fast-math in this build): <= 2 ulp
    __device__ void add(double& acc, int64_t m, int c) const {
        const f32x4 v = *(const f32x4*)(hlin + m * ldh + c);
        const f32x4 w = *(const f32x4*)(a + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (double)tanhf(v[j]) * (double)w[j];
    }
    __device__ float finish(double acc) const { return (float)acc; }
};
struct sum_term {                                                 // ser_attn_pool_v: sum_e (a + b)[m, e] w[e] + bias
    const float* a; int64_t lda; const float* b; int64_t ldb; const float* w; float bias;
    __device__ void add(double& acc, int64_t m, int c) const {
        const f32x4 va = *(const f32x4*)(a + m * lda + c), vb = *(const f32x4*)(b + m * ldb + c), vw = *(const f32x4*)(w + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fma((double)va[j] + (double)vb[j], (double)vw[j], acc);
    }
    __device__ float finish(double acc) const { return (float)(acc + (double)bias); }
};

template <class TERM>
__global__ __launch_bounds__(256) void tail_scores_kernel(TERM term, float* __restrict__ scores, int rows, int W) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;                                        // whole waves leave: the shuffles below stay wave-uniform
    double acc = 0.0;
    for (int c = lane * 4; c < W; c += 256) term.add(acc, m, c);
    acc = wave_sum_f64(acc);
    if (lane == 0) scores[m] = term.finish(acc);
}

// ------------------------------------------------------------------------------- weighted moments
// Block (column slab of 64, utterance).  Thread (rg = tid / 16, cq = tid % 16) owns columns 4 cq .. 4 cq + 3 of the slab and the frames
// t = rg, rg + 16, ...: w_t = exp(s_t - max_t s) in float64, sums of w, w x (and w x^2 with M2) in ascending t; the 16 row groups are
// merged in ascending rg.  The source is read once (every element by exactly one thread, 16 bytes at a time); the scores are re-read per
// slab (4 bytes a row).  Stores: the mean at out[b, col0 + c]; with M2 also sqrt(max(variance, 1e-5f)) at out[b, col0 + W + c].
struct one_src {                                                  // ser_asp_pool_v: x
    const float* x; int64_t ldx;
    __device__ void load(int64_t row, int col, double* xv) const {
        const f32x4 v = *(const f32x4*)(x + row * ldx + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (double)v[j];
    }
};
struct sum_src {                                                  // ser_attn_pool_v: a + b
    const float* a; int64_t lda; const float* b; int64_t ldb;
    __device__ void load(int64_t row, int col, double* xv) const {
        const f32x4 va = *(const f32x4*)(a + row * lda + col), vb = *(const f32x4*)(b + row * ldb + col);
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = (double)va[j] + (double)vb[j];
    }
};

#define POOL_SLAB 64
#define POOL_RG 16
template <bool M2, class SRC>
__global__ __launch_bounds__(256) void tail_moments_kernel(SRC src, const float* __restrict__ scores, const int32_t* __restrict__ frame_offs,
                                                           float* __restrict__ out, int64_t ldo, int col0, int W, int rows) {
    __shared__ float smax[4];
    __shared__ double red[POOL_RG][16][M2 ? 9 : 5];               // [row group][column quad][sum w | sum w x [4] | sum w x^2 [4]]
    const int b = blockIdx.y, tid = threadIdx.x;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;                                           // the offsets are the caller's contract; never read outside [0, rows)
    if (r1 > rows) r1 = rows;
    const int T = r1 - r0;
    const int c0 = blockIdx.x * POOL_SLAB;
    float* o = out + (int64_t)b * ldo + col0;
    if (T <= 0) {                                                 // an empty utterance: no frames to weigh
        if (tid < POOL_SLAB && c0 + tid < W) {
            o[c0 + tid] = 0.f;
            if (M2) o[W + c0 + tid] = (float)sqrt((double)1e-5f);
        }
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
    const int col = c0 + cq * 4;
    const bool live = col < W;                                    // W % 4 == 0: a quad is inside or outside as a whole
    double sw = 0.0, s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = rg; t < T; t += POOL_RG) {
        const double w = exp((double)s[t] - smx);
        sw += w;
        if (live) {
            double xv[4];
            src.load((int64_t)r0 + t, col, xv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s1[j] = fma(w, xv[j], s1[j]);
                if (M2) s2[j] = fma(w, xv[j] * xv[j], s2[j]);
            }
        }
    }
    red[rg][cq][0] = sw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[rg][cq][1 + j] = s1[j];
        if (M2) red[rg][cq][5 + j] = s2[j];
    }
    __syncthreads();
    if (tid < POOL_SLAB && c0 + tid < W) {                        // one thread per column of the slab
        const int q = tid >> 2, j = tid & 3;
        double w = 0.0, m1 = 0.0, m2 = 0.0;
        for (int g = 0; g < POOL_RG; ++g) {
            w += red[g][q][0];
            m1 += red[g][q][1 + j];
            if (M2) m2 += red[g][q][5 + j];
        }
        const double mu = m1 / w;
        o[c0 + tid] = (float)mu;
        if (M2) {
            double var = m2 / w - mu * mu;
            if (!(var >= (double)1e-5f)) var = (double)1e-5f;     // .clamp(min=1e-5) (pooling.py:56)
            o[W + c0 + tid] = (float)sqrt(var);
        }
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
    hipLaunchKernelGGL(tail_scores_kernel<asp_term>, dim3((unsigned)((a->rows + 3) / 4)), dim3(256), 0, s, asp_term{a->hlin, a->ldh, a->a},
                       a->scores, a->rows, a->D);
    hipLaunchKernelGGL((tail_moments_kernel<true, one_src>), dim3((unsigned)((a->D + POOL_SLAB - 1) / POOL_SLAB), (unsigned)a->B), dim3(256), 0, s,
                       one_src{a->x, a->ldx}, a->scores, a->frame_offs, a->out, a->ldo, 0, a->D, a->rows);
    return ser_check_launch("ser_asp_pool");
}

extern "C" int ser_attn_pool_v(const ser_attn_pool_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_attn_pool: null pointer");
    if (!a->a || !a->b || !a->w || !a->frame_offs || !a->scores || !a->out) return ser_fail(-1, "ser_attn_pool: null pointer");
    if (a->B <= 0 || a->B > 65535 || a->E <= 0 || (a->E % 4) || a->rows <= 0 || a->max_frames <= 0 || a->max_frames > a->rows || a->col0 < 0)
        return ser_fail(-2, "ser_attn_pool: bad B=%d E=%d (E %% 4 == 0) rows=%d max_frames=%d col0=%d", a->B, a->E, a->rows, a->max_frames, a->col0);
    if (a->lda < a->E || a->ldb < a->E || (a->lda % 4) || (a->ldb % 4) || a->ldo < (int64_t)a->col0 + a->E)
        return ser_fail(-2, "ser_attn_pool: bad pitches lda=%lld ldb=%lld (>= E, multiples of 4) ldo=%lld (>= col0 + E)", (long long)a->lda,
                        (long long)a->ldb, (long long)a->ldo);
    if ((((uintptr_t)a->a | (uintptr_t)a->b | (uintptr_t)a->w) & 15) != 0) return ser_fail(-2, "ser_attn_pool: a, b and w must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tail_scores_kernel<sum_term>, dim3((unsigned)((a->rows + 3) / 4)), dim3(256), 0, s,
                       sum_term{a->a, a->lda, a->b, a->ldb, a->w, a->bias}, a->scores, a->rows, a->E);
    hipLaunchKernelGGL((tail_moments_kernel<false, sum_src>), dim3((unsigned)((a->E + POOL_SLAB - 1) / POOL_SLAB), (unsigned)a->B), dim3(256), 0, s,
                       sum_src{a->a, a->lda, a->b, a->ldb}, a->scores, a->frame_offs, a->out, a->ldo, a->col0, a->E, a->rows);
    return ser_check_launch("ser_attn_pool");
}

// ------------------------------------------------------------------------------- LayerNorm in front of the fusion classifier
// One block per row: float64 statistics, the normalised row rounded to fp32.
__global__ __launch_bounds__(256) void tail_ln_kernel(const float* __restrict__ p, int64_t ldp, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, float* __restrict__ xn, int K) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const float* x = p + (int64_t)b * ldp;
    double mean, rstd;
    row_stats_f64(x, K, eps, red, mean, rstd);
    for (int k = threadIdx.x; k < K; k += 256) xn[(int64_t)b * K + k] = (float)(((double)x[k] - mean) * rstd * (double)gamma[k] + (double)beta[k]);
}

// ------------------------------------------------------------------------------- hidden units (first Linear)
// One wave per hidden unit j: its W1 row sits in registers (KV 16-byte chunks per lane, lane l owns columns 4 l + 256 i), and the wave
// walks the B rows of p (pitch ldp): hidden[b, j] = fp32(sum_k p[b, k] W1[j, k] + b1[j]), through a ReLU with RELU; products added per
// lane in ascending column, then the butterfly.
template <int KV, bool RELU>
__global__ __launch_bounds__(256) void tail_hidden_kernel(const float* __restrict__ p, int64_t ldp, const float* __restrict__ W1,
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
        acc = wave_sum_f64(acc) + bias;
        if (RELU) acc = acc > 0.0 ? acc : 0.0;
        if (lane == 0) hidden[(int64_t)b * H + j] = (float)acc;
    }
}

// the register plan of a W1 row: K <= 4096 in 1, 2, 4, 8 or 16 chunks a lane
template <bool RELU>
static void tail_hidden_launch(const float* p, int64_t ldp, const float* W1, const float* b1, float* hidden, int B, int K, int H, hipStream_t s) {
    const dim3 grid((unsigned)((H + 3) / 4)), block(256);
    const int chunks = K <= 256 ? 1 : (K <= 512 ? 2 : (K <= 1024 ? 4 : (K <= 2048 ? 8 : 16)));
    ser_with_mode<1, 2, 4, 8, 16>(chunks, [&](auto KV) {
        hipLaunchKernelGGL((tail_hidden_kernel<KV(), RELU>), grid, block, 0, s, p, ldp, W1, b1, hidden, B, K, H);
    });
}

// ------------------------------------------------------------------------------- outputs (second Linear)
// One block per row; thread t owns units t, t + 256, ... and runs its n_out partial dot products over them in ascending order.  With LN
// the units first pass LayerNorm(H) and a ReLU.
#define TAIL_NOUT_MAX 8
template <bool LN>
__global__ __launch_bounds__(256) void tail_out_kernel(const float* __restrict__ hidden, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, const float* __restrict__ W2,
                                                       const float* __restrict__ b2, float* __restrict__ out, int H, int n_out) {
    __shared__ double redo[4][TAIL_NOUT_MAX];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* h = hidden + (int64_t)b * H;
    double mean = 0.0, rstd = 1.0;
    if constexpr (LN) {
        __shared__ double red[4];
        row_stats_f64(h, H, eps, red, mean, rstd);
    }
    double acc[TAIL_NOUT_MAX];
#pragma unroll
    for (int o = 0; o < TAIL_NOUT_MAX; ++o) acc[o] = 0.0;
    for (int k = tid; k < H; k += 256) {
        double y = (double)h[k];
        if constexpr (LN) {
            y = (y - mean) * rstd * (double)gamma[k] + (double)beta[k];
            y = y > 0.0 ? y : 0.0;
        }
#pragma unroll
        for (int o = 0; o < TAIL_NOUT_MAX; ++o)
            if (o < n_out) acc[o] = fma(y, (double)W2[(int64_t)o * H + k], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < TAIL_NOUT_MAX; ++o) {
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
    if (a->n_out < 1 || a->n_out > TAIL_NOUT_MAX) return ser_fail(-2, "ser_mlp_head: n_out=%d (1..%d)", a->n_out, TAIL_NOUT_MAX);
    if (a->B <= 0 || a->H <= 0 || a->K <= 0 || (a->K % 4) || a->K > 4096 || a->ldp < a->K || (a->ldp % 4))
        return ser_fail(-2, "ser_mlp_head: bad B=%d H=%d K=%d (K %% 4 == 0, K <= 4096) ldp=%lld (>= K, multiple of 4)", a->B, a->H, a->K,
                        (long long)a->ldp);
    if ((((uintptr_t)a->p | (uintptr_t)a->W1) & 15) != 0) return ser_fail(-2, "ser_mlp_head: p and W1 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    tail_hidden_launch<false>(a->p, a->ldp, a->W1, a->b1, a->hidden, a->B, a->K, a->H, s);
    hipLaunchKernelGGL(tail_out_kernel<true>, dim3((unsigned)a->B), dim3(256), 0, s, a->hidden, a->gamma, a->beta, a->eps, a->W2, a->b2, a->out,
                       a->H, a->n_out);
    return ser_check_launch("ser_mlp_head");
}

extern "C" int ser_fusion_cls_v(const ser_fusion_cls_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_fusion_cls: null pointer");
    if (!a->p || !a->gamma || !a->beta || !a->W1 || !a->b1 || !a->W2 || !a->b2 || !a->xn || !a->hidden || !a->out)
        return ser_fail(-1, "ser_fusion_cls: null pointer");
    if (a->n_out < 1 || a->n_out > TAIL_NOUT_MAX) return ser_fail(-2, "ser_fusion_cls: n_out=%d (1..%d)", a->n_out, TAIL_NOUT_MAX);
    if (a->B <= 0 || a->B > 65535 || a->H1 <= 0 || a->K <= 0 || (a->K % 4) || a->K > 4096 || a->ldp < a->K)
        return ser_fail(-2, "ser_fusion_cls: bad B=%d H1=%d K=%d (K %% 4 == 0, K <= 4096) ldp=%lld (>= K)", a->B, a->H1, a->K, (long long)a->ldp);
    if ((((uintptr_t)a->xn | (uintptr_t)a->W1) & 15) != 0) return ser_fail(-2, "ser_fusion_cls: xn and W1 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tail_ln_kernel, dim3((unsigned)a->B), dim3(256), 0, s, a->p, a->ldp, a->gamma, a->beta, a->eps, a->xn, a->K);
    tail_hidden_launch<true>(a->xn, a->K, a->W1, a->b1, a->hidden, a->B, a->K, a->H1, s);
    hipLaunchKernelGGL(tail_out_kernel<false>, dim3((unsigned)a->B), dim3(256), 0, s, a->hidden, nullptr, nullptr, 0.f, a->W2, a->b2, a->out,
                       a->H1, a->n_out);
    return ser_check_launch("ser_fusion_cls");
}

// ------------------------------------------------------------------------------- layer-weighted frame mean
// pooled[b, d] = (1 / T_b) sum_t sum_l w_l s[l, r0_b + t, d].  The utterance's frames are cut into chunks of SER_LAYER_POOL_FC counted from
// its first row.  Block (256-column slab, chunk, utterance): wave g owns the chunk's frames g, g + 4, ... and lane q the columns
// 4 q .. 4 q + 3 of the slab (one 1 KiB row segment per wave and load); a thread adds its terms frame by frame, within a frame in ascending
// state, then the four waves are merged in ascending g and the chunk's partial goes to work[b, chunk, :] in float64.  Every element of s
// is read once, 16 bytes at a time.  A chunk past the utterance's last frame leaves at once.
__global__ __launch_bounds__(256) void layer_pool_chunk_kernel(const float* __restrict__ s, int64_t state_stride, int64_t lds,
                                                               const double* __restrict__ w, const int32_t* __restrict__ frame_offs,
                                                               double* __restrict__ work, int n_states, int D, int rows, int n_chunks) {
    __shared__ double red[4][256];
    const int b = blockIdx.z, chunk = blockIdx.y, tid = threadIdx.x;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;                                           // the launcher checked the host copy; never read outside [0, rows)
    if (r1 > rows) r1 = rows;
    const int t0 = chunk * SER_LAYER_POOL_FC;
    if (t0 >= r1 - r0) return;                                    // block-uniform
    const int t1 = min(t0 + SER_LAYER_POOL_FC, r1 - r0);
    const int g = tid >> 6, q = tid & 63;
    const int col = blockIdx.x * 256 + q * 4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < D) {                                                // D % 4 == 0: a quad is inside or outside as a whole
        for (int t = t0 + g; t < t1; t += 4) {
            const float* row = s + (int64_t)(r0 + t) * lds + col;
#pragma unroll 5
            for (int l = 0; l < n_states; ++l) {
                const f32x4 v = *(const f32x4*)(row + (int64_t)l * state_stride);
                const double wl = w[l];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fma(wl, (double)v[j], acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[g][q * 4 + j] = acc[j];
    __syncthreads();
    const int c = blockIdx.x * 256 + tid;                         // one thread per column of the slab
    if (c < D) work[((int64_t)b * n_chunks + chunk) * D + c] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// One thread per (utterance, column): the chunk partials in ascending chunk, the division by the frame count, one rounding.
__global__ __launch_bounds__(256) void layer_pool_finish_kernel(const double* __restrict__ work, const int32_t* __restrict__ frame_offs,
                                                                float* __restrict__ out, int64_t ldo, int D, int rows, int n_chunks) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > rows) r1 = rows;
    const int T = r1 - r0;
    if (T <= 0) { out[(int64_t)b * ldo + c] = 0.f; return; }
    const int used = min((T + SER_LAYER_POOL_FC - 1) / SER_LAYER_POOL_FC, n_chunks);
    const double* p = work + (int64_t)b * n_chunks * D + c;
    double sum = 0.0;
    for (int k = 0; k < used; ++k) sum += p[(int64_t)k * D];
    out[(int64_t)b * ldo + c] = (float)(sum / (double)T);
}

extern "C" int ser_layer_pool_v(const ser_layer_pool_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_layer_pool: null pointer");
    if (!a->s || !a->w || !a->frame_offs || !a->frame_offs_host || !a->work || !a->out) return ser_fail(-1, "ser_layer_pool: null pointer");
    if (a->n_states < 1) return ser_fail(-2, "ser_layer_pool: n_states=%d (at least 1)", a->n_states);
    if (a->B <= 0 || a->B > 65535 || a->D <= 0 || (a->D % 4) || a->rows <= 0 || a->max_frames <= 0 || a->max_frames > a->rows)
        return ser_fail(-2, "ser_layer_pool: bad B=%d (1..65535) D=%d (D %% 4 == 0) rows=%d max_frames=%d (<= rows)", a->B, a->D, a->rows,
                        a->max_frames);
    const int64_t n_chunks = ((int64_t)a->max_frames + SER_LAYER_POOL_FC - 1) / SER_LAYER_POOL_FC;
    if (n_chunks > 65535) return ser_fail(-2, "ser_layer_pool: max_frames=%d is beyond %d chunks of %d frames", a->max_frames, 65535, SER_LAYER_POOL_FC);
    if (a->lds < a->D || (a->lds % 4) || (a->state_stride % 4) || a->ldo < a->D || (a->n_states > 1 && a->state_stride <= 0))
        return ser_fail(-2, "ser_layer_pool: bad pitches lds=%lld (>= D, multiple of 4) state_stride=%lld (multiple of 4) ldo=%lld (>= D)",
                        (long long)a->lds, (long long)a->state_stride, (long long)a->ldo);
    if ((((uintptr_t)a->s) & 15) != 0 || (((uintptr_t)a->w | (uintptr_t)a->work) & 7) != 0)
        return ser_fail(-2, "ser_layer_pool: s must be 16-byte aligned, w and work 8-byte aligned");
    if (a->work_elems < (int64_t)a->B * n_chunks * a->D)
        return ser_fail(-2, "ser_layer_pool: work holds %lld doubles, B * ceil(max_frames / %d) * D = %lld are needed", (long long)a->work_elems,
                        SER_LAYER_POOL_FC, (long long)((int64_t)a->B * n_chunks * a->D));
    for (int b = 0; b < a->B; ++b) {                              // the host copy of the offsets: what the grid and the reads rely on
        const int64_t r0 = a->frame_offs_host[b], r1 = a->frame_offs_host[b + 1];
        if (r0 < 0 || r1 > a->rows || r1 < r0) return ser_fail(-2, "ser_layer_pool: utterance %d owns rows %lld..%lld outside [0, %d]", b, (long long)r0, (long long)r1, a->rows);
        if (r1 == r0) return ser_fail(-2, "ser_layer_pool: utterance %d is empty (no frame to average)", b);
        if (r1 - r0 > a->max_frames) return ser_fail(-2, "ser_layer_pool: utterance %d has %lld frames, max_frames=%d", b, (long long)(r1 - r0), a->max_frames);
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned slabs = (unsigned)((a->D + 255) / 256);
    hipLaunchKernelGGL(layer_pool_chunk_kernel, dim3(slabs, (unsigned)n_chunks, (unsigned)a->B), dim3(256), 0, st, a->s, a->state_stride, a->lds, a->w,
                       a->frame_offs, a->work, a->n_states, a->D, a->rows, (int)n_chunks);
    hipLaunchKernelGGL(layer_pool_finish_kernel, dim3(slabs, (unsigned)a->B), dim3(256), 0, st, a->work, a->frame_offs, a->out, a->ldo, a->D, a->rows,
                       (int)n_chunks);
    return ser_check_launch("ser_layer_pool");
}

// ------------------------------------------------------------------------------- projector and classifier on the pooled rows
// cls_tail_kernel (tail_common.h, shared with ser_xvec_tail_v) in the form that never rounds the projector unit.
extern "C" int ser_cls_tail_v(const ser_cls_tail_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_cls_tail: null pointer");
    if (!a->pooled || !a->P || !a->bp || !a->C || !a->bc || !a->out) return ser_fail(-1, "ser_cls_tail: null pointer");
    if (a->proj < 1 || a->proj > CLS_TAIL_MAX || a->n_labels < 1 || a->n_labels > CLS_TAIL_MAX)
        return ser_fail(-2, "ser_cls_tail: proj=%d n_labels=%d (1..%d each)", a->proj, a->n_labels, CLS_TAIL_MAX);
    if (a->B <= 0 || a->B > 65535 || a->D <= 0 || (a->D % 4) || a->ldp < a->D || (a->ldp % 4) || a->ldo < a->n_labels)
        return ser_fail(-2, "ser_cls_tail: bad B=%d D=%d (D %% 4 == 0) ldp=%lld (>= D, multiple of 4) ldo=%lld (>= n_labels)", a->B, a->D,
                        (long long)a->ldp, (long long)a->ldo);
    if ((((uintptr_t)a->pooled | (uintptr_t)a->P) & 15) != 0) return ser_fail(-2, "ser_cls_tail: pooled and P must be 16-byte aligned");
    hipLaunchKernelGGL(cls_tail_kernel<false>, dim3((unsigned)a->B), dim3(1024), 0, (hipStream_t)stream, a->pooled, a->ldp, a->P, a->bp, a->C, a->bc,
                       a->out, a->ldo, a->D, a->proj, a->n_labels, (float*)nullptr, (int64_t)0);
    return ser_check_launch("ser_cls_tail");
}
