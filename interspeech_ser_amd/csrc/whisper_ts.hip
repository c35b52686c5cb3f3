// Whisper token timestamps from the decoder's cross-attention (include/ser_hip.h, "a33"): four entry points.
//   ser_dec_keep_q_v   a step's capture: the alignment heads' cross queries of one layer -> keep[pos] (a copy; a command-list op)
//   ser_ts_weights_v   after the loop: per (utterance, alignment head, token row) the softmax over ALL keys of the fp32 cross cache,
//                      float64 dot products and float64 softmax, stored as fp32 for frames < F_b only
//   ser_ts_matrix_v    z-score over the utterance's own token rows, median of `width` along the frames (reflect), mean over the heads,
//                      one rounding to fp32
//   ser_dtw_v          HF's _dynamic_time_warping on -matrix: one block per utterance, thread = token row, an anti-diagonal wavefront over
//                      three diagonals of fp32 costs in LDS, one barrier per diagonal, 2-bit back pointers packed per row (32 cells a word),
//                      one backtrack over bands of SER_TS_BAND frames staged in LDS
// No atomics on data.  Every sum has an order that is a function of the utterance alone (the key count, its row count, the head list).
#include "ser_common.h"
#include <math.h>

constexpr int TT = SER_TS_THREADS;
constexpr int BAND = SER_TS_BAND;
constexpr int BW = BAND / 32;                                      // back-pointer words of a row in a band
constexpr int RT = 4;                                              // token rows of a weights block (they share every key they read)
constexpr int KMAX = SER_TS_MAX_KEYS;
static_assert(BAND % 32 == 0 && TT % 64 == 0 && KMAX % 256 == 0, "whole words and waves");

static inline int64_t dtw_words(int max_frames) { return ((int64_t)max_frames + 31) / 32; }

// ---------------------------------------------------------------------------------------------------------------- capture
__global__ __launch_bounds__(64) void dec_keep_q_kernel(ser_dec_keep_q_args a) {
    const int h = blockIdx.x, b = blockIdx.y, l = threadIdx.x;
    const int p = *a.pos;
    const int hd = a.head[h];
    if (p < 0 || p >= a.max_pos || hd < 0 || hd >= a.H) return;    // (refused on the host as well: never an address outside keep)
    a.keep[(((int64_t)p * a.B + b) * a.n_align + a.slot0 + h) * 64 + l] = a.q[(int64_t)b * a.ldq + hd * 64 + l];
}

extern "C" int ser_dec_keep_q_v(const ser_dec_keep_q_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_dec_keep_q: null arguments");
    if (!a->q || !a->pos || !a->keep) return ser_fail(-1, "ser_dec_keep_q: null pointer");
    if (a->B < 1 || a->B > 65535 || a->H < 1 || a->max_pos < 1 || a->n_heads < 1 || a->n_heads > SER_TS_KEEP_HEADS || a->slot0 < 0 ||
        a->n_align < a->slot0 + a->n_heads)
        return ser_fail(-2, "ser_dec_keep_q: B=%d (1..65535) H=%d max_pos=%d n_heads=%d (1..%d) slot0=%d n_align=%d (>= slot0 + n_heads)", a->B, a->H,
                        a->max_pos, a->n_heads, SER_TS_KEEP_HEADS, a->slot0, a->n_align);
    for (int h = 0; h < a->n_heads; ++h)
        if (a->head[h] < 0 || a->head[h] >= a->H) return ser_fail(-2, "ser_dec_keep_q: head[%d]=%d outside [0, H=%d)", h, a->head[h], a->H);
    if (a->ldq < (int64_t)a->H * 64) return ser_fail(-3, "ser_dec_keep_q: ldq=%lld (>= H * 64)", (long long)a->ldq);
    hipLaunchKernelGGL(dec_keep_q_kernel, dim3((unsigned)a->n_heads, (unsigned)a->B), dim3(64), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_dec_keep_q_v");
}

// ---------------------------------------------------------------------------------------------------------------- weights
// Block (row tile, head, utterance), 256 threads.  Thread t takes keys t, t + 256, ...: a key's 64 floats are read once and meet the RT
// queries of the tile (float64 in LDS).  Row maximum: exact.  Row sum: a thread adds its keys in ascending order, the lanes of a wave meet by
// xor shuffles (a + b is commutative: both partners hold the same bits), the four waves are added in wave order.
__global__ __launch_bounds__(256) void ts_weights_kernel(ser_ts_weights_args a) {
    __shared__ double s_q[RT][64];
    __shared__ double s_s[RT][KMAX];
    __shared__ double s_red[RT][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hd = blockIdx.y, b = blockIdx.z, r0 = blockIdx.x * RT;
    int n = a.n_rows[b], F = a.n_frames[b];
    if (n > a.max_rows) n = a.max_rows;                            // (ser_ts_matrix_v reports such an utterance)
    if (F > a.n_keys) F = a.n_keys;
    if (F > a.ld_w) F = (int)a.ld_w;
    if (r0 >= n || F < 1) return;                                  // block-uniform
    const int layer = a.head_layer[hd], hidx = a.head_index[hd];
    for (int i = tid; i < RT * 64; i += 256) {
        const int r = r0 + (i >> 6), p = a.pos0 + r;
        float q = 0.f;
        if (r < n && p < a.max_pos) q = a.keep[(((int64_t)p * a.B + b) * a.n_align + hd) * 64 + (i & 63)];
        s_q[i >> 6][i & 63] = (double)q;
    }
    __syncthreads();
    const float* kb = a.cross + (int64_t)layer * a.layer_stride + (int64_t)b * a.batch_stride + hidx * 64;
    const double scale = (double)a.scale;
    double mx[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) mx[r] = -INFINITY;
    for (int s = tid; s < a.n_keys; s += 256) {
        const float4* kp = (const float4*)(kb + (int64_t)s * a.ldc);
        double acc[RT];
#pragma unroll
        for (int r = 0; r < RT; ++r) acc[r] = 0.0;
#pragma unroll 4
        for (int c = 0; c < 16; ++c) {
            const float4 k4 = kp[c];
            const double k0 = k4.x, k1 = k4.y, k2 = k4.z, k3 = k4.w;
#pragma unroll
            for (int r = 0; r < RT; ++r) {
                acc[r] = fma(s_q[r][4 * c], k0, acc[r]);
                acc[r] = fma(s_q[r][4 * c + 1], k1, acc[r]);
                acc[r] = fma(s_q[r][4 * c + 2], k2, acc[r]);
                acc[r] = fma(s_q[r][4 * c + 3], k3, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const double v = acc[r] * scale;
            s_s[r][s] = v;
            mx[r] = fmax(mx[r], v);                                // fmax drops a NaN; the sum below keeps it
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx[r] = fmax(mx[r], __shfl_xor(mx[r], o, 64));
        if (lane == 0) s_red[r][wv] = mx[r];
    }
    __syncthreads();
    double sum[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        mx[r] = fmax(fmax(s_red[r][0], s_red[r][1]), fmax(s_red[r][2], s_red[r][3]));
        sum[r] = 0.0;
    }
    for (int s = tid; s < a.n_keys; s += 256) {                    // a thread reads back the scores it wrote itself
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const double e = exp(s_s[r][s] - mx[r]);
            s_s[r][s] = e;
            sum[r] += e;
        }
    }
    __syncthreads();                                               // every wave has read the maxima
#pragma unroll
    for (int r = 0; r < RT; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum[r] += __shfl_xor(sum[r], o, 64);
        if (lane == 0) s_red[r][wv] = sum[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (r0 + r >= n) continue;                                 // block-uniform
        const double tot = ((s_red[r][0] + s_red[r][1]) + s_red[r][2]) + s_red[r][3];
        float* wr = a.w + (((int64_t)b * a.n_align + hd) * a.max_rows + r0 + r) * a.ld_w;
        for (int s = tid; s < F; s += 256) wr[s] = (float)(s_s[r][s] / tot);
    }
}

extern "C" int ser_ts_weights_v(const ser_ts_weights_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_ts_weights: null arguments");
    if (!a->keep || !a->cross || !a->n_rows || !a->n_frames || !a->w) return ser_fail(-1, "ser_ts_weights: null pointer");
    if (a->B < 1 || a->B > 65535 || a->n_align < 1 || a->n_align > SER_TS_MAX_HEADS || a->n_keys < 1 || a->n_keys > SER_TS_MAX_KEYS ||
        a->max_rows < 1 || a->max_pos < 1 || a->pos0 < 0 || a->n_layers < 1 || a->H < 1)
        return ser_fail(-2, "ser_ts_weights: B=%d (1..65535) n_align=%d (1..%d) n_keys=%d (1..%d) max_rows=%d max_pos=%d pos0=%d n_layers=%d H=%d", a->B,
                        a->n_align, SER_TS_MAX_HEADS, a->n_keys, SER_TS_MAX_KEYS, a->max_rows, a->max_pos, a->pos0, a->n_layers, a->H);
    for (int h = 0; h < a->n_align; ++h)
        if (a->head_layer[h] < 0 || a->head_layer[h] >= a->n_layers || a->head_index[h] < 0 || a->head_index[h] >= a->H)
            return ser_fail(-2, "ser_ts_weights: alignment head %d = (layer %d, head %d) outside %d layers of %d heads", h, a->head_layer[h],
                            a->head_index[h], a->n_layers, a->H);
    if (a->ldc < (int64_t)a->H * 64 || (a->ldc & 3) || (a->layer_stride & 3) || (a->batch_stride & 3) || a->batch_stride < a->ldc * a->n_keys ||
        a->layer_stride < 0 || a->ld_w < 1)
        return ser_fail(-3, "ser_ts_weights: bad pitches ldc=%lld (>= H * 64, % 4) batch_stride=%lld (>= n_keys ldc, % 4) layer_stride=%lld ld_w=%lld",
                        (long long)a->ldc, (long long)a->batch_stride, (long long)a->layer_stride, (long long)a->ld_w);
    if (((uintptr_t)a->cross) & 15) return ser_fail(-3, "ser_ts_weights: cross must be 16-byte aligned");
    const unsigned tiles = (unsigned)((a->max_rows + RT - 1) / RT);
    hipLaunchKernelGGL(ts_weights_kernel, dim3(tiles, (unsigned)a->n_align, (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_ts_weights_v");
}

// ---------------------------------------------------------------------------------------------------------------- matrix
// Statistics: one thread per (utterance, head, frame), the token rows in ascending order -- two passes, mean then the biased variance.
__global__ __launch_bounds__(256) void ts_stats_kernel(ser_ts_matrix_args a) {
#pragma clang fp contract(off)                                     // d * d is rounded before it is added, as the numpy statement rounds it
    const int f = blockIdx.x * 256 + threadIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int n = a.n_rows[b], F = a.n_frames[b];
    const bool bad = n < 0 || n > a.max_rows || F < 0 || F > a.max_frames;
    if (f == 0 && hd == 0) a.status[b] = bad ? SER_TS_BAD_SHAPE : (n >= 1 && F < 1 ? SER_TS_NO_FRAMES : 0);
    if (bad || f >= F || n < 1) return;
    const float* w = a.w + ((int64_t)b * a.n_align + hd) * a.max_rows * a.ld_w + f;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += (double)w[(int64_t)r * a.ld_w];
    const double mean = s / (double)n;
    double v = 0.0;
    for (int r = 0; r < n; ++r) {
        const double d = (double)w[(int64_t)r * a.ld_w] - mean;
        v += d * d;
    }
    double* st = a.stats + (((int64_t)b * a.n_align + hd) * a.max_frames + f) * 2;
    st[0] = mean;
    st[1] = sqrt(v / (double)n);
}

// One thread per (utterance, token row, frame): per head the window's z-scores, their median by rank counting (a selection: exact), the
// heads added in list order.
template <int W>
__global__ __launch_bounds__(256) void ts_matrix_kernel(ser_ts_matrix_args a) {
    const int f = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, b = blockIdx.z;
    const int n = a.n_rows[b], F = a.n_frames[b];
    if (n < 0 || n > a.max_rows || F < 0 || F > a.max_frames || r >= n || f >= F) return;
    constexpr int PAD = W / 2;
    const bool filt = F > PAD;                                     // HF: an input no wider than the pad comes back as it is
    double sum = 0.0;
    bool nonfinite = false;
    for (int hd = 0; hd < a.n_align; ++hd) {
        const float* w = a.w + (((int64_t)b * a.n_align + hd) * a.max_rows + r) * a.ld_w;
        const double* st = a.stats + ((int64_t)b * a.n_align + hd) * a.max_frames * 2;
        double z[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            int c = filt ? f + k - PAD : f;
            c = c < 0 ? -c : c;
            c = c >= F ? 2 * (F - 1) - c : c;
            z[k] = ((double)w[c] - st[2 * c]) / st[2 * c + 1];
            nonfinite |= !(fabs(z[k]) < (double)INFINITY);
        }
        double med = z[PAD];
        if (filt) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                int rank = 0;
#pragma unroll
                for (int m = 0; m < W; ++m) rank += (z[m] < z[k]) || (z[m] == z[k] && m < k);
                if (rank == PAD) med = z[k];
            }
        }
        sum += med;
    }
    const float out = (float)(sum / (double)a.n_align);
    nonfinite |= !(fabsf(out) < INFINITY);
    a.matrix[((int64_t)b * a.max_rows + r) * a.ld_m + f] = out;
    if (nonfinite && n >= 2) a.status[b] = SER_TS_NONFINITE;       // every writer stores the same word; a single row is NaN by the rule
}

extern "C" int ser_ts_matrix_v(const ser_ts_matrix_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_ts_matrix: null arguments");
    if (!a->w || !a->n_rows || !a->n_frames || !a->stats || !a->matrix || !a->status) return ser_fail(-1, "ser_ts_matrix: null pointer");
    if (a->B < 1 || a->B > 65535 || a->n_align < 1 || a->n_align > SER_TS_MAX_HEADS || a->max_rows < 1 || a->max_rows > 65535 || a->max_frames < 1)
        return ser_fail(-2, "ser_ts_matrix: B=%d (1..65535) n_align=%d (1..%d) max_rows=%d (1..65535) max_frames=%d", a->B, a->n_align, SER_TS_MAX_HEADS,
                        a->max_rows, a->max_frames);
    if (a->width != 1 && a->width != 3 && a->width != 5 && a->width != 7 && a->width != 9)
        return ser_fail(-2, "ser_ts_matrix: median width %d (1, 3, 5, 7 or 9)", a->width);
    if (a->ld_w < a->max_frames || a->ld_m < a->max_frames)
        return ser_fail(-3, "ser_ts_matrix: bad pitches ld_w=%lld ld_m=%lld (>= max_frames)", (long long)a->ld_w, (long long)a->ld_m);
    if (((uintptr_t)a->stats) & 7) return ser_fail(-3, "ser_ts_matrix: stats must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned fb = (unsigned)((a->max_frames + 255) / 256);
    hipLaunchKernelGGL(ts_stats_kernel, dim3(fb, (unsigned)a->n_align, (unsigned)a->B), dim3(256), 0, st, *a);
    const dim3 grid(fb, (unsigned)a->max_rows, (unsigned)a->B);
    switch (a->width) {
        case 1: hipLaunchKernelGGL(ts_matrix_kernel<1>, grid, dim3(256), 0, st, *a); break;
        case 3: hipLaunchKernelGGL(ts_matrix_kernel<3>, grid, dim3(256), 0, st, *a); break;
        case 5: hipLaunchKernelGGL(ts_matrix_kernel<5>, grid, dim3(256), 0, st, *a); break;
        case 7: hipLaunchKernelGGL(ts_matrix_kernel<7>, grid, dim3(256), 0, st, *a); break;
        default: hipLaunchKernelGGL(ts_matrix_kernel<9>, grid, dim3(256), 0, st, *a); break;
    }
    return ser_check_launch("ser_ts_matrix_v");
}

// ---------------------------------------------------------------------------------------------------------------- DTW
// s_c[d % 3][i] is cost[i][d - i]: the cell (i, j) of diagonal d = i + j reads (i-1, j-1) from diagonal d - 2 and (i-1, j), (i, j-1) from
// d - 1.  An entry nobody has written is +inf, which is exactly cost[i][0] and cost[0][j > 0]; cost[0][0] = 0 sits in s_c[0][0] until
// thread 0 overwrites it at d = 3.  Thread tid owns row i = tid + 1 for the whole utterance: its matrix row is read a block of 8 diagonals
// ahead, its back pointers collect in a register and leave as one 64-bit word per 32 frames.
__global__ __launch_bounds__(TT) void dtw_kernel(ser_dtw_args a, unsigned long long* __restrict__ bp, int64_t W) {
    __shared__ float s_c[3][TT + 1];
    __shared__ unsigned long long s_bp[TT * BW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.n_rows[b], M = a.n_frames[b];
    if (N < 0 || N > a.max_rows || N > TT || M < 0 || M > a.max_frames) {
        if (tid == 0) a.status[b] = SER_TS_BAD_SHAPE;
        return;                                                    // block-uniform
    }
    if (tid == 0 && a.path_len) a.path_len[b] = 0;
    if (N == 0 || M == 0) {
        if (tid == 0) a.status[b] = N == 0 ? 0 : SER_TS_NO_FRAMES;
        return;
    }
    for (int i = tid; i < 3 * (TT + 1); i += TT) (&s_c[0][0])[i] = i == 0 ? 0.f : INFINITY;
    const int i = tid + 1;
    const bool mine = i <= N;
    const float* mrow = a.matrix + ((int64_t)b * a.max_rows + (mine ? tid : 0)) * a.ld_m;
    unsigned long long* bprow = bp + ((int64_t)b * a.max_rows + tid) * W;
    // Row i stands in column c = d - i - 1 at diagonal d.  The diagonals go in blocks of 8: at a block's start every thread takes over the 8
    // matrix entries it loaded one block ago and issues the loads of the block after this one (clamped into the row, so no branch surrounds
    // a load and nothing waits for one before the next block's start: they are in flight across this block's 8 barriers).
    float cur[8], nxt[8];
    auto col = [&](int d) {
        int c = d - i - 1;
        c = c < 0 ? 0 : c;
        return c < M ? c : M - 1;
    };
#pragma unroll
    for (int k = 0; k < 8; ++k) nxt[k] = mrow[col(2 + k)];
    unsigned long long acc = 0;
    __syncthreads();
    for (int d0 = 2; d0 <= N + M; d0 += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) cur[k] = nxt[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) nxt[k] = mrow[col(d0 + 8 + k)];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int d = d0 + k;
            if (d > N + M) break;                                  // block-uniform
            const int j = d - i;
            float* cd = s_c[d % 3];
            const float* p1 = s_c[(d + 2) % 3];
            const float* p2 = s_c[(d + 1) % 3];
            if (mine && j >= 1 && j <= M) {
                const int c = j - 1;
                const float x = -cur[k];
                const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
                float cc;
                unsigned long long t;
                if (c0 < c1 && c0 < c2) { cc = c0; t = 0; }
                else if (c1 < c0 && c1 < c2) { cc = c1; t = 1; }
                else { cc = c2; t = 2; }
                cd[i] = (float)((double)x + (double)cc);
                acc |= t << (2 * (c & 31));
                if ((c & 31) == 31 || j == M) {
                    bprow[c >> 5] = acc;
                    acc = 0;
                }
            }
            if (tid == 0) cd[0] = INFINITY;
            __syncthreads();
        }
    }
    const float fin = s_c[(N + M) % 3][N];
    if (tid == 0) a.status[b] = fabsf(fin) < INFINITY ? 0 : SER_TS_NONFINITE;
    __threadfence_block();
    __syncthreads();                                               // every back-pointer word is visible to the block
    // ---- the backtrack: at most N + M dependent reads, once.  The block stages the band of BAND frames the walk stands in (all N rows);
    // one thread walks it until the walk leaves the band.  Row 0 is forced left, column 0 up.
    int32_t* first = a.first_frame + (int64_t)b * a.ld_t;
    const int64_t pl = (int64_t)a.max_rows + a.max_frames;
    int32_t* ptext = a.path_text ? a.path_text + (int64_t)b * pl : nullptr;
    int32_t* ptime = a.path_time ? a.path_time + (int64_t)b * pl : nullptr;
    __shared__ int s_i, s_j, s_len;
    if (tid == 0) { s_i = N; s_j = M; s_len = 0; }
    __syncthreads();
    const int Wn = (M + 31) / 32;
    while (true) {                                                 // block-uniform: s_i, s_j are read behind a barrier
        const int wi = s_i, wj = s_j;
        if (wi <= 0 && wj <= 0) break;
        const int band = wj > 0 ? (wj - 1) / BAND : 0;
        __syncthreads();                                           // everyone has read s_i, s_j before thread 0 moves them
        for (int k = tid; k < N * BW; k += TT) {
            const int r = k / BW, w = band * BW + k % BW;
            s_bp[k] = w < Wn ? bp[((int64_t)b * a.max_rows + r) * W + w] : 0ull;
        }
        __syncthreads();
        if (tid == 0) {
            int ci = wi, cj = wj, len = s_len;
            while (ci > 0 || cj > 0) {
                if (ci > 0 && cj > 0 && (cj - 1) / BAND != band) break;
                if (ci >= 1) first[ci - 1] = cj - 1;               // the last write is the walk's earliest visit of the row
                if (ptext) ptext[len] = ci - 1;
                if (ptime) ptime[len] = cj - 1;
                ++len;
                int t;
                if (ci == 0) t = 2;
                else if (cj == 0) t = 1;
                else {
                    const int c = cj - 1;
                    t = (int)((s_bp[(ci - 1) * BW + ((c >> 5) % BW)] >> (2 * (c & 31))) & 3ull);
                }
                if (t == 0) { --ci; --cj; }
                else if (t == 1) --ci;
                else --cj;
            }
            s_i = ci; s_j = cj; s_len = len;
            if (a.path_len) a.path_len[b] = len;
        }
        __syncthreads();
    }
}

extern "C" int64_t ser_dtw_work_bytes(int32_t B, int32_t max_rows, int32_t max_frames) {
    if (B < 1 || max_rows < 1 || max_rows > SER_TS_THREADS || max_frames < 1) return -1;
    return 8 * (int64_t)B * max_rows * dtw_words(max_frames);
}

extern "C" int ser_dtw_v(const ser_dtw_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_dtw: null arguments");
    if (!a->matrix || !a->n_rows || !a->n_frames || !a->work || !a->first_frame || !a->status) return ser_fail(-1, "ser_dtw: null pointer");
    if ((a->path_text == nullptr) != (a->path_time == nullptr) || (a->path_text == nullptr) != (a->path_len == nullptr))
        return ser_fail(-1, "ser_dtw: path_text, path_time and path_len come together");
    if (a->B < 1 || a->B > 65535 || a->max_rows < 1 || a->max_rows > SER_TS_THREADS || a->max_frames < 1)
        return ser_fail(-2, "ser_dtw: B=%d (1..65535) max_rows=%d (1..%d) max_frames=%d (at least 1)", a->B, a->max_rows, SER_TS_THREADS, a->max_frames);
    const int64_t need = ser_dtw_work_bytes(a->B, a->max_rows, a->max_frames);
    if (a->work_bytes < need)
        return ser_fail(-2, "ser_dtw: work holds %lld bytes, %lld are needed (ser_dtw_work_bytes)", (long long)a->work_bytes, (long long)need);
    if (a->ld_m < a->max_frames || a->ld_t < a->max_rows)
        return ser_fail(-3, "ser_dtw: bad pitches ld_m=%lld (>= max_frames) ld_t=%lld (>= max_rows)", (long long)a->ld_m, (long long)a->ld_t);
    if ((((uintptr_t)a->matrix) & 3) != 0 || (((uintptr_t)a->work) & 7) != 0) return ser_fail(-3, "ser_dtw: matrix must be 4-byte aligned, work 8-byte aligned");
    hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)a->B), dim3(TT), 0, (hipStream_t)stream, *a, (unsigned long long*)a->work, dtw_words(a->max_frames));
    return ser_check_launch("ser_dtw_v");
}
