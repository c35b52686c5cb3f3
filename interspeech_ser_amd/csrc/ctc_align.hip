// CTC forced alignment of a packed ragged batch (include/ser_hip.h, "a32"): ser_ctc_align_v, two kernels behind one entry point.
//   ctc_lse_kernel    a grid over all rows: lse64[t], the float64 log-sum-exp of the row's V columns (the lane-group pattern of ctc.hip)
//   ctc_align_kernel  one block per utterance: the Viterbi trellis over its frames (float64 alpha, two rows in LDS, one barrier per
//                     frame, two back-pointer bits per cell packed by wave ballots), one backtrack, then parallel passes over the frames
//                     and the tokens for pos / frame_score / starts / ends / tok_score
// No atomics on data; the only floating-point sums are the lse's (a fixed lane split and shuffle order, functions of V alone) and a
// token's mean (one thread, frame order): every output of an utterance is a pure function of its own logits and target.
#include "ser_common.h"
#include <math.h>

constexpr int AT = SER_CTC_ALIGN_THREADS;                  // threads of an alignment block
constexpr int NS = (2 * SER_CTC_ALIGN_MAX_TOKENS + 1 + AT - 1) / AT;   // states per thread: state s = tid + k AT, k < NS
constexpr int SMAX = NS * AT;                              // >= 2 MAX_TOKENS + 1
static_assert(AT % 64 == 0 && SMAX % 64 == 0, "a wave's ballot packs 64 consecutive states");

static inline int64_t align_bp_words(int max_tokens) { return 2 * (((int64_t)2 * max_tokens + 1 + 63) / 64); }   // uint64 words per frame

// ---------------------------------------------------------------------------------------------------------------- lse64
// G lanes of a wave take one row (ctc_argmax_kernel's split): the row's max, then sum exp(x - max) in float64, lane l adding columns
// l, l + G, ... in order and the lanes meeting by xor shuffles (a + b is commutative, so both partners hold the same bits).  The order is
// a function of V alone.  Columns >= V are never read.
template <int G>
__global__ __launch_bounds__(256) void ctc_lse_kernel(const float* __restrict__ z, int64_t ldz, double* __restrict__ lse, int rows, int V) {
    const int l = threadIdx.x & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + (threadIdx.x / G);
    const bool live = row < rows;                                             // uniform over a group; dead groups still shuffle
    const float* zr = z + (live ? row : 0) * ldz;
    float m = -INFINITY;
    if (live)
        for (int c = l; c < V; c += G) m = fmaxf(m, zr[c]);                   // fmaxf drops a NaN; the sum below keeps it
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    double s = 0.0;
    if (live)
        for (int c = l; c < V; c += G) s += exp((double)zr[c] - (double)m);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (!live || l != 0) return;
    lse[row] = (double)m + log(s);                                            // NaN for a row with a NaN or +inf, or all -inf
}

// ---------------------------------------------------------------------------------------------------------------- trellis
// s_alpha[p][2 + s] is alpha[.][s] of one frame; entries 0 and 1 stay -inf, so s - 1 and s - 2 need no branch at s = 0, 1.  The row
// "before frame 0" is -0.0 at state 0 and -inf elsewhere: -0.0 + e == e for every e (signed zeros included), so frame 0 comes out as the
// rule's initial row through the same three reads as every other frame.
__global__ __launch_bounds__(AT) void ctc_align_kernel(const float* __restrict__ z, int64_t ldz, const int32_t* __restrict__ frame_offs,
                                                       const int32_t* __restrict__ targets, const int32_t* __restrict__ tgt_offs,
                                                       const double* __restrict__ lse, int32_t* __restrict__ path, float* __restrict__ fsc,
                                                       unsigned long long* __restrict__ bp, int64_t bp_words, int32_t* __restrict__ starts,
                                                       int32_t* __restrict__ ends, float* __restrict__ tok_score, int64_t ld_tok,
                                                       int32_t* __restrict__ status, double* __restrict__ path_logit, int32_t* __restrict__ pos,
                                                       float* __restrict__ frame_score, int rows, int V, int blank, int max_frames,
                                                       int max_tokens, int n_targets) {
    __shared__ double s_alpha[2][2 + SMAX];
    __shared__ int s_end;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    const int g0 = tgt_offs[b], g1 = tgt_offs[b + 1];
    const int T = r1 - r0, L = g1 - g0;
    // ---- what is refused per utterance: every check comes before the index it guards
    if (r0 < 0 || r1 > rows || T < 0 || T > max_frames || g0 < 0 || g1 > n_targets || L < 0 || L > max_tokens || L > SER_CTC_ALIGN_MAX_TOKENS) {
        if (tid == 0) status[b] = SER_CTC_ALIGN_BAD_TARGET;
        return;                                                               // block-uniform
    }
    const int32_t* y = targets + g0;
    const int S = 2 * L + 1;
    int lab[NS];
    bool skip[NS];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = tid + k * AT;
        lab[k] = blank;
        skip[k] = false;
        if (s < S && (s & 1)) {
            const int v = y[s >> 1];
            bad |= (v < 0 || v >= V || v == blank);
            lab[k] = v;
            skip[k] = s >= 3 && v != y[(s >> 1) - 1];
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) status[b] = SER_CTC_ALIGN_BAD_TARGET;
        return;
    }
    int rep = 0;
    for (int j0 = 0; j0 < L; j0 += AT) {                                      // block-uniform
        const int j = j0 + tid;
        rep += __syncthreads_count(j > 0 && j < L && y[j] == y[j - 1]);
    }
    if (T < 1 || T < L + rep) {
        if (tid == 0) status[b] = SER_CTC_ALIGN_INFEASIBLE;
        return;
    }
    // ---- the trellis
    for (int i = tid; i < 2 + SMAX; i += AT) {
        s_alpha[0][i] = -INFINITY;
        s_alpha[1][i] = i == 2 ? -0.0 : -INFINITY;                            // the row before frame 0
    }
    const float* zr = z + (int64_t)r0 * ldz;
    unsigned long long* bpb = bp + (int64_t)b * max_frames * bp_words;
    const int Wb = 2 * ((S + 63) / 64);                                       // this utterance's words per frame (<= bp_words)
    // A thread's labels are fixed for the utterance (a state that does not exist reads the blank column: a legal address, the value is
    // unused).  The loads of frame t + 1 are issued once frame t's values have been converted, with no branch around them, and nothing
    // between there and the barrier waits for them: they are in flight across frame t's LDS reads, its writes and its barrier.
    float e[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) e[k] = zr[lab[k]];
    __syncthreads();
    for (int t = 0; t < T; ++t) {
        const double* prev = s_alpha[(t + 1) & 1];
        double* cur = s_alpha[t & 1];
        double ed[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            bad |= !(e[k] < INFINITY);                                        // a NaN or +inf in a read column
            ed[k] = (double)e[k];
            asm volatile("" : "+v"(ed[k]));                                   // converted HERE, ahead of the next frame's loads
        }
        asm volatile("" ::: "memory");
        const float* zn = zr + (int64_t)(t + 1 < T ? t + 1 : t) * ldz;
#pragma unroll
        for (int k = 0; k < NS; ++k) e[k] = zn[lab[k]];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = tid + k * AT;
            if ((s & ~63) >= S) continue;                                     // wave-uniform: none of the wave's 64 states exists
            int mv = 0;
            if (s < S) {
                double best = prev[2 + s];
                const double a1 = prev[1 + s];
                const double a2 = skip[k] ? prev[s] : -INFINITY;
                if (a1 > best) { best = a1; mv = 1; }                         // strictly greater: the smaller jump wins a tie
                if (a2 > best) { best = a2; mv = 2; }
                cur[2 + s] = best + ed[k];
            }
            const unsigned long long b0 = __ballot(mv & 1), b1 = __ballot(mv & 2);
            if (lane == 0) {
                unsigned long long* w = bpb + (int64_t)t * Wb + 2 * (s >> 6);
                w[0] = b0;
                w[1] = b1;
            }
        }
        __syncthreads();
    }
    const double* fin = s_alpha[(T - 1) & 1];
    if (tid == 0) {
        int end = S - 1;
        if (L > 0 && !(fin[2 + S - 1] > fin[2 + S - 2])) end = S - 2;
        const double score = fin[2 + end];
        path_logit[b] = score;
        s_end = end;
        bad |= !(fabs(score) < (double)INFINITY);
    }
    if (__syncthreads_or(bad)) {                                              // (also: s_end and every back-pointer word are visible)
        if (tid == 0) status[b] = SER_CTC_ALIGN_NONFINITE;
        return;
    }
    // ---- the backtrack: T dependent reads, once per utterance.  The block copies the back pointers of a chunk of frames into the LDS
    // the alpha rows no longer need, then one thread walks the chunk from its last frame to its first.
    unsigned long long* s_bp = (unsigned long long*)&s_alpha[0][0];
    const int FC = (2 * (2 + SMAX)) / Wb;                                     // frames per chunk (>= 64)
    int32_t* pth = path + r0;
    int st = s_end;
    for (int hi = T - 1; hi >= 1; hi -= FC) {                                 // block-uniform
        const int lo = hi - FC + 1 < 1 ? 1 : hi - FC + 1;
        const int n = (hi - lo + 1) * Wb;
        const unsigned long long* src = bpb + (int64_t)lo * Wb;
        for (int i = tid; i < n; i += AT) s_bp[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            for (int t = hi; t >= lo; --t) {
                pth[t] = st;
                const unsigned long long* w = s_bp + (t - lo) * Wb + 2 * (st >> 6);
                int mv = (int)((w[0] >> (st & 63)) & 1ull) | ((int)((w[1] >> (st & 63)) & 1ull) << 1);
                mv = mv > st ? st : mv;                                       // (never on a finite path: the state stays >= 0)
                st -= mv;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        pth[0] = st;
        status[b] = 0;
    }
    __syncthreads();                                                          // the path is visible to the block
    // ---- per frame: pos, frame_score, and the first / one-past-last frame of every token
    int32_t* stb = starts + (int64_t)b * ld_tok;
    int32_t* enb = ends + (int64_t)b * ld_tok;
    float* fs = fsc + r0;
    for (int t = tid; t < T; t += AT) {
        const int s = pth[t];
        const int j = (s & 1) ? (s >> 1) : -1;
        const int c = j >= 0 ? y[j] : blank;
        const float v = (float)((double)zr[(int64_t)t * ldz + c] - lse[r0 + t]);
        fs[t] = v;
        if (pos) pos[r0 + t] = j;
        if (frame_score) frame_score[r0 + t] = v;
        if (j >= 0) {
            if (t == 0 || pth[t - 1] != s) stb[j] = t;
            if (t == T - 1 || pth[t + 1] != s) enb[j] = t + 1;
        }
    }
    __syncthreads();
    // ---- per token: the float64 mean of its frames' scores, summed in frame order
    float* tsb = tok_score + (int64_t)b * ld_tok;
    for (int j = tid; j < L; j += AT) {
        const int t0 = stb[j], t1 = enb[j];
        double sum = 0.0;
        for (int t = t0; t < t1; ++t) sum += (double)fs[t];
        tsb[j] = (float)(sum / (double)(t1 - t0));
    }
}

extern "C" int64_t ser_ctc_align_work_bytes(int32_t rows, int32_t B, int32_t max_frames, int32_t max_tokens) {
    if (rows < 1 || B < 1 || max_frames < 1 || max_tokens < 0 || max_tokens > SER_CTC_ALIGN_MAX_TOKENS) return -1;
    return 16 * (int64_t)rows + 8 * (int64_t)B * max_frames * align_bp_words(max_tokens);
}

extern "C" int ser_ctc_align_v(const ser_ctc_align_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_ctc_align: null arguments");
    if (!a->z || !a->frame_offs || !a->targets || !a->tgt_offs || !a->work || !a->starts || !a->ends || !a->tok_score || !a->status || !a->path_logit)
        return ser_fail(-1, "ser_ctc_align: null pointer");
    if (a->B < 1 || a->B > 65535 || a->V < 1 || a->rows < 1 || a->max_frames < 1 || a->n_targets < 0)
        return ser_fail(-2, "ser_ctc_align: B=%d (1..65535) V=%d rows=%d max_frames=%d (at least 1 each) n_targets=%d", a->B, a->V, a->rows,
                        a->max_frames, a->n_targets);
    if (a->max_tokens < 0 || a->max_tokens > SER_CTC_ALIGN_MAX_TOKENS)
        return ser_fail(-2, "ser_ctc_align: max_tokens=%d outside [0, %d]", a->max_tokens, SER_CTC_ALIGN_MAX_TOKENS);
    if (a->blank < 0 || a->blank >= a->V) return ser_fail(-2, "ser_ctc_align: blank=%d outside [0, V=%d)", a->blank, a->V);
    const int64_t need = ser_ctc_align_work_bytes(a->rows, a->B, a->max_frames, a->max_tokens);
    if (a->work_bytes < need)
        return ser_fail(-2, "ser_ctc_align: work holds %lld bytes, %lld are needed (ser_ctc_align_work_bytes)", (long long)a->work_bytes, (long long)need);
    if (a->ldz < a->V || a->ld_tok < a->max_tokens)
        return ser_fail(-3, "ser_ctc_align: bad pitches ldz=%lld (>= V) ld_tok=%lld (>= max_tokens)", (long long)a->ldz, (long long)a->ld_tok);
    if ((((uintptr_t)a->z) & 3) != 0 || (((uintptr_t)a->work) & 7) != 0 || (((uintptr_t)a->path_logit) & 7) != 0)
        return ser_fail(-3, "ser_ctc_align: z must be 4-byte aligned, work and path_logit 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* lse = (double*)a->work;                                           // [rows] float64 | [rows] path states | [rows] frame scores | back pointers
    int32_t* path = (int32_t*)(lse + a->rows);
    float* fsc = (float*)(path + a->rows);
    unsigned long long* bp = (unsigned long long*)((char*)a->work + 16 * (int64_t)a->rows);
    const int G = a->V <= 32 ? 8 : (a->V <= 64 ? 16 : (a->V <= 128 ? 32 : 64));
    const int64_t blocks = ((int64_t)a->rows + (256 / G) - 1) / (256 / G);
#define CTC_LSE(GG) hipLaunchKernelGGL(ctc_lse_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, a->z, a->ldz, lse, a->rows, a->V)
    if (G == 8) CTC_LSE(8);
    else if (G == 16) CTC_LSE(16);
    else if (G == 32) CTC_LSE(32);
    else CTC_LSE(64);
#undef CTC_LSE
    hipLaunchKernelGGL(ctc_align_kernel, dim3((unsigned)a->B), dim3(AT), 0, st, a->z, a->ldz, a->frame_offs, a->targets, a->tgt_offs, lse, path, fsc,
                       bp, align_bp_words(a->max_tokens), a->starts, a->ends, a->tok_score, a->ld_tok, a->status, a->path_logit, a->pos,
                       a->frame_score, a->rows, a->V, a->blank, a->max_frames, a->max_tokens, a->n_targets);
    return ser_check_launch("ser_ctc_align_v");
}
