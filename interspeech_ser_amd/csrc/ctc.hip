// Greedy CTC decoding of a packed ragged batch (include/ser_hip.h, "a31"): ser_ctc_greedy_v, two kernels behind one entry point.
//   ctc_argmax_kernel    a grid over all rows: per frame the winning column, its margin over the runner-up, the error bit
//   ctc_collapse_kernel  one block per utterance: blanks and repeats dropped, the kept tokens with their runs' first and one-past-last frame
// No atomics on data (the error word's rare OR is the only one), no floating-point sum at all: every output is a pure function of the
// utterance's own logits, so it is bit-identical at any batch composition.
#include "ser_common.h"
#include "top2_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------------- argmax
// G lanes of a wave take one frame (G = 8, 16, 32 or 64, the smallest with 4 G >= V, so V = 32 is one 16-byte load per lane and eight
// frames per wave); a block of 256 threads takes 256 / G consecutive frames.  Lane l reads columns 4 l .. 4 l + 3, then 4 (l + G) ..: a
// quad that ends inside V is one 16-byte load, the quad that straddles V is read column by column, columns >= V are never read.  The
// lanes' (v1, i1, v2) triples meet by xor shuffles inside the group.  top2_merge is associative and commutative (top2_common.h), so
// neither G nor the order of the shuffles can change a result.
template <int G>
__global__ __launch_bounds__(256) void ctc_argmax_kernel(const float* __restrict__ z, int64_t ldz, int32_t* __restrict__ tok,
                                                         float* __restrict__ margin, int32_t* __restrict__ frame_ids,
                                                         float* __restrict__ frame_margin, uint32_t* __restrict__ err, int rows, int V) {
    const int l = threadIdx.x & (G - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / G) + (threadIdx.x / G);
    const bool live = row < rows;                                             // uniform over a group; dead groups still shuffle
    Top2 t = {-INFINITY, 0x7fffffff, -INFINITY};
    if (live) {
        const float* zr = z + row * ldz;
        auto take = [&](float x, int v) {
            x = (x != x) ? INFINITY : x;                                      // a NaN wins, and a non-finite winner sets the error bit
            if (x > t.v1 || (x == t.v1 && v < t.i1)) { t.v2 = t.v1; t.v1 = x; t.i1 = v; }
            else t.v2 = fmaxf(t.v2, x);
        };
        for (int c = l * 4; c < V; c += G * 4) {
            if (c + 4 <= V) {
                const f32x4 q = *(const f32x4*)(zr + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) take(q[j], c + j);
            } else {
                for (int v = c; v < V; ++v) take(zr[v], v);
            }
        }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        Top2 y;
        y.v1 = __shfl_xor(t.v1, o, 64); y.i1 = __shfl_xor(t.i1, o, 64); y.v2 = __shfl_xor(t.v2, o, 64);
        t = top2_merge(t, y);
    }
    if (!live || l != 0) return;
    const float m = t.v1 - t.v2;                                              // one fp32 subtraction; +inf when V == 1 (v2 = -inf)
    tok[row] = t.i1;
    margin[row] = m;
    if (frame_ids) frame_ids[row] = t.i1;
    if (frame_margin) frame_margin[row] = m;
    if (!(fabsf(t.v1) <= 3.0e38f)) atomicOr(err, (uint32_t)SER_CTC_ERR_NONFINITE);
}

// ---------------------------------------------------------------------------------------------------------------- collapse
// One block of SER_CTC_CHUNK threads per utterance, a thread per frame of the chunk.  s_tok[0] is the last token of the previous chunk
// (-1 ahead of the utterance's first frame: no token equals it), s_tok[1 .. CHUNK] the chunk's, s_tok[CHUNK + 1] the first of the next
// chunk (-1 past the utterance's end).  Frame t is KEPT when it opens a non-blank run and is a run's LAST when it closes one; both are
// numbered by the exclusive scan of the keep flags -- ballot and popcount inside a wave, the four wave totals through LDS -- plus the
// count the earlier chunks carried.  A run has exactly one opening and one closing frame, so the closing frame of run j is the one whose
// inclusive count is j + 1, in whichever chunk it falls: a run that straddles a chunk boundary needs nothing but the carried count.
__global__ __launch_bounds__(SER_CTC_CHUNK) void ctc_collapse_kernel(const int32_t* __restrict__ tok, const float* __restrict__ margin,
                                                                     const int32_t* __restrict__ frame_offs, int32_t* __restrict__ ids,
                                                                     int32_t* __restrict__ starts, int32_t* __restrict__ ends, int64_t ld_tok,
                                                                     int32_t* __restrict__ counts, float* __restrict__ min_margin, int rows,
                                                                     int blank, int max_frames) {
    constexpr int C = SER_CTC_CHUNK, W = SER_CTC_CHUNK / 64;
    __shared__ int32_t s_tok[C + 2];
    __shared__ int32_t s_cnt[W];
    __shared__ float s_min[W];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int r0 = frame_offs[b], r1 = frame_offs[b + 1];
    if (r0 < 0) r0 = 0;                                                       // never read outside [0, rows) nor write past max_frames
    if (r1 > rows) r1 = rows;
    int T = r1 - r0;
    T = T < 0 ? 0 : (T > max_frames ? max_frames : T);
    const int32_t* tk = tok + r0;
    int32_t* idb = ids + (int64_t)b * ld_tok;
    int32_t* stb = starts + (int64_t)b * ld_tok;
    int32_t* enb = ends + (int64_t)b * ld_tok;
    int base = 0;                                                             // tokens kept by the earlier chunks
    int prev_last = -1;                                                       // the last token of the previous chunk
    float mn = INFINITY;
    for (int t0 = 0; t0 < T; t0 += C) {                                       // block-uniform
        const int t = t0 + tid;
        const bool valid = t < T;
        const int mine = valid ? tk[t] : -1;
        s_tok[tid + 1] = mine;
        if (tid == 0) {
            s_tok[0] = prev_last;
            s_tok[C + 1] = (t0 + C < T) ? tk[t0 + C] : -1;
        }
        if (valid && min_margin) mn = fminf(mn, margin[r0 + t]);
        __syncthreads();
        const int before = s_tok[tid], after = s_tok[tid + 2];
        const bool real = valid && mine != blank;
        const bool keep = real && mine != before;
        const bool last = real && mine != after;
        const unsigned long long bal = __ballot(keep);
        const int in_wave = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int ahead = base, total = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int c = s_cnt[w];
            ahead += w < wave ? c : 0;
            total += c;
        }
        const int j = ahead + in_wave;                                        // kept tokens ahead of this frame, in the whole utterance
        if (keep) { idb[j] = mine; stb[j] = t; }
        if (last) enb[j + (keep ? 1 : 0) - 1] = t + 1;                        // (a run's last frame follows its opening: the index is >= 0)
        base += total;
        prev_last = s_tok[C];                                                 // a full chunk's last token; unused after a partial one
        __syncthreads();                                                      // before the next chunk overwrites s_tok / s_cnt
    }
    if (min_margin) {                                                         // min is exact, associative and commutative: order-free
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
        if (lane == 0) s_min[wave] = mn;
        __syncthreads();
        if (tid == 0) {
            float m = s_min[0];
#pragma unroll
            for (int w = 1; w < W; ++w) m = fminf(m, s_min[w]);
            min_margin[b] = m;
        }
    }
    if (tid == 0) counts[b] = base;
}

extern "C" int ser_ctc_greedy_v(const ser_ctc_greedy_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_ctc_greedy: null arguments");
    if (!a->z || !a->frame_offs || !a->work || !a->ids || !a->starts || !a->ends || !a->counts || !a->err)
        return ser_fail(-1, "ser_ctc_greedy: null pointer");
    if (a->B < 1 || a->B > 65535 || a->V < 1 || a->rows < 1 || a->max_frames < 1)
        return ser_fail(-2, "ser_ctc_greedy: B=%d (1..65535) V=%d rows=%d max_frames=%d (at least 1 each)", a->B, a->V, a->rows, a->max_frames);
    if (a->work_elems < 2 * (int64_t)a->rows) return ser_fail(-2, "ser_ctc_greedy: work holds %lld words, 2 * rows = %lld are needed", (long long)a->work_elems, 2 * (long long)a->rows);
    if (a->blank < 0 || a->blank >= a->V) return ser_fail(-2, "ser_ctc_greedy: blank=%d outside [0, V=%d)", a->blank, a->V);
    if (a->ldz < a->V || (a->ldz % 4) || a->ld_tok < a->max_frames)
        return ser_fail(-3, "ser_ctc_greedy: bad pitches ldz=%lld (>= V, multiple of 4) ld_tok=%lld (>= max_frames)", (long long)a->ldz,
                        (long long)a->ld_tok);
    if ((((uintptr_t)a->z) & 15) != 0 || (((uintptr_t)a->work) & 3) != 0) return ser_fail(-3, "ser_ctc_greedy: z must be 16-byte aligned, work 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int32_t* tok = a->work;
    float* margin = (float*)(a->work + a->rows);
    const int G = a->V <= 32 ? 8 : (a->V <= 64 ? 16 : (a->V <= 128 ? 32 : 64));
    const int64_t blocks = ((int64_t)a->rows + (256 / G) - 1) / (256 / G);
#define CTC_ARGMAX(GG)                                                                                                                      \
    hipLaunchKernelGGL(ctc_argmax_kernel<GG>, dim3((unsigned)blocks), dim3(256), 0, st, a->z, a->ldz, tok, margin, a->frame_ids, a->frame_margin, \
                       a->err, a->rows, a->V)
    if (G == 8) CTC_ARGMAX(8);
    else if (G == 16) CTC_ARGMAX(16);
    else if (G == 32) CTC_ARGMAX(32);
    else CTC_ARGMAX(64);
#undef CTC_ARGMAX
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)a->B), dim3(SER_CTC_CHUNK), 0, st, tok, margin, a->frame_offs, a->ids, a->starts, a->ends,
                       a->ld_tok, a->counts, a->min_margin, a->rows, a->blank, a->max_frames);
    return ser_check_launch("ser_ctc_greedy_v");
}
