// Whisper segment timestamps (include/ser_hip.h, "a36"): ser_dec_select_ts_v, the greedy select of a decode step with the timestamp rule of
// HF's WhisperTimeStampLogitsProcessor between the static mask and the argmax.  One block per row.  A column's masked value is a function
// of (its logit, its mask entry, five row-uniform bounds), so the row is never stored: pass 1 reduces the text and the timestamp columns to
// one Top2 triple each, pass 2 sums exp(x - max) over the live timestamp columns in float64 (at most V - ts_begin of them: 1 501 of 51 866),
// and thread 0 decides.  Every reduction is a fixed tree over (thread, wave) slots that depend on V and ts_begin alone, and a block reads
// nothing of another row: a row alone and in a batch give the same bits.  The bookkeeping behind the choice is ser_dec_select_v's.
#include "ser_common.h"
#include "top2_common.h"
#include <math.h>

#define SEG_THREADS 512
#define SEG_WAVES (SEG_THREADS / 64)

__device__ __forceinline__ Top2 seg_wave_top2(Top2 t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 y;
        y.v1 = __shfl_xor(t.v1, o, 64); y.i1 = __shfl_xor(t.i1, o, 64); y.v2 = __shfl_xor(t.v2, o, 64);
        t = top2_merge(t, y);
    }
    return t;
}

__device__ __forceinline__ void seg_take(Top2& t, float x, int v) {
    if (x > t.v1 || (x == t.v1 && v < t.i1)) { t.v2 = t.v1; t.v1 = x; t.i1 = v; }
    else t.v2 = fmaxf(t.v2, x);
}

__global__ __launch_bounds__(SEG_THREADS) void dec_select_ts_kernel(ser_dec_select_ts_args A) {
    const ser_dec_select_args& a = A.base;
    __shared__ Top2 part_text[SEG_WAVES], part_ts[SEG_WAVES];
    __shared__ double part_sum[SEG_WAVES];
    __shared__ int part_last[SEG_WAVES], part_nan[SEG_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int p = *a.pos;
    const bool pos_ok = p >= 0 && p + 1 < a.max_pos;
    const int pc = pos_ok ? p : 0;
    const int forced = a.forced[pc], phase = a.phase[pc];
    const int fin = a.finished[b];
    const bool scan = pos_ok && !fin && forced < 0;                           // block-uniform, as everything derived from it
    const int n = pc + 1 - A.begin_index;                                     // generated tokens of the row; < 0: a prompt step, no rule
    const bool rule = n >= 0;
    const int V = a.V, tsb = A.ts_begin;
    const Top2 none = {-INFINITY, 0x7fffffff, -INFINITY};
    Top2 text = none, ts = none;
    double L = -INFINITY;
    int nan_seen = 0;
    if (scan) {
        const int32_t* row = a.ids + (int64_t)b * a.ld_ids;
        // the live columns: v >= lo_all, v != no_ts, and text v >= lo_text or timestamp ts_lo <= v < ts_hi
        int lo_all = 0, lo_text = 0, ts_lo = tsb, ts_hi = V, no_ts = -1;
        if (rule) {
            no_ts = A.no_ts;
            const bool last_ts = n >= 1 && row[p] >= tsb;
            const bool pen_ts = n < 2 || row[p - 1] >= tsb;
            if (last_ts && pen_ts) ts_lo = V;                                 // a closed pair: text has to follow
            if (last_ts && !pen_ts) lo_all = a.eos;                           // an opening timestamp or eos has to follow
            int last = -1;                                                    // the position of the row's last timestamp token
            for (int j = A.begin_index + tid; j <= p; j += SEG_THREADS) last = row[j] >= tsb ? j : last;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
            if ((tid & 63) == 0) part_last[wave] = last;
            __syncthreads();
            last = part_last[0];
#pragma unroll
            for (int w = 1; w < SEG_WAVES; ++w) last = max(last, part_last[w]);
            if (last >= 0) {
                const int t = row[last];
                const int64_t bound = (last_ts && !pen_ts) ? (int64_t)t : (int64_t)t + 1;
                if (bound > ts_lo) ts_lo = bound > V ? V : (int)bound;
            }
            if (n == 0) {
                lo_text = tsb;
                if (A.max_initial >= 0 && (int64_t)tsb + A.max_initial + 1 < V) ts_hi = tsb + A.max_initial + 1;
            }
        }
        const float* z = a.logits + (int64_t)b * a.ldl;
        const float* mk = a.mask + (int64_t)(phase < 0 ? 0 : (phase > 2 ? 2 : phase)) * a.ldm;
        auto masked = [&](int v) -> float {                                   // columns >= V (the padded vocabulary) are never read
            float x = z[v] + mk[v];
            if (x != x) { nan_seen = 1; x = INFINITY; }                       // a NaN wins where it is live, and fails the batch wherever it is
            const bool live = v >= lo_all && v != no_ts && (v < tsb ? v >= lo_text : (v >= ts_lo && v < ts_hi));
            return live ? x : -INFINITY;
        };
        const int text_end = rule ? tsb : V;                                  // a prompt step has text columns only
#pragma unroll 4
        for (int v = tid; v < text_end; v += SEG_THREADS) seg_take(text, masked(v), v);
        for (int v = text_end + tid; v < V; v += SEG_THREADS) seg_take(ts, masked(v), v);
        text = seg_wave_top2(text);
        ts = seg_wave_top2(ts);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nan_seen |= __shfl_xor(nan_seen, o, 64);
        if ((tid & 63) == 0) { part_text[wave] = text; part_ts[wave] = ts; part_nan[wave] = nan_seen; }
        __syncthreads();
        text = part_text[0]; ts = part_ts[0]; nan_seen = part_nan[0];
#pragma unroll
        for (int w = 1; w < SEG_WAVES; ++w) { text = top2_merge(text, part_text[w]); ts = top2_merge(ts, part_ts[w]); nan_seen |= part_nan[w]; }
        if (rule) {
            // L = log sum_{v >= ts_begin} exp(x[v]) = m + log sum exp(x[v] - m), m the largest timestamp value; a masked column adds exp(-inf) = 0
            const double m = (double)ts.v1;
            double s = 0.0;
            if (fabs(m) <= 3.0e38) {
                for (int v = tsb + tid; v < V; v += SEG_THREADS) s += exp((double)masked(v) - m);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if ((tid & 63) == 0) part_sum[wave] = s;
            __syncthreads();
            if (tid == 0) {
                s = part_sum[0];
#pragma unroll
                for (int w = 1; w < SEG_WAVES; ++w) s += part_sum[w];
                L = fabs(m) <= 3.0e38 ? m + log(s) : m;                       // all masked: -inf; a +inf or NaN column: +inf, and the batch fails
            }
        }
    }
    __syncthreads();                                                          // every thread has read *pos before thread 0 takes the ticket
    if (tid != 0) return;
    uint32_t err = pos_ok ? 0u : 4u;                                          // bit 2: the position left the ids buffer
    int tok = a.pad;
    float margin = INFINITY;                                                  // nothing was decided: forced, finished
    double gap = INFINITY;
    if (scan) {
        Top2 t = text;
        if (rule) {
            const double M = (double)text.v1;
            if (L > M) t = ts;                                                // the timestamps together outweigh the best text token
            else t = top2_merge(text, ts);                                    // L == M keeps the text columns
            if (fabs(L) <= 3.0e38 && fabs(M) <= 3.0e38) gap = fabs(L - M);
        }
        tok = t.i1 < V ? t.i1 : a.pad;
        margin = t.v1 - t.v2;
        if (!(fabsf(t.v1) <= 3.0e38f) || nan_seen) err |= 1u;                 // bit 0: the winner is not finite, or the row holds a NaN
    } else if (!fin && forced >= 0) {
        tok = forced;
    }
    int fin_after = fin;
    if (pos_ok) {
        a.ids[(int64_t)b * a.ld_ids + p + 1] = tok;
        a.margin[(int64_t)b * a.ld_margin + p] = margin;
        A.ts_gap[(int64_t)b * A.ld_gap + p] = gap;
        if (!fin && tok == a.eos) { a.finished[b] = 1; fin_after = 1; }
    }
    if (err) atomicOr(a.err, err);
    // ser_dec_select_v's tickets: the block that takes the last one publishes the count of unfinished rows and advances the position;
    // every other block has read *pos (and its id row) before it took its own
    atomicAdd(&a.work[1], fin_after ? 0 : 1);
    __threadfence();
    if (atomicAdd(&a.work[0], 1) == a.B - 1) {
        *a.unfinished = atomicExch(&a.work[1], 0);
        atomicExch(&a.work[0], 0);
        if (pos_ok) *a.pos = p + 1;
    }
}

extern "C" int ser_dec_select_ts_v(const ser_dec_select_ts_args* A, void* stream) {
    if (!A) return ser_fail(-1, "ser_dec_select_ts: null arguments");
    const ser_dec_select_args* a = &A->base;
    if (!a->logits || !a->mask || !a->phase || !a->forced || !a->ids || !a->finished || !a->margin || !A->ts_gap || !a->pos || !a->unfinished ||
        !a->work || !a->err)
        return ser_fail(-1, "ser_dec_select_ts: null pointer");
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_dec_select_ts: B=%d (1..65535)", a->B);
    if (a->V <= 1 || a->ldl < a->V || a->ldm < a->V) return ser_fail(-3, "ser_dec_select_ts: V=%d, ldl=%lld, ldm=%lld (V >= 2, pitches >= V)", a->V, (long long)a->ldl, (long long)a->ldm);
    if (a->max_pos < 2 || a->ld_ids < a->max_pos || a->ld_margin < a->max_pos - 1 || A->ld_gap < a->max_pos - 1)
        return ser_fail(-4, "ser_dec_select_ts: max_pos=%d, ld_ids=%lld, ld_margin=%lld, ld_gap=%lld", a->max_pos, (long long)a->ld_ids,
                        (long long)a->ld_margin, (long long)A->ld_gap);
    if (A->ts_begin < 1 || A->ts_begin >= a->V || A->no_ts < 0 || A->no_ts >= a->V || a->eos < 0 || a->eos >= a->V)
        return ser_fail(-5, "ser_dec_select_ts: ts_begin=%d, no_ts=%d, eos=%d (0 < ts_begin < V=%d; no_ts and eos inside the vocabulary)",
                        A->ts_begin, A->no_ts, a->eos, a->V);
    if (A->begin_index < 1 || A->begin_index >= a->max_pos || A->max_initial < -1)
        return ser_fail(-6, "ser_dec_select_ts: begin_index=%d (1..max_pos - 1), max_initial=%d (>= -1)", A->begin_index, A->max_initial);
    hipLaunchKernelGGL(dec_select_ts_kernel, dim3(a->B), dim3(SEG_THREADS), 0, (hipStream_t)stream, *A);
    return ser_check_launch("ser_dec_select_ts_v");
}
