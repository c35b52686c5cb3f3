// Whisper transcript scores (include/ser_hip.h, "a38"): ser_dec_select_score_v, the two greedy selects of a decode step in a form that also
// scores what it chooses.  rule == 0: ser_dec_select_v's choice; rule != 0: ser_dec_select_ts_v's.  One block of 512 threads per row, and
// the row is never stored: pass 1 reduces the text and the timestamp columns to one Top2 triple each (the unscored kernels' pass), pass 2
// sums exp(x - max) in float64 over the text columns around the best text value and over the timestamp columns around the best timestamp
// value -- the second sum is ser_dec_select_ts_v's, statement for statement, so ts_gap comes out with its bits -- and thread 0 joins the two
// around the winner: logprob = (x[tok] - max x) - log sum exp(x - max x), whose first term is 0 for an argmax.  The step at position 0
// also reads the RAW row (no mask, no rule) for the no-speech probability: two passes of its own, once per run.  Every reduction is a fixed
// tree over (thread, wave) slots that depend on V and ts_begin alone, and a block reads nothing of another row: a row alone and in a batch
// give the same bits.  Top2's merge is associative, so token and margin are those of the 256-thread ser_dec_select_v.
#include "ser_common.h"
#include "top2_common.h"
#include <math.h>

#define SC_THREADS 512
#define SC_WAVES (SC_THREADS / 64)

__device__ __forceinline__ Top2 sc_wave_top2(Top2 t) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 y;
        y.v1 = __shfl_xor(t.v1, o, 64); y.i1 = __shfl_xor(t.i1, o, 64); y.v2 = __shfl_xor(t.v2, o, 64);
        t = top2_merge(t, y);
    }
    return t;
}

__device__ __forceinline__ void sc_take(Top2& t, float x, int v) {
    if (x > t.v1 || (x == t.v1 && v < t.i1)) { t.v2 = t.v1; t.v1 = x; t.i1 = v; }
    else t.v2 = fmaxf(t.v2, x);
}

// the sum of a block's per-thread values over the fixed tree: xor shuffles inside a wave, then the waves' slots in ascending order.
// Valid on thread 0; `part` is one array per call site (no barrier guards its reuse).
__device__ __forceinline__ double sc_block_sum(double s, double* part, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    s = part[0];
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(SC_THREADS) void dec_select_score_kernel(ser_dec_select_score_args S) {
    const ser_dec_select_ts_args& A = S.ts;
    const ser_dec_select_args& a = A.base;
    __shared__ Top2 part_text[SC_WAVES], part_ts[SC_WAVES];
    __shared__ double part_sum_ts[SC_WAVES], part_sum_text[SC_WAVES], part_sum_raw[SC_WAVES];
    __shared__ float part_max[SC_WAVES];
    __shared__ int part_last[SC_WAVES], part_nan[SC_WAVES], part_bad[SC_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int p = *a.pos;
    const bool pos_ok = p >= 0 && p + 1 < a.max_pos;
    const int pc = pos_ok ? p : 0;
    const int forced = a.forced[pc], phase = a.phase[pc];
    const int fin = a.finished[b];
    const bool scan = pos_ok && !fin && forced < 0;                           // block-uniform, as everything derived from it
    const bool with_rule = S.rule != 0;
    const int n = with_rule ? pc + 1 - A.begin_index : -1;                    // generated tokens of the row; < 0: no rule at this step
    const bool rule = n >= 0;
    const int V = a.V, tsb = with_rule ? A.ts_begin : V;                      // without the rule every column is a text column
    const float* z = a.logits + (int64_t)b * a.ldl;
    const Top2 none = {-INFINITY, 0x7fffffff, -INFINITY};
    Top2 text = none, ts = none;
    double L = -INFINITY, sum_text = 0.0, sum_ts = 0.0;
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
            for (int j = A.begin_index + tid; j <= p; j += SC_THREADS) last = row[j] >= tsb ? j : last;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
            if ((tid & 63) == 0) part_last[wave] = last;
            __syncthreads();
            last = part_last[0];
#pragma unroll
            for (int w = 1; w < SC_WAVES; ++w) last = max(last, part_last[w]);
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
        const float* mk = a.mask + (int64_t)(phase < 0 ? 0 : (phase > 2 ? 2 : phase)) * a.ldm;
        auto masked = [&](int v) -> float {                                   // columns >= V (the padded vocabulary) are never read
            float x = z[v] + mk[v];
            if (x != x) { nan_seen = 1; x = INFINITY; }                       // a NaN wins where it is live, and fails the batch wherever it is
            const bool live = v >= lo_all && v != no_ts && (v < tsb ? v >= lo_text : (v >= ts_lo && v < ts_hi));
            return live ? x : -INFINITY;
        };
        const int text_end = rule ? tsb : V;                                  // a step without the rule has text columns only
#pragma unroll 4
        for (int v = tid; v < text_end; v += SC_THREADS) sc_take(text, masked(v), v);
        for (int v = text_end + tid; v < V; v += SC_THREADS) sc_take(ts, masked(v), v);
        text = sc_wave_top2(text);
        ts = sc_wave_top2(ts);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nan_seen |= __shfl_xor(nan_seen, o, 64);
        if ((tid & 63) == 0) { part_text[wave] = text; part_ts[wave] = ts; part_nan[wave] = nan_seen; }
        __syncthreads();
        text = part_text[0]; ts = part_ts[0]; nan_seen = part_nan[0];
#pragma unroll
        for (int w = 1; w < SC_WAVES; ++w) { text = top2_merge(text, part_text[w]); ts = top2_merge(ts, part_ts[w]); nan_seen |= part_nan[w]; }
        const int seen = nan_seen;                                            // pass 2 reads the row again: what it flags is already known
        if (rule) {
            // ser_dec_select_ts_v's L = m + log sum_{v >= ts_begin} exp(x[v] - m), m the largest timestamp value, in its order of operations
            const double m = (double)ts.v1;
            double s = 0.0;
            if (fabs(m) <= 3.0e38) {
                for (int v = tsb + tid; v < V; v += SC_THREADS) s += exp((double)masked(v) - m);
            }
            s = sc_block_sum(s, part_sum_ts, tid);
            if (tid == 0) {
                sum_ts = s;
                L = fabs(m) <= 3.0e38 ? m + log(s) : m;                       // all masked: -inf; a +inf or NaN column: +inf, and the batch fails
            }
        }
        {
            // the text columns around their own maximum M: with the timestamps' sum, the normaliser of the whole processed row
            const double M = (double)text.v1;
            double s = 0.0;
            if (fabs(M) <= 3.0e38) {
#pragma unroll 2
                for (int v = tid; v < text_end; v += SC_THREADS) s += exp((double)masked(v) - M);
            }
            s = sc_block_sum(s, part_sum_text, tid);
            if (tid == 0) sum_text = s;
        }
        nan_seen = seen;
    }
    // position 0: softmax(raw row)[no_speech_token], whether or not the step scans (its token is forced or language-restricted)
    const bool first = pos_ok && p == 0;
    double no_speech = NAN;
    int raw_bad = 0;
    if (first) {
        float mx = -INFINITY;
        for (int v = tid; v < V; v += SC_THREADS) {
            const float x = z[v];
            raw_bad |= !(fabsf(x) <= 3.0e38f);
            mx = fmaxf(mx, x);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); raw_bad |= __shfl_xor(raw_bad, o, 64); }
        if ((tid & 63) == 0) { part_max[wave] = mx; part_bad[wave] = raw_bad; }
        __syncthreads();
        mx = part_max[0]; raw_bad = part_bad[0];
#pragma unroll
        for (int w = 1; w < SC_WAVES; ++w) { mx = fmaxf(mx, part_max[w]); raw_bad |= part_bad[w]; }
        double s = 0.0;
        if (!raw_bad) {
            for (int v = tid; v < V; v += SC_THREADS) s += exp((double)z[v] - (double)mx);
        }
        s = sc_block_sum(s, part_sum_raw, tid);
        if (tid == 0 && !raw_bad) no_speech = exp((double)z[S.no_speech_token] - (double)mx) / s;
    }
    __syncthreads();                                                          // every thread has read *pos before thread 0 takes the ticket
    if (tid != 0) return;
    uint32_t err = pos_ok ? 0u : 4u;                                          // bit 2: the position left the ids buffer
    if (raw_bad) err |= 1u;                                                   // bit 0: the row at position 0 holds a NaN or an infinity
    int tok = a.pad;
    float margin = INFINITY;                                                  // nothing was decided: forced, finished
    double gap = INFINITY, logprob = INFINITY;
    if (scan) {
        Top2 t = text;
        const double M = (double)text.v1, m = (double)ts.v1;
        bool fired = false;
        if (rule) {
            fired = L > M;
            if (fired) t = ts;                                                // the timestamps together outweigh the best text token
            else t = top2_merge(text, ts);                                    // L == M keeps the text columns
            if (fabs(L) <= 3.0e38 && fabs(M) <= 3.0e38) gap = fabs(L - M);
        }
        tok = t.i1 < V ? t.i1 : a.pad;
        margin = t.v1 - t.v2;
        if (!(fabsf(t.v1) <= 3.0e38f) || (with_rule && nan_seen)) err |= 1u;  // bit 0: the winner is not finite, or (the rule's form) the row holds a NaN
        // the winner is the largest live value w, so x[tok] - w = 0 and logprob = -log sum exp(x - w); w is M, m or the larger of the two
        const double w = (double)t.v1;
        logprob = NAN;
        if (fabs(w) <= 3.0e38) {
            double s;
            if (fired) s = sum_ts;                                            // every text column is -inf: the sum behind L
            else if (!rule) s = sum_text;
            else s = (fabs(M) <= 3.0e38 ? sum_text * (M == w ? 1.0 : exp(M - w)) : 0.0) + (fabs(m) <= 3.0e38 ? sum_ts * (m == w ? 1.0 : exp(m - w)) : 0.0);
            logprob = 0.0 - log(s);
        }
        if (!(fabs(logprob) <= 1.0e300)) err |= 1u;                           // bit 0: a decided row whose normaliser is not finite
    } else if (!fin && forced >= 0) {
        tok = forced;
    }
    int fin_after = fin;
    if (pos_ok) {
        a.ids[(int64_t)b * a.ld_ids + p + 1] = tok;
        a.margin[(int64_t)b * a.ld_margin + p] = margin;
        if (with_rule) A.ts_gap[(int64_t)b * A.ld_gap + p] = gap;
        S.logprob[(int64_t)b * S.ld_logprob + p] = logprob;
        if (first) S.no_speech[b] = no_speech;
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

extern "C" int ser_dec_select_score_v(const ser_dec_select_score_args* S, void* stream) {
    if (!S) return ser_fail(-1, "ser_dec_select_score: null arguments");
    const ser_dec_select_ts_args* A = &S->ts;
    const ser_dec_select_args* a = &A->base;
    if (!a->logits || !a->mask || !a->phase || !a->forced || !a->ids || !a->finished || !a->margin || !a->pos || !a->unfinished ||
        !a->work || !a->err || !S->logprob || !S->no_speech || (S->rule && !A->ts_gap))
        return ser_fail(-1, "ser_dec_select_score: null pointer");
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_dec_select_score: B=%d (1..65535)", a->B);
    if (a->V <= 1 || a->ldl < a->V || a->ldm < a->V) return ser_fail(-3, "ser_dec_select_score: V=%d, ldl=%lld, ldm=%lld (V >= 2, pitches >= V)", a->V, (long long)a->ldl, (long long)a->ldm);
    if (a->max_pos < 2 || a->ld_ids < a->max_pos || a->ld_margin < a->max_pos - 1 || S->ld_logprob < a->max_pos - 1 || (S->rule && A->ld_gap < a->max_pos - 1))
        return ser_fail(-4, "ser_dec_select_score: max_pos=%d, ld_ids=%lld, ld_margin=%lld, ld_logprob=%lld, ld_gap=%lld", a->max_pos,
                        (long long)a->ld_ids, (long long)a->ld_margin, (long long)S->ld_logprob, (long long)A->ld_gap);
    if (S->no_speech_token < 0 || S->no_speech_token >= a->V || (S->rule != 0 && S->rule != 1))
        return ser_fail(-7, "ser_dec_select_score: no_speech_token=%d (inside the vocabulary of %d), rule=%d (0 or 1)", S->no_speech_token, a->V, S->rule);
    if (S->rule) {
        if (A->ts_begin < 1 || A->ts_begin >= a->V || A->no_ts < 0 || A->no_ts >= a->V || a->eos < 0 || a->eos >= a->V)
            return ser_fail(-5, "ser_dec_select_score: ts_begin=%d, no_ts=%d, eos=%d (0 < ts_begin < V=%d; no_ts and eos inside the vocabulary)",
                            A->ts_begin, A->no_ts, a->eos, a->V);
        if (A->begin_index < 1 || A->begin_index >= a->max_pos || A->max_initial < -1)
            return ser_fail(-6, "ser_dec_select_score: begin_index=%d (1..max_pos - 1), max_initial=%d (>= -1)", A->begin_index, A->max_initial);
    }
    hipLaunchKernelGGL(dec_select_score_kernel, dim3(a->B), dim3(SC_THREADS), 0, (hipStream_t)stream, *S);
    return ser_check_launch("ser_dec_select_score_v");
}
