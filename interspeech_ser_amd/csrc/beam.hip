// Whisper beam search (include/ser_hip.h, "a34"): the two kernels a beam step adds to the decoder's.  ser_dec_attn_beam_v: ser_dec_attn_v's
// arithmetic, statement for statement, reading its keys and values through an ancestor table (self-attention) or through a row-to-cache
// divisor (cross-attention).  ser_beam_select_v: HF's beam bookkeeping of one step for every utterance, two launches: a scan over
// (chunk, beam, utterance) blocks -- partial log-sum-exp and partial top-2K of the masked logits -- and a merge of one block per utterance.
// Position, scores, finished set, flags and the trace live in device memory: a recorded step is replayed as it is (ser_run).
#include "ser_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------------- attention
// dec_attn_kernel (decode.hip) with two more ways to find a row of the cache.  Logical row b, key j < len - 1:
//   src != NULL   physical row src[parity][b][j], parity = (len - 1) & 1      (clamped to [0, B): a bad entry reads a valid row)
//   src == NULL   physical row b / row_div
// The append goes to physical row b (src != NULL) at position len - 1, where no table entry points yet.  A group of 16 lanes owns one key:
// its 16 lanes read the same table word (one broadcast load), and the four table words of an unrolled iteration are loaded before the
// first key row, so the dependent load is paid once per four keys.
#define DEC_GROUPS 16
template <int MODE>
__global__ __launch_bounds__(256) void dec_attn_beam_kernel(ser_dec_attn_beam_args x) {
    __shared__ float sm[DEC_GROUPS][68];
    const ser_dec_attn_args& a = x.base;
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, ln = tid & 15, grp = tid >> 4;
    int len = a.len_add + (a.lens ? a.lens[(int64_t)b * a.lens_stride] : 0);
    len = len < 1 ? 1 : (len > a.max_len ? a.max_len : len);                 // inside the cache whatever the length word holds
    const int64_t col = (int64_t)h * 64 + ln * 4;
    const int own = x.src ? b : b / x.row_div;
    float* kc = a.kcache + col;
    float* vc = a.vcache + col;
    const float* kn = a.k_new ? a.k_new + (int64_t)b * a.ld_new + col : nullptr;
    const float* vn = a.k_new ? a.v_new + (int64_t)b * a.ld_new + col : nullptr;
    const int last = len - 1;
    const int32_t* tab = x.src ? x.src + (int64_t)(last & 1) * x.src_parity_stride + (int64_t)b * x.ld_src : nullptr;
    auto phys = [&](int j) -> int64_t {                                       // the physical cache row of key j
        if (!tab) return own;
        int r = tab[j < x.ld_src ? j : x.ld_src - 1];
        return r < 0 ? 0 : (r >= a.B ? a.B - 1 : r);
    };
    if (kn && grp == (last & (DEC_GROUPS - 1))) {
        *(f32x4*)(kc + (int64_t)own * a.batch_stride + (int64_t)last * a.ldc) = *(const f32x4*)kn;
        *(f32x4*)(vc + (int64_t)own * a.batch_stride + (int64_t)last * a.ldc) = *(const f32x4*)vn;
    }
    const float qs = a.scale * 1.4426950408889634f;                          // base-2 softmax
    f32x4 q = *(const f32x4*)(a.q + (int64_t)b * a.ldq + col);
    q *= qs;
    float m = -INFINITY, l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    auto dot16 = [&](f32x4 k) -> float {
        float s = q[0] * k[0];
        s = fmaf(q[1], k[1], s); s = fmaf(q[2], k[2], s); s = fmaf(q[3], k[3], s);
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
        return s;
    };
    int j = grp;
    for (; j + 3 * DEC_GROUPS < len; j += 4 * DEC_GROUPS) {
        int64_t off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = j + u * DEC_GROUPS;
            off[u] = (kn && jj == last) ? -1 : phys(jj) * a.batch_stride + (int64_t)jj * a.ldc;
        }
        f32x4 k[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            k[u] = *(const f32x4*)(off[u] < 0 ? kn : kc + off[u]);
            v[u] = *(const f32x4*)(off[u] < 0 ? vn : vc + off[u]);
        }
        float s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = dot16(k[u]);
        const float mn = fmaxf(fmaxf(m, fmaxf(s[0], s[1])), fmaxf(s[2], s[3]));
        const float c = __builtin_amdgcn_exp2f(m - mn);
        l *= c;
        acc *= c;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float p = __builtin_amdgcn_exp2f(s[u] - mn);
            l += p;
            acc += p * v[u];
        }
        m = mn;
    }
    for (; j < len; j += DEC_GROUPS) {
        const bool fresh = kn && j == last;
        const int64_t off = fresh ? 0 : phys(j) * a.batch_stride + (int64_t)j * a.ldc;
        const f32x4 k = *(const f32x4*)(fresh ? kn : kc + off), v = *(const f32x4*)(fresh ? vn : vc + off);
        const float s = dot16(k);
        const float mn = fmaxf(m, s);
        const float c = __builtin_amdgcn_exp2f(m - mn), p = __builtin_amdgcn_exp2f(s - mn);
        l = l * c + p;
        acc = acc * c + p * v;
        m = mn;
    }
    *(f32x4*)&sm[grp][ln * 4] = acc;
    if (ln == 0) { sm[grp][64] = m; sm[grp][65] = l; }
    __syncthreads();
    if (tid < 64) {
        float M = sm[0][64];
#pragma unroll
        for (int g = 1; g < DEC_GROUPS; ++g) M = fmaxf(M, sm[g][64]);
        float L = 0.f, o = 0.f;
#pragma unroll
        for (int g = 0; g < DEC_GROUPS; ++g) {                               // a group without keys holds (-inf, 0, 0): weight 0
            const float w = __builtin_amdgcn_exp2f(sm[g][64] - M);
            L = fmaf(sm[g][65], w, L);
            o = fmaf(sm[g][tid], w, o);
        }
        const float r = o / L;
        unsigned short* dst = (unsigned short*)a.out_act + (int64_t)b * a.ldo_act + (int64_t)h * 64 + tid;
        if (mode_traits<MODE>::planes == 1) {
            *dst = f2bf(r);
        } else {
            unsigned short hi, lo;
            split2<MODE>(r, hi, lo);
            dst[0] = hi;
            dst[a.out_plane_stride] = lo;
        }
        if (mode_traits<MODE>::f16) range_report(a.range_flag, range_fold(0.f, r));
    }
}

extern "C" int ser_dec_attn_beam_v(const ser_dec_attn_beam_args* x, void* stream) {
    if (!x) return ser_fail(-1, "ser_dec_attn_beam: null arguments");
    const ser_dec_attn_args* a = &x->base;
    if (!a->q || !a->kcache || !a->vcache || !a->out_act) return ser_fail(-1, "ser_dec_attn_beam: null pointer");
    if ((a->k_new == nullptr) != (a->v_new == nullptr)) return ser_fail(-1, "ser_dec_attn_beam: k_new and v_new come together");
    if (a->dh != 64) return ser_fail(-2, "ser_dec_attn_beam: dh=%d (64: the head dim of every Whisper size)", a->dh);
    if (a->B <= 0 || a->B > 65535 || a->H <= 0 || a->H > 65535) return ser_fail(-3, "ser_dec_attn_beam: B=%d, H=%d (1..65535)", a->B, a->H);
    const int64_t D = (int64_t)a->H * 64;
    if (a->ldq < D || (a->ldq % 4) || a->ldc < D || (a->ldc % 4) || (a->batch_stride % 4) || a->batch_stride < 0 ||
        (a->k_new && (a->ld_new < D || (a->ld_new % 4))))
        return ser_fail(-4, "ser_dec_attn_beam: pitches must be >= H * 64 and multiples of 4 (ldq=%lld, ldc=%lld, ld_new=%lld, batch_stride=%lld)",
                        (long long)a->ldq, (long long)a->ldc, (long long)a->ld_new, (long long)a->batch_stride);
    if (a->B > 1 && a->batch_stride < (int64_t)a->max_len * a->ldc)
        return ser_fail(-4, "ser_dec_attn_beam: batch_stride=%lld overlaps the sequences' caches", (long long)a->batch_stride);
    if (((uintptr_t)a->q | (uintptr_t)a->kcache | (uintptr_t)a->vcache | (uintptr_t)a->k_new | (uintptr_t)a->v_new) & 15)
        return ser_fail(-5, "ser_dec_attn_beam: q, k_new, v_new and the caches must be 16-byte aligned");
    if (a->max_len <= 0 || a->lens_stride < 0 || (!a->lens && a->len_add < 1))
        return ser_fail(-6, "ser_dec_attn_beam: max_len=%d, lens_stride=%d, len_add=%d", a->max_len, a->lens_stride, a->len_add);
    if (a->ldo_act < D || a->out_plane_stride < 0) return ser_fail(-7, "ser_dec_attn_beam: ldo_act=%lld (>= H * 64)", (long long)a->ldo_act);
    if (x->src) {
        if (x->ld_src < a->max_len || x->src_parity_stride < (int64_t)a->B * x->ld_src)
            return ser_fail(-9, "ser_dec_attn_beam: ld_src=%d (>= max_len), src_parity_stride=%lld (>= B * ld_src)", x->ld_src, (long long)x->src_parity_stride);
    } else {
        if (x->row_div < 1) return ser_fail(-9, "ser_dec_attn_beam: row_div=%d (>= 1 without a table)", x->row_div);
        if (a->k_new) return ser_fail(-9, "ser_dec_attn_beam: rows that share a cache cannot append to it");
    }
    const dim3 grid(a->H, a->B), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (a->mode == SER_MODE_BF16) hipLaunchKernelGGL(dec_attn_beam_kernel<SER_MODE_BF16>, grid, block, 0, s, *x);
    else if (a->mode == SER_MODE_FP32X) hipLaunchKernelGGL(dec_attn_beam_kernel<SER_MODE_FP32X>, grid, block, 0, s, *x);
    else if (a->mode == SER_MODE_FP16X) hipLaunchKernelGGL(dec_attn_beam_kernel<SER_MODE_FP16X>, grid, block, 0, s, *x);
    else return ser_fail(-8, "ser_dec_attn_beam: mode %d (SER_MODE_BF16, FP32X or FP16X)", a->mode);
    return ser_check_launch("ser_dec_attn_beam_v");
}

// ---------------------------------------------------------------------------------------------------------------- select
// Candidate order everywhere: the larger value first, on equal values the lower index (token inside a row, parent * V + token across rows).
struct BeamF { float v; int i; };
struct BeamD { double v; int i; };
template <class T> __device__ __forceinline__ bool beam_before(const T& a, const T& b) { return a.v > b.v || (a.v == b.v && a.i < b.i); }
__device__ __forceinline__ BeamF beam_shfl(BeamF t, int o) { BeamF y; y.v = __shfl_xor(t.v, o, 64); y.i = __shfl_xor(t.i, o, 64); return y; }
__device__ __forceinline__ BeamD beam_shfl(BeamD t, int o) { BeamD y; y.v = __shfl_xor(t.v, o, 64); y.i = __shfl_xor(t.i, o, 64); return y; }

// The block's best candidate, known to every thread after ONE barrier (part: [2][4], the halves alternate with the round).
template <class T>
__device__ __forceinline__ T beam_block_best(T t, T (*part)[4], int round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T y = beam_shfl(t, o);
        if (beam_before(y, t)) t = y;
    }
    if ((threadIdx.x & 63) == 0) part[round & 1][threadIdx.x >> 6] = t;
    __syncthreads();
    T w = part[round & 1][0];
#pragma unroll
    for (int g = 1; g < 4; ++g) {
        const T y = part[round & 1][g];
        if (beam_before(y, w)) w = y;
    }
    return w;
}

__host__ __device__ static inline int beam_chunks(int V) { return (V + SER_BEAM_CHUNK - 1) / SER_BEAM_CHUNK; }

// work: double ms[B K nchunk][2] (max, sum of exp(z - max)) | BeamF top[B K nchunk][SER_BEAM_MAX_CAND]
extern "C" int64_t ser_beam_work_bytes(int32_t B, int32_t K, int32_t V) {
    if (B <= 0 || B > 65535 || K < 2 || K > SER_BEAM_MAX_K || V < 2 * K || beam_chunks(V) > SER_BEAM_MAX_CHUNKS) return -1;
    return (int64_t)B * K * beam_chunks(V) * (16 + 8 * SER_BEAM_MAX_CAND);
}

#define BEAM_PER (SER_BEAM_CHUNK / 256)
// Stage 1, block (chunk c, beam k, utterance b): columns [c CHUNK, min(V, (c + 1) CHUNK)) of row b K + k.  Thread t owns columns base + t +
// 256 u in registers.  The log-sum-exp partial is over the RAW logits (suppressed tokens count in the normaliser); the top-2K is over the
// masked ones, a NaN counting as +inf (it wins, and the merge fails the batch).
__global__ __launch_bounds__(256) void beam_scan_kernel(ser_beam_select_args a, int nchunk) {
    __shared__ BeamF part[2][4];
    __shared__ double dsum[4];
    const int c = blockIdx.x, k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    int p = *a.pos;
    p = p < 0 ? 0 : (p >= a.max_pos ? a.max_pos - 1 : p);
    int phase = a.phase[p];
    phase = phase < 0 ? 0 : (phase > 2 ? 2 : phase);
    const int64_t row = (int64_t)b * a.K + k;
    const float* z = a.logits + row * a.ldl;
    const float* mk = a.mask + (int64_t)phase * a.ldm;
    const int base = c * SER_BEAM_CHUNK;
    float raw[BEAM_PER], y[BEAM_PER];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < BEAM_PER; ++u) {
        const int v = base + tid + 256 * u;
        const bool in = v < a.V;                                              // padded vocabulary columns (>= V) are never read
        raw[u] = in ? z[v] : -INFINITY;
        float t = in ? raw[u] + mk[v] : -INFINITY;
        y[u] = (t != t) ? INFINITY : t;
        mx = fmaxf(mx, raw[u]);
    }
    // partial log-sum-exp: the block's maximum (exact), then float64 sums: a thread adds its columns in ascending order, the lanes meet by
    // xor shuffles, the four waves are added in wave order: a function of V alone
    BeamF mt = {mx, 0};
    mt = beam_block_best(mt, part, 0);
    const double M = (double)mt.v;
    double s = 0.0;
    if (mt.v > -INFINITY) {
#pragma unroll
        for (int u = 0; u < BEAM_PER; ++u)
            if (base + tid + 256 * u < a.V) s += exp((double)raw[u] - M);     // a NaN logit makes the sum NaN: the row fails
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) dsum[tid >> 6] = s;
    const int64_t slot = row * nchunk + c;
    double* ms = (double*)a.work;
    BeamF* top = (BeamF*)((char*)a.work + (int64_t)a.B * a.K * nchunk * 16) + slot * SER_BEAM_MAX_CAND;
    unsigned taken = 0;
    const int rounds = 2 * a.K + 1 < SER_BEAM_MAX_CAND ? 2 * a.K + 1 : SER_BEAM_MAX_CAND;     // 2K candidates and the first one cut (for the gap)
    for (int r = 0; r < rounds; ++r) {                                        // bounded by a launch argument
        BeamF t = {-INFINITY, 0x7fffffff};
#pragma unroll
        for (int u = 0; u < BEAM_PER; ++u) {
            const int v = base + tid + 256 * u;
            const BeamF cand = {y[u], v};
            if (v < a.V && !((taken >> u) & 1u) && beam_before(cand, t)) t = cand;
        }
        const BeamF w = beam_block_best(t, part, r + 1);
        const int rel = w.i - base;
        if (w.i != 0x7fffffff && (rel & 255) == tid) taken |= 1u << (rel >> 8);
        if (tid == 0) {
            BeamF o = w;
            if (!(w.v > -INFINITY)) o.i = -1;                                 // masked out or nothing left: no candidate
            top[r] = o;
        }
    }
    if (tid == 0) {                                                           // dsum was written before the rounds' barriers
        ms[2 * slot] = M;
        ms[2 * slot + 1] = ((dsum[0] + dsum[1]) + dsum[2]) + dsum[3];
    }
}

#define BEAM_M2 ((SER_BEAM_MAX_K * SER_BEAM_MAX_CHUNKS * SER_BEAM_MAX_CAND + 255) / 256)
// Stage 2, one block per utterance: the rows' log-sum-exp from the partials in chunk order, the accumulated score of every partial
// candidate, the best 2K + 1 of them (2K candidates and the first one cut, for the gap), and thread 0's bookkeeping: HF's
// GenerationMixin._beam_search restated with masks (tests/whisper_beam_ref.py is the statement).
__global__ __launch_bounds__(256) void beam_merge_kernel(ser_beam_select_args a, int nchunk) {
    __shared__ BeamD part[2][4];
    __shared__ double lse[SER_BEAM_MAX_K], run[SER_BEAM_MAX_K];
    __shared__ BeamD win[SER_BEAM_MAX_CAND];
    __shared__ int par_s[SER_BEAM_MAX_K], tok_s[SER_BEAM_MAX_K], live_s;
    const int b = blockIdx.x, tid = threadIdx.x, K = a.K, C2 = 2 * K;
    const int p = *a.pos;
    const bool pos_ok = p >= 0 && p + 1 < a.max_pos;
    const int pc = pos_ok ? p : 0;
    int32_t* st = a.state + 4 * b;                                            // n_fin, flag, done, done_step
    const bool live = pos_ok && !st[2];
    const double* ms = (const double*)a.work;
    const BeamF* top = (const BeamF*)((const char*)a.work + (int64_t)a.B * K * nchunk * 16);
    if (tid < K) {
        const int64_t s0 = ((int64_t)b * K + tid) * nchunk;
        double M = -INFINITY;
        for (int c = 0; c < nchunk; ++c) M = fmax(M, ms[2 * (s0 + c)]);
        double S = 0.0;
        for (int c = 0; c < nchunk; ++c) {
            const double mc = ms[2 * (s0 + c)];
            if (mc > -INFINITY) S += ms[2 * (s0 + c) + 1] * exp(mc - M);
            else if (mc != mc) S = mc;
        }
        lse[tid] = M + log(S);
        run[tid] = a.run[(int64_t)b * K + tid];
        par_s[tid] = tid;
        tok_s[tid] = a.pad;
    }
    __syncthreads();
    BeamD cand[BEAM_M2];
    const int per_row = nchunk * SER_BEAM_MAX_CAND, n_cand = K * per_row;
#pragma unroll
    for (int u = 0; u < BEAM_M2; ++u) {
        const int i = tid + 256 * u;
        BeamD t = {-INFINITY, 0x7fffffff};
        if (live && i < n_cand) {
            const int k = i / per_row, rem = i - k * per_row;
            const BeamF f = top[((int64_t)b * K + k) * per_row + rem];
            if ((rem % SER_BEAM_MAX_CAND) <= C2 && f.i >= 0 && f.i < a.V) {
                double s = ((double)f.v - lse[k]) + run[k];                   // log-softmax first, then the running score
                if (s != s) s = run[k] > -INFINITY ? INFINITY : -INFINITY;   // a live beam's NaN wins and fails the batch below; a dead beam decides nothing
                if (s > -INFINITY) { t.v = s; t.i = k * a.V + f.i; }
            }
        }
        cand[u] = t;
    }
    unsigned taken = 0;
    for (int r = 0; r <= C2; ++r) {
        BeamD t = {-INFINITY, 0x7fffffff};
#pragma unroll
        for (int u = 0; u < BEAM_M2; ++u)
            if (!((taken >> u) & 1u) && beam_before(cand[u], t)) t = cand[u];
        const BeamD w = beam_block_best(t, part, r);
#pragma unroll
        for (int u = 0; u < BEAM_M2; ++u)
            if (w.i != 0x7fffffff && cand[u].i == w.i) taken |= 1u << u;
        if (tid == 0) win[r] = w;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t err = pos_ok ? 0u : 4u;                                      // bit 2: the position left the ids buffer
        int done = st[2];
        if (live) {
            const int cur = p + 1;                                            // HF's cur_len: the tokens every row holds
            int n_ok = 0;
            for (int j = 0; j < C2; ++j) {
                if (win[j].i != 0x7fffffff) ++n_ok;
                if (win[j].i != 0x7fffffff && !(fabs(win[j].v) <= 1.7e308)) err |= 1u;       // bit 0: a winner that is not finite
            }
            if (n_ok < C2) err |= 8u;                                         // bit 3: fewer than 2K finite candidates
            double gap = INFINITY;
            if (n_ok == C2 && win[C2].i != 0x7fffffff) gap = fmin(gap, win[C2 - 1].v - win[C2].v);
            int32_t* tc = a.trace_cand + ((int64_t)pc * a.B + b) * C2 * 2;
            double* cs = a.cand_score + ((int64_t)pc * a.B + b) * C2;
            bool hit[SER_BEAM_MAX_CAND];
            int n_hit = 0;
            const bool at_max = cur + 1 >= a.max_length;
            for (int j = 0; j < C2; ++j) {
                const bool ok = win[j].i != 0x7fffffff;
                const int par = ok ? win[j].i / a.V : -1, tok = ok ? win[j].i - par * a.V : -1;
                tc[2 * j] = par; tc[2 * j + 1] = tok;
                cs[j] = win[j].v;
                hit[j] = ok && (tok == a.eos || at_max);
                n_hit += hit[j] || !ok;
            }
            // the running beams of the next step: the best K candidates that did not hit, in rank order
            int n_run = 0;
            double next_cut = -INFINITY;
            for (int j = 0; j < C2; ++j) {
                if (win[j].i == 0x7fffffff || hit[j]) continue;
                if (n_run < K) {
                    par_s[n_run] = win[j].i / a.V;
                    tok_s[n_run] = win[j].i - par_s[n_run] * a.V;
                    run[n_run] = win[j].v;
                    ++n_run;
                } else { next_cut = win[j].v; break; }
            }
            if (n_run == K && next_cut > -INFINITY) gap = fmin(gap, run[K - 1] - next_cut);
            for (int r = n_run; r < K; ++r) { par_s[r] = r; tok_s[r] = a.pad; run[r] = -INFINITY; }      // dead rows
            if ((hit[K - 1] || hit[K]) && win[K].i != 0x7fffffff) gap = fmin(gap, win[K - 1].v - win[K].v);
            // the finished set: only candidates of rank < K that hit enter, and none once the flag has dropped
            int n_fin = st[0];
            double* fs = a.fin_score + (int64_t)b * K;
            int32_t* fh = a.fin_handle + (int64_t)b * K * 2;
            if (st[1]) {
                const double den = a.lenpow[cur + 1 - a.prompt_len < 0 ? 0 : cur + 1 - a.prompt_len];
                for (int j = 0; j < K; ++j) {
                    if (!hit[j]) continue;
                    const double s = win[j].v / den;
                    if (n_fin == K) gap = fmin(gap, fabs(s - fs[K - 1]));
                    int at = n_fin;                                           // behind every entry that is not worse: the older one wins a tie
                    while (at > 0 && s > fs[at - 1]) --at;
                    if (at >= K) continue;
                    const int end = n_fin < K ? n_fin : K - 1;
                    for (int q = end; q > at; --q) { fs[q] = fs[q - 1]; fh[2 * q] = fh[2 * q - 2]; fh[2 * q + 1] = fh[2 * q - 1]; }
                    fs[at] = s; fh[2 * at] = p; fh[2 * at + 1] = j;
                    if (n_fin < K) ++n_fin;
                }
            }
            st[0] = n_fin;
            // the early-stop flag, a sticky AND: can the best running beam still beat the worst finished one?
            if (n_fin == K) {
                const double best = run[0] / a.lenpow[cur + 1 - a.prompt_len < 1 ? 1 : cur + 1 - a.prompt_len];
                if (run[0] > -INFINITY) gap = fmin(gap, fabs(best - fs[K - 1]));
                if (!(best > fs[K - 1])) st[1] = 0;
            }
            if (!st[1] || n_hit == C2) { done = 1; st[2] = 1; st[3] = p; }
            a.gaps[(int64_t)pc * a.B + b] = gap;
            for (int r = 0; r < K; ++r) a.run[(int64_t)b * K + r] = run[r];
        }
        live_s = live;
        if (err) atomicOr(a.err, err);
        // the block that takes the last ticket publishes the count of utterances not done and advances the position: every other block
        // has read *pos before it took its own ticket (ser_dec_select_v's scheme)
        atomicAdd(&a.ticket[1], done ? 0 : 1);
    }
    __syncthreads();
    if (pos_ok) {
        // frozen utterances keep stepping: identity parents, pad tokens
        const int R0 = b * K;
        if (tid < K) {
            int par = par_s[tid];
            par = par < 0 ? 0 : (par >= K ? K - 1 : par);
            par_s[tid] = par;
            a.ids[(int64_t)(R0 + tid) * a.ld_ids + p + 1] = tok_s[tid];
            int32_t* tr = a.trace_run + (((int64_t)p * a.B + b) * K + tid) * 2;
            tr[0] = live_s ? par : -1;
            tr[1] = tok_s[tid];
        }
        __syncthreads();
        if (a.src) {                                                          // the ancestor table's next half: src'[r][j] = src[parent(r)][j], src'[r][p] = parent(r)
            const int32_t* from = a.src + (int64_t)(p & 1) * a.src_parity_stride;
            int32_t* to = a.src + (int64_t)((p + 1) & 1) * a.src_parity_stride;
            for (int i = tid; i < K * a.max_pos; i += 256) {                  // bounded by launch arguments
                const int r = i / a.max_pos, j = i - r * a.max_pos;
                if (j > p) continue;
                const int pr = R0 + par_s[r];
                to[(int64_t)(R0 + r) * a.ld_src + j] = j < p ? from[(int64_t)pr * a.ld_src + j] : pr;
            }
        }
    }
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(&a.ticket[0], 1) == a.B - 1) {
            *a.unfinished = atomicExch(&a.ticket[1], 0);
            atomicExch(&a.ticket[0], 0);
            if (pos_ok) *a.pos = p + 1;
        }
    }
}

extern "C" int ser_beam_select_v(const ser_beam_select_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_beam_select: null arguments");
    if (!a->logits || !a->mask || !a->phase || !a->lenpow || !a->ids || !a->run || !a->fin_score || !a->fin_handle || !a->state || !a->trace_run ||
        !a->trace_cand || !a->cand_score || !a->gaps || !a->work || !a->pos || !a->unfinished || !a->ticket || !a->err)
        return ser_fail(-1, "ser_beam_select: null pointer");
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_beam_select: B=%d (1..65535)", a->B);
    if (a->K < 2 || a->K > SER_BEAM_MAX_K) return ser_fail(-2, "ser_beam_select: K=%d (2..%d)", a->K, SER_BEAM_MAX_K);
    if (a->V < 2 * a->K || a->ldl < a->V || a->ldm < a->V || beam_chunks(a->V) > SER_BEAM_MAX_CHUNKS)
        return ser_fail(-3, "ser_beam_select: V=%d, ldl=%lld, ldm=%lld (2 K <= V <= %d, pitches >= V)", a->V, (long long)a->ldl, (long long)a->ldm,
                        SER_BEAM_MAX_CHUNKS * SER_BEAM_CHUNK);
    if (a->max_pos < 2 || a->ld_ids < a->max_pos || a->max_length < 2 || a->max_length > a->max_pos || a->prompt_len < 1 || a->prompt_len >= a->max_length)
        return ser_fail(-4, "ser_beam_select: max_pos=%d, ld_ids=%lld, max_length=%d, prompt_len=%d", a->max_pos, (long long)a->ld_ids, a->max_length, a->prompt_len);
    if (a->src && (a->ld_src < a->max_pos || a->src_parity_stride < (int64_t)a->B * a->K * a->ld_src))
        return ser_fail(-5, "ser_beam_select: ld_src=%d (>= max_pos), src_parity_stride=%lld (>= B K ld_src)", a->ld_src, (long long)a->src_parity_stride);
    if (a->work_bytes < ser_beam_work_bytes(a->B, a->K, a->V) || ((uintptr_t)a->work & 7))
        return ser_fail(-6, "ser_beam_select: work_bytes=%lld (>= ser_beam_work_bytes = %lld, 8-byte aligned)", (long long)a->work_bytes,
                        (long long)ser_beam_work_bytes(a->B, a->K, a->V));
    const int nchunk = beam_chunks(a->V);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(beam_scan_kernel, dim3(nchunk, a->K, a->B), dim3(256), 0, s, *a, nchunk);
    int rc = ser_check_launch("ser_beam_select_v (scan)");
    if (rc) return rc;
    hipLaunchKernelGGL(beam_merge_kernel, dim3(a->B), dim3(256), 0, s, *a, nchunk);
    return ser_check_launch("ser_beam_select_v (merge)");
}
