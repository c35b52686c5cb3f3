// Whisper decoder, one token per sequence and step (include/ser_hip.h, "a25"): the three kernels of a decode step that are neither a GEMM
// nor a LayerNorm.  ser_dec_embed_v: token + position rows.  ser_dec_attn_v: one query per (sequence, head) over an fp32 K/V cache, with the
// append of the step's own k / v row.  ser_dec_select_v: masked greedy choice, end-of-sequence bookkeeping, and the advance of the position.
// The position lives in device memory and no pointer changes between steps, so a recorded step is replayed as it is (ser_run).
#include "ser_common.h"
#include "top2_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------------------- embed
__global__ __launch_bounds__(256) void dec_embed_kernel(ser_dec_embed_args a) {
    const int b = blockIdx.x;
    int p = *a.pos;
    p = p < 0 ? 0 : (p >= a.max_pos ? a.max_pos - 1 : p);
    int id = a.ids[(int64_t)b * a.ld_ids + p];
    id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);                  // a bad id reads a valid row: never out of bounds
    const f32x4* te = (const f32x4*)(a.embed_tokens + (int64_t)id * a.D);
    const f32x4* pe = (const f32x4*)(a.embed_positions + (int64_t)p * a.D);
    f32x4* o = (f32x4*)(a.out + (int64_t)b * a.ldo);
    for (int c = threadIdx.x; c < a.D / 4; c += blockDim.x) o[c] = te[c] + pe[c];
}

extern "C" int ser_dec_embed_v(const ser_dec_embed_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_dec_embed: null arguments");
    if (!a->ids || !a->pos || !a->embed_tokens || !a->embed_positions || !a->out) return ser_fail(-1, "ser_dec_embed: null pointer");
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_dec_embed: B=%d (1..65535)", a->B);
    if (a->D <= 0 || (a->D % 4) || a->ldo < a->D || (a->ldo % 4)) return ser_fail(-3, "ser_dec_embed: D=%d, ldo=%lld (D %% 4 == 0, ldo >= D, ldo %% 4 == 0)", a->D, (long long)a->ldo);
    if (a->vocab <= 0 || a->max_pos <= 0 || a->ld_ids < a->max_pos) return ser_fail(-4, "ser_dec_embed: vocab=%d, max_pos=%d, ld_ids=%lld", a->vocab, a->max_pos, (long long)a->ld_ids);
    if (((uintptr_t)a->embed_tokens | (uintptr_t)a->embed_positions | (uintptr_t)a->out) & 15) return ser_fail(-5, "ser_dec_embed: tables and output must be 16-byte aligned");
    hipLaunchKernelGGL(dec_embed_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_dec_embed_v");
}

// ---------------------------------------------------------------------------------------------------------------- attention
// One block of 256 threads per (head, sequence): 16 groups of 16 lanes, a lane owns 4 of the head's 64 columns (one 16-byte load per K and
// per V row, straight to registers; 16 lanes = one 256-byte row).  Group g takes keys g, g + 16, g + 32, ...: four keys per iteration, one
// online-softmax rescale per four.  The 16 partial (max, sum, context) triples meet in LDS and are merged in ascending group order.  All of
// it depends on (len, the sequence's own data) only: a sequence alone and in a batch give the same bits.
#define DEC_GROUPS 16
template <int MODE>
__global__ __launch_bounds__(256) void dec_attn_kernel(ser_dec_attn_args a) {
    __shared__ float sm[DEC_GROUPS][68];
    const int h = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, ln = tid & 15, grp = tid >> 4;
    int len = a.len_add + (a.lens ? a.lens[(int64_t)b * a.lens_stride] : 0);
    len = len < 1 ? 1 : (len > a.max_len ? a.max_len : len);                 // inside the cache whatever the length word holds
    const int64_t col = (int64_t)h * 64 + ln * 4;
    float* kc = a.kcache + (int64_t)b * a.batch_stride + col;
    float* vc = a.vcache + (int64_t)b * a.batch_stride + col;
    const float* kn = a.k_new ? a.k_new + (int64_t)b * a.ld_new + col : nullptr;
    const float* vn = a.k_new ? a.v_new + (int64_t)b * a.ld_new + col : nullptr;
    const int last = len - 1;
    // the append: the group that owns key len - 1 stores the step's own k / v columns of this head at that row, and reads them from the
    // projection's output rather than back from the cache.  No other block touches these columns.
    if (kn && grp == (last & (DEC_GROUPS - 1))) {
        *(f32x4*)(kc + (int64_t)last * a.ldc) = *(const f32x4*)kn;
        *(f32x4*)(vc + (int64_t)last * a.ldc) = *(const f32x4*)vn;
    }
    const float qs = a.scale * 1.4426950408889634f;                          // base-2 softmax
    f32x4 q = *(const f32x4*)(a.q + (int64_t)b * a.ldq + col);
    q *= qs;
    float m = -INFINITY, l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    auto krow = [&](int j) -> const float* { return (kn && j == last) ? kn : kc + (int64_t)j * a.ldc; };
    auto vrow = [&](int j) -> const float* { return (kn && j == last) ? vn : vc + (int64_t)j * a.ldc; };
    auto dot16 = [&](f32x4 k) -> float {
        float s = q[0] * k[0];
        s = fmaf(q[1], k[1], s); s = fmaf(q[2], k[2], s); s = fmaf(q[3], k[3], s);
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64); s += __shfl_xor(s, 8, 64);
        return s;
    };
    int j = grp;
    for (; j + 3 * DEC_GROUPS < len; j += 4 * DEC_GROUPS) {
        f32x4 k[4], v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { k[u] = *(const f32x4*)krow(j + u * DEC_GROUPS); v[u] = *(const f32x4*)vrow(j + u * DEC_GROUPS); }
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
        const f32x4 k = *(const f32x4*)krow(j), v = *(const f32x4*)vrow(j);
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

extern "C" int ser_dec_attn_v(const ser_dec_attn_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_dec_attn: null arguments");
    if (!a->q || !a->kcache || !a->vcache || !a->out_act) return ser_fail(-1, "ser_dec_attn: null pointer");
    if ((a->k_new == nullptr) != (a->v_new == nullptr)) return ser_fail(-1, "ser_dec_attn: k_new and v_new come together");
    if (a->dh != 64) return ser_fail(-2, "ser_dec_attn: dh=%d (64: the head dim of every Whisper size)", a->dh);
    if (a->B <= 0 || a->B > 65535 || a->H <= 0 || a->H > 65535) return ser_fail(-3, "ser_dec_attn: B=%d, H=%d (1..65535)", a->B, a->H);
    const int64_t D = (int64_t)a->H * 64;
    if (a->ldq < D || (a->ldq % 4) || a->ldc < D || (a->ldc % 4) || (a->batch_stride % 4) || a->batch_stride < 0 ||
        (a->k_new && (a->ld_new < D || (a->ld_new % 4))))
        return ser_fail(-4, "ser_dec_attn: pitches must be >= H * 64 and multiples of 4 (ldq=%lld, ldc=%lld, ld_new=%lld, batch_stride=%lld)",
                        (long long)a->ldq, (long long)a->ldc, (long long)a->ld_new, (long long)a->batch_stride);
    if (a->B > 1 && a->batch_stride < (int64_t)a->max_len * a->ldc)
        return ser_fail(-4, "ser_dec_attn: batch_stride=%lld overlaps the sequences' caches", (long long)a->batch_stride);
    if (((uintptr_t)a->q | (uintptr_t)a->kcache | (uintptr_t)a->vcache | (uintptr_t)a->k_new | (uintptr_t)a->v_new) & 15)
        return ser_fail(-5, "ser_dec_attn: q, k_new, v_new and the caches must be 16-byte aligned");
    if (a->max_len <= 0 || a->lens_stride < 0 || (!a->lens && a->len_add < 1)) return ser_fail(-6, "ser_dec_attn: max_len=%d, lens_stride=%d, len_add=%d", a->max_len, a->lens_stride, a->len_add);
    if (a->ldo_act < D || a->out_plane_stride < 0) return ser_fail(-7, "ser_dec_attn: ldo_act=%lld (>= H * 64)", (long long)a->ldo_act);
    const dim3 grid(a->H, a->B), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (a->mode == SER_MODE_BF16) hipLaunchKernelGGL(dec_attn_kernel<SER_MODE_BF16>, grid, block, 0, s, *a);
    else if (a->mode == SER_MODE_FP32X) hipLaunchKernelGGL(dec_attn_kernel<SER_MODE_FP32X>, grid, block, 0, s, *a);
    else if (a->mode == SER_MODE_FP16X) hipLaunchKernelGGL(dec_attn_kernel<SER_MODE_FP16X>, grid, block, 0, s, *a);
    else return ser_fail(-8, "ser_dec_attn: mode %d (SER_MODE_BF16, FP32X or FP16X)", a->mode);
    return ser_check_launch("ser_dec_attn_v");
}

// ---------------------------------------------------------------------------------------------------------------- select
// Top2 / top2_merge: top2_common.h (shared with ctc.hip)
__global__ __launch_bounds__(256) void dec_select_kernel(ser_dec_select_args a) {
    __shared__ Top2 part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int p = *a.pos;
    const bool pos_ok = p >= 0 && p + 1 < a.max_pos;
    const int pc = pos_ok ? p : 0;
    const int forced = a.forced[pc], phase = a.phase[pc];
    const int fin = a.finished[b];
    Top2 t = {-INFINITY, 0x7fffffff, -INFINITY};
    const bool scan = pos_ok && !fin && forced < 0;
    if (scan) {                                                               // block-uniform
        const float* z = a.logits + (int64_t)b * a.ldl;
        const float* mk = a.mask + (int64_t)(phase < 0 ? 0 : (phase > 2 ? 2 : phase)) * a.ldm;
        for (int v = tid; v < a.V; v += 256) {                                // padded vocabulary columns (>= V) are never read
            float x = z[v] + mk[v];
            x = (x != x) ? INFINITY : x;                                      // a NaN wins, and a non-finite winner fails the batch below
            if (x > t.v1 || (x == t.v1 && v < t.i1)) { t.v2 = t.v1; t.v1 = x; t.i1 = v; }
            else t.v2 = fmaxf(t.v2, x);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            Top2 y;
            y.v1 = __shfl_xor(t.v1, o, 64); y.i1 = __shfl_xor(t.i1, o, 64); y.v2 = __shfl_xor(t.v2, o, 64);
            t = top2_merge(t, y);
        }
        if ((tid & 63) == 0) part[tid >> 6] = t;
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t err = pos_ok ? 0u : 4u;                                          // bit 2: the position left the ids buffer
    int tok = a.pad;
    float margin = INFINITY;                                                  // nothing was decided: forced, finished
    if (scan) {
        t = top2_merge(top2_merge(part[0], part[1]), top2_merge(part[2], part[3]));
        tok = t.i1 < a.V ? t.i1 : a.pad;
        margin = t.v1 - t.v2;
        if (!(fabsf(t.v1) <= 3.0e38f)) err |= 1u;                             // bit 0: the winning masked logit is not finite
    } else if (!fin && forced >= 0) {
        tok = forced;
    }
    int fin_after = fin;
    if (pos_ok) {
        a.ids[(int64_t)b * a.ld_ids + p + 1] = tok;
        a.margin[(int64_t)b * a.ld_margin + p] = margin;
        if (!fin && tok == a.eos) { a.finished[b] = 1; fin_after = 1; }
    }
    if (err) atomicOr(a.err, err);
    // the block that takes the last ticket publishes the count of unfinished rows and advances the position: every other block has read
    // *pos before it took its own ticket
    atomicAdd(&a.work[1], fin_after ? 0 : 1);
    __threadfence();
    if (atomicAdd(&a.work[0], 1) == a.B - 1) {
        *a.unfinished = atomicExch(&a.work[1], 0);
        atomicExch(&a.work[0], 0);
        if (pos_ok) *a.pos = p + 1;
    }
}

extern "C" int ser_dec_select_v(const ser_dec_select_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_dec_select: null arguments");
    if (!a->logits || !a->mask || !a->phase || !a->forced || !a->ids || !a->finished || !a->margin || !a->pos || !a->unfinished || !a->work || !a->err)
        return ser_fail(-1, "ser_dec_select: null pointer");
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_dec_select: B=%d (1..65535)", a->B);
    if (a->V <= 1 || a->ldl < a->V || a->ldm < a->V) return ser_fail(-3, "ser_dec_select: V=%d, ldl=%lld, ldm=%lld (V >= 2, pitches >= V)", a->V, (long long)a->ldl, (long long)a->ldm);
    if (a->max_pos < 2 || a->ld_ids < a->max_pos || a->ld_margin < a->max_pos - 1)
        return ser_fail(-4, "ser_dec_select: max_pos=%d, ld_ids=%lld, ld_margin=%lld", a->max_pos, (long long)a->ld_ids, (long long)a->ld_margin);
    hipLaunchKernelGGL(dec_select_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_dec_select_v");
}
