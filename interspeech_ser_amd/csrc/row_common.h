// Where a row kernel starts (rowops.hip, deberta.hip): the wave-per-row pass "row kept in registers (D <= 2048, D % 4 == 0), two-pass
// mean / variance, LayerNorm tail".  (The run-time mode -> template dispatch they start from, ser_with_mode, is in ser_common.h.)
#pragma once
#include "ser_common.h"

// The conformer layers' sigmoid (GLU and swish): accurate expf and a true division, not gru_sigmoid's intrinsics.
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// A lane owns 4 consecutive columns of every 256-column chunk: f(i, c) for chunk i and the lane's first column c of it (may be >= D).
template <class F>
__device__ __forceinline__ void row_chunks(int lane, F&& f) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f(i, i * 256 + lane * 4);
}

// Row sources: the lane's 4 values at column c.
struct row_ptr {                                                  // a row in memory
    const float* p;
    __device__ __forceinline__ f32x4 operator()(int c) const { return *(const f32x4*)(p + c); }
};
struct row_sum3 {                                                 // (a + b) + c: RoBERTa's word + position + token type
    const float *a, *b, *c3;
    __device__ __forceinline__ f32x4 operator()(int c) const {
        return (*(const f32x4*)(a + c) + *(const f32x4*)(b + c)) + *(const f32x4*)(c3 + c);
    }
};

// v <- the row (zeros past D); returns its mean.
template <class SRC>
__device__ __forceinline__ float row_load(f32x4 (&v)[8], SRC src, int lane, int D) {
    float s = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) { v[i] = src(c); s += v[i][0] + v[i][1] + v[i][2] + v[i][3]; }
        else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    });
    return wave_sum(s) / (float)D;
}

__device__ __forceinline__ float row_rstd(const f32x4 (&v)[8], float mean, float eps, int lane, int D) {
    float q = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; q += d * d; }
        }
    });
    return rsqrtf(wave_sum(q) / (float)D + eps);
}

// The LayerNorm tail: y = (v - mean) * rstd * g + b, GELU if asked, zeros if !keep (a masked row), to the fp32 row `of` and / or the
// operand planes of row `oa` (either may be NULL).  Returns the lane's range_fold maximum of what went to f16 planes, for range_report.
template <int MODE>
__device__ __forceinline__ float row_ln_store(const f32x4 (&v)[8], float mean, float rstd, const float* __restrict__ g,
                                              const float* __restrict__ b, int gelu, bool keep, float* __restrict__ of,
                                              unsigned short* __restrict__ oa, int64_t plane, int lane, int D) {
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            const f32x4 gg = *(const f32x4*)(g + c), bb = *(const f32x4*)(b + c);
            f32x4 y;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = (v[i][j] - mean) * rstd * gg[j] + bb[j];
                y[j] = keep ? (gelu ? gelu_erf(t) : t) : 0.f;
            }
            if (of) *(f32x4*)(of + c) = y;
            if (oa) store_act4<MODE>(oa + c, plane, y[0], y[1], y[2], y[3]);
            if constexpr (mode_traits<MODE>::f16) { if (oa) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, y[j]); } }
        }
    });
    return ramax;
}
