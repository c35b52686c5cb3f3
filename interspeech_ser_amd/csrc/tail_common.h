// What the utterance-level tails share across files (pool.hip, xvector.hip): the float64 wave sum and the two-Linear tail kernel behind
// ser_cls_tail_v and ser_xvec_tail_v.
#pragma once
#include "ser_common.h"

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------- two Linears on B rows
// One block of 1024 threads per utterance.  Hidden unit j (wave v owns j = v, v + 16, ...): lane l adds pooled[b, c] P[j, c] over its
// columns 4 l + 256 i in ascending i (16-byte loads), then the butterfly, + bp[j]; the unit stays in LDS in float64.  Label n (same wave
// rule): lane l adds hid[k] C[n, k] over k = l, l + 64, ... ascending, the butterfly, + bc[n], one rounding at the store.
// EMB (ser_xvec_tail_v): the unit is rounded once to fp32, stored at emb[b, j], and the second Linear reads that fp32 value.  Without
// EMB the unit is never rounded (ser_cls_tail_v) and `emb` is not touched.
#define CLS_TAIL_MAX 2048
template <bool EMB>
__global__ __launch_bounds__(1024) void cls_tail_kernel(const float* __restrict__ pooled, int64_t ldp, const float* __restrict__ P,
                                                        const float* __restrict__ bp, const float* __restrict__ Cw, const float* __restrict__ bc,
                                                        float* __restrict__ out, int64_t ldo, int D, int proj, int n_labels,
                                                        float* __restrict__ emb, int64_t lde) {
    __shared__ double hid[CLS_TAIL_MAX];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* x = pooled + (int64_t)b * ldp;
    for (int j = wave; j < proj; j += 16) {
        const float* pr = P + (int64_t)j * D;
        double acc = 0.0;
        for (int c = lane * 4; c < D; c += 256) {
            const f32x4 v = *(const f32x4*)(x + c), u = *(const f32x4*)(pr + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fma((double)v[e], (double)u[e], acc);
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) {
            if constexpr (EMB) {
                const float e32 = (float)(acc + (double)bp[j]);
                emb[(int64_t)b * lde + j] = e32;
                hid[j] = (double)e32;
            } else {
                hid[j] = acc + (double)bp[j];
            }
        }
    }
    __syncthreads();
    for (int n = wave; n < n_labels; n += 16) {
        const float* cr = Cw + (int64_t)n * proj;
        double acc = 0.0;
        for (int k = lane; k < proj; k += 64) acc = fma(hid[k], (double)cr[k], acc);
        acc = wave_sum_f64(acc);
        if (lane == 0) out[(int64_t)b * ldo + n] = (float)(acc + (double)bc[n]);
    }
}
