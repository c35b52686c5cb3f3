// a5r  ser_resample: the resampling half of librosa.load(path, sr=16000) (preprocess_speech.py:47) for a ragged, mixed-rate batch.
// Kaiser (beta 14) polyphase FIR, the filter of scipy.signal.resample_poly (parity with librosa's soxr_hq unpinned); ser_hip.h states
// the arithmetic.  fp32 samples x float64 coefficients, float64 accumulation in ascending input index, one rounding at the store.
#include "ser_common.h"

#define RS_TILE SER_RESAMPLE_TILE       // output samples of one block
#define RS_SPAN 6400                    // floats of LDS for the tile's input span: RS_TILE * down / up + 2 * half / up + 2 <= 6 266 up to 96 kHz

// ceil(a / b) for b > 0 and any sign of a
__device__ __forceinline__ int rs_cdiv(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// Block (tile, utterance).  With q = m * down + half, output m sums x[j] * h[q - j * up] over ceil((q - 2 half) / up) <= j <= floor(q / up),
// clipped to [0, n).  Everything per lane is 32-bit and relative to the tile: q = jb * up + r with jb = floor(q0 / up) of the tile's
// first output and r = q0 % up + i * down < up + RS_TILE * down.  Consecutive lanes walk the phases (m * down) % up, so one tap of a wave
// reads coefficients inside a window of `up` doubles (L2-resident bank, <= 100 KB), and samples from LDS.  A tile whose span does not
// fit RS_SPAN (down / up > 6: rates above 96 kHz) reads its samples from global memory instead: same sums, same order.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ wav, const int64_t* __restrict__ in_offs,
                                                       const int64_t* __restrict__ out_offs, const int32_t* __restrict__ ups,
                                                       const int32_t* __restrict__ downs, const int32_t* __restrict__ halves,
                                                       const int64_t* __restrict__ bank_offs, const double* __restrict__ bank,
                                                       float* __restrict__ out) {
    __shared__ float sx[RS_SPAN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t o0 = out_offs[b], n_out = out_offs[b + 1] - o0;
    const int64_t m0 = (int64_t)blockIdx.x * RS_TILE;
    if (m0 >= n_out) return;
    const int64_t i0 = in_offs[b], n = in_offs[b + 1] - i0;
    const int cnt = (int)((n_out - m0 < RS_TILE) ? n_out - m0 : RS_TILE);
    const float* x = wav + i0;
    float* y = out + o0 + m0;
    const int up = ups[b], down = downs[b];
    if (up == 1 && down == 1) {                                   // a 16 kHz utterance of a mixed batch: a copy, bit for bit
        for (int i = tid; i < cnt; i += 256) y[i] = (m0 + i < n) ? x[m0 + i] : 0.f;
        return;
    }
    const int half = halves[b];
    const double* h = bank + bank_offs[b];
    const int64_t q0 = m0 * down + half;
    const int64_t jb = q0 / up;
    const int r0 = (int)(q0 - jb * up);
    // input span of the tile, absolute then clipped: [s0, s1]
    int64_t s0 = jb + rs_cdiv(r0 - 2 * half, up), s1 = jb + (r0 + (cnt - 1) * down) / up;
    if (s0 < 0) s0 = 0;
    if (s1 > n - 1) s1 = n - 1;
    const int64_t span = s1 - s0 + 1;                              // <= 0: the tile lies wholly beyond the samples (zeros)
    const bool staged = span <= RS_SPAN;
    if (staged) {
        for (int i = tid; i < (int)span; i += 256) sx[i] = x[s0 + i];
        __syncthreads();
    }
    const int lo_clip = (int)(s0 - jb), hi_clip = (int)(s1 - jb);                  // relative to jb
    for (int i = tid; i < cnt; i += 256) {
        const int r = r0 + i * down;
        int jl = rs_cdiv(r - 2 * half, up), jh = r / up;           // relative to jb
        if (jl < lo_clip) jl = lo_clip;
        if (jh > hi_clip) jh = hi_clip;
        int k = r - jl * up;                                       // coefficient of the first (lowest) sample; steps down by up
        double acc = 0.0;
        if (staged) {
            const float* p = sx + (jl - lo_clip);
            for (int j = jl; j <= jh; ++j, k -= up) acc += (double)(*p++) * h[k];
        } else {
            const float* p = x + (jb + jl);
            for (int j = jl; j <= jh; ++j, k -= up) acc += (double)(*p++) * h[k];
        }
        y[i] = (float)acc;
    }
}

extern "C" int ser_resample_v(const ser_resample_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_resample: null pointer");
    if (!a->wav || !a->in_offs || !a->out_offs || !a->up || !a->down || !a->half || !a->bank_off || !a->bank || !a->out)
        return ser_fail(-1, "ser_resample: null pointer");
    if (a->B <= 0 || a->B > 65535 || a->total_in <= 0 || a->total_out <= 0 || a->max_out <= 0 || a->max_out > a->total_out)
        return ser_fail(-2, "ser_resample: bad B / sample totals / longest output");
    const int64_t tiles = (a->max_out + RS_TILE - 1) / RS_TILE;
    if (tiles > 0x7fffffff) return ser_fail(-2, "ser_resample: bad B / sample totals / longest output");
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, a->B), dim3(256), 0, (hipStream_t)stream, a->wav, a->in_offs, a->out_offs,
                       a->up, a->down, a->half, a->bank_off, a->bank, a->out);
    return ser_check_launch("ser_resample");
}
