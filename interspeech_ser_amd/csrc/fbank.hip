// w2v-BERT 2.0's front end (ser_hip.h a28): HF SeamlessM4TFeatureExtractor for one utterance alone -- Kaldi-style log-mel filter banks of
// 400-sample frames every 160, normalised per mel bin over the utterance's own frames and stacked `stride` frames to a row.  The reference
// has no counterpart: its speech script feeds raw samples (preprocess_speech.py:43-50).  Two plain-grid launches, float64 accumulation in a
// fixed order, one rounding to fp32 per stored value; no atomics: a row is a function of its own utterance alone.
#include "ser_common.h"

#define FB_WIN 400
#define FB_HOP 160
#define FB_BINS 257
#define FB_FR 8                               // frames per block
#define FB_SPAN (FB_WIN + (FB_FR - 1) * FB_HOP)
#define FB_THREADS 320                        // five waves: threads 0 .. 256 own one DFT bin each
#define FB_MAX_MELS 128
#define FB_MEL_FLOOR 1.192092955078125e-07

// Block = FB_FR frames of one utterance.  The frames' samples (times 2^15) sit in LDS once; each frame's mean is 32 strided partial sums
// merged in ascending order; z = the mean-free, pre-emphasised frame in float64; thread k < 257 accumulates X[k] of all FB_FR frames in
// ascending j (the 16-byte table entry of (j, k) is read once per FB_FR frames); then the power spectrum, the mel rows over their own bins,
// the floor and the log, rounded once.
__global__ __launch_bounds__(FB_THREADS) void fbank_frames_kernel(ser_fbank_args a) {
    __shared__ float xs[FB_SPAN];
    __shared__ double part[FB_FR][32];
    __shared__ double mean[FB_FR];
    __shared__ double z[FB_FR][FB_WIN];
    __shared__ double pw[FB_FR][FB_BINS + 1];
    const int b = blockIdx.y, f0 = blockIdx.x * FB_FR, tid = threadIdx.x;
    const int m0 = a.mel_offs[b], F = a.mel_offs[b + 1] - m0;
    if (f0 >= F) return;                                                   // block-uniform
    const int64_t s0 = a.sample_offs[b], len = a.sample_offs[b + 1] - s0;
    for (int i = tid; i < FB_SPAN; i += FB_THREADS) {
        const int64_t s = (int64_t)f0 * FB_HOP + i;
        xs[i] = s < len ? a.wav[s0 + s] * 32768.0f : 0.f;                  // (frames at or past F are never stored)
    }
    __syncthreads();
    if (tid < FB_FR * 32) {
        const int f = tid >> 5, i = tid & 31;
        double s = 0.0;
        for (int j = i; j < FB_WIN; j += 32) s += (double)xs[f * FB_HOP + j];
        part[f][i] = s;
    }
    __syncthreads();
    if (tid < FB_FR) {
        double s = 0.0;
        for (int i = 0; i < 32; ++i) s += part[tid][i];
        mean[tid] = s / (double)FB_WIN;
    }
    __syncthreads();
    for (int i = tid; i < FB_FR * FB_WIN; i += FB_THREADS) {
        const int f = i / FB_WIN, j = i - f * FB_WIN;
        const double y = (double)xs[f * FB_HOP + j] - mean[f];
        z[f][j] = j ? y - 0.97 * ((double)xs[f * FB_HOP + j - 1] - mean[f]) : y * (1.0 - 0.97);
    }
    __syncthreads();
    if (tid < FB_BINS) {
        double re[FB_FR], im[FB_FR];
#pragma unroll
        for (int f = 0; f < FB_FR; ++f) { re[f] = 0.0; im[f] = 0.0; }
        const double2* tp = (const double2*)a.dft + tid;
#pragma unroll 2
        for (int j = 0; j < FB_WIN; ++j) {
            const double2 c = tp[(int64_t)j * FB_BINS];
#pragma unroll
            for (int f = 0; f < FB_FR; ++f) {
                const double x = z[f][j];
                re[f] = fma(x, c.x, re[f]);
                im[f] = fma(x, c.y, im[f]);
            }
        }
#pragma unroll
        for (int f = 0; f < FB_FR; ++f) pw[f][tid] = re[f] * re[f] + im[f] * im[f];
    }
    __syncthreads();
    for (int i = tid; i < FB_FR * a.n_mels; i += FB_THREADS) {
        const int f = i / a.n_mels, m = i - f * a.n_mels;
        if (f0 + f >= F) continue;
        const double* mr = a.melw + (int64_t)m * FB_BINS;
        const int k0 = a.mel_range[2 * m], k1 = a.mel_range[2 * m + 1];
        double acc = 0.0;
        for (int k = k0; k < k1; ++k) acc = fma(mr[k], pw[f][k], acc);
        a.work[(int64_t)(m0 + f0 + f) * a.n_mels + m] = (float)log(acc > FB_MEL_FLOOR ? acc : FB_MEL_FLOOR);
    }
}

// Block = (utterance, 16 mel bins): thread (bin, part) sums its bin over frames part, part + 16, ... in ascending order, the 16 parts merge
// in ascending order -- mean first, then the squared deviations (two passes: the unbiased variance HF takes) -- and the block writes the
// normalised values of its bins into the stacked rows.
__global__ __launch_bounds__(256) void fbank_norm_kernel(ser_fbank_args a) {
    __shared__ double red[16][17];
    __shared__ double stat[16][2];
    const int b = blockIdx.x, tid = threadIdx.x, bin = tid & 15, part = tid >> 4;
    const int m = blockIdx.y * 16 + bin;
    const int m0 = a.mel_offs[b], F = a.mel_offs[b + 1] - m0;
    const int row0 = a.frame_offs[b], T = a.frame_offs[b + 1] - row0;
    const bool live = m < a.n_mels;
    const float* src = a.work + (int64_t)m0 * a.n_mels + (live ? m : 0);
    double s = 0.0;
    if (live) for (int f = part; f < F; f += 16) s += (double)src[(int64_t)f * a.n_mels];
    red[bin][part] = s;
    __syncthreads();
    if (part == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += red[bin][i];
        stat[bin][0] = t / (double)F;
    }
    __syncthreads();
    const double mu = stat[bin][0];
    s = 0.0;
    if (live) for (int f = part; f < F; f += 16) { const double d = (double)src[(int64_t)f * a.n_mels] - mu; s = fma(d, d, s); }
    __syncthreads();
    red[bin][part] = s;
    __syncthreads();
    if (part == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += red[bin][i];
        stat[bin][1] = 1.0 / sqrt(t / (double)(F - 1) + 1e-7);
    }
    __syncthreads();
    if (!live) return;
    const double inv = stat[bin][1];
    for (int f = part; f < T * a.stride; f += 16) {
        const int row = f / a.stride, sidx = f - row * a.stride;
        a.out[(int64_t)(row0 + row) * a.ldo + sidx * a.n_mels + m] = (float)(((double)src[(int64_t)f * a.n_mels] - mu) * inv);
    }
}

extern "C" int ser_fbank_v(const ser_fbank_args* a, void* stream) {
    if (!a || !a->wav || !a->sample_offs || !a->mel_offs || !a->frame_offs || !a->dft || !a->melw || !a->mel_range || !a->work || !a->out)
        return ser_fail(-1, "ser_fbank: null pointer");
    if (a->B <= 0 || a->B > 65535 || a->max_mel_frames <= 0) return ser_fail(-2, "ser_fbank: bad B=%d / max_mel_frames=%d", a->B, a->max_mel_frames);
    if (a->n_mels < 1 || a->n_mels > FB_MAX_MELS || a->stride < 1 || a->stride > 4 || a->ldo < (int64_t)a->stride * a->n_mels)
        return ser_fail(-2, "ser_fbank: n_mels=%d (1..%d) / stride=%d (1..4) / ldo=%lld unsupported", a->n_mels, FB_MAX_MELS, a->stride, (long long)a->ldo);
    hipLaunchKernelGGL(fbank_frames_kernel, dim3((a->max_mel_frames + FB_FR - 1) / FB_FR, a->B), dim3(FB_THREADS), 0, (hipStream_t)stream, *a);
    if (int rc = ser_check_launch("ser_fbank")) return rc;
    hipLaunchKernelGGL(fbank_norm_kernel, dim3(a->B, (a->n_mels + 15) / 16), dim3(256), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_fbank");
}
