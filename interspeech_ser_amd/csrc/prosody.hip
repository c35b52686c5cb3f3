// The prosody stream's own kernels (ser_hip.h a26): the NS3 20-bin log-mel with melspec_linear behind it (ser_prosody_mel_v), the first
// quantizer's code lookup (ser_fvq_v) and the fp32 rows -> operand planes pass with the ReLU of the feed-forward block (ser_act_rows_v).
// The reference computes all of this on the CPU, one file at a time (preprocessing/preprocess_ns3_prosody.py:41-60, src/ns3/melspec.py,
// src/ns3/quantize/fvq.py).  No atomics on float data: a frame's result is a function of its own utterance alone.
#include "row_common.h"

#define PM_HOP 200
#define PM_WIN 800                            // Hann window; n_fft = 1024 only sets the bin spacing
#define PM_LEAD 300                           // frame t reads samples 200 t - 300 .. 200 t + 499 of the zero-padded utterance
#define PM_FR 16                              // frames per block: 4 per wave
#define PM_SPAN (PM_WIN + (PM_FR - 1) * PM_HOP)
#define PM_MAX_BINS 64                        // one lane per bin
#define PM_MAX_MELS 32

// Wave w accumulates frames 4 w .. 4 w + 3 of the block, lane = DFT bin: X_f[k] = sum_j x_f[j] * (w[j] cos, -w[j] sin)(k, j) in float64
// and ascending j.  The samples of the block's frames (reflected at both ends of the utterance) sit in LDS once; the 16-byte table entry
// of (j, bin) is read once per four frames.  Then |X| with its 1e-9, the mel rows, the clamp and the log in float64 (one rounding at the
// store), and melspec_linear (+ the position-0 vector, folded into its bias on the host) in fp32 FMAs from the rounded log-mel.
__global__ __launch_bounds__(256) void prosody_mel_kernel(ser_prosody_mel_args a) {
    __shared__ float xs[PM_SPAN];
    __shared__ double mag[PM_FR][PM_MAX_BINS];
    __shared__ float melv[PM_FR][PM_MAX_MELS];
    const int b = blockIdx.y, f0 = blockIdx.x * PM_FR, tid = threadIdx.x;
    const int row0 = a.frame_offs[b], T = a.frame_offs[b + 1] - row0;
    if (f0 >= T) return;                                                   // block-uniform
    const int64_t s0 = a.sample_offs[b];
    const int64_t len = a.sample_offs[b + 1] - s0, lp = (int64_t)T * PM_HOP;  // lp: the length after the zero padding
    for (int i = tid; i < PM_SPAN; i += 256) {
        int64_t s = (int64_t)f0 * PM_HOP - PM_LEAD + i;
        if (s < 0) s = -s;
        if (s >= lp) s = 2 * (lp - 1) - s;
        xs[i] = (s >= 0 && s < len) ? a.wav[s0 + s] : 0.f;                 // (frames at or past T read zeros and are never stored)
    }
    __syncthreads();
    const int bin = tid & 63, fw = (tid >> 6) * 4;
    double re[4] = {0.0, 0.0, 0.0, 0.0}, im[4] = {0.0, 0.0, 0.0, 0.0};
    if (bin < a.n_bins) {
        const double2* tp = (const double2*)a.dft + bin;
        const float* xf = xs + fw * PM_HOP;
#pragma unroll 2
        for (int j = 0; j < PM_WIN; ++j) {
            const double2 c = tp[(int64_t)j * a.n_bins];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const double x = (double)xf[f * PM_HOP + j];
                re[f] = fma(x, c.x, re[f]);
                im[f] = fma(x, c.y, im[f]);
            }
        }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) mag[fw + f][bin] = bin < a.n_bins ? sqrt(re[f] * re[f] + im[f] * im[f] + 1e-9) : 0.0;
    __syncthreads();
    const double clip = (double)1e-5f;                                     // torch.clamp(min=1e-5) on an fp32 tensor
    for (int i = tid; i < PM_FR * a.n_mels; i += 256) {
        const int f = i / a.n_mels, m = i - f * a.n_mels;
        const float* mr = a.mel + (int64_t)m * a.n_bins;
        double acc = 0.0;
        for (int k = 0; k < a.n_bins; ++k) acc = fma((double)mr[k], mag[f][k], acc);
        const float v = (float)log(acc > clip ? acc : clip);
        melv[f][m] = v;
        if (a.mel_out && f0 + f < T) a.mel_out[(int64_t)(row0 + f0 + f) * a.n_mels + m] = v;
    }
    if (!a.out) return;
    __syncthreads();
    for (int d = tid; d < a.D; d += 256) {
        float acc[PM_FR];
        const float bias = a.lin_b[d];
#pragma unroll
        for (int f = 0; f < PM_FR; ++f) acc[f] = bias;
        const float* wr = a.lin_w + (int64_t)d * a.n_mels;
        for (int m = 0; m < a.n_mels; ++m) {
            const float w = wr[m];
#pragma unroll
            for (int f = 0; f < PM_FR; ++f) acc[f] = fmaf(w, melv[f][m], acc[f]);
        }
#pragma unroll
        for (int f = 0; f < PM_FR; ++f)
            if (f0 + f < T) a.out[(int64_t)(row0 + f0 + f) * a.ldo + d] = acc[f];
    }
}

extern "C" int ser_prosody_mel_v(const ser_prosody_mel_args* a, void* stream) {
    if (!a || !a->wav || !a->sample_offs || !a->frame_offs || !a->dft || !a->mel || (!a->mel_out && !a->out))
        return ser_fail(-1, "ser_prosody_mel: null pointer");
    if (a->out && (!a->lin_w || !a->lin_b || a->D <= 0 || a->ldo < a->D)) return ser_fail(-1, "ser_prosody_mel: out needs lin_w, lin_b, D >= 1, ldo >= D");
    if (a->B <= 0 || a->B > 65535 || a->max_frames <= 0) return ser_fail(-2, "ser_prosody_mel: bad B=%d / max_frames=%d", a->B, a->max_frames);
    if (a->n_bins < 1 || a->n_bins > PM_MAX_BINS || a->n_mels < 1 || a->n_mels > PM_MAX_MELS)
        return ser_fail(-2, "ser_prosody_mel: n_bins=%d (1..%d) / n_mels=%d (1..%d) unsupported", a->n_bins, PM_MAX_BINS, a->n_mels, PM_MAX_MELS);
    hipLaunchKernelGGL(prosody_mel_kernel, dim3((a->max_frames + PM_FR - 1) / PM_FR, a->B), dim3(256), 0, (hipStream_t)stream, *a);
    return ser_check_launch("ser_prosody_mel");
}

// ------------------------------------------------------------------------------------------------------------- code lookup
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Wave per row.  z_e = W_in z + b_in (float64 partial sums per lane, butterfly), e = z_e / max(|z_e|, 1e-12); lane l scans the codes
// l, l + 64, ... in ascending order for the two smallest |e|^2 - 2 e.c + |c|^2 (float64), the wave merges them with the lower index on
// equal distances; then the chosen row of the table is copied out.
template <int MODE>
__global__ __launch_bounds__(256) void fvq_kernel(ser_fvq_args a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int D = a.D;
    const float* zr = a.z + (int64_t)row * a.ldz;
    double ze[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            const f32x4 v = *(const f32x4*)(zr + c);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const f32x4 w = *(const f32x4*)(a.w_in + (int64_t)k * D + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) ze[k] = fma((double)v[j], (double)w[j], ze[k]);
            }
        }
    });
    double n2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { ze[k] = wave_sum_f64(ze[k]) + (double)a.b_in[k]; n2 = fma(ze[k], ze[k], n2); }
    const bool bad = !(n2 < (double)INFINITY);                              // a NaN or an Inf among the eight
    const double inv = 1.0 / fmax(sqrt(n2), 1e-12);
    double ee = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { ze[k] *= inv; ee = fma(ze[k], ze[k], ee); }
    double d1 = (double)INFINITY, d2 = (double)INFINITY;
    int i1 = 0x7fffffff;
    for (int n = lane; n < a.n_codes; n += 64) {
        const f32x4 c0 = *(const f32x4*)(a.codes + (int64_t)n * 8), c1 = *(const f32x4*)(a.codes + (int64_t)n * 8 + 4);
        double dot = 0.0, cc = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dot = fma(ze[k], (double)c0[k], dot); cc = fma((double)c0[k], (double)c0[k], cc);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dot = fma(ze[4 + k], (double)c1[k], dot); cc = fma((double)c1[k], (double)c1[k], cc);
        }
        const double d = ee - 2.0 * dot + cc;
        if (d < d1) { d2 = d1; d1 = d; i1 = n; }
        else if (d < d2) d2 = d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od1 = __shfl_xor(d1, o, 64), od2 = __shfl_xor(d2, o, 64);
        const int oi1 = __shfl_xor(i1, o, 64);
        d2 = fmin(fmin(d2, od2), fmax(d1, od1));
        if (od1 < d1 || (od1 == d1 && oi1 < i1)) { d1 = od1; i1 = oi1; }
    }
    const int idx = (i1 >= 0 && i1 < a.n_codes) ? i1 : 0;                  // (no comparison holds against a NaN: row 0, and the error word)
    if (lane == 0) {
        a.idx[row] = idx;
        if (a.gap) a.gap[row] = (float)(d2 - d1);
        if (bad && a.err) atomicOr(a.err, 1u);
    }
    const float* tr = a.table + (int64_t)idx * a.ld_table;
    float* of = a.out_f32 ? a.out_f32 + (int64_t)row * a.ldo_f32 : nullptr;
    unsigned short* oa = a.out_act ? (unsigned short*)a.out_act + (int64_t)row * a.ldo_act : nullptr;
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            const f32x4 v = *(const f32x4*)(tr + c);
            if (of) *(f32x4*)(of + c) = v;
            if (oa) {
                store_act4<MODE>(oa + c, a.out_plane_stride, v[0], v[1], v[2], v[3]);
                if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
            }
        }
    });
    if constexpr (mode_traits<MODE>::f16) range_report(a.range_flag, ramax);
}

extern "C" int ser_fvq_v(const ser_fvq_args* a, void* stream) {
    if (!a || !a->z || !a->w_in || !a->b_in || !a->codes || !a->table || !a->idx || (!a->out_f32 && !a->out_act))
        return ser_fail(-1, "ser_fvq: null pointer");
    if (a->D % 4 || a->D > 2048 || a->D <= 0 || a->rows <= 0 || a->n_codes < 1) return ser_fail(-2, "ser_fvq: D=%d rows=%d n_codes=%d unsupported", a->D, a->rows, a->n_codes);
    if (a->code_dim != 8) return ser_fail(-2, "ser_fvq: code_dim=%d (8: the factorized quantizers' codebook_dim)", a->code_dim);
    if ((a->ldz % 4) || (a->ld_table % 4) || a->ld_table < a->D || (a->out_f32 && a->ldo_f32 % 4) || (a->out_act && a->ldo_act % 4))
        return ser_fail(-3, "ser_fvq: pitches must be multiples of 4");
    dim3 grid((a->rows + 3) / 4), block(256);
    const int mode = a->out_act ? a->mode : SER_MODE_BF16;                  // (no planes: any instantiation)
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(mode, [&](auto M) {
            hipLaunchKernelGGL(fvq_kernel<M()>, grid, block, 0, (hipStream_t)stream, *a);
        }))
        return ser_fail(-4, "ser_fvq: bad mode %d", mode);
    return ser_check_launch("ser_fvq");
}

// ------------------------------------------------------------------------------------------------ fp32 rows -> operand planes
// Wave per row on the row skeleton: max(x, 0) when asked, to row out_rowmap[m] (or m) of the operand planes, with the range guard.
template <int MODE>
__global__ __launch_bounds__(256) void act_rows_kernel(const float* __restrict__ x, int64_t ldx, unsigned short* __restrict__ oa, int64_t ldoa,
                                                       int64_t plane, const int32_t* __restrict__ rowmap, int relu, int rows, int D,
                                                       uint32_t* __restrict__ rflag) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * ldx;
    unsigned short* orow = oa + (int64_t)(rowmap ? rowmap[row] : row) * ldoa;
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            f32x4 v = *(const f32x4*)(xr + c);
            if (relu) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];    // (a NaN stays a NaN: the guard sees it)
            }
            store_act4<MODE>(orow + c, plane, v[0], v[1], v[2], v[3]);
            if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
        }
    });
    if constexpr (mode_traits<MODE>::f16) range_report(rflag, ramax);
}

extern "C" int ser_act_rows_v(const ser_act_rows_args* a, void* stream) {
    if (!a || !a->x || !a->out_act) return ser_fail(-1, "ser_act_rows: null pointer");
    if (a->D % 4 || a->D > 2048 || a->D <= 0 || a->rows <= 0) return ser_fail(-2, "ser_act_rows: D=%d rows=%d unsupported", a->D, a->rows);
    if ((a->ldx % 4) || (a->ldo_act % 4)) return ser_fail(-3, "ser_act_rows: pitches must be multiples of 4");
    if (a->relu != 0 && a->relu != 1) return ser_fail(-2, "ser_act_rows: relu=%d must be 0 or 1", a->relu);
    dim3 grid((a->rows + 3) / 4), block(256);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(act_rows_kernel<M()>, grid, block, 0, (hipStream_t)stream, a->x, a->ldx, (unsigned short*)a->out_act, a->ldo_act,
                               a->out_plane_stride, a->out_rowmap, a->relu, a->rows, a->D, a->range_flag);
        }))
        return ser_fail(-4, "ser_act_rows: bad mode %d", a->mode);
    return ser_check_launch("ser_act_rows");
}
