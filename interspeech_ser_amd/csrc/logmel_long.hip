// Whisper long-form features (ser_logmel_long_v, ser_mel_window_v; include/ser_hip.h "a37").
//
// HF's long-form call runs WhisperFeatureExtractor over the WHOLE file (truncation=False): one reflect pad of 200 samples about the
// file's own first and last sample, F = len // 160 kept frames (the STFT's last frame is dropped), and ONE max - 8 floor over the file's
// F frames (feature_extraction_whisper.py:128-130).  A 30 s window of the seek loop is a slice [seek, seek + nf) of that, zero-padded to
// 3000 frames (generation_whisper.py _get_input_segment).  ser_logmel_whisper (logmel.hip) reflects at sample 480000 and takes a
// per-window maximum, so it cannot make these windows; its kernels stay as they are and this file shares their constants and the
// twiddle / Hann table of ser_logmel_init (logmel_common.h).
//
//   logmel_long_kernel   one block per entry of a tile table (file, first frame): the fp64-MFMA DFT tile of logmel.hip over 32 frames of
//                        one file -> raw log10 mel rows [n_mels][pitch_b] at the file's base, and the tile's maximum over its frames
//                        < F_b into the tile's own slot
//   logmel_long_max      one block per file: the maximum of the file's slots (max is exact and commutes: a file alone and in a batch
//                        gives the same bits; the loop order is fixed anyway)
//   logmel_long_finish   (max(x, file max - 8) + 4) / 4 in place over [n_mels][pitch_b]
//   mel_window_kernel    out[b, m, 0:nf] = file row m at [seek, seek + nf), out[b, m, nf:3000] = +0.0f
#include "logmel_common.h"

__device__ __forceinline__ int lml_frames(int64_t len) { return (int)(len / LM_HOP); }
__device__ __forceinline__ int lml_pitch(int F) { return (F + 3) & ~3; }

// The tile body is logmel_kernel's (same operand lane maps, same order of every sum): what differs is where a frame comes from (the
// file's own reflect pad; frames >= F_b are zeros), where a row goes (pitch_b) and which frames enter the maximum (those < F_b).
__global__ __launch_bounds__(256, 3) void logmel_long_kernel(const float* __restrict__ wav, const int64_t* __restrict__ offs,
                                                          const int32_t* __restrict__ tiles, const int64_t* __restrict__ bases,
                                                          const float* __restrict__ mel, int n_mels, int B,
                                                          const double2* __restrict__ tw, float* __restrict__ out,
                                                          float* __restrict__ tmax) {
    __shared__ __attribute__((aligned(16))) float lds[LM_FR * LM_XP];       // windowed frames, later the power spectrum
    const int b = tiles[2 * blockIdx.x], f0 = tiles[2 * blockIdx.x + 1], tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    if (b < 0 || b >= B || f0 < 0) return;                   // block-uniform: a table that does not belong to this batch launches nothing
    const int64_t s0 = offs[b];
    const int64_t len = offs[b + 1] - s0;
    const int F = lml_frames(len), pitch = lml_pitch(F);
    if (f0 >= F || len < LM_NFFT / 2 + 1) return;
    const float* hann = (const float*)((const char*)tw + LM_TW_BYTES);
    for (int i = tid; i < LM_FR * LM_NFFT; i += 256) {
        const int f = i / LM_NFFT, n = i - f * LM_NFFT;
        float x = 0.f;
        if (f0 + f < F) {                                    // s <= 160 (F - 1) + 199 < len + 40: one reflection lands inside the file
            int64_t s = (int64_t)(f0 + f) * LM_HOP - LM_NFFT / 2 + n;
            if (s < 0) s = -s;
            if (s >= len) s = 2 * (len - 1) - s;
            x = wav[s0 + s];
        }
        lds[f * LM_XP + n] = x * hann[n];
    }
    __syncthreads();

    constexpr int NB = 4;                                    // column blocks per wave (wave 0 uses all four, the others three)
    const int nb = wave == 0 ? 4 : 3;
    const int li = lane & 15, kk = lane >> 4;
    f64x4 re[2][NB], im[2][NB];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int q = 0; q < NB; ++q) { re[rt][q] = (f64x4){0.0, 0.0, 0.0, 0.0}; im[rt][q] = (f64x4){0.0, 0.0, 0.0, 0.0}; }
    const double2* twl = tw + (size_t)kk * (LM_BB * 16) + wave * 16 + li;       // + step * 4 rows, + q * 64 columns
    double a0 = (double)lds[li * LM_XP + kk], a1 = (double)lds[(16 + li) * LM_XP + kk];
    double2 c[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) c[q] = (q < nb) ? twl[q * 64] : make_double2(0.0, 0.0);
    for (int st = 0; st < LM_NFFT / 4; ++st) {
        const int sn = st + 1 < LM_NFFT / 4 ? st + 1 : st;
        const double n0 = (double)lds[li * LM_XP + 4 * sn + kk];
        const double n1 = (double)lds[(16 + li) * LM_XP + 4 * sn + kk];
        double2 cn[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q)
            cn[q] = (q < nb) ? twl[(size_t)sn * 4 * (LM_BB * 16) + q * 64] : make_double2(0.0, 0.0);
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            if (q < nb) {                                    // wave-uniform
                re[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c[q].x, re[0][q], 0, 0, 0);
                im[0][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, c[q].y, im[0][q], 0, 0, 0);
                re[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c[q].x, re[1][q], 0, 0, 0);
                im[1][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, c[q].y, im[1][q], 0, 0, 0);
            }
        }
        a0 = n0; a1 = n1;
#pragma unroll
        for (int q = 0; q < NB; ++q) c[q] = cn[q];
    }
    __syncthreads();                                         // every wave is done with the frames: reuse the LDS
    float* pw = lds;                                         // [LM_FR][LM_PP]
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int q = 0; q < NB; ++q)
            if (q < nb) {
                const int bin = (wave + 4 * q) * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float fr = (float)re[rt][q][r], fi = (float)im[rt][q][r];
                    pw[(rt * 16 + kk + 4 * r) * LM_PP + bin] = fr * fr + fi * fi;
                }
            }
    __syncthreads();
    // mel projection + log10: thread = (mel, half of the frames); 16 consecutive frames of one mel row are 64 contiguous bytes
    float lmax = -INFINITY;
    for (int m = tid & 127; m < n_mels; m += 128) {
        const int fb = (tid >> 7) * (LM_FR / 2);
        float acc[LM_FR / 2];
#pragma unroll
        for (int f = 0; f < LM_FR / 2; ++f) acc[f] = 0.f;
        for (int k0 = 0; k0 < LM_BINS; k0 += 8) {
            float w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = (k0 + u < LM_BINS) ? mel[(k0 + u) * n_mels + m] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int f = 0; f < LM_FR / 2; ++f) acc[f] = fmaf(w[u], pw[(fb + f) * LM_PP + k0 + u], acc[f]);
        }
        float* orow = out + bases[b] + (int64_t)m * pitch + f0 + fb;
#pragma unroll
        for (int f4 = 0; f4 < LM_FR / 2; f4 += 4) {
            if (f0 + fb + f4 < pitch) {                      // pitch_b is a multiple of 4: a quad lies inside the row or behind it
                f32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // the 1e-10 guard's logarithm is the constant -10, as in logmel_kernel: silence must be exactly (-10 + 4) / 4
                    v[j] = acc[f4 + j] > 1e-10f ? log10f(acc[f4 + j]) : -10.0f;
                    if (f0 + fb + f4 + j < F) lmax = fmaxf(lmax, v[j]);      // the pitch's pad (zero frames: -10) is not the file's
                }
                *(f32x4*)(orow + f4) = v;
            }
        }
    }
    // tile maximum -> its own slot: no atomics, no reset
    __shared__ float wmax[4];
    lmax = wave_max(lmax);
    if ((tid & 63) == 0) wmax[tid >> 6] = lmax;
    __syncthreads();
    if (tid == 0) tmax[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
}

// files [B][4]: F_b, pitch_b, the file's first slot, its number of slots
__global__ __launch_bounds__(256) void logmel_long_max(const float* __restrict__ tmax, const int32_t* __restrict__ files, int n_tiles,
                                                        float* __restrict__ fmax) {
    const int b = blockIdx.x;
    int first = files[4 * b + 2], n = files[4 * b + 3];
    if (first < 0 || n < 0 || first > n_tiles) { first = 0; n = 0; }
    if (n > n_tiles - first) n = n_tiles - first;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, tmax[first + i]);
    __shared__ float red[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) fmax[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void logmel_long_finish(float* __restrict__ out, const int64_t* __restrict__ offs,
                                                           const int64_t* __restrict__ bases, const float* __restrict__ fmax, int n_mels) {
    const int b = blockIdx.y;
    const int pitch = lml_pitch(lml_frames(offs[b + 1] - offs[b]));
    const int64_t per = (int64_t)n_mels * pitch;                     // a multiple of 4
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= per) return;
    const float mx = fmax[b];
    f32x4* o = (f32x4*)(out + bases[b] + i);
    f32x4 v = *o;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (fmaxf(v[j], mx - 8.0f) + 4.0f) / 4.0f;
    *o = v;
}

// rows [B][5] int64: base, pitch, F, seek, nf.  grid (ceil(750 / 256), n_mels, B); a thread writes one quad of a 3000-frame row.
__global__ __launch_bounds__(256) void mel_window_kernel(const float* __restrict__ src, const int64_t* __restrict__ rows,
                                                          float* __restrict__ out, int n_mels) {
    const int b = blockIdx.z, m = blockIdx.y;
    const int t4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (t4 >= LM_FRAMES) return;
    const int64_t base = rows[5 * b], pitch = rows[5 * b + 1], F = rows[5 * b + 2], seek = rows[5 * b + 3];
    int64_t nf = rows[5 * b + 4];
    if (seek < 0 || seek > F) nf = 0;                        // the launcher refused such a row on the host's copy: never read outside the file
    else if (nf > F - seek) nf = F - seek;
    const float* row = src + base + (int64_t)m * pitch + seek;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (t4 + j < nf) ? row[t4 + j] : 0.0f;
    *(f32x4*)(out + ((int64_t)b * n_mels + m) * LM_FRAMES + t4) = v;
}

extern "C" int ser_logmel_long_v(const ser_logmel_long_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_logmel_long: null arguments");
    if (!a->wav || !a->sample_offs || !a->sample_offs_host || !a->mel || !a->out || !a->bases || !a->tiles || !a->files || !a->table ||
        !a->scratch)
        return ser_fail(-1, "ser_logmel_long: null pointer");
    if (a->B <= 0 || a->n_mels <= 0 || a->B > 65535) return ser_fail(-1, "ser_logmel_long: B = %d, n_mels = %d", a->B, a->n_mels);
    int64_t tiles = 0, max_pitch = 0;
    for (int b = 0; b < a->B; ++b) {
        const int64_t len = a->sample_offs_host[b + 1] - a->sample_offs_host[b];
        if (len < LM_NFFT / 2 + 1)
            return ser_fail(-1, "ser_logmel_long: file %d has %lld samples (the reflect pad of 200 needs at least 201)", b, (long long)len);
        if (len / LM_HOP > INT32_MAX - 64) return ser_fail(-1, "ser_logmel_long: file %d is too long", b);
        const int64_t F = len / LM_HOP, pitch = (F + 3) & ~(int64_t)3;
        tiles += (F + LM_FR - 1) / LM_FR;
        if (pitch > max_pitch) max_pitch = pitch;
    }
    if (tiles != a->n_tiles || tiles > INT32_MAX)
        return ser_fail(-1, "ser_logmel_long: n_tiles = %d, the lengths give %lld", a->n_tiles, (long long)tiles);
    if (max_pitch != a->max_pitch) return ser_fail(-1, "ser_logmel_long: max_pitch = %d, the lengths give %lld", a->max_pitch, (long long)max_pitch);
    hipStream_t s = (hipStream_t)stream;
    const double2* tw = (const double2*)a->table;
    float* tmax = a->scratch;
    float* fmax = a->scratch + a->n_tiles;
    hipLaunchKernelGGL(logmel_long_kernel, dim3((unsigned)a->n_tiles), dim3(256), 0, s, a->wav, a->sample_offs, a->tiles, a->bases, a->mel,
                       a->n_mels, a->B, tw, a->out, tmax);
    hipLaunchKernelGGL(logmel_long_max, dim3(a->B), dim3(256), 0, s, tmax, a->files, a->n_tiles, fmax);
    const int64_t per = (int64_t)a->n_mels * a->max_pitch;
    hipLaunchKernelGGL(logmel_long_finish, dim3((unsigned)((per / 4 + 255) / 256), a->B), dim3(256), 0, s, a->out, a->sample_offs, a->bases,
                       fmax, a->n_mels);
    return ser_check_launch("ser_logmel_long");
}

extern "C" int ser_mel_window_v(const ser_mel_window_args* a, void* stream) {
    if (!a) return ser_fail(-1, "ser_mel_window: null arguments");
    if (!a->src || !a->rows || !a->rows_host || !a->out) return ser_fail(-1, "ser_mel_window: null pointer");
    if (a->B <= 0 || a->B > 65535 || a->n_mels <= 0 || a->n_mels > 65535)
        return ser_fail(-1, "ser_mel_window: B = %d, n_mels = %d", a->B, a->n_mels);
    for (int b = 0; b < a->B; ++b) {
        const int64_t* r = a->rows_host + 5 * b;
        const int64_t base = r[0], pitch = r[1], F = r[2], seek = r[3], nf = r[4];
        if (nf < 1 || nf > LM_FRAMES) return ser_fail(-1, "ser_mel_window: row %d has nf = %lld (1..3000)", b, (long long)nf);
        if (seek < 0 || seek + nf > F)
            return ser_fail(-1, "ser_mel_window: row %d reads frames [%lld, %lld) of a file of %lld", b, (long long)seek, (long long)(seek + nf), (long long)F);
        if (base < 0 || pitch < F) return ser_fail(-1, "ser_mel_window: row %d has base %lld, pitch %lld for %lld frames", b, (long long)base, (long long)pitch, (long long)F);
    }
    hipLaunchKernelGGL(mel_window_kernel, dim3((LM_FRAMES / 4 + 255) / 256, a->n_mels, a->B), dim3(256), 0, (hipStream_t)stream, a->src, a->rows,
                       a->out, a->n_mels);
    return ser_check_launch("ser_mel_window");
}
