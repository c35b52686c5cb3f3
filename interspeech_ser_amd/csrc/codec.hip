// The speaker half of the 512-wide third stream (ser_hip.h a27): FACodecEncoderV2.block, the waveform-rate stack of weight-normed
// convolutions around anti-aliased SnakeBeta activations (src/ns3/facodec.py ResidualUnit / EncoderBlock, src/ns3/alias_free_torch).  The
// reference runs it on the CPU, one file at a time (preprocessing/preprocess_ns3_prosody_speaker.py:41-60).  Three kernels over channels-last
// fp32 rows of a packed ragged batch: a whole ResidualUnit per launch for the narrow levels (ser_codec_unit_v), the narrow strided
// convolution with the activation fused on its input (ser_codec_conv_v), and the activation as the producer of ser_gemm's operand copy for
// the wide levels (ser_snake_v).  Every edge rule -- the two replicate clamps of an activation, the zero padding of a convolution -- acts at
// the utterance's own ends, tiles start at the utterance's first row, and every sum runs in ascending tap, then ascending input channel:
// a result is a function of its own utterance alone (no atomics on float data), so a batched run is bit-equal to a batch of one.
#include "ser_common.h"
#include <math.h>

#define CODEC_TAPS 12
#define CODEC_UNIT_THREADS 512
#define CODEC_CONV_THREADS 256
#define CODEC_MAX_LDS (160 * 1024)
#define SNAKE_ROWS 32                       // output rows per block of ser_snake_v
#define SNAKE_COLS 64                       // channels per block

// Activation1d, first half, at the doubled rate: s[m] = u + sin^2(u e^alpha) / (e^beta + 1e-9) with u[m] = 2 sum_i xp[i] f[m + 15 - 2 i] over
// the replicate-padded input (5 a side), i.e. for m = 2 t + p the six taps f[2 e + 5 + p] on x[clamp(t - e)], e = -2 - p .. 3 - p (ascending
// tap index).  x(j): the caller's accessor, which clamps j to the utterance.
template <class X>
__device__ __forceinline__ float snake_up(X&& x, int m, const float (&f)[CODEC_TAPS], float ea, float ib) {
    const int t = m >> 1, p = m & 1;
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        const int e = q - 2 - p;
        acc = fmaf(x(t - e), f[2 * q + 1 - p], acc);                 // 2 e + 5 + p = 2 q + 1 - p
    }
    const float u = 2.f * acc;
    const float sn = sinf(u * ea);
    return fmaf(sn * sn, ib, u);
}
// second half: a[t] = sum_k sp[2 t + k] f[k] over s replicate-padded by (5, 6), i.e. s[clamp(2 t + k - 5, 0, 2 T - 1)]; s(m) clamps.
template <class S>
__device__ __forceinline__ float snake_down(S&& s, int t, const float (&f)[CODEC_TAPS]) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < CODEC_TAPS; ++k) acc = fmaf(s(2 * t + k - 5), f[k], acc);
    return acc;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ void load_taps(float (&f)[CODEC_TAPS], const float* __restrict__ taps) {
#pragma unroll
    for (int k = 0; k < CODEC_TAPS; ++k) f[k] = taps[k];
}
static inline int odd(int n) { return n | 1; }                     // LDS row pitches: odd, so that a transposing store spreads over the banks

// ------------------------------------------------------------------------------------------------ one ResidualUnit, C <= 32
// y = x + W1 Act2(conv_k_d(Act1(x)) + b7) + b1 on a time tile of SER_CODEC_TILE rows of one utterance.  Everything between x and y lives in
// LDS, channel-major ([c][row]: consecutive lanes take consecutive rows of one channel):
//   xs  rows t0 - hk - 12 ..   (hk = (k / 2) d)      the input, with the halo both activations and the convolution reach
//   sb  the doubled-rate snake values (first of Act1, later of Act2)
//   ab  Act1(x) on t0 - hk - 6 .., zero outside the utterance (the convolution's padding); later Act2(h) on the tile
//   hb  the convolution's output on t0 - 6 ..
struct unit_lds { int nx, ns, na, nh, px, ps, pa, ph; };
static inline unit_lds unit_layout(int k, int d) {
    unit_lds L;
    const int hk = (k / 2) * d;
    L.nx = SER_CODEC_TILE + 2 * (hk + 12);
    L.na = SER_CODEC_TILE + 2 * (hk + 6);
    L.ns = 2 * L.na + 10;
    L.nh = SER_CODEC_TILE + 12;
    L.px = odd(L.nx); L.ps = odd(L.ns); L.pa = odd(L.na); L.ph = odd(L.nh);
    return L;
}

__global__ __launch_bounds__(CODEC_UNIT_THREADS) void codec_unit_kernel(ser_codec_unit_args a, unit_lds L) {
    extern __shared__ float lds[];
    const int C = a.C, k = a.k, d = a.dilation, hk = (k / 2) * d;
    const int b = blockIdx.y;
    const int64_t base = a.row_offs[b];
    const int T = a.row_offs[b + 1] - a.row_offs[b];
    const int t0 = blockIdx.x * SER_CODEC_TILE;
    if (t0 >= T) return;
    float* xs = lds;
    float* sb = xs + C * L.px;
    float* ab = sb + C * L.ps;
    float* hb = ab + C * L.pa;
    const int lo_x = t0 - hk - 12, lo_a = t0 - hk - 6, lo_s = 2 * lo_a - 5, lo_h = t0 - 6, lo_s2 = 2 * t0 - 5;
    const int tid = threadIdx.x, nth = CODEC_UNIT_THREADS;
    float f[CODEC_TAPS];
    load_taps(f, a.taps);

    {   // x rows of the window that exist
        const int j0 = lo_x < 0 ? 0 : lo_x, j1 = lo_x + L.nx < T ? lo_x + L.nx : T;
        const float* src = a.x + (base + j0) * C;
        for (int i = tid; i < (j1 - j0) * C; i += nth) xs[(i % C) * L.px + (j0 - lo_x) + i / C] = src[i];
    }
    __syncthreads();
    for (int i = tid; i < C * L.ns; i += nth) {
        const int c = i / L.ns, mi = i - c * L.ns, m = lo_s + mi;
        if (m >= 0 && m < 2 * T) {
            const float* xc = xs + c * L.px - lo_x;
            sb[c * L.ps + mi] = snake_up([&](int j) { return xc[clampi(j, 0, T - 1)]; }, m, f, a.ea1[c], a.ib1[c]);
        }
    }
    __syncthreads();
    for (int i = tid; i < C * L.na; i += nth) {
        const int c = i / L.na, ri = i - c * L.na, t = lo_a + ri;
        float v = 0.f;
        if (t >= 0 && t < T) {
            const float* sc = sb + c * L.ps - lo_s;
            v = snake_down([&](int m) { return sc[clampi(m, 0, 2 * T - 1)]; }, t, f);
        }
        ab[c * L.pa + ri] = v;
    }
    __syncthreads();
    const int G = C / 4;
    {   // the dilated convolution: a wave takes 64 rows of one group of 4 output channels (its weights are wave-uniform)
        const int r64 = (L.nh + 63) & ~63;
        for (int i = tid; i < G * r64; i += nth) {
            const int g = i / r64, ri = i - g * r64, t = lo_h + ri;
            if (ri >= L.nh || t < 0 || t >= T) continue;
            const int n = g * 4;
            f32x4 acc = *(const f32x4*)(a.b7 + n);
            const float* ar = ab + (t - hk - lo_a);
            for (int tap = 0; tap < k; ++tap)
                for (int c = 0; c < C; ++c) {
                    const float v = ar[c * L.pa + tap * d];
                    const f32x4 w = *(const f32x4*)(a.w7 + (int64_t)(tap * C + c) * C + n);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[j], v, acc[j]);
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) hb[(n + j) * L.ph + ri] = acc[j];
        }
    }
    __syncthreads();
    for (int i = tid; i < C * (2 * SER_CODEC_TILE + 10); i += nth) {
        const int ns2 = 2 * SER_CODEC_TILE + 10;
        const int c = i / ns2, mi = i - c * ns2, m = lo_s2 + mi;
        if (m >= 0 && m < 2 * T) {
            const float* hc = hb + c * L.ph - lo_h;
            sb[c * L.ps + mi] = snake_up([&](int j) { return hc[clampi(j, 0, T - 1)]; }, m, f, a.ea2[c], a.ib2[c]);
        }
    }
    __syncthreads();
    for (int i = tid; i < C * SER_CODEC_TILE; i += nth) {
        const int c = i / SER_CODEC_TILE, ri = i - c * SER_CODEC_TILE, t = t0 + ri;
        if (t < T) {
            const float* sc = sb + c * L.ps - lo_s2;
            ab[c * L.pa + ri] = snake_down([&](int m) { return sc[clampi(m, 0, 2 * T - 1)]; }, t, f);
        }
    }
    __syncthreads();
    for (int i = tid; i < G * SER_CODEC_TILE; i += nth) {          // SER_CODEC_TILE is a multiple of 64: g is wave-uniform
        const int g = i / SER_CODEC_TILE, ri = i - g * SER_CODEC_TILE, t = t0 + ri;
        if (t >= T) continue;
        const int n = g * 4;
        f32x4 acc = *(const f32x4*)(a.b1 + n);
        for (int c = 0; c < C; ++c) {
            const float v = ab[c * L.pa + ri];
            const f32x4 w = *(const f32x4*)(a.w1 + (int64_t)c * C + n);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[j], v, acc[j]);
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = xs[(n + j) * L.px + (t - lo_x)] + acc[j];
        *(f32x4*)(a.y + (base + t) * C + n) = o;
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int ser_codec_unit_v(const ser_codec_unit_args* a, void* stream) {
    if (!a || !a->x || !a->y || !a->row_offs || !a->taps || !a->ea1 || !a->ib1 || !a->w7 || !a->b7 || !a->ea2 || !a->ib2 || !a->w1 || !a->b1)
        return ser_fail(-1, "ser_codec_unit: null pointer");
    if (a->C <= 0 || a->C % 8 || a->C > 32) return ser_fail(-2, "ser_codec_unit: C=%d must be a multiple of 8, at most 32 (wider levels: ser_snake_v + ser_gemm)", a->C);
    if (a->k < 1 || a->k % 2 == 0 || a->k > 7) return ser_fail(-2, "ser_codec_unit: k=%d must be odd, at most 7", a->k);
    if (a->dilation < 1 || a->dilation > 9) return ser_fail(-2, "ser_codec_unit: dilation=%d unsupported (1..9)", a->dilation);
    if (a->rows < 0 || a->max_rows < 0 || a->max_rows > a->rows) return ser_fail(-2, "ser_codec_unit: bad rows=%d / max_rows=%d", a->rows, a->max_rows);
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_codec_unit: bad B=%d", a->B);
    if (a->x == a->y) return ser_fail(-3, "ser_codec_unit: y must not be x (a tile reads its neighbours' rows)");
    if (!aligned16(a->x) || !aligned16(a->y) || !aligned16(a->w7) || !aligned16(a->w1) || !aligned16(a->b7) || !aligned16(a->b1))
        return ser_fail(-3, "ser_codec_unit: x, y, weights and biases must be 16-byte aligned");
    if (a->max_rows == 0) return 0;
    const unit_lds L = unit_layout(a->k, a->dilation);
    const int lds = a->C * (L.px + L.ps + L.pa + L.ph) * (int)sizeof(float);
    if (lds > CODEC_MAX_LDS) return ser_fail(-5, "ser_codec_unit: C=%d k=%d dilation=%d needs %d bytes of LDS", a->C, a->k, a->dilation, lds);
    static std::atomic<bool> ready{false};
    if (hipError_t e = ser_lds_optin(codec_unit_kernel, CODEC_MAX_LDS, ready)) return ser_fail((int)e, "ser_codec_unit: cannot raise dynamic LDS to %d", CODEC_MAX_LDS);
    dim3 grid((a->max_rows + SER_CODEC_TILE - 1) / SER_CODEC_TILE, a->B);
    hipLaunchKernelGGL(codec_unit_kernel, grid, dim3(CODEC_UNIT_THREADS), lds, (hipStream_t)stream, *a, L);
    return ser_check_launch("ser_codec_unit");
}

// ------------------------------------------------------------------------------------------------ narrow strided convolution
// out[t][n] = bias[n] + sum_tap sum_c w[tap C_in + c][n] v[t stride - pad + tap][c], v = Act(x) when ea is given, else x; v is zero outside
// [0, L), L = the rows the utterance owns in x (in_offs); the output rows come from out_offs.  conv_in reads the unpadded waveform and
// writes the padded length's rows: the zeros the reference pads the wave with are the zeros beyond L.
struct conv_lds { int to, nq, nx, ns, pq, px, ps; };
static inline conv_lds conv_layout(int k, int stride, bool act) {
    conv_lds L;
    L.to = SER_CODEC_TILE / stride > 0 ? SER_CODEC_TILE / stride : 1;
    L.nq = (L.to - 1) * stride + k;
    L.nx = act ? L.nq + 12 : 0;
    L.ns = act ? 2 * L.nq + 10 : 0;
    L.pq = odd(L.nq); L.px = act ? odd(L.nx) : 0; L.ps = act ? odd(L.ns) : 0;
    return L;
}

__global__ __launch_bounds__(CODEC_CONV_THREADS) void codec_conv_kernel(ser_codec_conv_args a, conv_lds L) {
    extern __shared__ float lds[];
    const int C = a.C_in, N = a.C_out, k = a.k, s = a.stride;
    const int b = blockIdx.y;
    const int64_t ibase = a.in_offs[b];
    const int64_t avail64 = a.in_offs[b + 1] - ibase;
    const int64_t obase = a.out_offs[b];
    const int To = a.out_offs[b + 1] - a.out_offs[b];
    const int t0 = blockIdx.x * L.to;
    if (t0 >= To) return;
    const int Lin = avail64 < 0x3fffffff ? (int)avail64 : 0x3fffffff, avail = Lin;    // (2 Lin stays an int)
    const int lo_q = t0 * s - a.pad;
    const int tid = threadIdx.x, nth = CODEC_CONV_THREADS;
    float* qb = lds;                                             // the convolution's input rows lo_q .. lo_q + nq - 1, channel-major
    if (a.ea) {
        float* xs = qb + C * L.pq;
        float* sb = xs + C * L.px;
        const int lo_x = lo_q - 6, lo_s = 2 * lo_q - 5;
        float f[CODEC_TAPS];
        load_taps(f, a.taps);
        {
            const int j0 = lo_x < 0 ? 0 : lo_x, j1 = lo_x + L.nx < Lin ? lo_x + L.nx : Lin;
            for (int i = tid; i < (j1 - j0) * C; i += nth) {
                const int j = j0 + i / C, c = i % C;
                xs[c * L.px + (j - lo_x)] = j < avail ? a.x[(ibase + j) * C + c] : 0.f;
            }
        }
        __syncthreads();
        for (int i = tid; i < C * L.ns; i += nth) {
            const int c = i / L.ns, mi = i - c * L.ns, m = lo_s + mi;
            if (m >= 0 && m < 2 * Lin) {
                const float* xc = xs + c * L.px - lo_x;
                sb[c * L.ps + mi] = snake_up([&](int j) { return xc[clampi(j, 0, Lin - 1)]; }, m, f, a.ea[c], a.ib[c]);
            }
        }
        __syncthreads();
        for (int i = tid; i < C * L.nq; i += nth) {
            const int c = i / L.nq, ri = i - c * L.nq, t = lo_q + ri;
            float v = 0.f;
            if (t >= 0 && t < Lin) {
                const float* sc = sb + c * L.ps - lo_s;
                v = snake_down([&](int m) { return sc[clampi(m, 0, 2 * Lin - 1)]; }, t, f);
            }
            qb[c * L.pq + ri] = v;
        }
    } else {
        for (int i = tid; i < C * L.nq; i += nth) {
            const int ri = i / C, c = i - ri * C, j = lo_q + ri;
            qb[c * L.pq + ri] = (j >= 0 && j < avail) ? a.x[(ibase + j) * C + c] : 0.f;
        }
    }
    __syncthreads();
    const int G = N / 4;
    const int r64 = (L.to + 63) & ~63;
    for (int i = tid; i < G * r64; i += nth) {
        const int g = i / r64, ri = i - g * r64, t = t0 + ri;
        if (ri >= L.to || t >= To) continue;
        const int n = g * 4;
        f32x4 acc = a.bias ? *(const f32x4*)(a.bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f};
        const float* qr = qb + ri * s;
        for (int tap = 0; tap < k; ++tap)
            for (int c = 0; c < C; ++c) {
                const float v = qr[c * L.pq + tap];
                const f32x4 w = *(const f32x4*)(a.w + (int64_t)(tap * C + c) * N + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[j], v, acc[j]);
            }
        *(f32x4*)(a.y + (obase + t) * a.ldy + n) = acc;
    }
}

extern "C" int ser_codec_conv_v(const ser_codec_conv_args* a, void* stream) {
    if (!a || !a->x || !a->y || !a->in_offs || !a->out_offs || !a->w) return ser_fail(-1, "ser_codec_conv: null pointer");
    if (a->ea && (!a->ib || !a->taps)) return ser_fail(-1, "ser_codec_conv: the activation needs ea, ib and taps");
    if (!(a->C_in == 1 || a->C_in == 8 || a->C_in == 16 || a->C_in == 32))
        return ser_fail(-2, "ser_codec_conv: C_in=%d must be 1, 8, 16 or 32 (wider levels: ser_snake_v + ser_gemm)", a->C_in);
    if (a->C_out <= 0 || a->C_out % 8) return ser_fail(-2, "ser_codec_conv: C_out=%d must be a multiple of 8", a->C_out);
    if (a->k < 1 || a->k > 16 || a->stride < 1 || a->stride > 8 || a->pad < 0 || a->pad > a->k)
        return ser_fail(-2, "ser_codec_conv: k=%d (1..16) / stride=%d (1..8) / pad=%d (0..k) unsupported", a->k, a->stride, a->pad);
    if (a->rows < 0 || a->max_out_rows < 0 || a->max_out_rows > a->rows) return ser_fail(-2, "ser_codec_conv: bad rows=%d / max_out_rows=%d", a->rows, a->max_out_rows);
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_codec_conv: bad B=%d", a->B);
    if (a->ldy < a->C_out || a->ldy % 4) return ser_fail(-3, "ser_codec_conv: ldy=%lld must be a multiple of 4, at least C_out", (long long)a->ldy);
    if (!aligned16(a->y) || !aligned16(a->w) || !aligned16(a->bias)) return ser_fail(-3, "ser_codec_conv: y, w and bias must be 16-byte aligned");
    if (a->max_out_rows == 0) return 0;
    const conv_lds L = conv_layout(a->k, a->stride, a->ea != nullptr);
    const int lds = a->C_in * (L.pq + L.px + L.ps) * (int)sizeof(float);
    if (lds > CODEC_MAX_LDS) return ser_fail(-5, "ser_codec_conv: C_in=%d k=%d stride=%d needs %d bytes of LDS", a->C_in, a->k, a->stride, lds);
    static std::atomic<bool> ready{false};
    if (hipError_t e = ser_lds_optin(codec_conv_kernel, CODEC_MAX_LDS, ready)) return ser_fail((int)e, "ser_codec_conv: cannot raise dynamic LDS to %d", CODEC_MAX_LDS);
    dim3 grid((a->max_out_rows + L.to - 1) / L.to, a->B);
    hipLaunchKernelGGL(codec_conv_kernel, grid, dim3(CODEC_CONV_THREADS), lds, (hipStream_t)stream, *a, L);
    return ser_check_launch("ser_codec_conv");
}

// ------------------------------------------------------------------------------------------------ Activation1d -> operand planes (wide levels)
// A block takes SNAKE_ROWS rows x SNAKE_COLS channels of one utterance: the input rows (6 more a side) and the doubled-rate snake values
// sit in LDS as [row][channel] (consecutive lanes take consecutive channels); a thread finishes 4 channels of a row and stores them as
// operand planes at row out_rowmap[m] (a zero-halo'd layout: the rows between utterances are the caller's zeros and are never written).
template <int MODE>
__global__ __launch_bounds__(256) void snake_kernel(ser_snake_args a) {
    __shared__ float xs[(SNAKE_ROWS + 12) * SNAKE_COLS];
    __shared__ float sb[(2 * SNAKE_ROWS + 10) * SNAKE_COLS];
    const int b = blockIdx.z, c0 = blockIdx.y * SNAKE_COLS;
    const int64_t base = a.row_offs[b];
    const int T = a.row_offs[b + 1] - a.row_offs[b];
    const int t0 = blockIdx.x * SNAKE_ROWS;
    if (t0 >= T) return;
    const int lo_x = t0 - 6, lo_s = 2 * t0 - 5, tid = threadIdx.x;
    float f[CODEC_TAPS];
    load_taps(f, a.taps);
    {
        const int j0 = lo_x < 0 ? 0 : lo_x, j1 = lo_x + SNAKE_ROWS + 12 < T ? lo_x + SNAKE_ROWS + 12 : T;
        for (int i = tid; i < (j1 - j0) * (SNAKE_COLS / 4); i += 256) {
            const int j = j0 + i / (SNAKE_COLS / 4), c = (i % (SNAKE_COLS / 4)) * 4;
            *(f32x4*)(xs + (j - lo_x) * SNAKE_COLS + c) = *(const f32x4*)(a.x + (base + j) * a.ldx + c0 + c);
        }
    }
    __syncthreads();
    {
        const int c = tid & (SNAKE_COLS - 1);
        const float ea = a.ea[c0 + c], ib = a.ib[c0 + c];
        for (int mi = tid / SNAKE_COLS; mi < 2 * SNAKE_ROWS + 10; mi += 256 / SNAKE_COLS) {
            const int m = lo_s + mi;
            if (m >= 0 && m < 2 * T)
                sb[mi * SNAKE_COLS + c] = snake_up([&](int j) { return xs[(clampi(j, 0, T - 1) - lo_x) * SNAKE_COLS + c]; }, m, f, ea, ib);
        }
    }
    __syncthreads();
    float ramax = 0.f;
    for (int i = tid; i < SNAKE_ROWS * (SNAKE_COLS / 4); i += 256) {
        const int ri = i / (SNAKE_COLS / 4), c = (i % (SNAKE_COLS / 4)) * 4, t = t0 + ri;
        if (t >= T) continue;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CODEC_TAPS; ++k) {
            const f32x4 s = *(const f32x4*)(sb + (clampi(2 * t + k - 5, 0, 2 * T - 1) - lo_s) * SNAKE_COLS + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaf(s[j], f[k], v[j]);
        }
        const int64_t row = base + t;
        if (a.out_f32) *(f32x4*)(a.out_f32 + row * a.ldo_f32 + c0 + c) = v;
        if (a.out_act) {
            const int64_t orow = a.out_rowmap ? a.out_rowmap[row] : row;
            store_act4<MODE>((unsigned short*)a.out_act + orow * a.ldo_act + c0 + c, a.out_plane_stride, v[0], v[1], v[2], v[3]);
            if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
        }
    }
    if constexpr (mode_traits<MODE>::f16) range_report(a.range_flag, ramax);
}

extern "C" int ser_snake_v(const ser_snake_args* a, void* stream) {
    if (!a || !a->x || !a->row_offs || !a->taps || !a->ea || !a->ib || (!a->out_act && !a->out_f32)) return ser_fail(-1, "ser_snake: null pointer");
    if (a->C <= 0 || a->C % SNAKE_COLS) return ser_fail(-2, "ser_snake: C=%d must be a multiple of %d (narrower levels: ser_codec_unit_v / ser_codec_conv_v)", a->C, SNAKE_COLS);
    if (a->rows < 0 || a->max_rows < 0 || a->max_rows > a->rows) return ser_fail(-2, "ser_snake: bad rows=%d / max_rows=%d", a->rows, a->max_rows);
    if (a->B <= 0 || a->B > 65535) return ser_fail(-2, "ser_snake: bad B=%d", a->B);
    if (a->ldx < a->C || a->ldx % 4 || (a->out_f32 && (a->ldo_f32 < a->C || a->ldo_f32 % 4)) || (a->out_act && (a->ldo_act < a->C || a->ldo_act % 4)))
        return ser_fail(-3, "ser_snake: pitches must be multiples of 4, at least C");
    if (!aligned16(a->x) || !aligned16(a->out_f32) || ((uintptr_t)a->out_act & 7)) return ser_fail(-3, "ser_snake: x / out_f32 must be 16-byte, out_act 8-byte aligned");
    if (a->max_rows == 0) return 0;
    dim3 grid((a->max_rows + SNAKE_ROWS - 1) / SNAKE_ROWS, a->C / SNAKE_COLS, a->B);
    const int mode = a->out_act ? a->mode : SER_MODE_BF16;                  // (no planes: any instantiation)
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(mode, [&](auto M) {
            hipLaunchKernelGGL(snake_kernel<M()>, grid, dim3(256), 0, (hipStream_t)stream, *a);
        }))
        return ser_fail(-4, "ser_snake: bad mode %d", mode);
    return ser_check_launch("ser_snake");
}
