// The wav2vec2-conformer encoders' own kernels (ser_hip.h a35; HF modeling_wav2vec2_conformer.py): the rotation of the layer-normed rows in
// front of linear_q / linear_k (ser_rope_rows_v) and the positional term of the Transformer-XL scores (ser_relpos_bias_v; the attention that
// reads it is an instantiation of attention.hip's kernel, ser_attention_rb_v).  The family's convolution module (ser_conformer_conv_bn_v:
// centred window, BatchNorm in eval) is an instantiation of conformer.hip's one body.  The reference ships no conformer encoder; its heads
// take any [T, D] stream (bin/train_cat_bimodal_lazy_1head.py:220-228).  Plain grids, fixed summation orders, no atomics on float data.
#include "row_common.h"

// ------------------------------------------------------------------------------------------------------------------- rotary rows
// Wave per row on the row skeleton: a lane's 4 columns of every 256-column chunk lie in one half of one head (dh % 8 == 0), their partners
// dh / 2 columns away in the same row.  The row's utterance is found by bisection of frame_offs: lo ends at the last b with
// frame_offs[b] <= row.
template <int MODE>
__global__ __launch_bounds__(256) void rope_rows_kernel(ser_rope_rows_args a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    int lo = 0, hi = a.B;                                                   // invariant: frame_offs[lo] <= row, (hi == B or frame_offs[hi] > row)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.frame_offs[mid] <= row) lo = mid; else hi = mid;
    }
    int t = row - a.frame_offs[lo];
    t = t < 0 ? 0 : (t >= a.table_T ? a.table_T - 1 : t);                   // never outside the tables, whatever the offsets say
    const int D = a.D, dh = a.dh, half = dh >> 1;
    const float* xr = a.x + (int64_t)row * a.ldx;
    const float* cr = a.cos_t + (int64_t)t * dh;
    const float* sr = a.sin_t + (int64_t)t * dh;
    unsigned short* orow = (unsigned short*)a.out_act + (int64_t)row * a.ldo_act;
    float ramax = 0.f;
    row_chunks(lane, [&](int i, int c) {
        if (c < D) {
            const int d = c % dh;                                           // channel inside the head
            const bool first = d < half;
            const f32x4 x = *(const f32x4*)(xr + c), xp = *(const f32x4*)(xr + (first ? c + half : c - half));
            const f32x4 cs = *(const f32x4*)(cr + d), sn = *(const f32x4*)(sr + d);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaf(first ? -xp[j] : xp[j], sn[j], x[j] * cs[j]);
            store_act4<MODE>(orow + c, a.out_plane_stride, v[0], v[1], v[2], v[3]);
            if constexpr (mode_traits<MODE>::f16) { for (int j = 0; j < 4; ++j) ramax = range_fold(ramax, v[j]); }
        }
    });
    if constexpr (mode_traits<MODE>::f16) range_report(a.range_flag, ramax);
}

extern "C" int ser_rope_rows_v(const ser_rope_rows_args* a, void* stream) {
    if (!a || !a->x || !a->cos_t || !a->sin_t || !a->frame_offs || !a->out_act) return ser_fail(-1, "ser_rope_rows: null pointer");
    if (a->D % 4 || a->D <= 0 || a->D > 2048 || a->dh <= 0 || a->dh % 8 || a->D % a->dh)
        return ser_fail(-2, "ser_rope_rows: D=%d (multiple of 4 and of dh, <= 2048) / dh=%d (multiple of 8) unsupported", a->D, a->dh);
    if (a->B <= 0 || a->rows <= 0 || a->max_frames <= 0 || a->table_T < a->max_frames)
        return ser_fail(-2, "ser_rope_rows: bad B=%d / rows=%d / max_frames=%d / table_T=%d (the tables must hold max_frames positions)", a->B,
                        a->rows, a->max_frames, a->table_T);
    if ((a->ldx % 4) || a->ldx < a->D || (a->ldo_act % 4) || a->ldo_act < a->D) return ser_fail(-3, "ser_rope_rows: pitches must be multiples of 4 and >= D");
    dim3 grid((a->rows + 3) / 4), block(256);
    if (!ser_with_mode<SER_MODE_FP32X, SER_MODE_BF16, SER_MODE_FP16, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(rope_rows_kernel<M()>, grid, block, 0, (hipStream_t)stream, *a);
        }))
        return ser_fail(-4, "ser_rope_rows: bad mode %d", a->mode);
    return ser_check_launch("ser_rope_rows");
}

// ------------------------------------------------------------------------------------------------------- relative-position bias
// Block = 32 query rows x 64 keys of one (utterance, head); 256 threads.  LDS: the 32 query rows' q + off as fp32 [32][64], and the window
// of P_h the tile needs -- distances i - j from i0 - j0 - 63 to i0 - j0 + 31, 95 rows -- with a row pitch of 65 floats (the 64 lanes of a
// wave read 64 different rows at the same d: 64 different banks).  Thread (wave w, lane l) takes key j0 + l for the 8 query rows
// i0 + 8 w .. + 7, each dot product in ascending d.  Keys T .. 64 ceil(T / 64) - 1 of a row are written as zeros; rows past T are not
// written.  Every index into P is inside [0, 2 P_T): max_frames <= P_T is checked by the launcher, and T <= max_frames by the clamp below.
#define RPB_Q 32
#define RPB_K 64
#define RPB_WIN (RPB_Q + RPB_K - 1)
template <int MODE>
__global__ __launch_bounds__(256) void relpos_bias_kernel(ser_relpos_bias_args a, int nkt_max) {
    __shared__ float ps[RPB_WIN * 65];
    __shared__ float qs[RPB_Q * 64];
    const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
    const int row0 = a.frame_offs[b];
    int T = a.frame_offs[b + 1] - row0;
    T = T > a.max_frames ? a.max_frames : T;                               // block-uniform; the plan's max_frames bounds every index
    const int nk = (T + RPB_K - 1) / RPB_K;
    const int qt = blockIdx.x / nkt_max, kt = blockIdx.x - qt * nkt_max;
    const int i0 = qt * RPB_Q, j0 = kt * RPB_K;
    if (i0 >= T || kt >= nk) return;                                       // block-uniform
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // window row w holds P_h(r) for r = rmin + w, rmin = i0 - j0 - 63; distances no (query < T, key < T) pair of the tile has stay zero
    const int rmin = i0 - j0 - (RPB_K - 1);
    for (int e = tid; e < RPB_WIN * 16; e += 256) {
        const int w = e >> 4, d4 = (e & 15) * 4;
        const int r = rmin + w;
        f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (r > -T && r < T) v = *(const f32x4*)(a.P + (int64_t)(a.P_T + r) * a.ldp + h * 64 + d4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ps[w * 65 + d4 + j] = v[j];
    }
    const float* off = a.off + h * 64;
    for (int e = tid; e < RPB_Q * 64; e += 256) {
        const int qi = e >> 6, d = e & 63;
        const int i = i0 + qi < T ? i0 + qi : T - 1;
        const unsigned short* qr = (const unsigned short*)a.qkv + (int64_t)(row0 + i) * a.ld + a.q_col + h * 64 + d;
        float v = elem2f<MODE>(qr[0]);
        if (mode_traits<MODE>::planes == 2) v += elem2f<MODE>(qr[a.plane_stride]);
        qs[e] = v + off[d];
    }
    __syncthreads();
    const int j = j0 + lane;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int qi = wave * 8 + e, i = i0 + qi;
        if (i >= T) break;                                                 // wave-uniform
        const float* q = qs + qi * 64;
        const float* pr = ps + (qi - lane + (RPB_K - 1)) * 65;             // window row of i - j: (i0 + qi) - (j0 + lane) - rmin
        float s = 0.f;
#pragma unroll 16
        for (int d = 0; d < 64; ++d) s = fmaf(q[d], pr[d], s);
        a.pb[((int64_t)(row0 + i) * a.H + h) * a.ld_pb + j] = j < T ? s : 0.f;
    }
}

extern "C" int ser_relpos_bias_v(const ser_relpos_bias_args* a, void* stream) {
    if (!a || !a->qkv || !a->P || !a->off || !a->frame_offs || !a->pb) return ser_fail(-1, "ser_relpos_bias: null pointer");
    if (a->dh != 64 || a->H <= 0 || a->B <= 0 || (int64_t)a->B * a->H > 65535 || a->q_col < 0)
        return ser_fail(-2, "ser_relpos_bias: B=%d H=%d dh=%d unsupported (head dim 64, B H <= 65535)", a->B, a->H, a->dh);
    if (a->max_frames <= 0 || a->rows < a->max_frames || a->P_T < a->max_frames)
        return ser_fail(-2, "ser_relpos_bias: bad max_frames=%d / rows=%d / P_T=%d (P must hold the distances of max_frames)", a->max_frames,
                        a->rows, a->P_T);
    const int nkt = (a->max_frames + RPB_K - 1) / RPB_K, nqt = (a->max_frames + RPB_Q - 1) / RPB_Q;
    if ((a->ld_pb % 64) || a->ld_pb < (int64_t)nkt * RPB_K || (a->ldp % 4) || a->ldp < (int64_t)a->H * 64 || (a->ld % 4))
        return ser_fail(-3, "ser_relpos_bias: ld_pb=%lld must be a multiple of 64 and >= %d; ldp >= H dh; pitches multiples of 4",
                        (long long)a->ld_pb, nkt * RPB_K);
    dim3 grid(nqt * nkt, a->B * a->H), block(256);
    if (!ser_with_mode<SER_MODE_BF16, SER_MODE_FP32X, SER_MODE_FP16X>(a->mode, [&](auto M) {
            hipLaunchKernelGGL(relpos_bias_kernel<M()>, grid, block, 0, (hipStream_t)stream, *a, nkt);
        }))
        return ser_fail(-4, "ser_relpos_bias: bad mode %d", a->mode);
    return ser_check_launch("ser_relpos_bias");
}
