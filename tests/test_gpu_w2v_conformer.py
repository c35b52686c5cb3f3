"""GPU: the wav2vec2-conformer encoders on libserhip -- the new kernels against float64 statements (tests/w2vconf_ref.py), the encoder end to
end against the HF fixtures of both position types, the speech driver and the predictor behind it.

Bounds (tests/test_gpu_w2vbert.py's, restated).
* plane_term(mode, amax): what the operand planes cannot hold of a value of magnitude amax -- half a bf16 ulp in bf16, half a bf16 ulp of
  the lo plane (itself at most half a bf16 ulp of the value) in fp32x; nothing in f16x where 4 x the fp32 twin's distance leaves room
  (the convolution), and f16x_term -- half an fp16 ulp of the lo plane: hi + lo keep 22 bits, an fp32 result has 24 -- where the bound is a
  count of fp32 ulps (the rotation), as tests/test_gpu_w2vbert.py::test_swish_rows adds it.
* ser_rope_rows_v: x' = fma(x_pair, sin, x cos) is two products and one sum: at most 2 fp32 ulp of |x cos| + |x_pair sin| per element,
  plus the plane terms.
* ser_conformer_conv_bn_v: at most 4 x the distance of the same arithmetic in torch fp32 from the float64 statement, plus the plane term.
* ser_relpos_bias_v + ser_attention_rb_v: tests/test_gpu_kernels.py::test_attention's per-mode bounds (3e-2 bf16, 1e-4 fp32x / f16x); the
  bias adds one fp32 term per logit.
* end to end: tests/test_gpu_e2e.py's gates, max|a - b| / max(1, max|b|) < 1e-3 (f16x, fp32x), 3e-2 (bf16).
"""
import ctypes
import hashlib
import json
import math
import os
import wave

import numpy as np
import pytest
import torch

import w2vconf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, FP32X, FP16X = 1, 2, 4
MODES = {"bf16": BF16, "fp32x": FP32X, "f16x": FP16X}
E2E_TOL = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}
CASES = (("tiny_w2v_conformer_rope", "TINY_W2V_CONFORMER_ROPE"), ("tiny_w2v_conformer_rel", "TINY_W2V_CONFORMER_REL"))
# sha256 of ser_conformer_conv_v's output planes (D 128, K 7, f16x, frames (1, 2, 30, 31, 37, 5), conv_inputs seed 135) from the library
# built at the commit before this family was added: the kernel keeps its bits
PARENT_CONV_DIGEST = "e4633d2d87787c8e4947bfc24e147e7188ba63f33497f531dd03f84e4ba24c9a"
# sha256 of output planes from the library built at the commit before the two conformer families were put on one convolution body and one
# biased-attention launcher: the kernels keep their bits.
# ser_conformer_conv_bn_v: D 1280 (the second 1024-column slab partly filled), K 31, frames (1, 8, 9, 37) -- a window longer than the
# utterance, one SER_CCONV_TILE, a tile plus one row, several tiles -- conv_inputs seed 1311
PARENT_CONV_BN_1280_DIGESTS = {
    "bf16": "4b8ece3a9763d05bb580de28f6214c273c9166dfbc584c5c6bf34f54aa5bdb56",
    "fp32x": "8d8bd1912765ade4bb8a7d3e8541f3ff2526676b282707e847557966f132da71",
    "f16x": "e07efacc5a67c9758112c17922794693e8e2c8ddf7f9adeddd302035a04ae528",
}
# ser_relpos_bias_v + ser_attention_rb_v: H 3, frames (1, 33, 99, 130), P_T 256, f16x, attention_rb_inputs seed 300
PARENT_ATTENTION_RB_DIGEST = "d6302030b3e033ea6a8018cfd2d757a4757ed9f7630f3ae56b5689e25a77922c"


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def ulp_bf16(v):
    return 2.0 ** (math.floor(math.log2(max(float(v), 1e-30))) - 7)


def ulp_f16(v):
    return 2.0 ** max(math.floor(math.log2(max(float(v), 1e-30))) - 10, -24)


def plane_term(mode, amax):
    if mode == BF16:
        return 0.5 * ulp_bf16(amax)
    if mode == FP32X:
        return 0.5 * ulp_bf16(0.5 * ulp_bf16(amax))
    return 0.0


def f16x_term(mode, amax):
    return 0.5 * ulp_f16(0.5 * ulp_f16(amax)) if mode == FP16X else 0.0


def act_dtype(mode):
    return torch.float16 if mode == FP16X else torch.bfloat16


def planes_of(mode):
    return 1 if mode == BF16 else 2


def to_act(x, mode):
    dt = act_dtype(mode)
    hi = x.to(dt)
    if mode == BF16:
        return hi[None].contiguous().to(DEV)
    return torch.stack([hi, (x - hi.float()).to(dt)]).contiguous().to(DEV)


def act_value(t):
    return t.double().sum(0)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu().contiguous().view(torch.int16)


def planes_digest(t):
    return hashlib.sha256(_bits(t).numpy().tobytes()).hexdigest()


def offsets(frames):
    return np.concatenate([[0], np.cumsum(frames)])


# --------------------------------------------------------------------------------------------------------------------- rotary rows
ROPE_ROWS = (1, 99, 130)


def run_rope(L, x, frames, dh, mode, table_T=None):
    from interspeech_ser_amd.weights import rotary_inv_freq, rotary_tables
    M, D = x.shape
    table_T = max(frames) if table_T is None else table_T
    cos, sin = rotary_tables(table_T, rotary_inv_freq(dh, 10000))
    xd, cd, sd_ = x.to(DEV), cos.to(DEV), sin.to(DEV)
    fo = torch.tensor(offsets(frames), dtype=torch.int32, device=DEV)
    out = torch.zeros(planes_of(mode), M + 1, D, dtype=act_dtype(mode), device=DEV)       # a canary row behind the last
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.RopeRowsArgs()
    a.x, a.ldx, a.cos_t, a.sin_t, a.frame_offs = xd.data_ptr(), D, cd.data_ptr(), sd_.data_ptr(), fo.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = out.data_ptr(), D, (M + 1) * D, flag.data_ptr()
    a.B, a.rows, a.D, a.dh, a.table_T, a.max_frames, a.mode = len(frames), M, D, dh, table_T, max(frames), mode
    L.check(L.lib.ser_rope_rows_v(ctypes.byref(a), stream()), "ser_rope_rows_v")
    torch.cuda.synchronize()
    host = out.cpu()
    assert not bool(host[:, M].any()), "ser_rope_rows_v wrote behind its rows"
    return host[:, :M], int(flag.item())


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("D", [128, 192])
def test_rope_rows(L, D, mode):
    m, dh, frames = MODES[mode], 64, list(ROPE_ROWS)
    M = sum(frames)
    x = torch.from_numpy(np.random.default_rng(D).standard_normal((M, D)).astype(np.float32)) * 2.0      # numpy's stream: the same rows on every host
    out, bits = run_rope(L, x, frames, dh, m)
    offs = offsets(frames)
    worst = 0.0
    for b, T in enumerate(frames):
        xb = x[offs[b]: offs[b + 1]].double()
        cos, sin = R.rotary_tables(T, dh, 10000.0)
        ref = R.rotate(xb, D // dh, cos, sin)
        xh = xb.view(T, D // dh, dh)
        rot = torch.cat([-xh[..., dh // 2:], xh[..., : dh // 2]], dim=-1)
        mag = ((xh * cos[:, None, :]).abs() + (rot * sin[:, None, :]).abs()).reshape(T, D)
        amax = float(ref.abs().max())
        bound = 2.0 * torch.from_numpy(np.spacing(mag.numpy().astype(np.float32)).astype(np.float64)) + plane_term(m, amax) + f16x_term(m, amax)
        err = (act_value(out[:, offs[b]: offs[b + 1]]) - ref).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), (b, float((err / bound).max()))
        # the position is the frame index INSIDE the utterance: an utterance of the batch equals the same utterance alone
        alone, _ = run_rope(L, x[offs[b]: offs[b + 1]].contiguous(), [T], dh, m)
        assert torch.equal(_bits(alone), _bits(out[:, offs[b]: offs[b + 1]])), (b, "batch of one")
        # ... and a longer table changes nothing
        longer, _ = run_rope(L, x[offs[b]: offs[b + 1]].contiguous(), [T], dh, m, table_T=T + 77)
        assert torch.equal(_bits(alone), _bits(longer))
    print(f"W2VCONF rope D={D} {mode}: worst err / bound {worst:.3f}")
    assert bits == 0


def test_rope_rows_reports_the_fp16_range_and_refuses_a_short_table(L):
    x = torch.randn(7, 128, generator=torch.Generator().manual_seed(2))
    _, bits = run_rope(L, x, [3, 4], 64, FP16X)
    assert bits == 0
    x[5, 70] = 1.0e5
    _, bits = run_rope(L, x, [3, 4], 64, FP16X)
    assert bits & 1
    _, bits = run_rope(L, x, [3, 4], 64, FP32X)
    assert bits == 0
    a = L.RopeRowsArgs()
    t = torch.zeros(8, device=DEV)
    a.x = a.cos_t = a.sin_t = a.frame_offs = a.out_act = t.data_ptr()
    a.ldx = a.ldo_act = 128
    a.B, a.rows, a.D, a.dh, a.table_T, a.max_frames, a.mode = 1, 5, 128, 64, 4, 5, FP16X
    assert L.lib.ser_rope_rows_v(ctypes.byref(a), stream()) < 0 and b"table_T" in L.lib.ser_last_error()


# ------------------------------------------------------------------------------------------------------------- convolution module
CONV_FRAMES = (1, 14, 16, 99)


def conv_inputs(D, K, M, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, 2 * D, generator=g)
    w = torch.randn(D, K, generator=g) / math.sqrt(K)
    return y, w, 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def conv_bn_statement(y, w, scale, shift, frames, dtype):
    outs, o = [], 0
    for T in frames:
        outs.append(R.conv_mid(y[o: o + T].to(dtype), w.to(dtype), scale.to(dtype), shift.to(dtype)))
        o += T
    return torch.cat(outs).double()


def run_conv_bn(L, y, w, scale, shift, frames, mode):
    D, K = w.shape
    M, B = sum(frames), len(frames)
    yd, wd, sc, sh = y.to(DEV), w.t().contiguous().to(DEV), scale.to(DEV), shift.to(DEV)
    fo = torch.tensor(offsets(frames), dtype=torch.int32, device=DEV)
    out = torch.zeros(planes_of(mode), M, D, dtype=act_dtype(mode), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.ConformerConvBnArgs()
    a.y, a.ldy, a.w, a.scale, a.shift, a.frame_offs = yd.data_ptr(), 2 * D, wd.data_ptr(), sc.data_ptr(), sh.data_ptr(), fo.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = out.data_ptr(), D, M * D, flag.data_ptr()
    a.B, a.D, a.K, a.max_frames, a.rows, a.mode = B, D, K, max(frames), M, mode
    L.check(L.lib.ser_conformer_conv_bn_v(ctypes.byref(a), stream()), "ser_conformer_conv_bn_v")
    torch.cuda.synchronize()
    return out.cpu(), int(flag.item())


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("D,K", [(128, 3), (128, 31), (192, 3), (192, 31), (1280, 7)])
def test_conformer_conv_bn(L, D, K, mode):
    m = MODES[mode]
    frames = list(CONV_FRAMES)
    y, w, scale, shift = conv_inputs(D, K, sum(frames), D + K)
    ref = conv_bn_statement(y, w, scale, shift, frames, torch.float64)
    twin = conv_bn_statement(y, w, scale, shift, frames, torch.float32)
    out, bits = run_conv_bn(L, y, w, scale, shift, frames, m)
    e_twin = float((twin - ref).abs().max())
    err = float((act_value(out) - ref).abs().max())
    bound = 4.0 * e_twin + plane_term(m, float(ref.abs().max()))
    print(f"W2VCONF conv_bn D={D} K={K} {mode}: err {err:.3e} twin {e_twin:.3e} ratio {err / e_twin:.2f} bound {bound:.3e}")
    assert bits == 0 and err <= bound, (err, bound)
    offs = offsets(frames)
    for b in range(len(frames)):
        y2 = y.clone()                                                       # both neighbours full of 1e30: zeros outside are zeros
        if b > 0:
            y2[offs[b - 1]: offs[b]] = 1e30
        if b + 1 < len(frames):
            y2[offs[b + 1]: offs[b + 2]] = 1e30
        out2, _ = run_conv_bn(L, y2, w, scale, shift, frames, m)
        alone, _ = run_conv_bn(L, y[offs[b]: offs[b + 1]].contiguous(), w, scale, shift, [frames[b]], m)
        assert torch.equal(_bits(out2[:, offs[b]: offs[b + 1]]), _bits(alone)), (b, "poisoned neighbour")
        assert torch.equal(_bits(out[:, offs[b]: offs[b + 1]]), _bits(alone)), (b, "batch of one")


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
def test_conformer_conv_bn_keeps_its_bits_in_the_second_slab(L, mode):
    D, K, frames = 1280, 31, [1, 8, 9, 37]
    y, w, scale, shift = conv_inputs(D, K, sum(frames), D + K)
    out, bits = run_conv_bn(L, y, w, scale, shift, frames, MODES[mode])
    digest = planes_digest(out)
    print(f"W2VCONF ser_conformer_conv_bn_v D={D} K={K} {mode} digest {digest}")
    assert bits == 0 and digest == PARENT_CONV_BN_1280_DIGESTS[mode]


def test_conformer_conv_keeps_its_bits(L):
    """ser_conformer_conv_v (w2v-BERT's causal LayerNorm form) on one shape of tests/test_gpu_w2vbert.py::test_conformer_conv"""
    D, K, frames = 128, 7, [1, 2, 30, 31, 37, 5]
    g = torch.Generator().manual_seed(D + K)
    M = sum(frames)
    y = torch.randn(M, 2 * D, generator=g)
    w = torch.randn(D, K, generator=g) / math.sqrt(K)
    gamma, beta = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    yd, wd, gd, bd = y.to(DEV), w.t().contiguous().to(DEV), gamma.to(DEV), beta.to(DEV)
    fo = torch.tensor(offsets(frames), dtype=torch.int32, device=DEV)
    out = torch.zeros(2, M, D, dtype=torch.float16, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.ConformerConvArgs()
    a.y, a.ldy, a.w, a.gamma, a.beta, a.frame_offs = yd.data_ptr(), 2 * D, wd.data_ptr(), gd.data_ptr(), bd.data_ptr(), fo.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag, a.eps = out.data_ptr(), D, M * D, flag.data_ptr(), 1e-5
    a.B, a.D, a.K, a.max_frames, a.rows, a.mode = len(frames), D, K, max(frames), M, FP16X
    L.check(L.lib.ser_conformer_conv_v(ctypes.byref(a), stream()), "ser_conformer_conv_v")
    torch.cuda.synchronize()
    digest = hashlib.sha256(out.cpu().contiguous().view(torch.int16).numpy().tobytes()).hexdigest()
    print(f"W2VCONF ser_conformer_conv_v digest {digest}")
    assert digest == PARENT_CONV_DIGEST


# ------------------------------------------------------------------------------------------------- relative bias + attention
ATTN_TS = (1, 33, 99, 130)


def run_attention_rb(L, qa, P, off, Ts, H, mode, plain=False, P_T=None):
    """ser_relpos_bias_v + ser_attention_rb_v (or, with `plain`, ser_attention_v) on the operand planes qa [planes, M, 3 D];
    P fp32 [2 P_T, D] with row P_T + r = P(r)"""
    dh, D, M = 64, H * 64, sum(Ts)
    fo = torch.tensor(offsets(Ts), dtype=torch.int32, device=DEV)
    out = torch.zeros(planes_of(mode), M, D, dtype=act_dtype(mode), device=DEV)
    r = L.AttentionRbArgs()
    a = r.base
    a.qkv, a.ld, a.plane_stride, a.q_col, a.k_col, a.v_col, a.B = qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, len(Ts)
    a.frame_offs, a.max_frames, a.out, a.ldo, a.out_plane_stride = fo.data_ptr(), max(Ts), out.data_ptr(), D, M * D
    a.H, a.dh, a.scale, a.mode = H, dh, -1.0, mode
    pb = None
    if plain:
        L.check(L.lib.ser_attention_v(ctypes.byref(a), stream()), "ser_attention_v")
    else:
        ld_pb = -(-max(Ts) // 64) * 64
        Pd, od = P.to(DEV), off.to(DEV)
        pb = torch.full((M * H + 1, ld_pb), float("nan"), device=DEV)                   # a canary row behind the last
        t = L.RelposBiasArgs()
        t.qkv, t.ld, t.plane_stride, t.P, t.ldp, t.off = qa.data_ptr(), 3 * D, M * 3 * D, Pd.data_ptr(), D, od.data_ptr()
        t.frame_offs, t.pb, t.ld_pb = fo.data_ptr(), pb.data_ptr(), ld_pb
        t.q_col, t.B, t.H, t.dh, t.P_T, t.max_frames, t.rows, t.mode = 0, len(Ts), H, dh, P_T, max(Ts), M, mode
        L.check(L.lib.ser_relpos_bias_v(ctypes.byref(t), stream()), "ser_relpos_bias_v")
        r.pb, r.ld_pb = pb.data_ptr(), ld_pb
        L.check(L.lib.ser_attention_rb_v(ctypes.byref(r), stream()), "ser_attention_rb_v")
    torch.cuda.synchronize()
    if pb is not None:
        pb = pb.cpu()
        assert bool(torch.isnan(pb[-1]).all()), "ser_relpos_bias_v wrote behind its rows"
        pb = pb[:-1]
    return out.cpu(), pb


def attention_rb_inputs(H, M, P_T, mode):
    """operand planes of the packed q | k | v (q + u as the projection's epilogue leaves it: times c), the distance table P (row P_T + r =
    P(r)), off = (v - u) c, the two position biases and c"""
    dh, D = 64, H * 64
    g = torch.Generator().manual_seed(100 * H)
    c = dh ** -0.5 * 1.4426950408889634
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    P = torch.randn(2 * P_T, D, generator=g) * 0.7
    u, v = torch.randn(H, dh, generator=g) * 0.5, torch.randn(H, dh, generator=g) * 0.5
    pre = qkv.clone()
    pre[:, :D] = (pre[:, :D] + u.reshape(-1)) * c
    off = ((v.double() - u.double()) * c).reshape(-1).float()
    return to_act(pre, mode), P, off, u, v, c


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("H", [2, 3])
def test_relpos_bias_and_attention_rb(L, H, mode):
    m = MODES[mode]
    dh, D, Ts = 64, H * 64, list(ATTN_TS)
    M, P_T = sum(Ts), 256
    qa, P, off, u, v, c = attention_rb_inputs(H, M, P_T, m)
    qv = act_value(qa.cpu())
    offs = offsets(Ts)
    ref = torch.empty(M, D, dtype=torch.float64)
    bias_ref = []
    for b, T in enumerate(Ts):
        blk = qv[offs[b]: offs[b + 1]]
        qu, k, vv = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        qu = qu / c                                                                   # q + u
        Pw = P.double()[P_T - (T - 1): P_T + T].view(2 * T - 1, H, dh).transpose(0, 1)
        zero = torch.zeros(H, dh, dtype=torch.float64)
        s = R.relpos_scores(qu, k, Pw, zero, v.double() - u.double()) / math.sqrt(dh)  # (q + u) . k + (q + u + (v - u)) . P(i - j)
        bias_ref.append(s - qu @ k.transpose(1, 2) / math.sqrt(dh))
        ref[offs[b]: offs[b + 1]] = (torch.softmax(s, dim=-1) @ vv).permute(1, 0, 2).reshape(T, D)
    out, pb = run_attention_rb(L, qa, P, off, Ts, H, m, P_T=P_T)
    err = float((act_value(out) - ref).abs().max())
    tol = {BF16: 3e-2, FP32X: 1e-4, FP16X: 1e-4}[m]
    # the bias itself: fp32 FMAs over 64 terms of the operand planes' q, in the exp2 domain
    berr = 0.0
    for b, T in enumerate(Ts):
        got = pb[offs[b] * H: offs[b + 1] * H].view(T, H, -1).permute(1, 0, 2).double()
        berr = max(berr, float((got[:, :, :T] / 1.4426950408889634 - bias_ref[b]).abs().max()))
        assert not bool(got[:, :, T: -(-T // 64) * 64].any()), "keys T .. 64 ceil(T / 64) must be zeros"
    print(f"W2VCONF attention_rb H={H} {mode}: err {err:.3e} tol {tol:.0e}; bias err {berr:.3e}")
    assert err < tol and berr < 1e-4, (err, berr)
    # P = 0 and off = 0: the accumulators start at +0 as in the plain form -- the same bits
    zero, _ = run_attention_rb(L, qa, torch.zeros_like(P), torch.zeros_like(off), Ts, H, m, P_T=P_T)
    plain, _ = run_attention_rb(L, qa, None, None, Ts, H, m, plain=True)
    assert torch.equal(_bits(zero), _bits(plain))
    # every utterance alone, and a longer distance table, give the batch's bits
    for b, T in enumerate(Ts):
        P2 = torch.zeros(2 * 512, D)
        P2[512 - P_T: 512 + P_T] = P
        alone, pb1 = run_attention_rb(L, qa[:, offs[b]: offs[b + 1]].contiguous(), P2, off, [T], H, m, P_T=512)
        assert torch.equal(_bits(alone), _bits(out[:, offs[b]: offs[b + 1]])), (b, "batch of one")
        assert torch.equal(_bits(pb1[:, : -(-T // 64) * 64]), _bits(pb[offs[b] * H: offs[b + 1] * H, : -(-T // 64) * 64]))


def test_attention_rb_keeps_its_bits(L):
    H, Ts, P_T = 3, list(ATTN_TS), 256
    qa, P, off, _, _, _ = attention_rb_inputs(H, sum(Ts), P_T, FP16X)
    out, _ = run_attention_rb(L, qa, P, off, Ts, H, FP16X, P_T=P_T)
    digest = planes_digest(out)
    print(f"W2VCONF ser_attention_rb_v H={H} f16x digest {digest}")
    assert digest == PARENT_ATTENTION_RB_DIGEST


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def fixtures(golden_dir):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
    out = []
    for tag, gname in CASES:
        geo = getattr(C, gname)
        gold = np.load(os.path.join(golden_dir, tag + ".npz"))
        sd = synthetic_state_dict(geo, int(gold["seed"]))
        assert state_dict_digest(sd) == str(gold["digest"])
        lengths = [int(n) for n in gold["lengths"]]
        assert lengths == [400, 5500, 32000, 52000]
        waves = [R.synth_wave(int(gold[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
        out.append(dict(geo=geo, sd=sd, waves=waves, lengths=lengths, states=[torch.from_numpy(gold[f"states_{j}"]) for j in range(len(lengths))]))
    return out


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("case", [0, 1])
def test_end_to_end_against_hf(fixtures, case, mode):
    from interspeech_ser_amd.engine import ConformerSpeechEncoder, build_encoder
    fx = fixtures[case]
    geo = fx["geo"]
    enc = build_encoder(geo, fx["sd"], DEV, mode)
    assert isinstance(enc, ConformerSpeechEncoder)
    waves, lengths = fx["waves"], fx["lengths"]
    enc.use_tape = False                                                      # eager: one launch per kernel
    eager = enc.forward(enc.upload(waves), lengths)
    assert eager.take_range_bits() == 0 and len(eager) == geo.num_layers + 1
    eager_states = eager.states.clone()
    worst = 0.0
    for b, n in enumerate(lengths):
        assert eager.frames(b) == enc.frames(n) == fx["states"][b].shape[1] == (1, 16, 99, 162)[b]
        for layer in range(geo.num_layers + 1):
            worst = max(worst, rel_err(eager.utterance(b, layer).cpu(), fx["states"][b][layer]))
    print(f"W2VCONF e2e {geo.name} {mode}: worst {worst:.3e} (gate {E2E_TOL[mode]:.0e})")
    assert worst < E2E_TOL[mode], worst
    # the recorded command list: its first replay and a second one give the eager forward's bits
    enc.use_tape = True
    for _ in range(2):
        hs = enc.forward(enc.upload(waves), lengths)
        assert hs.take_range_bits() == 0 and torch.equal(_bits(hs.states), _bits(eager_states))
    # the ragged batch is its batches of one
    offs = eager.frame_offs
    for b, w in enumerate(waves):
        one = enc.forward(enc.upload([w]), [lengths[b]], slot=1)
        assert one.take_range_bits() == 0 and torch.equal(_bits(one.states), _bits(eager_states[:, offs[b]: offs[b + 1]])), b
    # a slot that starts small: its arena (and its position tables) grow under a recorded list, then hold a subset and the full batch
    for pick in ([0], [1, 2], [3, 0], [0, 1, 2, 3]):
        hs = enc.forward(enc.upload([waves[b] for b in pick]), [lengths[b] for b in pick], slot=2)
        want = torch.cat([eager_states[:, offs[b]: offs[b + 1]] for b in pick], dim=1)
        assert hs.take_range_bits() == 0 and torch.equal(_bits(hs.states), _bits(want)), pick
    # a state asked for alone stops the replay there and is the full forward's
    part = enc.forward(enc.upload(waves), lengths, last_state=1)
    assert part.computed == 2 and torch.equal(_bits(part.states[1]), _bits(eager_states[1]))
    assert part.take_range_bits() == 0


def test_other_modes_are_refused_by_the_encoder_and_replaced_by_the_driver(fixtures, capsys):
    from interspeech_ser_amd.driver import _Extractor
    from interspeech_ser_amd.engine import ConformerSpeechEncoder
    fx = fixtures[0]
    with pytest.raises(ValueError):
        ConformerSpeechEncoder(fx["geo"], fx["sd"], DEV, "f16mf")
    assert _Extractor.supported_mode(fx["geo"], "f16mf", False, "facebook/wav2vec2-conformer-rope-large") == "f16x"
    assert capsys.readouterr().out.count("using f16x") == 1
    assert _Extractor.supported_mode(fx["geo"], "bf16", False, "facebook/wav2vec2-conformer-rope-large") == "bf16"


# ------------------------------------------------------------------------------------------------------- drivers and predictor
def write_wav(path, x, rate=16000):
    pcm = (np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def _snapshot(tmp_path, geo):
    snap = tmp_path / ("w2v-conformer-tiny-" + geo.position_type)
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(dict(
        model_type="wav2vec2-conformer", hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
        intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel), conv_stride=list(geo.conv_stride),
        conv_bias=geo.conv_bias, feat_extract_norm="layer", hidden_act="swish", position_embeddings_type=geo.position_type,
        rotary_embedding_base=geo.rotary_base, max_source_positions=geo.max_source_positions,
        conv_depthwise_kernel_size=geo.conv_depthwise_kernel, layer_norm_eps=1e-5, add_adapter=False)))
    (snap / "preprocessor_config.json").write_text(json.dumps(dict(
        feature_extractor_type="Wav2Vec2FeatureExtractor", feature_size=1, do_normalize=True, sampling_rate=16000)))
    return snap


@pytest.mark.parametrize("case", [0, 1])
def test_speech_driver_on_a_snapshot_directory(fixtures, case, tmp_path, capsys):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.engine import build_encoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = fixtures[case]["geo"]
    snap = _snapshot(tmp_path, geo)
    assert C.resolve_geometry(str(snap)) == C.geometry_from_config(json.loads((snap / "config.json").read_text()), name=str(snap))
    wav_dir, out = tmp_path / "wavs", tmp_path / "feats"
    wav_dir.mkdir()
    lens = dict(a=400, b=16160, c=7000, short=300)
    waves = {k: write_wav(wav_dir / f"{k}.wav", R.synth_wave(7 + i, n)) for i, (k, n) in enumerate(lens.items())}
    rc = driver.run_speech(["--ssl_type", str(snap), "--wav_dir", str(wav_dir), "--save_path", str(out), "--synthetic_weights",
                            "--mode", "f16x", "--use_n_layer", "--n_layer", "2", "--batch_size", "4"])
    text = capsys.readouterr().out
    assert rc == 0, text
    fails = [ln for ln in text.splitlines() if ln.startswith("Failed to process")]
    assert len(fails) == 1 and "short.wav" in fails[0], text
    assert sorted(os.listdir(out)) == ["a.pt", "b.pt", "c.pt"]
    rgeo = C.resolve_geometry(str(snap))
    enc = build_encoder(rgeo, synthetic_state_dict(rgeo, 7), DEV, "f16x")     # --seed default
    for k in ("a", "b", "c"):
        got = torch.load(out / f"{k}.pt")
        assert got.dtype == torch.float32 and tuple(got.shape) == (geo.frames_for(lens[k]), geo.hidden)
        want = enc.forward(enc.upload([waves[k]]), [lens[k]]).utterance(0, 2).cpu()
        assert torch.equal(_bits(got), _bits(want)), k
    if case == 0:
        # a 44.1 kHz file with --resample: frames(ceil(n 16000 / 44100)) rows
        wav2, out2 = tmp_path / "wavs44", tmp_path / "feats44"
        wav2.mkdir()
        n44 = 30011
        write_wav(wav2 / "hi.wav", R.synth_wave(3, n44), rate=44100)
        rc = driver.run_speech(["--ssl_type", str(snap), "--wav_dir", str(wav2), "--save_path", str(out2), "--synthetic_weights",
                                "--mode", "f16x", "--resample"])
        text = capsys.readouterr().out
        assert rc == 0 and "Failed to process" not in text, text
        n16 = -(-n44 * 16000 // 44100)
        assert tuple(torch.load(out2 / "hi.pt").shape) == (geo.frames_for(n16), geo.hidden)


def test_fusion_predictor_behind_the_encoder(fixtures):
    import fusion_ref as FR
    from interspeech_ser_amd.engine import FusionHead, build_encoder
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, RowsStream, gather_rows
    from oracle.fusion_head import seeded_head_weights
    fx = fixtures[0]
    geo = fx["geo"]
    enc = build_encoder(geo, fx["sd"], DEV, "f16x")
    sd = seeded_head_weights(FR.head_shapes(geo.hidden, 64, h=64), 31)
    rng = np.random.default_rng(4)
    waves = fx["waves"][1:3]
    rows = [rng.standard_normal((7, 64)).astype(np.float32), rng.standard_normal((21, 64)).astype(np.float32)]
    pred = FusionPredictor([AudioStream(enc), RowsStream(64)], sd)
    got = pred.predict(waves, rows=rows)
    (src1, o1, _), (x2, o2, _) = pred.features(waves, rows=rows)
    assert o1 == [0, enc.frames(len(waves[0])), enc.frames(len(waves[0])) + enc.frames(len(waves[1]))]
    head = FusionHead(sd, geo.hidden, 64, DEV, "f16x")
    direct = head.forward(gather_rows(src1, o1), o1, x2, o2).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert got.shape == (2, 8) and np.array_equal(direct.view(np.int32), got.view(np.int32))


# ---------------------------------------------------------------------------------------------------- audio classification head
CLS_EPS = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}                   # tests/test_gpu_audio_cls.py's EPS_OTHER: this file's end-to-end gates


def _cls_fixture():
    import audio_cls_ref as AR

    class Fx(AR.Fixture):
        def hf_state_dict(self):
            """wrapper prefix + encoder tensors, and the head's, under Wav2Vec2ConformerForSequenceClassification's names"""
            from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
            enc = synthetic_state_dict(self.geometry(), self.seed)
            assert state_dict_digest(enc) == self.digest
            sd = {"wav2vec2_conformer." + k: v for k, v in enc.items()}
            sd.update({k: torch.from_numpy(np.array(v)) for k, v in self.head.items()})
            return sd
    return Fx("tiny_cls_w2v_conformer")


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_audio_classifier_matches_hf_float64(mode):
    """tests/test_gpu_audio_cls.py::test_predict_matches_hf_float64 on the conformer fixture: the three waveforms as one ragged batch and
    each alone are bit-equal, inside the bound of HF's float64 logits, with HF's label wherever its top-two margin exceeds twice the bound"""
    from interspeech_ser_amd.classify import AudioClassifier
    from interspeech_ser_amd.engine import ConformerSpeechEncoder
    from interspeech_ser_amd.weights import normalize_names
    fx = _cls_fixture()
    waves = fx.waves()
    assert fx.spec().architecture == "Wav2Vec2ConformerForSequenceClassification"
    clf = AudioClassifier(fx.geometry(), fx.spec(), normalize_names(fx.hf_state_dict()), DEV, mode, batch_size=16,
                          normalize=bool(fx.preprocessor.get("do_normalize", True)))
    assert clf.mode == mode and clf.labels == fx.spec().labels and isinstance(clf.enc, ConformerSpeechEncoder)
    ragged = clf.predict(waves)
    alone = np.stack([clf.predict([w])[0] for w in waves])
    assert ragged.shape == (3, fx.spec().num_labels) and not clf.failed
    assert np.array_equal(ragged.view(np.uint32), alone.view(np.uint32))
    eps, wide = CLS_EPS[mode], 0
    for j in range(3):
        bound = fx.logit_bound(eps, j)
        err = np.abs(ragged[j].astype(np.float64) - fx.logits64[j])
        print(f"W2VCONF audio_cls {mode} wave {j}: worst err / bound {float((err / bound).max()):.3e} (bound {float(bound.max()):.3e})")
        assert (err <= bound).all(), (j, float((err / bound).max()))
        top = np.sort(fx.logits64[j])[::-1]
        if top[0] - top[1] > 2 * bound.max():
            wide += 1
            assert int(np.argmax(ragged[j])) == int(np.argmax(fx.logits64[j]))
    if eps <= 1e-3:
        assert wide >= 2
