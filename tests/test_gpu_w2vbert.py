"""GPU: w2v-BERT 2.0 on libserhip -- the five kernels against float64 statements, the encoder end to end against the HF fixtures, the
speech driver and the predictor behind it.

Bounds.
* ser_fbank_v: everything up to the log runs in float64; what fp32 adds is the ONE rounding of a stored log-mel value (e = half an fp32
  ulp at the largest |log-mel| of the statement) and the one rounding of the stored row.  A normalised value z = (x - mean) / sd moves by at
  most 2 e / sd through its numerator and |z| sqrt(2) e / sd through sd (every sample moving by e moves an unbiased standard deviation of
  F >= 2 samples by at most e sqrt(F / (F - 1)) <= e sqrt(2)):  (2 + sqrt(2) max|z|) e / min sd + half an fp32 ulp at max|z|.  The inputs
  are chosen so that the statement's own min sd stays above 0.1 (asserted).
* ser_conformer_conv_v: tests/test_gpu_codec.py's convention -- at most 4 x the distance of the same arithmetic in torch fp32 from the
  float64 statement, plus what the operand planes' format cannot hold: half a bf16 ulp of the output magnitude in bf16, half a bf16 ulp of
  the lo plane (itself at most half a bf16 ulp of the output) in fp32x; nothing in f16x.
* ser_swish_rows_v: fp32 x / (1 + expf(-x)): expf 1 ulp (HIP math API), the add, the division and the product half an ulp each: 2.5 ulp
  relative, gated at 4; plus the same plane terms (f16x: hi + lo keep 22 bits, half an fp16 ulp of the lo plane).
* ser_attention_rk_v: tests/test_gpu_kernels.py::test_attention's per-mode bounds (3e-2 bf16, 1e-4 fp32x / f16x); the bias adds one fp32
  term per logit.
* end to end: tests/test_gpu_e2e.py's gates, max|a - b| / max(1, max|b|) < 1e-3 (f16x, fp32x), 3e-2 (bf16).

Measured on an MI355X: profiles/w2v_bert.txt.
"""
import hashlib
import json
import math
import os
import wave

import numpy as np
import pytest
import torch

import w2vbert_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, FP32X, FP16X = 1, 2, 4
MODES = {"bf16": BF16, "fp32x": FP32X, "f16x": FP16X}
E2E_TOL = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}
CASES = (("tiny_w2v_bert_d128h2", "TINY_W2V_BERT"), ("tiny_w2v_bert_d192h3", "TINY_W2V_BERT_H3"))
# sha256 of output planes from the library built at the commit before the two conformer families were put on one convolution body and one
# biased-attention launcher: the kernels keep their bits.
# ser_conformer_conv_v: D 1280 (the second 1024-column slab partly filled), K 31, frames (1, 8, 9, 37) -- a window longer than the
# utterance, one SER_CCONV_TILE, a tile plus one row, several tiles -- conv_inputs seed 1311
PARENT_CONV_1280_DIGESTS = {
    "bf16": "d1d9aea5549f543156b95e4422650c34a46a8c724e00e72cc9ce999566421f71",
    "fp32x": "98f1cfc1eb37aedc9c4a6f458204ee9d71aa25f10127a0bc7cef4332de27b3d9",
    "f16x": "c1327ff3c990bc9d65a5012745be3a8ca2056fa93304fbce84b7af802813a388",
}
# ser_relkey_table_v + ser_attention_rk_v: H 3, left_max 64, right_max 8, frames (1, 33, 99, 130), f16x, attention_rk_inputs seed 364
PARENT_ATTENTION_RK_DIGEST = "53330386ef15f2e9e6080c27d08ef8cff45152e1406cbe30e2603b48dc4e6302"


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
    """what the operand planes of `mode` cannot hold of a value of magnitude amax (see the module docstring)"""
    if mode == BF16:
        return 0.5 * ulp_bf16(amax)
    if mode == FP32X:
        return 0.5 * ulp_bf16(0.5 * ulp_bf16(amax))
    return 0.0


def act_dtype(mode):
    return torch.float16 if mode == FP16X else torch.bfloat16


def planes_of(mode):
    return 1 if mode == BF16 else 2


def to_act(x, mode):
    """fp32 CPU [rows, cols] -> device operand planes as ser_split_bf16 makes them: bf16, bf16 hi + lo, fp16 hi + lo"""
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


# --------------------------------------------------------------------------------------------------------------------------- fbank
FBANK_LENGTHS = (560, 720, 1055, 16160)


def run_fbank(L, waves):
    from interspeech_ser_amd.frontend import w2vbert_dft_table, w2vbert_mel_filters, w2vbert_mel_frames
    melw, rng = w2vbert_mel_filters(80)
    Fr = [w2vbert_mel_frames(len(w)) for w in waves]
    T = [f // 2 for f in Fr]
    B, M = len(waves), sum(T)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    wav = dev(np.concatenate(waves), torch.float32)
    so = dev(np.concatenate([[0], np.cumsum([len(w) for w in waves])]), torch.int64)
    mo = dev(np.concatenate([[0], np.cumsum(Fr)]), torch.int32)
    fo = dev(np.concatenate([[0], np.cumsum(T)]), torch.int32)
    dft, mw, mr = dev(w2vbert_dft_table(), torch.float64), dev(melw, torch.float64), dev(rng, torch.int32)
    work = torch.full((sum(Fr), 80), float("nan"), device=DEV)
    out = torch.full((M + 2, 160), float("nan"), device=DEV)              # a canary row on either side
    a = L.FbankArgs()
    a.wav, a.sample_offs, a.mel_offs, a.frame_offs = wav.data_ptr(), so.data_ptr(), mo.data_ptr(), fo.data_ptr()
    a.dft, a.melw, a.mel_range, a.work = dft.data_ptr(), mw.data_ptr(), mr.data_ptr(), work.data_ptr()
    a.out, a.ldo, a.B, a.max_mel_frames, a.n_mels, a.stride = out[1:].data_ptr(), 160, B, max(Fr), 80, 2
    import ctypes
    L.check(L.lib.ser_fbank_v(ctypes.byref(a), stream()), "ser_fbank_v")
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool(torch.isnan(host[0]).all()) and bool(torch.isnan(host[-1]).all()), "ser_fbank_v wrote outside its rows"
    assert not bool(torch.isnan(host[1:-1]).any()), "ser_fbank_v left a row unwritten"
    return host[1:-1], np.concatenate([[0], np.cumsum(T)])


def test_fbank_equals_the_float64_statement_and_a_batch_of_one(L):
    waves = [R.synth_wave(40 + i, n) for i, n in enumerate(FBANK_LENGTHS)]
    got, offs = run_fbank(L, waves)
    for b, w in enumerate(waves):
        lm = R.log_mel(w)
        sd = lm.std(0, ddof=1)
        ref = R.fbank_rows(w)
        assert sd.min() > 0.1, (len(w), sd.min())                             # the inputs keep the normalisation well conditioned
        zmax = float(np.abs(ref).max())
        e = 0.5 * ulp32(float(np.abs(lm).max()))
        bound = (2.0 + math.sqrt(2.0) * zmax) * e / float(sd.min()) + 0.5 * ulp32(zmax)
        mine = got[offs[b]: offs[b + 1]]
        err = float(np.abs(mine.numpy().astype(np.float64) - ref).max())
        print(f"W2VBERT fbank {len(w)} samples -> {ref.shape[0]} rows: err {err:.3e} bound {bound:.3e} (min sd {sd.min():.3f}, max|z| {zmax:.2f})")
        assert mine.shape == ref.shape and err <= bound, (len(w), err, bound)
        alone, _ = run_fbank(L, [w])
        assert torch.equal(_bits(alone), _bits(mine)), len(w)


# ------------------------------------------------------------------------------------------------------------- convolution module
CONV_FRAMES = (1, 2, 30, 31, 37, 5)


def conv_statement(y, w, gamma, beta, frames, dtype):
    """GLU -> causal depthwise conv per utterance -> LayerNorm -> swish, in `dtype` (float64: the statement; float32: the torch twin)"""
    y, w, gamma, beta = y.to(dtype), w.to(dtype), gamma.to(dtype), beta.to(dtype)
    D, K = w.shape
    outs, o = [], 0
    for T in frames:
        h = y[o: o + T]
        g = h[:, :D] * torch.sigmoid(h[:, D:])
        gp = torch.cat([torch.zeros(K - 1, D, dtype=dtype), g], 0)
        u = torch.zeros(T, D, dtype=dtype)
        for k in range(K):
            u = u + gp[k: k + T] * w[:, k][None, :]
        t = torch.nn.functional.layer_norm(u, (D,), gamma, beta, 1e-5)
        outs.append(t * torch.sigmoid(t))
        o += T
    return torch.cat(outs).double()


def run_conv(L, y, w, gamma, beta, frames, mode):
    import ctypes
    D, K = w.shape
    M, B = sum(frames), len(frames)
    yd, wd, gd, bd = y.to(DEV), w.t().contiguous().to(DEV), gamma.to(DEV), beta.to(DEV)
    fo = torch.tensor(np.concatenate([[0], np.cumsum(frames)]), dtype=torch.int32, device=DEV)
    out = torch.zeros(planes_of(mode), M, D, dtype=act_dtype(mode), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.ConformerConvArgs()
    a.y, a.ldy, a.w, a.gamma, a.beta, a.frame_offs = yd.data_ptr(), 2 * D, wd.data_ptr(), gd.data_ptr(), bd.data_ptr(), fo.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag, a.eps = out.data_ptr(), D, M * D, flag.data_ptr(), 1e-5
    a.B, a.D, a.K, a.max_frames, a.rows, a.mode = B, D, K, max(frames), M, mode
    L.check(L.lib.ser_conformer_conv_v(ctypes.byref(a), stream()), "ser_conformer_conv_v")
    torch.cuda.synchronize()
    return out.cpu(), int(flag.item())


def conv_inputs(D, K, M, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(M, 2 * D, generator=g)
    w = torch.randn(D, K, generator=g) / math.sqrt(K)
    return y, w, 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("D,K", [(128, 7), (128, 31), (1024, 7), (1024, 31), (1280, 7)])
def test_conformer_conv(L, D, K, mode):
    m = MODES[mode]
    frames = list(CONV_FRAMES)
    y, w, gamma, beta = conv_inputs(D, K, sum(frames), D + K)
    ref = conv_statement(y, w, gamma, beta, frames, torch.float64)
    twin = conv_statement(y, w, gamma, beta, frames, torch.float32)
    out, bits = run_conv(L, y, w, gamma, beta, frames, m)
    e_twin = float((twin - ref).abs().max())
    err = float((act_value(out) - ref).abs().max())
    bound = 4.0 * e_twin + plane_term(m, float(ref.abs().max()))
    print(f"W2VBERT conv D={D} K={K} {mode}: err {err:.3e} twin {e_twin:.3e} ratio {err / e_twin:.2f} bound {bound:.3e}")
    assert bits == 0 and err <= bound, (err, bound)
    # isolation: utterance b - 1 full of 1e4 changes no bit of utterance b, which equals its batch of one
    offs = np.concatenate([[0], np.cumsum(frames)])
    for b in range(1, len(frames)):
        y2 = y.clone()
        y2[offs[b - 1]: offs[b]] = 1e4
        out2, _ = run_conv(L, y2, w, gamma, beta, frames, m)
        alone, _ = run_conv(L, y[offs[b]: offs[b + 1]].contiguous(), w, gamma, beta, [frames[b]], m)
        assert torch.equal(_bits(out2[:, offs[b]: offs[b + 1]]), _bits(alone)), (b, "poisoned neighbour")
        assert torch.equal(_bits(out[:, offs[b]: offs[b + 1]]), _bits(alone)), (b, "batch of one")


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
def test_conformer_conv_keeps_its_bits_in_the_second_slab(L, mode):
    D, K, frames = 1280, 31, [1, 8, 9, 37]
    y, w, gamma, beta = conv_inputs(D, K, sum(frames), D + K)
    out, bits = run_conv(L, y, w, gamma, beta, frames, MODES[mode])
    digest = planes_digest(out)
    print(f"W2VBERT ser_conformer_conv_v D={D} K={K} {mode} digest {digest}")
    assert bits == 0 and digest == PARENT_CONV_1280_DIGESTS[mode]


def test_conformer_conv_reports_the_fp16_range(L):
    y, w, gamma, beta = conv_inputs(128, 7, 9, 5)
    _, bits = run_conv(L, y, w, gamma, beta, [4, 5], FP16X)
    assert bits == 0
    _, bits = run_conv(L, y, w, gamma * 1e5, beta, [4, 5], FP16X)             # LayerNorm outputs of ~1e5: swish keeps them beyond 65 504
    assert bits & 1
    _, bits = run_conv(L, y, w, gamma * 1e5, beta, [4, 5], FP32X)             # bf16 planes have fp32's range: no guard
    assert bits == 0


# --------------------------------------------------------------------------------------------------------------------- swish rows
@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("rows,D", [(37, 256), (5, 4096)])
def test_swish_rows(L, rows, D, mode):
    import ctypes
    m = MODES[mode]
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows + D)) * 3.0
    ref = x.double() * torch.sigmoid(x.double())
    out = torch.zeros(planes_of(m), rows, D, dtype=act_dtype(m), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    a = L.SwishRowsArgs()
    a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = xd.data_ptr(), D, out.data_ptr(), D, rows * D, flag.data_ptr()
    a.mode, a.rows, a.D = m, rows, D
    L.check(L.lib.ser_swish_rows_v(ctypes.byref(a), stream()), "ser_swish_rows_v")
    torch.cuda.synchronize()
    amax = float(ref.abs().max())
    f16x_term = 0.5 * ulp_f16(0.5 * ulp_f16(amax)) if m == FP16X else 0.0
    bound = 4.0 * 2.0 ** -24 * amax + plane_term(m, amax) + f16x_term
    err = float((act_value(out.cpu()) - ref).abs().max())
    print(f"W2VBERT swish [{rows}, {D}] {mode}: err {err:.3e} bound {bound:.3e}")
    assert int(flag.item()) == 0 and err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------------- relative-key attention
ATTN_TS = (1, 9, 70, 200)


def run_attention_rk(L, qa, E, Ts, H, Lm, Rm, mode, plain=False):
    """ser_relkey_table_v + ser_attention_rk_v (or, with `plain`, ser_attention_v) on the operand planes qa [P, M, 3 D]"""
    import ctypes
    dh, D, M = 64, H * 64, sum(Ts)
    P = Lm + Rm + 1
    ld_qe = (P + 3) // 4 * 4
    fo = torch.tensor(np.concatenate([[0], np.cumsum(Ts)]), dtype=torch.int32, device=DEV)
    out = torch.zeros(planes_of(mode), M, D, dtype=act_dtype(mode), device=DEV)
    r = L.AttentionRkArgs()
    a = r.base
    a.qkv, a.ld, a.plane_stride, a.q_col, a.k_col, a.v_col, a.B = qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, len(Ts)
    a.frame_offs, a.max_frames, a.out, a.ldo, a.out_plane_stride = fo.data_ptr(), max(Ts), out.data_ptr(), D, M * D
    a.H, a.dh, a.scale, a.mode = H, dh, -1.0, mode
    if plain:
        L.check(L.lib.ser_attention_v(ctypes.byref(a), stream()), "ser_attention_v")
    else:
        Ed = E.to(DEV)
        qe = torch.full((M * H, ld_qe), float("nan"), device=DEV)
        t = L.RelkeyTableArgs()
        t.qkv, t.ld, t.plane_stride, t.E, t.qe, t.ld_qe = qa.data_ptr(), 3 * D, M * 3 * D, Ed.data_ptr(), qe.data_ptr(), ld_qe
        t.q_col, t.rows, t.H, t.dh, t.P, t.mode = 0, M, H, dh, P, mode
        L.check(L.lib.ser_relkey_table_v(ctypes.byref(t), stream()), "ser_relkey_table_v")
        r.qe, r.ld_qe, r.left_max, r.right_max = qe.data_ptr(), ld_qe, Lm, Rm
        L.check(L.lib.ser_attention_rk_v(ctypes.byref(r), stream()), "ser_attention_rk_v")
    torch.cuda.synchronize()
    return out.cpu()


def attention_rk_inputs(H, Lm, Rm, M, mode):
    """operand planes of the packed q | k | v (q as the projection's epilogue leaves it: times c), the distance embedding E, and c"""
    dh, D = 64, H * 64
    g = torch.Generator().manual_seed(100 * H + Lm)
    c = dh ** -0.5 * 1.4426950408889634
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    E = torch.randn(Lm + Rm + 1, dh, generator=g) * 0.5
    pre = qkv.clone()
    pre[:, :D] *= c
    return to_act(pre, mode), E, c


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("H,Lm,Rm", [(2, 64, 8), (3, 64, 8), (2, 5, 3), (3, 5, 3)])
def test_attention_rk(L, H, Lm, Rm, mode):
    m = MODES[mode]
    dh, D, Ts = 64, H * 64, list(ATTN_TS)
    M = sum(Ts)
    qa, E, c = attention_rk_inputs(H, Lm, Rm, M, m)
    qv = act_value(qa.cpu())
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        blk = qv[offs[b]: offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        q = q / c
        s = (q @ k.transpose(1, 2) + R.relkey_bias(q, E.double(), Lm, Rm)) / math.sqrt(dh)
        ref[offs[b]: offs[b + 1]] = (torch.softmax(s, dim=-1) @ v).permute(1, 0, 2).reshape(T, D)
    out = run_attention_rk(L, qa, E, Ts, H, Lm, Rm, m)
    err = float((act_value(out) - ref).abs().max())
    tol = {BF16: 3e-2, FP32X: 1e-4, FP16X: 1e-4}[m]
    print(f"W2VBERT attention_rk H={H} Lm={Lm} Rm={Rm} {mode}: err {err:.3e} tol {tol:.0e}")
    assert err < tol, err
    # E = 0: the accumulators start at +0 as in the plain form -- the same bits
    zero = run_attention_rk(L, qa, torch.zeros_like(E), Ts, H, Lm, Rm, m)
    plain = run_attention_rk(L, qa, None, Ts, H, Lm, Rm, m, plain=True)
    assert torch.equal(_bits(zero), _bits(plain))


def test_attention_rk_keeps_its_bits(L):
    H, Lm, Rm, Ts = 3, 64, 8, [1, 33, 99, 130]
    qa, E, _ = attention_rk_inputs(H, Lm, Rm, sum(Ts), FP16X)
    digest = planes_digest(run_attention_rk(L, qa, E, Ts, H, Lm, Rm, FP16X))
    print(f"W2VBERT ser_attention_rk_v H={H} Lm={Lm} Rm={Rm} f16x digest {digest}")
    assert digest == PARENT_ATTENTION_RK_DIGEST


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
        waves = [R.synth_wave(int(gold[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
        out.append(dict(geo=geo, sd=sd, waves=waves, lengths=lengths, states=[torch.from_numpy(gold[f"states_{j}"]) for j in range(len(lengths))]))
    return out


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("case", [0, 1])
def test_end_to_end_against_hf(fixtures, case, mode):
    from interspeech_ser_amd.engine import W2vBertEncoder, build_encoder
    fx = fixtures[case]
    geo = fx["geo"]
    enc = build_encoder(geo, fx["sd"], DEV, mode)
    assert isinstance(enc, W2vBertEncoder)
    waves, lengths = fx["waves"], fx["lengths"]
    enc.use_tape = False                                                      # eager: one launch per kernel
    eager = enc.forward(enc.upload(waves), lengths)
    assert eager.take_range_bits() == 0 and len(eager) == geo.num_layers + 1
    eager_states = eager.states.clone()
    worst = 0.0
    for b, n in enumerate(lengths):
        assert eager.frames(b) == enc.frames(n) == fx["states"][b].shape[1]
        for layer in range(geo.num_layers + 1):
            worst = max(worst, rel_err(eager.utterance(b, layer).cpu(), fx["states"][b][layer]))
    print(f"W2VBERT e2e {geo.name} {mode}: worst {worst:.3e} (gate {E2E_TOL[mode]:.0e})")
    assert worst < E2E_TOL[mode], worst
    # the recorded command list: its first replay and a second one give the eager forward's bits
    enc.use_tape = True
    for _ in range(2):
        hs = enc.forward(enc.upload(waves), lengths)
        assert hs.take_range_bits() == 0 and torch.equal(_bits(hs.states), _bits(eager_states))
    # the ragged batch of three is three batches of one
    offs = eager.frame_offs
    for b, w in enumerate(waves):
        one = enc.forward(enc.upload([w]), [lengths[b]], slot=1)
        assert torch.equal(_bits(one.states), _bits(eager_states[:, offs[b]: offs[b + 1]])), b
    # a slot that starts small: its arena grows under a recorded list (recorded again over the new buffers), then holds a subset and the
    # full batch again; every batch is its utterances' rows of the eager forward
    for pick in ([1], [0, 1, 2], [2, 0], [0, 1, 2]):
        hs = enc.forward(enc.upload([waves[b] for b in pick]), [lengths[b] for b in pick], slot=2)
        want = torch.cat([eager_states[:, offs[b]: offs[b + 1]] for b in pick], dim=1)
        assert hs.take_range_bits() == 0 and torch.equal(_bits(hs.states), _bits(want)), pick
    # a state asked for alone stops the replay there and is the full forward's
    part = enc.forward(enc.upload(waves), lengths, last_state=1)
    assert part.computed == 2 and torch.equal(_bits(part.states[1]), _bits(eager_states[1]))


def test_other_modes_are_refused_by_the_encoder_and_replaced_by_the_driver(fixtures, capsys):
    from interspeech_ser_amd.driver import _Extractor
    from interspeech_ser_amd.engine import W2vBertEncoder
    fx = fixtures[0]
    with pytest.raises(ValueError):
        W2vBertEncoder(fx["geo"], fx["sd"], DEV, "f16mf")
    assert _Extractor.supported_mode(fx["geo"], "f16mf", False, "facebook/w2v-bert-2.0") == "f16x"
    assert capsys.readouterr().out.count("using f16x") == 1
    assert _Extractor.supported_mode(fx["geo"], "bf16", False, "facebook/w2v-bert-2.0") == "bf16"


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
    snap = tmp_path / "w2v-bert-tiny"
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(dict(
        model_type="wav2vec2-bert", hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
        intermediate_size=geo.ffn, feature_projection_input_dim=160, hidden_act="swish", position_embeddings_type="relative_key",
        conv_depthwise_kernel_size=geo.conv_depthwise_kernel, left_max_position_embeddings=geo.left_max_positions,
        right_max_position_embeddings=geo.right_max_positions, layer_norm_eps=1e-5, add_adapter=False)))
    (snap / "preprocessor_config.json").write_text(json.dumps(dict(
        feature_extractor_type="SeamlessM4TFeatureExtractor", feature_size=80, num_mel_bins=80, stride=2, sampling_rate=16000)))
    return snap


def test_speech_driver_on_a_snapshot_directory(fixtures, tmp_path, capsys):
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.engine import build_encoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = fixtures[1]["geo"]
    snap = _snapshot(tmp_path, geo)
    wav_dir, out = tmp_path / "wavs", tmp_path / "feats"
    wav_dir.mkdir()
    lens = dict(a=560, b=16160, c=7000, short=500)
    waves = {k: write_wav(wav_dir / f"{k}.wav", R.synth_wave(7 + i, n)) for i, (k, n) in enumerate(lens.items())}
    rc = driver.run_speech(["--ssl_type", str(snap), "--wav_dir", str(wav_dir), "--save_path", str(out), "--synthetic_weights",
                            "--mode", "f16x", "--use_n_layer", "--n_layer", "2", "--batch_size", "4"])
    text = capsys.readouterr().out
    assert rc == 0, text
    fails = [ln for ln in text.splitlines() if ln.startswith("Failed to process")]
    assert len(fails) == 1 and "short.wav" in fails[0], text
    assert sorted(os.listdir(out)) == ["a.pt", "b.pt", "c.pt"]
    enc = build_encoder(geo, synthetic_state_dict(geo, 7), DEV, "f16x")       # --seed default
    for k in ("a", "b", "c"):
        got = torch.load(out / f"{k}.pt")
        assert got.dtype == torch.float32 and tuple(got.shape) == ((1 + (lens[k] - 400) // 160) // 2, geo.hidden)
        want = enc.forward(enc.upload([waves[k]]), [lens[k]]).utterance(0, 2).cpu()
        assert torch.equal(_bits(got), _bits(want)), k
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
    assert tuple(torch.load(out2 / "hi.pt").shape) == ((1 + (n16 - 400) // 160) // 2, geo.hidden)


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
    waves = fx["waves"][:2]
    rows = [rng.standard_normal((7, 64)).astype(np.float32), rng.standard_normal((21, 64)).astype(np.float32)]
    pred = FusionPredictor([AudioStream(enc), RowsStream(64)], sd)
    got = pred.predict(waves, rows=rows)
    (src1, o1, _), (x2, o2, _) = pred.features(waves, rows=rows)
    assert o1 == [0, enc.frames(len(waves[0])), enc.frames(len(waves[0])) + enc.frames(len(waves[1]))]
    head = FusionHead(sd, geo.hidden, 64, DEV, "f16x")
    direct = head.forward(gather_rows(src1, o1), o1, x2, o2).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert got.shape == (2, 8) and np.array_equal(direct.view(np.int32), got.view(np.int32))
