"""GPU: the bimodal fusion head as kernels (csrc/fusion.hip, engine.FusionHead, bimodal.BimodalPredictor, head.evaluate(engine="hip"))
against the float64 statement in tests/fusion_ref.py.

Gate of every comparison: device error against float64 <= 2 x max over the test's cases of (e_ref + e_split), where e_ref is the error of
the reference's own fp32 arithmetic and e_split the error operand rounding causes in the float64 statement -- what fp32 accumulation and
the operand width cost by themselves; the factor 2 covers the kernels' own accumulation order.  Each test prints the three numbers
(lines starting FUSION)."""
import csv
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fusion_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _offs(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _dev_rows(x, ld=None):
    """fp32 rows on the device at row pitch ``ld`` (default: contiguous); the padding columns hold NaN"""
    if ld is None:
        return _dev(x)
    t = torch.full((x.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    t[:, : x.shape[1]] = _dev(x)
    return t


def _report(what, err, e_ref, e_split):
    print(f"FUSION {what}: error {err:.3e}  e_ref {e_ref:.3e}  e_split {e_split:.3e}  gate {2.0 * (e_ref + e_split):.3e}")


def _split_f16(w):
    t = torch.as_tensor(w, dtype=torch.float32)
    hi = t.half()
    return torch.stack([hi, (t - hi.float()).half()]).contiguous()


# ------------------------------------------------------------------------------- ser_gru_v
class GruRunner:
    """one workspace, one error word and a launch counter for a sequence of launches (as engine.FusionHead keeps them per slot)"""

    def __init__(self, H, cluster):
        from interspeech_ser_amd import _lib
        r = ctypes.c_int32(0)
        self.H, self.cluster = H, cluster
        self.work_bytes = int(_lib.lib.ser_gru_work_bytes(H, cluster, ctypes.byref(r)))
        assert self.work_bytes >= 0
        self.R = r.value
        self.work = torch.zeros(max(self.work_bytes, 16), dtype=torch.uint8, device=DEV)
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.epoch = 1

    def __call__(self, gx, whh, bhh, lengths, mode=None):
        from interspeech_ser_amd import _lib
        H, offs = self.H, _offs(lengths)
        M, B = offs[-1], len(lengths)
        gxd, bd, wd = _dev(gx), _dev(bhh), _split_f16(whh).to(DEV)
        od = torch.tensor(offs, dtype=torch.int32, device=DEV)
        out = torch.full((M, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
        g = _lib.GruArgs()
        g.gx, g.ldgx, g.whh, g.whh_plane_stride, g.bhh, g.frame_offs = gxd.data_ptr(), 6 * H, wd.data_ptr(), 6 * H * H, bd.data_ptr(), od.data_ptr()
        g.out, g.ldo, g.work, g.work_bytes, g.err = out.data_ptr(), 2 * H, self.work.data_ptr(), self.work_bytes, self.err.data_ptr()
        act = None
        if mode is not None:
            planes, dt = {_lib.MODE_BF16: (1, torch.bfloat16), _lib.MODE_FP32X: (2, torch.bfloat16), _lib.MODE_FP16X: (2, torch.float16)}[mode]
            act = torch.zeros((planes, M, 2 * H), dtype=dt, device=DEV)
            g.out_act, g.ldo_act, g.out_plane_stride, g.mode = act.data_ptr(), 2 * H, M * 2 * H, mode
        g.B, g.H, g.rows, g.max_frames, g.cluster, g.epoch = B, H, M, max(lengths), self.cluster, self.epoch
        self.epoch += 1 + B // 16
        _lib.check(_lib.lib.ser_gru_v(ctypes.byref(g), torch.cuda.current_stream().cuda_stream), "ser_gru_v")
        torch.cuda.synchronize()
        assert int(self.err.item()) == 0, "ser_gru_v's error word is set"
        return out.cpu().numpy(), (None if act is None else act.float().sum(dim=0).cpu().numpy())


def _gru_inputs(H, lengths, seed):
    rng = np.random.default_rng(seed)
    M = sum(lengths)
    gx = rng.standard_normal((M, 6 * H)).astype(np.float32)
    whh = (rng.standard_normal((6 * H, H)) / np.sqrt(H)).astype(np.float32)
    bhh = (0.05 * rng.standard_normal(6 * H)).astype(np.float32)
    return gx, whh, bhh


def _gru_ref32(gx, whh, bhh, offs):
    """the recurrence in fp32 on the CPU (torch's convention and order), one utterance at a time"""
    H = whh.shape[1]
    out = np.zeros((gx.shape[0], 2 * H), dtype=np.float32)
    w, b = torch.from_numpy(whh), torch.from_numpy(bhh)
    for lo, hi in zip(offs[:-1], offs[1:]):
        for d in (0, 1):
            h = torch.zeros(H)
            wd, bd = w[d * 3 * H:(d + 1) * 3 * H], b[d * 3 * H:(d + 1) * 3 * H]
            for t in (range(hi - 1, lo - 1, -1) if d else range(lo, hi)):
                x = torch.from_numpy(gx[t, d * 3 * H:(d + 1) * 3 * H])
                gh = wd @ h + bd
                r = torch.sigmoid(x[:H] + gh[:H])
                z = torch.sigmoid(x[H:2 * H] + gh[H:2 * H])
                n = torch.tanh(x[2 * H:] + r * gh[2 * H:])
                h = (1 - z) * n + z * h
                out[t, d * H:(d + 1) * H] = h.numpy()
    return out


_GRU_REF = {}


def _gru_case(H, lengths, seed):
    key = (H, tuple(lengths), seed)
    if key not in _GRU_REF:
        gx, whh, bhh = _gru_inputs(H, lengths, seed)
        offs = _offs(lengths)
        ref = np.concatenate([R.bigru_from_gx(gx[a:b], whh, bhh) for a, b in zip(offs[:-1], offs[1:])])
        split = np.concatenate([R.bigru_from_gx(gx[a:b], whh, bhh, "f16x") for a, b in zip(offs[:-1], offs[1:])])
        _GRU_REF[key] = (gx, whh, bhh, ref, R.rel_err(_gru_ref32(gx, whh, bhh, offs), ref), R.rel_err(split, ref))
    return _GRU_REF[key]


GRU_LENGTHS = ((1, 2, 5, 37), (80,) * 17)            # ragged ends inside one column group; a second column group


@pytest.mark.parametrize("lengths", GRU_LENGTHS, ids=["1-2-5-37", "80x17"])
@pytest.mark.parametrize("H", [64, 512])
def test_gru_against_the_float64_statement(built_library, H, lengths):
    from interspeech_ser_amd import _lib
    cases = [_gru_case(H, ln, 7 + H) for ln in GRU_LENGTHS]
    gate = 2.0 * max(c[4] + c[5] for c in cases)
    gx, whh, bhh, ref, e_ref, e_split = _gru_case(H, lengths, 7 + H)
    run = GruRunner(H, 0)
    assert run.R == (1 if H == 64 else 32)
    got, act = run(gx, whh, bhh, lengths, mode=_lib.MODE_FP16X)
    err = R.rel_err(got, ref)
    _report(f"gru H={H} R={run.R} lengths={lengths[:4]}{'...' if len(lengths) > 4 else ''}", err, e_ref, e_split)
    assert np.isfinite(got).all() and err <= gate
    assert np.abs(act.astype(np.float64) - got).max() <= 2.0 ** -21         # the fp16 hi + lo operand copy of |h| < 1
    for mode, tol in ((_lib.MODE_BF16, 2.0 ** -8), (_lib.MODE_FP32X, 2.0 ** -16)):
        again, act = run(gx, whh, bhh, lengths, mode=mode)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.abs(act.astype(np.float64) - got).max() <= tol


@pytest.mark.parametrize("lengths", GRU_LENGTHS, ids=["1-2-5-37", "80x17"])
def test_gru_cluster_sizes_are_bit_equal(built_library, lengths):
    """R = 1 (block-local, weights streamed at H = 512), the chosen R = 32 (weights resident in LDS) and R = 8 (a cluster that streams)"""
    gx, whh, bhh, *_ = _gru_case(512, lengths, 7 + 512)
    outs = {r: GruRunner(512, r)(gx, whh, bhh, lengths)[0] for r in (1, 0, 8)}
    assert np.array_equal(outs[1].view(np.uint32), outs[0].view(np.uint32))
    assert np.array_equal(outs[1].view(np.uint32), outs[8].view(np.uint32))


@pytest.mark.parametrize("H,cluster", [(64, 0), (64, 2), (512, 0)])
def test_gru_utterance_alone_equals_its_batched_rows(built_library, H, cluster):
    lengths = GRU_LENGTHS[0]
    gx, whh, bhh, *_ = _gru_case(H, lengths, 7 + H)
    run = GruRunner(H, cluster)
    got, _ = run(gx, whh, bhh, lengths)
    offs = _offs(lengths)
    for i, n in enumerate(lengths):
        one, _ = run(gx[offs[i]:offs[i + 1]], whh, bhh, (n,))
        assert np.array_equal(one.view(np.uint32), got[offs[i]:offs[i + 1]].view(np.uint32)), (i, n)


def test_gru_consecutive_launches_over_one_workspace(built_library):
    """The stale-tag case: the second launch finds the first one's granules in the workspace -- same steps, same slots, other values.
    Both must come out right (here: bit-equal to the block-local form, which has no workspace), in either order of lengths."""
    H = 512
    a = _gru_case(H, GRU_LENGTHS[0], 7 + H)
    gxb, whhb, bhhb = _gru_inputs(H, (37, 5, 2, 1, 9), 99)
    local, cluster = GruRunner(H, 1), GruRunner(H, 0)
    want_a, want_b = local(a[0], a[1], a[2], GRU_LENGTHS[0])[0], local(gxb, whhb, bhhb, (37, 5, 2, 1, 9))[0]
    for _ in range(2):
        got_a = cluster(a[0], a[1], a[2], GRU_LENGTHS[0])[0]
        got_b = cluster(gxb, whhb, bhhb, (37, 5, 2, 1, 9))[0]
        assert np.array_equal(got_a.view(np.uint32), want_a.view(np.uint32))
        assert np.array_equal(got_b.view(np.uint32), want_b.view(np.uint32))
    cluster.epoch = 1                                                    # a caller that repeats an epoch: the launcher zeroes the workspace
    assert np.array_equal(cluster(a[0], a[1], a[2], GRU_LENGTHS[0])[0].view(np.uint32), want_a.view(np.uint32))
    assert R.rel_err(want_b, np.concatenate([R.bigru_from_gx(gxb[lo:hi], whhb, bhhb) for lo, hi in zip(_offs((37, 5, 2, 1, 9))[:-1], _offs((37, 5, 2, 1, 9))[1:])])) < 1e-5


# ------------------------------------------------------------------------------- ser_xattn_v
XATTN_PAIRS = ((1, 1), (1, 80), (37, 1), (17, 80), (80, 149))


def gpu_xattn(q, k, v, tq, tk, scale, mode=None):
    from interspeech_ser_amd import _lib
    E = q.shape[1]
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    qo, ko = (torch.tensor(_offs(t), dtype=torch.int32, device=DEV) for t in (tq, tk))
    out = torch.full((q.shape[0], E), float("nan"), dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = _lib.XattnArgs()
    x.q, x.ldq, x.k, x.ldk, x.v, x.ldv, x.q_offs, x.k_offs = qd.data_ptr(), E, kd.data_ptr(), E, vd.data_ptr(), E, qo.data_ptr(), ko.data_ptr()
    x.out_f32, x.ldo_f32, x.scale, x.range_flag = out.data_ptr(), E, scale, flag.data_ptr()
    x.B, x.E, x.q_rows, x.k_rows, x.max_q = len(tq), E, q.shape[0], k.shape[0], max(tq)
    act = None
    if mode is not None:
        act = torch.zeros((2, q.shape[0], E), dtype=torch.float16, device=DEV)
        x.out_act, x.ldo_act, x.out_plane_stride, x.mode = act.data_ptr(), E, q.shape[0] * E, mode
    _lib.check(_lib.lib.ser_xattn_v(ctypes.byref(x), torch.cuda.current_stream().cuda_stream), "ser_xattn_v")
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if act is None else act.float().sum(dim=0).cpu().numpy()), int(flag.item())


@pytest.mark.parametrize("E", [128, 1024])
def test_xattn_ragged_pairs(built_library, E):
    from interspeech_ser_amd import _lib
    rng = np.random.default_rng(E)
    tq, tk = [p[0] for p in XATTN_PAIRS], [p[1] for p in XATTN_PAIRS]
    q, k, v = (rng.standard_normal((sum(t), E)).astype(np.float32) for t in (tq, tk, tk))
    scale = float(E) ** -0.5
    qo, ko = _offs(tq), _offs(tk)
    ref = np.concatenate([R.xattn(q[qo[i]:qo[i + 1]], k[ko[i]:ko[i + 1]], v[ko[i]:ko[i + 1]], scale) for i in range(len(tq))])
    ref32 = np.concatenate([(torch.softmax(scale * (torch.from_numpy(q[qo[i]:qo[i + 1]]) @ torch.from_numpy(k[ko[i]:ko[i + 1]]).T), dim=1)
                             @ torch.from_numpy(v[ko[i]:ko[i + 1]])).numpy() for i in range(len(tq))])
    e_ref = R.rel_err(ref32, ref)
    got, act, bits = gpu_xattn(q, k, v, tq, tk, scale, mode=_lib.MODE_FP16X)
    err = R.rel_err(got, ref)
    _report(f"xattn E={E} pairs={XATTN_PAIRS}", err, e_ref, 0.0)
    assert np.isfinite(got).all() and err <= 2.0 * e_ref
    assert bits == 0 and np.abs(act.astype(np.float64) - got).max() <= 2.0 ** -21 * max(1.0, np.abs(got).max())
    assert np.array_equal(got[qo[2]:qo[3]], np.broadcast_to(v[ko[2]], (37, E)))                  # one key: the context is its value row
    for i in range(len(tq)):                                                                     # a pair alone: bit-equal to its batched rows
        one, _, _ = gpu_xattn(q[qo[i]:qo[i + 1]], k[ko[i]:ko[i + 1]], v[ko[i]:ko[i + 1]], [tq[i]], [tk[i]], scale)
        assert np.array_equal(one.view(np.uint32), got[qo[i]:qo[i + 1]].view(np.uint32)), XATTN_PAIRS[i]
    vbig = v.copy()
    vbig[ko[2]] = 70000.0                                               # pair (37, 1): its context IS this row, beyond fp16 -- the operand copy reports it
    assert gpu_xattn(q, k, vbig, tq, tk, scale, mode=_lib.MODE_FP16X)[2] & 1
    assert gpu_xattn(q, k, vbig, tq, tk, scale, mode=_lib.MODE_FP32X)[2] == 0


# ------------------------------------------------------------------------------- ser_attn_pool_v
def gpu_attn_pool(a, b, w, bias, lengths, col0=0, width=None, lda=None, ldb=None):
    from interspeech_ser_amd import _lib
    E, offs = a.shape[1], _offs(lengths)
    width = width or E
    ad, bd, wd = _dev_rows(a, lda), _dev_rows(b, ldb), _dev(w)
    od = torch.tensor(offs, dtype=torch.int32, device=DEV)
    scores = torch.empty(offs[-1], dtype=torch.float32, device=DEV)
    out = torch.full((len(lengths), width), float("nan"), dtype=torch.float32, device=DEV)
    p = _lib.AttnPoolArgs()
    p.a, p.lda, p.b, p.ldb, p.w, p.frame_offs, p.scores = ad.data_ptr(), lda or E, bd.data_ptr(), ldb or E, wd.data_ptr(), od.data_ptr(), scores.data_ptr()
    p.out, p.ldo, p.bias, p.col0, p.B, p.E, p.rows, p.max_frames = out.data_ptr(), width, bias, col0, len(lengths), E, offs[-1], max(lengths)
    _lib.check(_lib.lib.ser_attn_pool_v(ctypes.byref(p), torch.cuda.current_stream().cuda_stream), "ser_attn_pool_v")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("E", [128, 1024])
def test_attn_pool(built_library, E):
    lengths = (1, 16, 17, 149)
    rng = np.random.default_rng(3 * E)
    a, b = (rng.standard_normal((sum(lengths), E)).astype(np.float32) for _ in range(2))
    w, bias = (rng.standard_normal(E) / np.sqrt(E)).astype(np.float32), 0.3
    offs = _offs(lengths)
    ref = np.stack([R.attn_pool(a[lo:hi].astype(np.float64) + b[lo:hi], w, bias) for lo, hi in zip(offs[:-1], offs[1:])])
    ref32 = []
    for lo, hi in zip(offs[:-1], offs[1:]):
        x = torch.from_numpy(a[lo:hi]) + torch.from_numpy(b[lo:hi])
        ref32.append(((x * torch.softmax(x @ torch.from_numpy(w) + bias, dim=0)[:, None]).sum(dim=0)).numpy())
    e_ref = R.rel_err(np.stack(ref32), ref)
    got = gpu_attn_pool(a, b, w, bias, lengths, col0=E, width=2 * E)
    err = R.rel_err(got[:, E:], ref)
    _report(f"attn_pool E={E} lengths={lengths}", err, e_ref, 0.0)
    assert np.isnan(got[:, :E]).all() and err <= 2.0 * e_ref
    assert np.array_equal(got[0, E:], a[0] + b[0])                       # one frame gives a + b exactly
    for i, n in enumerate(lengths):
        one = gpu_attn_pool(a[offs[i]:offs[i + 1]], b[offs[i]:offs[i + 1]], w, bias, (n,))
        assert np.array_equal(one[0].view(np.uint32), got[i, E:].view(np.uint32))


def test_attn_pool_padded_rows_are_bit_equal(built_library):
    """row pitches beyond E (lda = E + 4, ldb = E + 8) and an output window inside a wider row (col0 = 4, ldo = E + 8): the same bits as
    contiguous rows, nothing written outside the window.  E = 68: a last slab with one live quad; 17 frames: two in row group 0"""
    E, lengths = 68, (1, 17)
    rng = np.random.default_rng(3 * E)
    a, b = (rng.standard_normal((sum(lengths), E)).astype(np.float32) for _ in range(2))
    w, bias = (rng.standard_normal(E) / np.sqrt(E)).astype(np.float32), 0.3
    flat = gpu_attn_pool(a, b, w, bias, lengths)
    padded = gpu_attn_pool(a, b, w, bias, lengths, col0=4, width=E + 8, lda=E + 4, ldb=E + 8)
    assert np.isfinite(flat).all() and np.array_equal(flat[0], a[0] + b[0])
    assert np.array_equal(padded[:, 4:4 + E].view(np.uint32), flat.view(np.uint32))
    assert np.isnan(padded[:, :4]).all() and np.isnan(padded[:, 4 + E:]).all()


# ------------------------------------------------------------------------------- ser_fusion_cls_v
def gpu_cls(p, gamma, beta, w1, b1, w2, b2, ldp=None):
    from interspeech_ser_amd import _lib
    B, K = p.shape
    H1, n_out = w1.shape[0], w2.shape[0]
    t = [_dev_rows(p, ldp)] + [_dev(v) for v in (gamma, beta, w1, b1, w2, b2)]
    xn, hidden = torch.empty((B, K), dtype=torch.float32, device=DEV), torch.empty((B, H1), dtype=torch.float32, device=DEV)
    out = torch.full((B, n_out), float("nan"), dtype=torch.float32, device=DEV)
    c = _lib.FusionClsArgs()
    c.p, c.ldp, c.gamma, c.beta, c.W1, c.b1, c.W2, c.b2 = t[0].data_ptr(), ldp or K, *(v.data_ptr() for v in t[1:])
    c.xn, c.hidden, c.out, c.eps, c.B, c.K, c.H1, c.n_out = xn.data_ptr(), hidden.data_ptr(), out.data_ptr(), 1e-5, B, K, H1, n_out
    _lib.check(_lib.lib.ser_fusion_cls_v(ctypes.byref(c), torch.cuda.current_stream().cuda_stream), "ser_fusion_cls_v")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("K,H1,n_out", [(2048, 512, 8), (256, 64, 3)])
def test_fusion_classifier(built_library, K, H1, n_out):
    rng = np.random.default_rng(K + n_out)
    p = (1.5 * rng.standard_normal((5, K)) + 0.4).astype(np.float32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32), (0.05 * rng.standard_normal(K)).astype(np.float32)
    w1, b1 = (rng.standard_normal((H1, K)) / np.sqrt(K)).astype(np.float32), (0.05 * rng.standard_normal(H1)).astype(np.float32)
    w2, b2 = (rng.standard_normal((n_out, H1)) / np.sqrt(H1)).astype(np.float32), (0.05 * rng.standard_normal(n_out)).astype(np.float32)
    ref = R.classifier(p, gamma, beta, w1, b1, w2, b2)
    tt = [torch.from_numpy(v) for v in (p, gamma, beta, w1, b1, w2, b2)]
    ref32 = F.linear(F.relu(F.linear(F.layer_norm(tt[0], (K,), tt[1], tt[2], 1e-5), tt[3], tt[4])), tt[5], tt[6]).numpy()
    e_ref = R.rel_err(ref32, ref)
    got = gpu_cls(p, gamma, beta, w1, b1, w2, b2)
    err = R.rel_err(got, ref)
    _report(f"fusion_cls K={K} H1={H1} n_out={n_out}", err, e_ref, 0.0)
    assert got.shape == (5, n_out) and err <= 2.0 * e_ref
    for i in range(5):
        assert np.array_equal(gpu_cls(p[i:i + 1], gamma, beta, w1, b1, w2, b2)[0].view(np.uint32), got[i].view(np.uint32))


def test_fusion_classifier_padded_rows_are_bit_equal(built_library):
    """input pitch beyond K (ldp = K + 8): the same bits as contiguous rows.  K = 384: two chunks a lane, the second partly dead"""
    K, H1, n_out = 384, 64, 3
    rng = np.random.default_rng(K + n_out)
    p = (1.5 * rng.standard_normal((3, K)) + 0.4).astype(np.float32)
    gamma, beta = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32), (0.05 * rng.standard_normal(K)).astype(np.float32)
    w1, b1 = (rng.standard_normal((H1, K)) / np.sqrt(K)).astype(np.float32), (0.05 * rng.standard_normal(H1)).astype(np.float32)
    w2, b2 = (rng.standard_normal((n_out, H1)) / np.sqrt(H1)).astype(np.float32), (0.05 * rng.standard_normal(n_out)).astype(np.float32)
    flat = gpu_cls(p, gamma, beta, w1, b1, w2, b2)
    assert np.isfinite(flat).all()
    assert np.array_equal(gpu_cls(p, gamma, beta, w1, b1, w2, b2, ldp=K + 8).view(np.uint32), flat.view(np.uint32))


# ------------------------------------------------------------------------------- engine.FusionHead
def _head_forward(head, xs1, xs2, slot=0):
    x1, x2 = _dev(np.concatenate(xs1)), _dev(np.concatenate(xs2))
    out = head.forward(x1, _offs([len(x) for x in xs1]), x2, _offs([len(x) for x in xs2]), slot=slot).cpu().numpy().copy()
    assert head.status(slot) == (0, 0)
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
def test_fusion_head_against_the_float64_statement(built_library, mode):
    from interspeech_ser_amd.engine import FusionHead
    worst = 0.0
    cases = [R.case_errors(320, 128, (1, 37, 149), seed, mode) for seed in (31, 5)]
    gate = 2.0 * max(c[4] + c[5] for c in cases)
    for seed, (sd, xs1, xs2, ref, e_ref, e_split) in zip((31, 5), cases):
        head = FusionHead(sd, 320, 128, DEV, mode)
        got = _head_forward(head, xs1, xs2)
        err = R.rel_err(got, ref)
        worst = max(worst, err)
        _report(f"FusionHead {mode} seed {seed} D1=320 D2=128 lengths=(1, 37, 149)", err, e_ref, e_split)
        for i in range(3):                                               # one at a time: bit-equal logits
            one = _head_forward(head, xs1[i:i + 1], xs2[i:i + 1])
            assert np.array_equal(one[0].view(np.uint32), got[i].view(np.uint32)), i
        # a slot that meets the smallest utterance first and grows for the batch
        assert np.array_equal(_head_forward(head, xs1[:1], xs2[:1], slot=1)[0].view(np.uint32), got[0].view(np.uint32))
        assert np.array_equal(_head_forward(head, xs1, xs2, slot=1).view(np.uint32), got.view(np.uint32))
    assert worst <= gate, (worst, gate)


def test_fusion_head_real_geometry(built_library):
    """HuBERT-xlarge + RoBERTa-large widths, a 10 s utterance (499 frames), 80 text rows"""
    from interspeech_ser_amd.engine import FusionHead
    sd, xs1, xs2, ref, e_ref, e_split = R.case_errors(1280, 1024, (499,), 31, "f16x")
    head = FusionHead(sd, 1280, 1024, DEV, "f16x")
    assert head.R == 32
    got = _head_forward(head, xs1, xs2)
    err = R.rel_err(got, ref)
    _report("FusionHead f16x D1=1280 D2=1024 T=499", err, e_ref, e_split)
    assert err <= 2.0 * (e_ref + e_split)


def test_fusion_head_refuses_what_it_cannot_run(built_library):
    from interspeech_ser_amd.engine import FusionHead
    sd, xs1, xs2 = R.seeded_case(128, 64, (3,), 1, t2=4, h=64)
    with pytest.raises(ValueError, match="multiples of 64"):
        FusionHead(sd, 100, 64, DEV)
    with pytest.raises(ValueError, match="lacks"):
        FusionHead({k: v for k, v in sd.items() if "text_gru" not in k}, 128, 64, DEV)
    with pytest.raises(ValueError, match="speech_projection.weight has shape"):
        FusionHead(sd, 192, 64, DEV)
    bad = dict(sd)
    bad["speech_gru.weight_hh_l0"] = sd["speech_gru.weight_hh_l0"].clone()
    bad["speech_gru.weight_hh_l0"][5, 7] = 1.0e5
    with pytest.raises(ValueError, match="speech_gru.weight_hh_l0"):
        FusionHead(bad, 128, 64, DEV, "bf16")                            # the recurrent weights are fp16 planes in every mode
    odd = R.seeded_case(128, 64, (3,), 1, t2=4, h=96)[0]
    with pytest.raises(ValueError, match="hidden width 96"):
        FusionHead(odd, 128, 64, DEV)
    head = FusionHead(sd, 128, 64, DEV)
    with pytest.raises(ValueError, match="empty speech utterance"):
        head.forward(_dev(xs1[0]), [0, 3, 3], _dev(np.concatenate([xs2[0], xs2[0]])), [0, 4, 8])
    assert _head_forward(head, xs1, xs2).shape == (1, 8)                 # h = 64: the block-local recurrence behind the same class


# ------------------------------------------------------------------------------- bimodal.BimodalPredictor
def test_bimodal_predictor_on_the_tiny_fixtures(built_library, golden_dir):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.bimodal import BimodalPredictor
    from interspeech_ser_amd.engine import FusionHead, SpeechEncoder, TextEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    from test_gpu_e2e import synth_wave
    gs, gt = np.load(os.path.join(golden_dir, "tiny_hubert_d320h4.npz")), np.load(os.path.join(golden_dir, "tiny_roberta_d128h2.npz"))
    lengths = [int(n) for n in gs["lengths"]]
    waves = [synth_wave(int(gs[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
    B = len(waves)
    ids = torch.from_numpy(np.stack([gt[f"ids_{j}"] for j in range(B)]))
    mask = torch.from_numpy(np.stack([gt[f"mask_{j}"] for j in range(B)]))
    speech = SpeechEncoder(C.TINY_HUBERT, synthetic_state_dict(C.TINY_HUBERT, int(gs["seed"])), DEV, mode="f16x")
    text = TextEncoder(C.TINY_ROBERTA, synthetic_state_dict(C.TINY_ROBERTA, int(gt["seed"])), DEV, mode="f16x")
    layer = C.TINY_HUBERT.num_layers - 1
    xs1 = [gs[f"states_{j}"][layer] for j in range(B)]                   # the oracle's states: what the two drivers' files would hold
    xs2 = [gt[f"states_{j}"][-1] for j in range(B)]
    from oracle.fusion_head import seeded_head_weights
    sd = seeded_head_weights(R.head_shapes(320, 128), 31)
    ref = R.batch_logits(sd, xs1, xs2)
    e_ref = R.rel_err(R.oracle_logits(sd, xs1, xs2), ref)
    e_split = R.rel_err(R.batch_logits(sd, xs1, xs2, "f16x"), ref)
    pred = BimodalPredictor(speech, text, sd, layer)
    got = pred.predict(waves, ids, mask)
    x1, o1, x2, o2, hs1, hs2 = pred.features(waves, ids, mask)           # the same states, fed to a head of its own: bit-equal logits
    head = FusionHead(sd, 320, 128, DEV, "f16x")
    direct = head.forward(x1, o1, x2, o2).cpu().numpy()
    assert head.status() == (0, 0) and got.shape == (B, 8) and got.dtype == np.float32
    assert np.array_equal(direct.view(np.uint32), got.view(np.uint32))
    e_states = max(max(R.rel_err(hs1.utterance(j, layer).cpu().numpy(), xs1[j]) for j in range(B)),
                   max(R.rel_err(hs2.utterance(j, -1).cpu().numpy(), xs2[j]) for j in range(B)))
    err = R.rel_err(got, ref)
    _report(f"BimodalPredictor f16x (device states vs the oracle's: {e_states:.3e})", err, e_ref, e_split)
    assert err <= 2.0 * (e_ref + e_split)
    with pytest.raises(ValueError, match="last four hidden states"):     # the fixture's encoder has two layers: three states
        BimodalPredictor(speech, text, sd, 0, use_average=True)
    with pytest.raises(IndexError):
        BimodalPredictor(speech, text, sd, C.TINY_HUBERT.num_layers + 1)
    with pytest.raises(ValueError, match="text encoder"):
        BimodalPredictor(speech, speech, sd, 0)


def test_bimodal_predictor_use_average_feeds_the_mean_of_the_last_four_states(built_library):
    """``use_average=True`` on a four-layer encoder (five states): the head's speech rows are the mean of the last four states, and the
    logits are bit-equal to a head of its own fed those rows."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.bimodal import BimodalPredictor
    from interspeech_ser_amd.engine import FusionHead, SpeechEncoder, TextEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import synth_wave
    geo = C.tiny_geometry(C.FAMILY_HUBERT, hidden=320, heads=4, ffn=384, pos_groups=4, layers=4)
    speech = SpeechEncoder(geo, synthetic_state_dict(geo, 3), DEV, mode="f16x")
    text = TextEncoder(C.TINY_ROBERTA, synthetic_state_dict(C.TINY_ROBERTA, 4), DEV, mode="f16x")
    waves = [synth_wave(1, 8000), synth_wave(2, 4000)]
    rng = np.random.default_rng(6)
    ids = torch.from_numpy(rng.integers(3, 300, (2, 12)))
    mask = torch.ones(2, 12, dtype=torch.int64)
    ids[1, 7:], mask[1, 7:] = 1, 0                                       # right-padded, RoBERTa's pad id
    sd = seeded_head_weights(R.head_shapes(320, 128), 31)
    pred = BimodalPredictor(speech, text, sd, 0, use_average=True)
    got = pred.predict(waves, ids, mask)
    x1, o1, x2, o2, hs1, hs2 = pred.features(waves, ids, mask)
    assert hs1.states.shape[0] == 5
    last4 = hs1.states[-4:, :o1[-1]].double().cpu().numpy()
    # three fp32 additions of partial sums up to 2, 3 and 4 max|state|, then an exact division by 4: at most 9/4 x 2^-24 max|state|
    assert np.abs(x1[:o1[-1]].cpu().numpy() - last4.mean(axis=0)).max() <= 3.0 * 2.0 ** -24 * np.abs(last4).max()
    direct = FusionHead(sd, 320, 128, DEV, "f16x").forward(x1, o1, x2, o2).cpu().numpy()
    assert got.shape == (2, 8) and np.isfinite(got).all()
    assert np.array_equal(direct.view(np.uint32), got.view(np.uint32))
    last = BimodalPredictor(speech, text, sd, 4).predict(waves, ids, mask)
    assert not np.array_equal(last, got)


# ------------------------------------------------------------------------------- head.evaluate(engine="hip") on files
EVAL_LENGTHS = (1, 37, 149, 12, 5, 21, 7, 2, 18, 16, 17, 3, 9, 4, 6, 8, 11, 10)                # 18 files: a batch of 16 and one of 2
EVAL_SEED, EVAL_T2 = 5, 16


@pytest.fixture(scope="module")
def eval_corpus(tmp_path_factory, built_library):
    import pandas as pd
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.frontend import feature_path, save_feature
    root = tmp_path_factory.mktemp("fusion_eval")
    lazy1, lazy2 = root / "hubert", root / "roberta"
    lazy1.mkdir()
    lazy2.mkdir()
    sd, xs1, xs2, ref, e_ref, e_split = R.case_errors(320, 128, EVAL_LENGTHS, EVAL_SEED, "f16x", t2=EVAL_T2)
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(len(EVAL_LENGTHS))]
    for name, a, b in zip(names, xs1, xs2):
        save_feature(torch.from_numpy(a), feature_path(str(lazy1), "/corpus/Audios/" + name))
        save_feature(torch.from_numpy(b), feature_path(str(lazy2), name))
    rng = np.random.default_rng(2)
    lab = pd.DataFrame(np.eye(8, dtype=np.float32)[rng.integers(0, 8, len(names))], columns=HD.CLASSES)
    lab.insert(0, "FileName", names)
    lab["Split_Set"] = "Development"
    lab.to_csv(root / "labels.csv", index=False)
    pd.DataFrame({"FileName": names, "transcription": ["x"] * len(names)}).to_csv(root / "text.csv", index=False)
    cfg = {"wav_dir": "/corpus/Audios", "txt_dir": str(root / "text.csv"), "lazy_dir1": str(lazy1), "lazy_dir2": str(lazy2),
           "label_path": str(root / "labels.csv"), "feat1_dim": 320, "feat2_dim": 128, "model_path": str(root / "exp"), "batch_size": 4}
    os.makedirs(cfg["model_path"])
    torch.save(sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
    with open(root / "cfg.json", "w") as f:
        json.dump(cfg, f)
    return dict(cfg=cfg, root=root, names=names, sd=sd, xs1=xs1, xs2=xs2, ref=ref, gate=2.0 * (e_ref + e_split))


def test_evaluate_hip_on_feature_files(eval_corpus, capsys):
    from interspeech_ser_amd import head as HD
    c = eval_corpus
    assert HD.main(["--config_path", str(c["root"] / "cfg.json"), "--engine", "hip"], evaluate_only=True) == 0
    log = capsys.readouterr().out
    assert f"{len(c['names'])} rows written, 0 files failed" in log, log
    with open(os.path.join(c["cfg"]["model_path"], "results", "dev.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Filename", "Prediction"] + [f"class_{i}_prob" for i in range(8)]
    assert [r[0] for r in rows[1:]] == c["names"]
    for row, lg in zip(rows[1:], c["ref"]):
        top = np.sort(lg)[::-1]
        gap = (top[0] - top[1]) / np.abs(lg).max()
        print(f"FUSION evaluate {row[0]}: float64 top-two gap {gap:.3e} of max|logit| (must exceed 1e-2)")
        assert gap > 1e-2, "choose another seed: the float64 top two logits are too close on this file"
        assert row[1] == HD.CLASS_LETTERS[int(np.argmax(lg))]
        # the printed logits: within the gate of the float64 ones, plus the half unit of the %.4f they are printed with
        assert np.abs(np.array([float(v) for v in row[2:]]) - lg).max() <= 5e-5 + c["gate"] * max(1.0, np.abs(c["ref"]).max())
    res = HD.evaluate(c["cfg"], seed=7, engine="hip", mode="fp32x")
    assert res["n"] == len(c["names"]) and res["failed"] == 0 and np.isfinite(res["eval_loss"]) and 0.0 <= res["eval_f1"] <= 1.0


def test_evaluate_hip_fails_a_file_through_the_range_guard(eval_corpus, tmp_path, capsys):
    """One speech file carries 1e5: in f16x its operand copy is beyond fp16, the batch is retried file by file and only that file is
    failed; fp32x (bf16 planes) writes every row."""
    import shutil
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.frontend import feature_path, save_feature
    c = eval_corpus
    cfg = dict(c["cfg"])
    lazy1 = tmp_path / "hubert"
    shutil.copytree(cfg["lazy_dir1"], lazy1)
    bad = c["xs1"][4].copy()
    bad[3, 10] = 1.0e5
    save_feature(torch.from_numpy(bad), feature_path(str(lazy1), c["names"][4]))
    cfg["lazy_dir1"], cfg["model_path"] = str(lazy1), str(tmp_path / "exp")
    os.makedirs(cfg["model_path"])
    shutil.copy(os.path.join(c["cfg"]["model_path"], "multimodal_ser.pt"), cfg["model_path"])
    res = HD.evaluate(cfg, seed=7, engine="hip", mode="f16x")
    log = capsys.readouterr().out
    assert res["failed"] == 1 and res["n"] == len(c["names"]) - 1 and log.count("Failed to process") == 1, log
    assert f"Failed to process {c['names'][4]}" in log and "fp16 operand range" in log
    with open(res["csv"], newline="") as f:
        assert [r[0] for r in csv.reader(f)][1:] == [n for n in c["names"] if n != c["names"][4]]
    res = HD.evaluate(cfg, seed=7, engine="hip", mode="fp32x")
    assert res["failed"] == 0 and res["n"] == len(c["names"])
