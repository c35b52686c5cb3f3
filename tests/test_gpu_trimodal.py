"""GPU: ser_xattn_mh_v, engine.TrimodalHead and head.score(engine="hip") against the float64 statements in tests/fusion_ref.py and
tests/fusion3_ref.py.

Gate of every comparison (the rule of tests/test_gpu_fusion.py): device error against float64 <= 2 x max over the
test's cases of (e_ref + e_split); e_ref = the error of the reference's own fp32 torch arithmetic, e_split = the error operand rounding
causes in the float64 statement, both computed here on the CPU.  Each test prints its numbers (lines starting TRIMODAL)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fusion3_ref as R3
import fusion_ref as R
import trimodal_corpus as TC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _offs(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _report(what, err, e_ref, e_split, gate):
    print(f"TRIMODAL {what}: error {err:.3e}  e_ref {e_ref:.3e}  e_split {e_split:.3e}  gate {gate:.3e}")


# ------------------------------------------------------------------------------- ser_xattn_mh_v
def gpu_xattn(q, k, v, tq, tk, scale, heads, mode=None, entry="mh"):
    """-> (ctx fp32 [Mq, E], the operand planes as raw 16-bit words [planes, Mq, E] or None, range bits).  ``entry="single"``: ser_xattn_v."""
    from interspeech_ser_amd import _lib
    E, Mq = q.shape[1], q.shape[0]
    qd, kd, vd = _dev(q), _dev(k), _dev(v)
    qo, ko = (torch.tensor(_offs(t), dtype=torch.int32, device=DEV) for t in (tq, tk))
    out = torch.full((Mq, E), float("nan"), dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = _lib.XattnMhArgs() if entry == "mh" else _lib.XattnArgs()
    x.q, x.ldq, x.k, x.ldk, x.v, x.ldv, x.q_offs, x.k_offs = qd.data_ptr(), E, kd.data_ptr(), E, vd.data_ptr(), E, qo.data_ptr(), ko.data_ptr()
    x.out_f32, x.ldo_f32, x.scale, x.range_flag = out.data_ptr(), E, scale, flag.data_ptr()
    x.B, x.E, x.q_rows, x.k_rows, x.max_q = len(tq), E, Mq, k.shape[0], max(tq)
    act = None
    if mode is not None:
        planes = 1 if mode == _lib.MODE_BF16 else 2
        act = torch.zeros((planes, Mq, E), dtype=torch.int16, device=DEV)
        x.out_act, x.ldo_act, x.out_plane_stride, x.mode = act.data_ptr(), E, Mq * E, mode
    if entry == "mh":
        x.heads = heads
        _lib.check(_lib.lib.ser_xattn_mh_v(ctypes.byref(x), torch.cuda.current_stream().cuda_stream), "ser_xattn_mh_v")
    else:
        assert heads == 1
        _lib.check(_lib.lib.ser_xattn_v(ctypes.byref(x), torch.cuda.current_stream().cuda_stream), "ser_xattn_v")
    torch.cuda.synchronize()
    return out.cpu().numpy(), (None if act is None else act.cpu().numpy()), int(flag.item())


def _mh_inputs(E, heads, tq, tk, seed):
    """K and V of head h carry a scale and an offset of their own: taking another head's keys or values moves the context by O(1)"""
    rng = np.random.default_rng(seed)
    dh = E // heads
    q = rng.standard_normal((sum(tq), E)).astype(np.float32)
    k = rng.standard_normal((sum(tk), E)).astype(np.float32)
    v = rng.standard_normal((sum(tk), E)).astype(np.float32)
    for h in range(heads):
        k[:, h * dh:(h + 1) * dh] *= 1.0 + 0.5 * h
        v[:, h * dh:(h + 1) * dh] += 3.0 * h
    return q, k, v


def _mh_refs(q, k, v, tq, tk, heads, swap=False):
    """(float64 context, fp32 torch context) of every pair alone, head by head; ``swap``: keys and values of the NEXT head (a wrong answer)"""
    E = q.shape[1]
    dh = E // heads
    scale = float(dh) ** -0.5
    qo, ko = _offs(tq), _offs(tk)
    ref, ref32 = np.zeros(q.shape), np.zeros(q.shape, dtype=np.float32)
    for i in range(len(tq)):
        for h in range(heads):
            c, ck = slice(h * dh, (h + 1) * dh), slice(((h + swap) % heads) * dh, ((h + swap) % heads + 1) * dh)
            qq, kk, vv = q[qo[i]:qo[i + 1], c], k[ko[i]:ko[i + 1], ck], v[ko[i]:ko[i + 1], ck]
            ref[qo[i]:qo[i + 1], c] = R.xattn(qq, kk, vv, scale)
            ref32[qo[i]:qo[i + 1], c] = (torch.softmax(scale * (torch.from_numpy(qq) @ torch.from_numpy(kk).T), dim=1) @ torch.from_numpy(vv)).numpy()
    return ref, ref32, scale


XMH_TQ, XMH_TK = (1, 17, 33), (1, 16, 17)             # a one-row tail tile (17, 33), a tile boundary (16 keys), a single key
XMH_SMALL = ((128, 1), (128, 2), (256, 4))
_XMH = {}


def _xmh_case(E, heads, tq, tk):
    key = (E, heads, tuple(tq), tuple(tk))
    if key not in _XMH:
        q, k, v = _mh_inputs(E, heads, tq, tk, 100 * E + heads)
        ref, ref32, scale = _mh_refs(q, k, v, tq, tk, heads)
        _XMH[key] = (q, k, v, ref, R.rel_err(ref32, ref), scale)
    return _XMH[key]


def _check_mh(E, heads, tq, tk, gate):
    q, k, v, ref, e_ref, scale = _xmh_case(E, heads, tq, tk)
    got, _, bits = gpu_xattn(q, k, v, tq, tk, scale, heads)
    err = R.rel_err(got, ref)
    _report(f"xattn_mh E={E} heads={heads} tq={tq} tk={tk}", err, e_ref, 0.0, gate)
    assert np.isfinite(got).all() and bits == 0 and err <= gate
    if heads > 1:                                                       # the inputs tell the heads apart: the swapped answer is O(1) away
        assert R.rel_err(_mh_refs(q, k, v, tq, tk, heads, swap=True)[0], ref) > 0.2
    qo, ko = _offs(tq), _offs(tk)
    for i in range(len(tq)):                                            # a pair alone: bit-equal to its batched rows
        one, _, _ = gpu_xattn(q[qo[i]:qo[i + 1]], k[ko[i]:ko[i + 1]], v[ko[i]:ko[i + 1]], [tq[i]], [tk[i]], scale, heads)
        assert np.array_equal(one.view(np.uint32), got[qo[i]:qo[i + 1]].view(np.uint32)), (i, tq[i], tk[i])
    return got, q, k, v, scale


@pytest.mark.parametrize("E,heads", XMH_SMALL)
def test_xattn_mh_against_the_float64_statement(built_library, E, heads):
    gate = 2.0 * max(_xmh_case(e, h, XMH_TQ, XMH_TK)[4] for e, h in XMH_SMALL)
    got, q, k, v, scale = _check_mh(E, heads, XMH_TQ, XMH_TK, gate)
    ko = _offs(XMH_TK)
    assert np.array_equal(got[0], v[ko[0]])                            # one key: the context is its value row, in every head


def test_xattn_mh_at_the_trimodal_shape(built_library):
    """E = 1024, two heads of 512 columns: prosody_attention at H = 512"""
    tq, tk = (24, 7), (5, 24)
    _check_mh(1024, 2, tq, tk, 2.0 * _xmh_case(1024, 2, tq, tk)[4])


@pytest.mark.parametrize("E", [128, 1024])
def test_xattn_mh_with_one_head_is_bit_equal_to_xattn(built_library, E):
    from interspeech_ser_amd import _lib
    tq, tk = ((1, 17, 33), (1, 16, 17)) if E == 128 else ((24, 7), (5, 24))
    q, k, v = _mh_inputs(E, 1, tq, tk, 7 + E)
    scale = float(E) ** -0.5
    for mode in (_lib.MODE_FP16X, _lib.MODE_FP32X, _lib.MODE_BF16):
        a, act_a, bits_a = gpu_xattn(q, k, v, tq, tk, scale, 1, mode=mode, entry="mh")
        b, act_b, bits_b = gpu_xattn(q, k, v, tq, tk, scale, 1, mode=mode, entry="single")
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode          # out_f32
        assert act_a.any() and np.array_equal(act_a, act_b) and bits_a == bits_b == 0, mode                  # out_act, plane by plane


def test_xattn_mh_range_guard(built_library):
    """the pair with one key has that key's value row as its context: a value beyond fp16 in head 1 is reported by the FP16X operand copy"""
    from interspeech_ser_amd import _lib
    E, heads = 128, 2
    q, k, v, ref, e_ref, scale = _xmh_case(E, heads, XMH_TQ, XMH_TK)
    vbig = v.copy()
    vbig[0, E // heads + 5] = 70000.0
    got, act, bits = gpu_xattn(q, k, vbig, XMH_TQ, XMH_TK, scale, heads, mode=_lib.MODE_FP16X)
    assert bits & 1 and got[0, E // heads + 5] == 70000.0
    assert gpu_xattn(q, k, vbig, XMH_TQ, XMH_TK, scale, heads, mode=_lib.MODE_FP32X)[2] == 0
    assert gpu_xattn(q, k, v, XMH_TQ, XMH_TK, scale, heads, mode=_lib.MODE_FP16X)[2] == 0


# ------------------------------------------------------------------------------- engine.TrimodalHead
def _forward(head, xs1, xs2, xs3, third_axis=False, slot=0):
    x1, x2, x3 = (_dev(np.concatenate(x)) for x in (xs1, xs2, xs3))
    if third_axis:
        x3 = x3[..., None]
    out = head.forward(x1, _offs([len(x) for x in xs1]), x2, _offs([len(x) for x in xs2]), x3, _offs([len(x) for x in xs3]), slot=slot).cpu().numpy().copy()
    assert head.status(slot) == (0, 0)
    return out


SMALL_DIMS = (64, 128, 64)
SMALL_LENGTHS = ((1, 17, 40), (5, 1, 16), (33, 2, 64))


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_trimodal_head_against_the_float64_statement(built_library, mode):
    from interspeech_ser_amd.engine import TrimodalHead
    cases = [R3.case_errors(SMALL_DIMS, SMALL_LENGTHS, seed, mode, h=64) for seed in (31, 5)]
    gate = 2.0 * max(c[5] + c[6] for c in cases)
    worst = 0.0
    for seed, (sd, xs1, xs2, xs3, ref, e_ref, e_split) in zip((31, 5), cases):
        head = TrimodalHead(sd, *SMALL_DIMS, DEV, mode, heads=(1, 1, 2))
        assert head.R == 1
        got = _forward(head, xs1, xs2, xs3)
        err = R.rel_err(got, ref)
        worst = max(worst, err)
        _report(f"TrimodalHead {mode} seed {seed} dims={SMALL_DIMS} H=64", err, e_ref, e_split, gate)
        for i in range(3):                                               # one at a time: bit-equal logits
            one = _forward(head, xs1[i:i + 1], xs2[i:i + 1], xs3[i:i + 1], third_axis=(i == 1))
            assert np.array_equal(one[0].view(np.uint32), got[i].view(np.uint32)), i
        # a slot that meets one utterance first and grows, on every side, for the batch
        assert np.array_equal(_forward(head, xs1[1:2], xs2[1:2], xs3[1:2], slot=1)[0].view(np.uint32), got[1].view(np.uint32))
        assert np.array_equal(_forward(head, xs1, xs2, xs3, slot=1).view(np.uint32), got.view(np.uint32))
        one_head = _forward(TrimodalHead(sd, *SMALL_DIMS, DEV, mode, heads=(1, 1, 1)), xs1, xs2, xs3)
        assert not np.array_equal(one_head, got)                         # the head count reaches the kernel
    assert worst <= gate, (worst, gate)


def test_trimodal_head_at_hidden_512(built_library):
    """the cluster recurrence (R = 32), two heads of 512 columns, classifier K = 3072"""
    from interspeech_ser_amd.engine import TrimodalHead
    dims, lengths = (128, 64, 512), ((24, 3), (7, 12), (16, 24))
    sd, xs1, xs2, xs3, ref, e_ref, e_split = R3.case_errors(dims, lengths, 31, "f16x", h=512)
    head = TrimodalHead(sd, *dims, DEV, "f16x")
    assert head.R == 32 and head.heads == (1, 1, 2) and head.E == 1024
    got = _forward(head, xs1, xs2, xs3)
    err = R.rel_err(got, ref)
    gate = 2.0 * (e_ref + e_split)
    _report(f"TrimodalHead f16x dims={dims} H=512 lengths={lengths}", err, e_ref, e_split, gate)
    assert err <= gate
    for i in range(2):
        one = _forward(head, xs1[i:i + 1], xs2[i:i + 1], xs3[i:i + 1])
        assert np.array_equal(one[0].view(np.uint32), got[i].view(np.uint32)), i


def test_trimodal_head_refuses_what_it_cannot_run_and_ignores_extra_keys(built_library):
    from interspeech_ser_amd.engine import FusionHead, TrimodalHead
    sd, xs1, xs2, xs3 = R3.seeded_case(SMALL_DIMS, ((3,), (4,), (2,)), 1, h=64)
    with pytest.raises(ValueError, match="multiples of 64"):
        TrimodalHead(sd, 64, 128, 100, DEV)
    with pytest.raises(ValueError, match="lacks"):
        TrimodalHead({k: v for k, v in sd.items() if "prosody_gru" not in k}, *SMALL_DIMS, DEV)
    with pytest.raises(ValueError, match="heads="):
        TrimodalHead(sd, *SMALL_DIMS, DEV, heads=(1, 1, 4))              # dh = 32
    with pytest.raises(ValueError, match="heads="):
        TrimodalHead(sd, *SMALL_DIMS, DEV, heads=(1, 2))
    head = TrimodalHead(sd, *SMALL_DIMS, DEV)
    with pytest.raises(ValueError, match="empty prosody utterance"):
        head.forward(_dev(xs1[0]), [0, 3], _dev(xs2[0]), [0, 4], _dev(xs3[0]), [0, 0])
    with pytest.raises(ValueError, match="same number"):
        head.forward(_dev(xs1[0]), [0, 3], _dev(xs2[0]), [0, 4], _dev(xs3[0]), [0, 1, 2])
    got = _forward(head, xs1, xs2, xs3)
    extra = dict(sd)
    extra["classifier_neutral.0.weight"] = torch.randn(64, 384)
    extra["classifier_neutral.3.bias"] = torch.randn(1)
    assert np.array_equal(_forward(TrimodalHead(extra, *SMALL_DIMS, DEV), xs1, xs2, xs3), got)
    sd2, a, b = R.seeded_case(64, 128, (3,), 1, t2=4, h=64)              # FusionHead: the same rule, pinned
    extra2 = dict(sd2)
    extra2["neutral_classifier.0.weight"] = torch.randn(64, 256)
    o = [0, 3], [0, 4]
    want = FusionHead(sd2, 64, 128, DEV).forward(_dev(a[0]), o[0], _dev(b[0]), o[1]).cpu().numpy()
    assert np.array_equal(FusionHead(extra2, 64, 128, DEV).forward(_dev(a[0]), o[0], _dev(b[0]), o[1]).cpu().numpy(), want)


def test_trimodal_head_range_guard_through_the_third_stream(built_library):
    from interspeech_ser_amd.engine import TrimodalHead
    sd, xs1, xs2, xs3, *_ = R3.case_errors(SMALL_DIMS, SMALL_LENGTHS, 5, "f16x", h=64)
    bad = [x.copy() for x in xs3]
    bad[1][1, 9] = 7.0e4
    x1, x2, x3 = (_dev(np.concatenate(x)) for x in (xs1, xs2, bad))
    o = [_offs([len(x) for x in xs]) for xs in (xs1, xs2, xs3)]
    head = TrimodalHead(sd, *SMALL_DIMS, DEV, "f16x")
    head.forward(x1, o[0], x2, o[1], x3, o[2])
    bits, err = head.status()
    assert bits & 1 and err == 0 and "fp16 operand range" in TrimodalHead.failure(bits, err)
    head.forward(x1, o[0], x2, o[1], _dev(np.concatenate(xs3)), o[2])    # the word was cleared: a clean batch reads clean
    assert head.status() == (0, 0)
    wide = TrimodalHead(sd, *SMALL_DIMS, DEV, "fp32x")                   # bf16 planes hold 7e4
    wide.forward(x1, o[0], x2, o[1], x3, o[2])
    assert wide.status() == (0, 0)


# ------------------------------------------------------------------------------- head.score(engine="hip") on files
@pytest.mark.parametrize("modalities", [2, 3])
def test_score_hip_against_torch_on_feature_files(built_library, tmp_path, capsys, modalities):
    from interspeech_ser_amd import head as HD
    ref = TC.float64_logits(modalities)
    e_ref = R.rel_err(TC.torch_logits(modalities), ref)
    e_split = R.rel_err(TC.float64_logits(modalities, "f16x"), ref)
    gate, scale = 2.0 * (e_ref + e_split), max(1.0, float(np.abs(ref).max()))
    for lg in ref:
        top = np.sort(lg)[::-1]
        assert (top[0] - top[1]) / np.abs(lg).max() > 1e-2, "choose another seed: the float64 top two logits are too close on a file"
    outs = {}
    for ranking in (False, True):
        c = TC.make(tmp_path / ("r" if ranking else "p"), modalities, ranking=ranking)
        res_t = HD.score(c["cfg"], seed=7, device="cpu", engine="torch", modalities=modalities, test_csv=c["test_csv"])
        torch_rows = TC.read_csv(res_t["csv"])
        assert HD.main(["--config_path", c["cfg_path"], "--engine", "hip", "--test_csv", c["test_csv"]], score_only=True, modalities=modalities) == 0
        assert "5 rows written, 0 files failed" in capsys.readouterr().out
        hip_rows = TC.read_csv(res_t["csv"])
        assert hip_rows[0] == torch_rows[0] == ["FileName", "Prediction"] + [f"class_{i}_prob" for i in range(8)]
        assert hip_rows[1] == torch_rows[1] == c["names"]
        assert hip_rows[2] == torch_rows[2] == [HD.CLASS_LETTERS[int(np.argmax(lg))] for lg in ref]
        err = float(np.abs(hip_rows[3] - ref).max()) / scale
        _report(f"score hip modalities={modalities} ranking={ranking} (printed rows vs float64)", err, e_ref, e_split, gate)
        assert np.abs(hip_rows[3] - ref).max() <= 5e-5 + gate * scale                          # half a unit of the %.4f the rows are printed with
        assert np.abs(hip_rows[3] - torch_rows[3]).max() <= 1e-4 + (gate + e_ref) * scale      # triangle: the torch rows are e_ref from float64
        outs[ranking] = open(res_t["csv"], "rb").read()
    assert outs[True] == outs[False]                                                            # the ranking checkpoint's extra keys change nothing


def test_score_hip_drops_exactly_the_file_the_range_guard_fails(built_library, tmp_path, capsys):
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.frontend import feature_path, save_feature
    c = TC.make(tmp_path, 3)
    bad = c["xs"][2][3].copy()
    bad[2, 11] = 7.0e4
    save_feature(torch.from_numpy(bad), feature_path(c["cfg"]["lazy_dir3"], c["names"][3]))
    res = HD.score(c["cfg"], seed=7, engine="hip", mode="f16x", modalities=3, test_csv=c["test_csv"])
    log = capsys.readouterr().out
    assert res["failed"] == 1 and res["n"] == 4 and log.count("Failed to process") == 1, log
    assert f"Failed to process {c['names'][3]}" in log and "fp16 operand range" in log
    assert TC.read_csv(res["csv"])[1] == [n for n in c["names"] if n != c["names"][3]]
    res = HD.score(c["cfg"], seed=7, engine="hip", mode="fp32x", modalities=3, test_csv=c["test_csv"])
    assert res["failed"] == 0 and res["n"] == 5
