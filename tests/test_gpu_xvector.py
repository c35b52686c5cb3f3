"""GPU: the x-vector head -- ser_stat_pool_v, ser_layer_mix_v and ser_xvec_tail_v against their float64 statements
(tests/xvector_ref.py), batch invariance bit for bit, the launchers' refusals, engine.XVectorHead on handed-in states,
SpeakerEmbedder.embed against HF's float64 embeddings and logits of the fixtures (tests/golden/tiny_xvec_*.npz) and the command line.

Bounds.  u = 2^-53; a column of n rows x_t with A = max|x_t|, mu its mean, M2 = sum (x_t - mu)^2, S1 = sum |x_t - mu|, c chunks.

ser_stat_pool_v, the mean.  Every intermediate (a chunk's sum / its count, the running mean of the merge) is at most A in magnitude and
fewer than n + 4 c + 8 float64 roundings stand behind the result, each at most u * 2 A; then one fp32 rounding:
    |mean - ref| <= 2^-24 |ref| + (n + 4 c + 8) * 2 u * A.
The std.  A chunk mean carries e_m <= (n + 2) u A, so a centred term d = x - m_c is off by at most u |d| + e_m and the chunk's sum of
squares by (n + 3) u sum d^2 + 2 e_m sum |d| (the exact shift identity sum (x - m')^2 = sum (x - m)^2 + n (m - m')^2 only adds a term of
second order in u).  The merge adds delta^2 n_a n_c / (n_a + n_c) with delta off by at most 4 (n + 16) u A; sum_c |delta_c| w_c <=
(c + 1) S1 because |delta_c| is at most the mean absolute deviation of the chunk plus that of the rows before it.  Together, generously,
    |M2' - M2| <= tolM2 = 4 (n + 16) u M2 + 8 (n + 16) (c + 2) u A S1,
    |std - ref| <= 2^-24 ref + [ sqrt((M2 + tolM2) / (n - 1)) - sqrt(M2 / (n - 1)) ] + 4 u ref
(the bracket is the exact propagation through the root and stays finite for a constant column, M2 = 0).  For a column N(10^3, (10^-2)^2)
of 101 rows tolM2 / M2 ~ 5e-8, below the fp32 rounding; the one-pass formula sum x^2 - (sum x)^2 / n loses ~1e-5 of M2 there in float64
and misses the bound, which the test shows with that formula written out.

ser_layer_mix_v.  The fp32 copy is the float64 statement (products and sums rounded one by one, ascending state) rounded once: exact.  The
operand planes hold that fp32 value y to the format's split precision: fp16 hi + lo 2^-22 |y| + 2^-24 (lo is an fp16 subnormal below
2^-14: an absolute floor), bf16 hi + lo 2^-16 |y|, one bf16 plane 2^-8 |y|.

ser_xvec_tail_v: ser_cls_tail_v's bound (tests/test_gpu_audio_cls.py), 2^-23 |ref| + 2^-40 * (sum of the absolute terms), for the
embedding from the float64 statement and for the logits from the statement applied to the STORED fp32 embedding.

End to end.  The gate is 2 x the fixture's stored gain for the mode (tools/make_golden_xvector.py: the worst of 8 seeded sign-pattern
perturbations of the hidden states of the size of the family's hidden-state gate, pushed through the float64 statement; the factor 2
because eight random patterns are not the worst case), by the metric max|a - b| / max(1, max|b|).  The gains are the generator's, as first
computed: no gate was adjusted after a run (the observed errors are in profiles/xvector_parity.txt, printed here as XVEC_PARITY lines).
"""
import csv
import ctypes
import json
import wave

import numpy as np
import pytest
import torch

import xvector_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
U = 2.0 ** -53


def _fc():
    from interspeech_ser_amd import _lib
    return _lib.STAT_POOL_FC


def _counts():
    FC = _fc()
    return [2, 3, FC - 1, FC, FC + 1, 3 * FC + 5]


# ------------------------------------------------------------------------------- 1. ser_stat_pool_v against float64
def _run_stat(x_dev, offs, D, relu, ldo=None, max_frames=None, work_elems=None, expect=0, x_ptr=None):
    from interspeech_ser_amd import _lib
    B, FC = len(offs) - 1, _fc()
    ldo = 2 * D + 4 if ldo is None else ldo
    mf = int(np.diff(offs).max()) if max_frames is None else max_frames
    chunks = -(-max(mf, 1) // FC)
    work = torch.full((B * chunks * 2 * D,), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((B + 1, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    offs_dev = torch.tensor(offs, dtype=torch.int32, device=DEV)
    host = (ctypes.c_int32 * len(offs))(*[int(o) for o in offs])
    a = _lib.StatPoolArgs()
    a.x, a.ldx = (x_dev.data_ptr() if x_ptr is None else x_ptr), x_dev.stride(0)
    a.frame_offs, a.frame_offs_host = offs_dev.data_ptr(), ctypes.cast(host, ctypes.c_void_p)
    a.work, a.work_elems, a.out, a.ldo = work.data_ptr(), (work.numel() if work_elems is None else work_elems), out.data_ptr(), ldo
    a.B, a.D, a.rows, a.max_frames, a.relu = B, D, x_dev.shape[0], mf, relu
    rc = _lib.lib.ser_stat_pool_v(ctypes.byref(a) if expect != "null" else None, torch.cuda.current_stream().cuda_stream)
    assert rc == (-1 if expect == "null" else expect), (rc, _lib.lib.ser_last_error())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _stat_bounds(x64):
    """(mean ref, std ref, mean bound, std bound) of one utterance's rows [n, D] in float64"""
    n = x64.shape[0]
    c = -(-n // _fc())
    mu = x64.mean(axis=0)
    dev = x64 - mu
    M2, S1, A = (dev ** 2).sum(axis=0), np.abs(dev).sum(axis=0), np.abs(x64).max(axis=0)
    std = np.sqrt(M2 / (n - 1))
    tol = 4 * (n + 16) * U * M2 + 8 * (n + 16) * (c + 2) * U * A * S1
    b_mean = 2.0 ** -24 * np.abs(mu) + (n + 4 * c + 8) * 2 * U * A
    b_std = 2.0 ** -24 * std + (np.sqrt((M2 + tol) / (n - 1)) - std) + 4 * U * std
    return mu, std, b_mean, b_std


def _stat_case(kind, seed):
    """fp32 rows [total + 5, ldx = 104] with sentinel (NaN) columns beyond D = 100 and NaN rows beyond the batch, and the offsets"""
    g = np.random.default_rng(seed)
    counts, D, ldx = _counts(), 100, 104
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    x = np.full((int(offs[-1]) + 5, ldx), np.nan, dtype=np.float32)
    if kind == "offset":
        x[: offs[-1], :D] = (1e3 + 1e-2 * g.standard_normal((int(offs[-1]), D))).astype(np.float32)
    else:
        x[: offs[-1], :D] = (g.standard_normal((int(offs[-1]), D)) * g.uniform(0.1, 30.0, size=(1, D))).astype(np.float32)
    return x, offs, D


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kind", ["plain", "offset"])
def test_stat_pool_matches_float64(kind, relu):
    x, offs, D = _stat_case(kind, seed=11 + relu)
    got = _run_stat(torch.from_numpy(x).to(DEV), offs, D, relu)
    B = len(offs) - 1
    worst, naive_worst = 0.0, 0.0
    for b in range(B):
        x64 = x[offs[b]:offs[b + 1], :D].astype(np.float64)
        if relu:
            x64 = np.maximum(x64, 0.0)
        mu, std, b_mean, b_std = _stat_bounds(x64)
        e_mean, e_std = np.abs(got[b, :D].astype(np.float64) - mu), np.abs(got[b, D:2 * D].astype(np.float64) - std)
        worst = max(worst, float((e_mean / np.maximum(b_mean, 1e-300)).max()), float((e_std / np.maximum(b_std, 1e-300)).max()))
        assert (e_mean <= b_mean).all() and (e_std <= b_std).all(), (b, worst)
        n = x64.shape[0]
        naive = np.sqrt(np.maximum(((x64 ** 2).sum(axis=0) - x64.sum(axis=0) ** 2 / n) / (n - 1), 0.0))       # one pass, in float64
        naive_worst = max(naive_worst, float((np.abs(np.float32(naive).astype(np.float64) - std) / np.maximum(b_std, 1e-300)).max()))
    print(f"STAT_POOL {kind} relu={relu}: worst err / bound {worst:.3f}; the one-pass formula {naive_worst:.1f}")
    if kind == "offset":
        assert naive_worst > 1.0            # the case is honest: sum x^2 - (sum x)^2 / n misses the bound the kernel is held to
    assert (got[:B, 2 * D:] == SENTINEL).all() and (got[B] == SENTINEL).all()             # nothing outside [B, 2 D] is written


def test_stat_pool_is_batch_invariant():
    x, offs, D = _stat_case("plain", seed=5)
    counts = _counts()
    whole = _run_stat(torch.from_numpy(x).to(DEV), offs, D, 1)[: len(counts)]
    for b, c in enumerate(counts):                                                        # each utterance alone: its batch mates dropped
        one = np.ascontiguousarray(x[offs[b]:offs[b + 1]])
        alone = _run_stat(torch.from_numpy(one).to(DEV), np.array([0, c], dtype=np.int32), D, 1)[0]
        assert np.array_equal(alone.view(np.uint32), whole[b].view(np.uint32)), (b, c)
    order = [3, 0, 5, 1, 4, 2]                                                            # the batch permuted
    perm = np.concatenate([x[offs[b]:offs[b + 1]] for b in order], axis=0)
    poffs = np.concatenate([[0], np.cumsum([counts[b] for b in order])]).astype(np.int32)
    got = _run_stat(torch.from_numpy(np.ascontiguousarray(perm)).to(DEV), poffs, D, 1)[: len(counts)]
    for i, b in enumerate(order):
        assert np.array_equal(got[i].view(np.uint32), whole[b].view(np.uint32)), b


def test_stat_pool_refusals_launch_nothing():
    from interspeech_ser_amd import _lib
    x, offs, D = _stat_case("plain", seed=6)
    x_dev = torch.from_numpy(x).to(DEV)
    err = _lib.lib.ser_last_error
    out = _run_stat(x_dev, offs, D, 1, expect="null")
    assert b"ser_stat_pool: null pointer" in err() and (out == SENTINEL).all()
    out = _run_stat(x_dev, offs, 98, 1, expect=-2)                                         # D % 4
    assert b"D=98" in err() and (out == SENTINEL).all()
    out = _run_stat(x_dev, np.array([0, 5, 6, 20], dtype=np.int32), D, 1, expect=-2)       # T_b < 2, by index
    assert b"utterance 1 has 1 rows" in err() and (out == SENTINEL).all()
    out = _run_stat(x_dev, np.array([0, 9, 5, 20], dtype=np.int32), D, 1, max_frames=15, expect=-2)      # descending offsets
    assert b"utterance 1 owns rows 9..5" in err() and (out == SENTINEL).all()
    out = _run_stat(x_dev, offs, D, 1, work_elems=100, expect=-2)                          # a short workspace
    assert b"work holds 100" in err() and (out == SENTINEL).all()
    out = _run_stat(x_dev, np.array([0, 5, x.shape[0] + 1], dtype=np.int32), D, 1, max_frames=20, expect=-2)
    assert b"outside [0," in err() and (out == SENTINEL).all()


# ------------------------------------------------------------------------------- 2. ser_layer_mix_v
def _decode(planes: torch.Tensor) -> np.ndarray:
    return planes.double().sum(dim=0).cpu().numpy()


@pytest.mark.parametrize("n_states", [1, 3, 13])
@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_layer_mix_matches_float64(mode, n_states):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import _DTYPE, _PLANES, _operand_mode
    m = _operand_mode(mode)
    rows, D, lds, extra = 37, 192, 200, 3
    g = np.random.default_rng(100 * n_states + m)
    s = (g.standard_normal((n_states, rows + extra, lds)) * g.uniform(0.1, 30.0, size=(n_states, 1, 1))).astype(np.float32)
    w = R.softmax64(g.standard_normal(n_states).astype(np.float32)) if n_states > 1 else np.ones(1)
    s_dev, w_dev = torch.from_numpy(s).to(DEV), torch.from_numpy(w).to(DEV)
    planes = torch.full((_PLANES[m], rows + 1, D + 8), 7.0, dtype=_DTYPE[m], device=DEV)
    f32 = torch.full((rows + 1, D + 4), SENTINEL, dtype=torch.float32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _lib.LayerMixArgs()
    a.s, a.state_stride, a.lds, a.w = s_dev.data_ptr(), s_dev.stride(0), lds, w_dev.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride = planes.data_ptr(), D + 8, planes.stride(0)
    a.out_f32, a.ldo_f32, a.range_flag = f32.data_ptr(), D + 4, flag.data_ptr()
    a.n_states, a.mode, a.rows, a.D = n_states, m, rows, D
    assert _lib.lib.ser_layer_mix_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0, _lib.lib.ser_last_error()
    torch.cuda.synchronize()
    ref = R.layer_mix(s[:, :rows, :D], w).astype(np.float32)                              # the float64 sum, rounded once
    got = f32.cpu().numpy()
    assert np.array_equal(got[:rows, :D].view(np.uint32), ref.view(np.uint32))
    assert (got[rows] == SENTINEL).all() and (got[:, D:] == SENTINEL).all()
    y = ref.astype(np.float64)
    tol = {"f16x": 2.0 ** -22 * np.abs(y) + 2.0 ** -24, "fp32x": 2.0 ** -16 * np.abs(y), "bf16": 2.0 ** -8 * np.abs(y)}[mode]
    dec = _decode(planes)
    err = np.abs(dec[:rows, :D] - y)
    print(f"LAYER_MIX {mode} n_states={n_states}: operand err / split precision {float((err / tol).max()):.3f}")
    assert (err <= tol).all() and (dec[rows] == 7.0 * _PLANES[m]).all() and (dec[:, D:] == 7.0 * _PLANES[m]).all()
    assert int(flag.item()) == 0


@pytest.mark.parametrize("mode,bits", [("f16x", 3), ("fp32x", 0)])
def test_layer_mix_reports_to_the_range_guard(mode, bits):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import _DTYPE, _PLANES, _operand_mode
    m = _operand_mode(mode)
    s = torch.ones((1, 5, 64), dtype=torch.float32, device=DEV)
    s[0, 3, 17] = 70000.0                                                                 # beyond 65 504
    w = torch.ones(1, dtype=torch.float64, device=DEV)
    planes = torch.zeros((_PLANES[m], 5, 64), dtype=_DTYPE[m], device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _lib.LayerMixArgs()
    a.s, a.state_stride, a.lds, a.w = s.data_ptr(), 0, 64, w.data_ptr()
    a.out_act, a.ldo_act, a.out_plane_stride, a.range_flag = planes.data_ptr(), 64, planes.stride(0), flag.data_ptr()
    a.n_states, a.mode, a.rows, a.D = 1, m, 5, 64
    assert _lib.lib.ser_layer_mix_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0, _lib.lib.ser_last_error()
    torch.cuda.synchronize()
    assert int(flag.item()) == bits


# ------------------------------------------------------------------------------- 3. ser_xvec_tail_v against float64
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("dim,labels", [(24, 24), (512, 130), (40, 1)])
def test_xvec_tail_matches_float64(dim, labels, B):
    from interspeech_ser_amd import _lib
    D, lds, lde, ldo = 200, 208, dim + 3, labels + 5
    g = np.random.default_rng(dim + labels + B)
    f = lambda *shape: g.standard_normal(shape).astype(np.float32)                        # noqa: E731
    stats, F, bf, Cw, bc = f(B, lds), f(dim, D), f(dim), f(labels, dim), f(labels)
    dev = [torch.from_numpy(x).to(DEV) for x in (stats, F, bf, Cw, bc)]
    emb = torch.full((B + 1, lde), SENTINEL, dtype=torch.float32, device=DEV)
    out = torch.full((B + 1, ldo), SENTINEL, dtype=torch.float32, device=DEV)
    a = _lib.XvecTailArgs()
    a.stats, a.lds, a.F, a.bf, a.C, a.bc = dev[0].data_ptr(), lds, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), dev[4].data_ptr()
    a.emb, a.lde, a.logits, a.ldo, a.B, a.D, a.dim, a.n_labels = emb.data_ptr(), lde, out.data_ptr(), ldo, B, D, dim, labels
    assert _lib.lib.ser_xvec_tail_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0, _lib.lib.ser_last_error()
    torch.cuda.synchronize()
    got_e, got_l = emb.cpu().numpy(), out.cpu().numpy()
    x = stats[:, :D].astype(np.float64)
    ref_e = x @ F.astype(np.float64).T + bf
    mag_e = np.abs(x) @ np.abs(F).astype(np.float64).T + np.abs(bf)
    err_e = np.abs(got_e[:B, :dim].astype(np.float64) - ref_e)
    bound_e = 2.0 ** -23 * np.abs(ref_e) + 2.0 ** -40 * mag_e
    e32 = got_e[:B, :dim].astype(np.float64)                                              # the stored fp32 embedding: what HF's classifier reads
    ref_l = e32 @ Cw.astype(np.float64).T + bc
    mag_l = np.abs(e32) @ np.abs(Cw).astype(np.float64).T + np.abs(bc)
    err_l = np.abs(got_l[:B, :labels].astype(np.float64) - ref_l)
    bound_l = 2.0 ** -23 * np.abs(ref_l) + 2.0 ** -40 * mag_l
    print(f"XVEC_TAIL dim={dim} labels={labels} B={B}: worst err / bound {float((err_e / bound_e).max()):.3f} (emb) "
          f"{float((err_l / bound_l).max()):.3f} (logits)")
    assert (err_e <= bound_e).all() and (err_l <= bound_l).all()
    assert (got_e[:B, dim:] == SENTINEL).all() and (got_e[B] == SENTINEL).all()
    assert (got_l[:B, labels:] == SENTINEL).all() and (got_l[B] == SENTINEL).all()


# ------------------------------------------------------------------------------- fixtures
_REFS, _EMB = {}, {}


def _fixture(name):
    if name not in _REFS:
        fx = R.Fixture(name)
        _REFS[name] = (fx, fx.waves(), fx.hf_state_dict())
    return _REFS[name]


def _embedder(name, mode):
    from interspeech_ser_amd.weights import normalize_names
    from interspeech_ser_amd.xvector import SpeakerEmbedder
    if (name, mode) not in _EMB:
        fx, waves, sd = _fixture(name)
        _EMB[(name, mode)] = SpeakerEmbedder(fx.geometry(), fx.spec(), normalize_names(sd), DEV, mode, batch_size=16,
                                             normalize=bool(fx.preprocessor.get("do_normalize", True)))
    return _EMB[(name, mode)]


# ------------------------------------------------------------------------------- 4. the TDNN stack in isolation
def _handed_in(fx, order, extra=9, fill=0.0):
    """the fixture's float64 hidden states of the waveforms ``order`` as one packed fp32 tensor with ``extra`` rows behind them"""
    from interspeech_ser_amd.engine import HiddenStates
    parts = [fx.states64[j].astype(np.float32) for j in order]
    offs = np.concatenate([[0], np.cumsum([p.shape[1] for p in parts])])
    s = np.full((parts[0].shape[0], int(offs[-1]) + extra, parts[0].shape[2]), fill, dtype=np.float32)
    s[:, : offs[-1]] = np.concatenate(parts, axis=1)
    return HiddenStates(torch.from_numpy(s).to(DEV), offs), parts


def _nan_fill(bf):
    for op in bf["ops"]:
        op.t.fill_(float("nan"))
    for k in ("y", "stats", "rows"):
        bf[k].fill_(float("nan"))
    bf["work"].fill_(float("nan"))


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_head_on_handed_in_states(name, mode):
    fx = _fixture(name)[0]
    head = _embedder(name, mode).head
    order = list(fx.good)
    hs, parts = _handed_in(fx, order)
    slot = 5
    got = head.forward_rows(hs, slot=slot).cpu().numpy().copy()
    dim = head.dim
    for i, p in enumerate(parts):                                                         # per utterance, against the float64 statement
        e, l = R.head_outputs(p.astype(np.float64), fx.head, fx.weighted, fx.kernel, fx.dilation)
        me, ml = R.metric(got[i, :dim], e), R.metric(got[i, dim:], l)
        print(f"XVEC_HEAD {name} {mode} wave {order[i]}: emb {me:.3e} (gate {2 * fx.gain_emb[mode]:.3e}) logits {ml:.3e} (gate {2 * fx.gain_logits[mode]:.3e})")
        assert me <= 2 * fx.gain_emb[mode] and ml <= 2 * fx.gain_logits[mode]
    # every row outside the batch's own rows NaN: the states' tail rows, and every buffer of the slot (gap rows, tail rows, the padded
    # columns' sources) before the run
    hs_nan, _ = _handed_in(fx, order, fill=float("nan"))
    _nan_fill(head._bufs[slot])
    again = head.forward_rows(hs_nan, slot=slot).cpu().numpy().copy()
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    # a neighbour's rows NaN too: it leaves the comparison (the fp16 planes saturate a NaN to a finite value, which is what the range
    # guard is for, so its own row says nothing), the others do not move
    victim = 2
    o = hs_nan.frame_offs
    hs_nan.states[:, o[victim]: o[victim + 1]] = float("nan")
    _nan_fill(head._bufs[slot])
    third = head.forward_rows(hs_nan, slot=slot).cpu().numpy().copy()
    keep = [i for i in range(len(order)) if i != victim]
    assert np.array_equal(third[keep].view(np.uint32), got[keep].view(np.uint32))
    # permuted and alone: bit-identical rows
    perm = [order[i] for i in (3, 0, 4, 2, 1)]
    hs_p, _ = _handed_in(fx, perm)
    got_p = head.forward_rows(hs_p, slot=slot).cpu().numpy().copy()
    for i, j in enumerate(perm):
        assert np.array_equal(got_p[i].view(np.uint32), got[order.index(j)].view(np.uint32)), j
    hs_1, _ = _handed_in(fx, [fx.two])
    assert np.array_equal(head.forward_rows(hs_1, slot=slot).cpu().numpy()[0].view(np.uint32), got[order.index(fx.two)].view(np.uint32))


def test_head_refusals():
    from interspeech_ser_amd.engine import XVectorHead
    fx = _fixture("tiny_xvec_wavlm")[0]
    emb = _embedder("tiny_xvec_wavlm", "f16x")
    hs, _ = _handed_in(fx, [0, fx.two])
    hs.frame_offs[-1] -= 1                                                                # the second utterance one frame short: T' = 1
    with pytest.raises(ValueError, match="utterance 1: 15 encoder frames leave 1 TDNN output rows"):
        emb.head.forward_rows(hs, slot=6)
    head = {k: torch.from_numpy(np.array(v)) for k, v in fx.head.items() if not k.startswith("objective")}
    for key, shape in (("projector.weight", (48, 128)), ("tdnn.1.kernel.weight", (64, 64)), ("feature_extractor.weight", (24, 100))):
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            XVectorHead(emb.enc, dict(head, **{key: torch.zeros(shape)}), fx.spec())


# ------------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_embed_matches_hf_float64(name, mode):
    """The six waveforms as one ragged batch: the T' = 1 waveform is a NaN row and an entry of ``.failed``, the other five are inside
    the gate of HF's float64 embeddings and logits and bit-identical to a run without that waveform."""
    fx, waves, _ = _fixture(name)
    emb = _embedder(name, mode)
    assert emb.mode == mode
    all_e = emb.embed(waves, with_logits=True)
    all_l = emb.logits
    assert all_e.shape == (6, fx.spec().xvector_output_dim) and all_e.dtype == np.float32 and all_l.shape[0] == 6
    assert [i for i, _ in emb.failed] == [fx.one] and "TDNN output rows" in str(emb.failed[0][1])
    assert np.isnan(all_e[fx.one]).all() and np.isnan(all_l[fx.one]).all()
    five_e = emb.embed([waves[j] for j in fx.good], with_logits=True)
    assert not emb.failed
    assert np.array_equal(five_e.view(np.uint32), all_e[fx.good].view(np.uint32))
    assert np.array_equal(emb.logits.view(np.uint32), all_l[fx.good].view(np.uint32))
    assert emb.embed(waves[:1]) is not None and emb.logits is None                        # the logits only when asked for
    for j in fx.good:
        me, ml = R.metric(all_e[j], fx.emb64[j]), R.metric(all_l[j], fx.logits64[j])
        print(f"XVEC_PARITY {name} {mode} wave {j} ({fx.lengths[j]} samples): emb {me:.3e} / gate {2 * fx.gain_emb[mode]:.3e}, "
              f"logits {ml:.3e} / gate {2 * fx.gain_logits[mode]:.3e}")
        assert me <= 2 * fx.gain_emb[mode] and ml <= 2 * fx.gain_logits[mode], (j, me, ml)


# ------------------------------------------------------------------------------- 6. the command line
def _write_pcm16(path, x, sr=16000):
    pcm = np.clip(np.round(np.asarray(x, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def test_command_line(tmp_path, capsys):
    from safetensors.torch import save_file
    from interspeech_ser_amd.xvector import run_embed
    name = "tiny_xvec_wavlm_base"
    fx, waves, sd = _fixture(name)
    snap = tmp_path / "snapshot"
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(fx.config))
    (snap / "preprocessor_config.json").write_text(json.dumps(fx.preprocessor))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(snap / "model.safetensors"))
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    files = {f"u{j}.wav": _write_pcm16(wav_dir / f"u{j}.wav", waves[j]) for j in (0, 2, fx.two, fx.one)}
    good = [f"u{j}.wav" for j in (0, 2, fx.two)]
    want = _embedder(name, "f16x").embed([files[n] for n in good])
    trials = tmp_path / "trials.txt"
    trials.write_text(f"u0.wav u2.wav\nu2.wav u{fx.two}.wav\n")
    save, scores = tmp_path / "emb", tmp_path / "scores.csv"
    argv = ["--model", str(snap), "--wav_dir", str(wav_dir), "--save_path", str(save), "--mode", "f16mf", "--trials", str(trials),
            "--scores_csv", str(scores)]
    assert run_embed(argv) == 0
    out = capsys.readouterr().out
    assert "--mode f16mf is not implemented for the x-vector head" in out and "using f16x" in out and "numerics mode f16x" in out
    assert sorted(p.name for p in save.iterdir()) == sorted(n[:-4] + ".pt" for n in good)
    for i, n in enumerate(good):
        t = torch.load(str(save / (n[:-4] + ".pt")))
        assert t.shape == (40,) and t.dtype == torch.float32
        assert np.array_equal(t.numpy().view(np.uint32), want[i].view(np.uint32))
    assert f"Failed to process {wav_dir / f'u{fx.one}.wav'}: utterance 0" in out and "3 embeddings written" in out and "1 files failed" in out
    with open(scores, newline="") as f:
        rows = list(csv.reader(f))
    assert [r[:2] for r in rows] == [["u0.wav", "u2.wav"], ["u2.wav", f"u{fx.two}.wav"]]
    for r, (i, k) in zip(rows, ((0, 1), (1, 2))):
        a, b = want[i].astype(np.float64), want[k].astype(np.float64)
        assert abs(float(r[2]) - float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))) <= 1e-14
