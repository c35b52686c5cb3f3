"""GPU: the Whisper decoder's kernels (csrc/decode.hip) against float64, and engine.WhisperDecoder / transcribe.WhisperTranscriber against
HF's recorded logits and tokens (tests/golden/tiny_whisper_dec_d128h2.npz; float64 statement: tests/whisper_dec_ref.py).

Token equality is asserted only where it follows from the logit gate: the fixture's decided positions all have a masked top-1 - top-2 of
at least 4 g, g = 1e-3 max(1, max|logits|) (asserted on the CPU, tests/test_whisper_decoder_host.py); a device whose logits stay within g
moves each of two logits by at most g and keeps the argmax, position after position."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import whisper_dec_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, FP32X, FP16X = 1, 2, 4
MODE_NAME = {BF16: "bf16", FP32X: "fp32x", FP16X: "f16x"}
LENS = (1, 2, 15, 16, 17, 63, 64, 65, 447, 1500)
MAX_LEN = 1500
GUARD = 4                                     # canary rows before and after every cache
CANARY = 12345.0
GARBAGE = 0x7B7B                              # bf16 1.3e36 / fp16 61280: no kernel output looks like it


def stream():
    return torch.cuda.current_stream().cuda_stream


def unit_roundoff(mode):
    """(u, eta) of the operand format, as tests/test_gpu_frontends.py derives them: v is held as v (1 + d) + e, |d| <= u, |e| <= eta"""
    dt = torch.float16 if mode == FP16X else torch.bfloat16
    half_eps = torch.finfo(dt).eps / 2.0
    return (half_eps if mode == BF16 else half_eps * half_eps), torch.finfo(dt).smallest_normal * torch.finfo(dt).eps / 2.0


def planes_value(words, mode):
    """int16 planes [P, ...] -> float64 value"""
    return words.view(torch.float16 if mode == FP16X else torch.bfloat16).double().sum(0).numpy()


# ---------------------------------------------------------------------------------------------------------------- ser_dec_attn_v
@functools.lru_cache(maxsize=None)
def attn_case(H, B):
    """Shared, never written: q [B, D], caches [B, MAX_LEN, D] and new rows [B, D] (fp32, host) and per length case the rows' lengths."""
    D = 64 * H
    rng = np.random.default_rng(100 * H + B)
    q = rng.standard_normal((B, D)).astype(np.float32)
    k = rng.standard_normal((B, MAX_LEN, D)).astype(np.float32)
    v = (rng.standard_normal((B, MAX_LEN, D)) * 1.5 + 0.25).astype(np.float32)
    kn = rng.standard_normal((B, D)).astype(np.float32)
    vn = rng.standard_normal((B, D)).astype(np.float32)
    lens = [[LENS[(i + 3 * b) % len(LENS)] for b in range(B)] for i in range(len(LENS))]       # a different len per row; row 0 walks LENS
    return q, k, v, kn, vn, lens


def attn_reference(q, K, V, scale, H):
    """(float64 context [D], numpy fp32 context [D], floor [D]) of one sequence over keys K / V [n, D].
    floor: what fp32 rounding may move the result by, from the kernel's arithmetic.  A score is a 64-term fp32 dot product scaled once:
    |ds| <= (64 + 2) 2^-24 sum_d |q_d k_d| scale log2(e) in base-2 units; a weight p = 2^(s - m) then carries a relative error of
    ln2 ds + 2^-23 (v_exp_f32) + 2^-24 (s - m) ~ ln2 ds + 2^-22; each of numerator and denominator is a sum of n terms accumulated in groups
    (at most n / 16 + 4 sequential adds per group, 16 merges): (n / 16 + 24) 2^-24 relative to sum p |v|.  So
    |d out| <= (2 (ln2 ds + 2^-22) + 2 (n / 16 + 24) 2^-24) max|v|."""
    n, D = K.shape
    q64, K64, V64 = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    out64, out32, floor = np.empty(D), np.empty(D, dtype=np.float32), np.empty(D)
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        s = (K64[:, sl] @ q64[sl]) * scale
        w = np.exp(s - s.max())
        out64[sl] = (w / w.sum()) @ V64[:, sl]
        s32 = (K[:, sl] @ q[sl]) * np.float32(scale)
        w32 = np.exp(s32 - s32.max())
        out32[sl] = (w32 / w32.sum()) @ V[:, sl]
        ds = 66 * 2.0 ** -24 * float((np.abs(K64[:, sl]) @ np.abs(q64[sl])).max()) * scale * math.log2(math.e)
        floor[sl] = (2 * (math.log(2) * ds + 2.0 ** -22) + 2 * (n / 16 + 24) * 2.0 ** -24) * float(np.abs(V64[:, sl]).max())
    return out64, out32, floor


def launch_attn(q, k, v, lens, H, mode, new=None, flag=None):
    """One launch over device copies with NaN at cache rows >= len, canary rows around the caches and a garbage-filled output.
    Returns (out words int16 [P, B + 2, D + 8] host, k cache host [B, GUARD + MAX_LEN + GUARD, D], v cache host, the same two before)."""
    from interspeech_ser_amd import _lib
    B, D = q.shape
    rows = GUARD + MAX_LEN + GUARD
    kc = torch.full((B, rows, D), CANARY, dtype=torch.float32, device=DEV)
    vc = torch.full((B, rows, D), CANARY, dtype=torch.float32, device=DEV)
    for b in range(B):
        n = lens[b] - (1 if new is not None else 0)          # with an append, row len - 1 is not in the cache yet
        kc[b, GUARD: GUARD + n] = torch.from_numpy(k[b, :n]).to(DEV)
        vc[b, GUARD: GUARD + n] = torch.from_numpy(v[b, :n]).to(DEV)
        kc[b, GUARD + n: GUARD + MAX_LEN] = float("nan")
        vc[b, GUARD + n: GUARD + MAX_LEN] = float("nan")
    before = (kc.cpu().numpy().copy(), vc.cpu().numpy().copy())
    P = 1 if mode == BF16 else 2
    out = torch.full((P, B + 2, D + 8), GARBAGE, dtype=torch.int16, device=DEV)
    qd = torch.from_numpy(q).to(DEV)
    ld = torch.tensor(lens, dtype=torch.int32, device=DEV)
    a = _lib.DecAttnArgs()
    a.q, a.ldq = qd.data_ptr(), D
    keep = []
    if new is not None:
        kn, vn = torch.from_numpy(new[0]).to(DEV), torch.from_numpy(new[1]).to(DEV)
        keep += [kn, vn]
        a.k_new, a.v_new, a.ld_new = kn.data_ptr(), vn.data_ptr(), D
    a.kcache, a.vcache, a.ldc, a.batch_stride = kc.data_ptr() + GUARD * D * 4, vc.data_ptr() + GUARD * D * 4, D, rows * D
    a.lens, a.lens_stride, a.len_add = ld.data_ptr(), 1, 0
    a.out_act, a.ldo_act, a.out_plane_stride = out.data_ptr() + (D + 8) * 2, D + 8, (B + 2) * (D + 8)
    a.range_flag = None if flag is None else flag.data_ptr()
    a.scale, a.B, a.H, a.dh, a.max_len, a.mode = 0.125, B, H, 64, MAX_LEN, mode
    _lib.check(_lib.lib.ser_dec_attn_v(C.byref(a), stream()), "ser_dec_attn_v")
    torch.cuda.synchronize()
    return out.cpu(), kc.cpu().numpy(), vc.cpu().numpy(), before


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [2, 20])
def test_dec_attn_equals_float64(H, B, mode, append):
    """Every length case: |planes - float64| <= 2 e_ref + floor + u_mode |ref| + eta_mode (e_ref: numpy fp32's distance from the float64
    statement, floor: attn_reference), with NaN in every cache row at and beyond len, canaries around the caches and the output, and, with
    an append, the new row at len - 1 and nowhere else.  A row alone equals the same row in the batch bit for bit."""
    q, k, v, kn, vn, cases = attn_case(H, B)
    D = 64 * H
    u, eta = unit_roundoff(mode)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for lens in cases:
        kk, vv = k.copy(), v.copy()
        if append:
            for b in range(B):
                kk[b, lens[b] - 1], vv[b, lens[b] - 1] = kn[b], vn[b]
        out, kc, vc, before = launch_attn(q, kk, vv, lens, H, mode, new=(kn, vn) if append else None, flag=flag)
        assert bool((out[:, 0] == GARBAGE).all()) and bool((out[:, B + 1] == GARBAGE).all()) and bool((out[:, :, D:] == GARBAGE).all()), "output canaries"
        val = planes_value(out[:, 1: B + 1, :D].contiguous(), mode)
        for b in range(B):
            n = lens[b]
            ref, ref32, floor = attn_reference(q[b], kk[b, :n], vv[b, :n], 0.125, H)
            e_ref = float(np.abs(ref32.astype(np.float64) - ref).max())
            err = np.abs(val[b] - ref)
            tol = 2 * e_ref + floor + u * np.abs(ref) + eta
            worst = max(worst, float((err / tol).max()))
            assert np.isfinite(val[b]).all() and (err <= tol).all(), (lens, b, float(err.max()), float((err / tol).max()))
            for cache, was, new_row in ((kc, before[0], kn), (vc, before[1], vn)):
                expect = was[b].copy()
                if append:
                    expect[GUARD + n - 1] = new_row[b]
                assert np.array_equal(cache[b].view(np.uint32), expect.view(np.uint32)), (lens, b, "the cache changed outside the appended row")
        if B > 1:
            b = B - 1
            alone = launch_attn(q[b: b + 1], kk[b: b + 1], vv[b: b + 1], lens[b: b + 1], H, mode, new=(kn[b: b + 1], vn[b: b + 1]) if append else None)[0]
            assert torch.equal(alone[:, 1, :D], out[:, 1 + b, :D]), (lens, "a row alone differs from the same row in a batch")
    assert int(flag.item()) == 0
    print(f"DECATTN H {H} B {B} {MODE_NAME[mode]} append {append}: worst err / gate {worst:.3f}")


def test_dec_attn_reports_fp16_overflow_and_refuses_bad_arguments():
    from interspeech_ser_amd import _lib
    q, k, v, kn, vn, cases = attn_case(2, 1)
    big = v.copy()
    big[0, 0, 5] = 3.0e5                                                      # one value beyond fp16's range reaches the context of len = 1
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    launch_attn(q, k, big, [1], 2, FP16X, flag=flag)
    assert int(flag.item()) & 1
    a = _lib.DecAttnArgs()
    a.q = a.kcache = a.vcache = a.out_act = 256
    a.ldq = a.ldc = a.ldo_act = 128
    a.B, a.H, a.dh, a.max_len, a.mode, a.len_add = 1, 2, 80, 8, FP16X, 1
    assert _lib.lib.ser_dec_attn_v(C.byref(a), None) < 0 and b"dh=80" in _lib.lib.ser_last_error()
    a.dh, a.mode = 64, 3
    assert _lib.lib.ser_dec_attn_v(C.byref(a), None) < 0 and b"mode 3" in _lib.lib.ser_last_error()


# ---------------------------------------------------------------------------------------------------------------- ser_dec_select_v
V, VPAD, MAXPOS = 522, 528, 16


def run_select(logits, *, pos=3, forced=None, phase=None, finished=None, mask=None, eos=7, pad=0):
    """One launch.  logits fp32 [B, VPAD] (host).  Returns dict of the state afterwards (host)."""
    from interspeech_ser_amd import _lib
    B = logits.shape[0]
    lg = torch.from_numpy(logits).to(DEV)
    mk = torch.zeros((3, V), dtype=torch.float32, device=DEV) if mask is None else torch.from_numpy(mask.astype(np.float32)).to(DEV)
    ph = torch.zeros(MAXPOS, dtype=torch.int32, device=DEV) if phase is None else torch.tensor(phase, dtype=torch.int32, device=DEV)
    fo = torch.full((MAXPOS,), -1, dtype=torch.int32, device=DEV) if forced is None else torch.tensor(forced, dtype=torch.int32, device=DEV)
    ids = torch.full((B + 2, MAXPOS), -9, dtype=torch.int32, device=DEV)
    fin = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    fin[B] = -9
    if finished is not None:
        fin[:B] = torch.tensor(finished, dtype=torch.int32)
    margin = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float32, device=DEV)
    word = torch.tensor([pos, -9, 0, 0, 0, -9], dtype=torch.int32, device=DEV)            # pos, unfinished, work[2], err, canary
    a = _lib.DecSelectArgs()
    a.logits, a.ldl, a.mask, a.ldm, a.phase, a.forced = lg.data_ptr(), logits.shape[1], mk.data_ptr(), V, ph.data_ptr(), fo.data_ptr()
    a.ids, a.ld_ids, a.finished = ids.data_ptr() + MAXPOS * 4, MAXPOS, fin.data_ptr()
    a.margin, a.ld_margin = margin.data_ptr() + MAXPOS * 4, MAXPOS
    a.pos, a.unfinished, a.work, a.err = word.data_ptr(), word.data_ptr() + 4, word.data_ptr() + 8, word.data_ptr() + 16
    a.B, a.V, a.eos, a.pad, a.max_pos = B, V, eos, pad, MAXPOS
    _lib.check(_lib.lib.ser_dec_select_v(C.byref(a), stream()), "ser_dec_select_v")
    torch.cuda.synchronize()
    ids_h, mg, w, f = ids.cpu().numpy(), margin.cpu().numpy(), word.cpu().numpy(), fin.cpu().numpy()
    assert (ids_h[0] == -9).all() and (ids_h[B + 1] == -9).all() and (mg[0] == -9).all() and (mg[B + 1] == -9).all() and f[B] == -9 and w[5] == -9
    written = np.zeros_like(ids_h[1: B + 1], dtype=bool)
    if 0 <= pos < MAXPOS - 1:
        written[:, pos + 1] = True
    assert (ids_h[1: B + 1][~written] == -9).all(), "ids changed outside column pos + 1"
    assert w[2] == 0 and w[3] == 0, "the ticket words must be left zero"
    return dict(token=ids_h[1: B + 1, min(pos + 1, MAXPOS - 1)], margin=mg[1: B + 1, min(max(pos, 0), MAXPOS - 1)], finished=f[:B], pos=int(w[0]),
                unfinished=int(w[1]), err=int(w[4]))


def base_logits(B, seed=0):
    z = np.random.default_rng(seed).standard_normal((B, VPAD)).astype(np.float32)
    z[:, V:] = 100.0                                                          # padded vocabulary columns hold the largest value
    return z


def test_select_argmax_ties_masks_padding_and_margin():
    z = base_logits(5)
    z[0, [17, 300, 521]] = 9.0                                                # a three-way tie: the lowest index wins, margin 0
    z[1, 40] = 50.0                                                           # a masked maximum loses
    z[3, 200] = 8.0
    z[3, 201] = 8.0 - 2.0 ** -20                                              # a margin of a few ulps survives fp32
    mask = np.zeros((3, V))
    mask[0, 40] = -np.inf
    mask[1] = -np.inf
    mask[1, 77] = 0.0                                                         # everything masked but one token
    r = run_select(z, mask=mask)
    zm = z[:, :V].astype(np.float64) + mask[0]
    assert r["token"].tolist() == [int(np.argmax(row)) for row in zm] and r["token"][0] == 17 and r["token"][1] != 40 and (r["token"] < V).all()
    want = np.array([R.top2_margin(row) for row in zm])
    assert np.all(np.abs(r["margin"] - want) <= 2.0 ** -23 * np.abs(z[:, :V]).max()), (r["margin"], want)     # one fp32 add and one subtraction
    assert r["margin"][0] == 0.0 and r["margin"][3] == np.float32(2.0 ** -20)
    assert r["err"] == 0 and r["pos"] == 4 and r["unfinished"] == 5 and not r["finished"].any()
    one = run_select(z, mask=mask, phase=[0, 0, 0, 1] + [0] * (MAXPOS - 4))
    assert (one["token"] == 77).all() and np.isinf(one["margin"]).all() and one["err"] == 0
    many = run_select(np.tile(z, (60, 1)), mask=mask)                         # 300 rows: 300 blocks take tickets
    assert many["unfinished"] == 300 and many["pos"] == 4 and many["token"].tolist() == r["token"].tolist() * 60


def test_select_forced_finished_eos_and_errors():
    z = base_logits(4, seed=1)
    z[2, 7] = 30.0                                                            # row 2 chooses eos (7)
    forced = [-1] * MAXPOS
    r = run_select(z, finished=[0, 1, 0, 0], pad=3)
    assert r["token"][1] == 3 and r["token"][2] == 7 and r["finished"].tolist() == [0, 1, 1, 0] and r["unfinished"] == 2 and r["err"] == 0
    assert np.isinf(r["margin"][1]) and np.isfinite(r["margin"][[0, 2, 3]]).all()
    forced[3] = 11
    nan = z.copy()
    nan[:, :V] = np.nan                                                       # a forced position does not read the logits
    f = run_select(nan, forced=forced, finished=[0, 1, 0, 0], pad=3)
    assert f["token"].tolist() == [11, 3, 11, 11] and f["err"] == 0 and f["pos"] == 4 and np.isinf(f["margin"]).all()
    forced[3] = 7                                                             # a forced eos finishes the row as well
    assert run_select(z, forced=forced)["finished"].all()
    bad = z.copy()
    bad[1, 400] = np.nan
    e = run_select(bad)
    assert e["err"] & 1 and e["token"][1] == 400                              # a NaN wins and fails the batch
    inf = z.copy()
    inf[0, :V] = -np.inf
    assert run_select(inf)["err"] & 1                                         # everything -inf: no finite winner
    fin = run_select(bad, finished=[0, 1, 0, 0])
    assert fin["err"] == 0                                                    # ... but a finished row's logits decide nothing
    end = run_select(z, pos=MAXPOS - 1)
    assert end["err"] & 4 and end["pos"] == MAXPOS - 1                        # the position left the buffer: nothing written, not advanced


# ---------------------------------------------------------------------------------------------------------------- ser_dec_embed_v
def test_dec_embed_is_the_fp32_sum():
    from interspeech_ser_amd import _lib
    rng = np.random.default_rng(3)
    Vv, T, D, B = 522, 64, 128, 5
    te, pe = rng.standard_normal((Vv, D)).astype(np.float32), rng.standard_normal((T, D)).astype(np.float32)
    ids = rng.integers(0, Vv, (B, T)).astype(np.int32)
    ids[0, 9], ids[1, 9] = 0, Vv - 1
    t_te, t_pe, t_ids = torch.from_numpy(te).to(DEV), torch.from_numpy(pe).to(DEV), torch.from_numpy(ids).to(DEV)
    for pos in (0, 9, T - 1):
        out = torch.full((B + 2, D + 4), CANARY, dtype=torch.float32, device=DEV)
        p = torch.tensor([pos], dtype=torch.int32, device=DEV)
        a = _lib.DecEmbedArgs()
        a.ids, a.ld_ids, a.pos, a.embed_tokens, a.embed_positions = t_ids.data_ptr(), T, p.data_ptr(), t_te.data_ptr(), t_pe.data_ptr()
        a.out, a.ldo, a.B, a.D, a.vocab, a.max_pos = out.data_ptr() + (D + 4) * 4, D + 4, B, D, Vv, T
        _lib.check(_lib.lib.ser_dec_embed_v(C.byref(a), stream()), "ser_dec_embed_v")
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert np.array_equal(o[1: B + 1, :D], te[ids[:, pos]] + pe[pos]), pos
        assert (o[0] == CANARY).all() and (o[B + 1] == CANARY).all() and (o[:, D:] == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir)


@functools.lru_cache(maxsize=None)
def decoder(mode):
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = R.load_fixture(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    return WhisperDecoder(geo, sd, DEV, mode, spec)


def enc_dev(enc, rows):
    return torch.from_numpy(np.ascontiguousarray(enc[rows])).to(DEV).reshape(-1, enc.shape[-1])


def teacher_forced_device(dec, enc_row, ids, spec):
    """logits [n, V] (host) of one utterance fed ``ids`` position by position through the recorded step"""
    pl = dec.begin(1, spec, forced_ids=[int(t) for t in ids])
    dec.project_cross(pl, enc_dev(enc_row[None], slice(None)))
    out = []
    for _ in range(len(ids)):
        dec._run_step(pl, with_logits=True)
        out.append(pl["logits"][0, : dec.geo.decoder_vocab_size].clone())
    torch.cuda.synchronize()
    assert int(pl["err"].item()) == 0 and (pl["range_flag"] is None or int(pl["range_flag"].item()) == 0)
    assert pl["ids"][0, : len(ids)].cpu().tolist() == [int(t) for t in ids]
    return torch.stack(out).cpu().numpy().astype(np.float64)


def logit_errors(mode, fx):
    gold, geo, sd, spec, enc = fx
    dec = decoder(mode)
    seqs, ref = gold["a_sequences"], gold["a_logits"].astype(np.float64)
    g = R.gate(ref, seqs, spec)
    worst = max(float(np.abs(teacher_forced_device(dec, enc[b], seqs[b], spec) - ref[b]).max()) for b in range(seqs.shape[0]))
    return worst, g


@pytest.mark.parametrize("mode", ["fp32x", "f16x"])
def test_teacher_forced_logits_within_the_gate(fx, mode):
    """every position of HF's own greedy path, every row: |device - HF| <= g = 1e-3 max(1, max|logits|)"""
    worst, g = logit_errors(mode, fx)
    print(f"DECLOGITS {mode}: worst |device - HF| {worst:.3e}, g {g:.3e}, ratio {worst / g:.3f}")
    assert worst <= g, (worst, g)


# worst |device - HF| over the same positions in bf16, measured once on the MI355X (profiles/transcribe.txt, 2026-10-18): 1.498e-02,
# 3.77 g at g = 3.977e-03
BF16_MEASURED = 1.498e-02


def test_teacher_forced_logits_bf16_measured(fx):
    """bf16 operands round every GEMM input to 8 bits: no gate from first principles, and no token equality is asserted in this mode.  The
    figure is measured and held to twice the value measured once on the MI355X."""
    worst, g = logit_errors("bf16", fx)
    print(f"DECLOGITS bf16: worst |device - HF| {worst:.3e}, g {g:.3e}, ratio {worst / g:.3f}")
    assert worst <= 2 * BF16_MEASURED, (worst, BF16_MEASURED)


@pytest.mark.parametrize("mode", ["fp32x", "f16x"])
def test_greedy_decoding_equals_hf(fx, mode):
    gold, geo, sd, spec, enc = fx
    dec = decoder(mode)
    seqs = gold["a_sequences"]
    g = R.gate(gold["a_logits"].astype(np.float64), seqs, spec)
    res = dec.generate(enc_dev(enc, slice(None)), 3)
    assert not res.failed and res.err == 0
    assert np.array_equal(res.sequences, seqs)                                # tokens, eos / pad tails, the stop step (the length)
    assert np.array_equal(res.languages, gold["a_languages"])
    for b in range(3):
        row = seqs[b, spec.PROMPT_LEN:].tolist()
        assert res.lists[b] == (row[:row.index(spec.eos_token_id)] if spec.eos_token_id in row else row)
    dec_pos = R.decided(seqs, spec)
    stored = np.array([res.margins[b, p] for b, p in dec_pos])
    assert np.isfinite(stored).all() and stored.min() >= 2 * g, (stored.min(), g)
    undecided = np.ones_like(res.margins, dtype=bool)
    for b, p in dec_pos:
        undecided[b, p] = False
    assert np.isinf(res.margins[undecided]).all()
    again = dec.generate(enc_dev(enc, slice(None)), 3)                        # a second replay of the recorded step list
    assert np.array_equal(again.sequences, res.sequences) and np.array_equal(again.margins.view(np.uint32), res.margins.view(np.uint32))
    for b in range(3):                                                        # batch of one == batched, bit for bit
        one = dec.generate(enc_dev(enc, slice(b, b + 1)), 1)
        n = one.sequences.shape[1]
        assert np.array_equal(one.sequences[0], res.sequences[b, :n]) and (res.sequences[b, n:] == spec.pad_token_id).all()
        assert np.array_equal(one.margins[0].view(np.uint32), res.margins[b, : n - 1].view(np.uint32))
    given = dec.generate(enc_dev(enc, slice(None)), 3, language=int(gold["l_language"]))
    assert np.array_equal(given.sequences, gold["l_sequences"]) and np.isinf(given.margins[:, 0]).all()


def test_decoder_modes_and_failure_word(fx, capsys):
    """a mode without a decoder form falls back to f16x with one printed line; a NaN in the encoder states fails the batch (never a silent token)"""
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = fx
    d = WhisperDecoder(geo, sd, DEV, "f16mf", spec)
    assert d.mode_name == "f16x" and "using 'f16x'" in capsys.readouterr().out
    bad = enc.copy()
    bad[1, 700, 3] = np.nan
    res = decoder("fp32x").generate(enc_dev(bad, slice(None)), 3)
    assert res.failed and res.err & 1
    res16 = decoder("f16x").generate(enc_dev(bad, slice(None)), 3)
    assert res16.failed


def synth_wave(seed, n):
    """oracle/make_golden.py's recipe: 0.1 N(0, 1) + a 220 Hz sine at 0.2"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    return np.clip(0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t), -1.0, 1.0).astype(np.float32)


def test_transcriber_waves_to_ids(fx):
    """case "b": two ragged waveforms through the tiny encoder and the decoder -> HF's ids, by WhisperTranscriber"""
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd.engine import WhisperEncoder
    from interspeech_ser_amd.transcribe import WhisperTranscriber
    from interspeech_ser_amd.weights import synthetic_state_dict
    gold, geo, sd, spec, _ = fx
    enc = WhisperEncoder(geo, synthetic_state_dict(Cfg.TINY_WHISPER, int(gold["b_encoder_weight_seed"])), DEV, "f16x")
    waves = [synth_wave(int(s), int(n)) for s, n in zip(gold["b_wave_seeds"], gold["b_lengths"])]
    hs = enc.forward(enc.upload(waves), [len(w) for w in waves])
    last = hs.states[-1].reshape(2, -1, geo.hidden)[:, ::50].cpu().numpy()
    ref = gold["b_enc_last"]
    assert np.abs(last - ref).max() <= 1e-3 * max(1.0, float(np.abs(ref).max()))
    tr = WhisperTranscriber(enc, decoder("f16x"), spec)
    seqs = gold["b_sequences"]
    want = []
    for row in seqs[:, spec.PROMPT_LEN:].tolist():
        want.append(row[:row.index(spec.eos_token_id)] if spec.eos_token_id in row else row)
    assert tr.transcribe(waves) == want
    assert tr.last_languages == gold["b_languages"].tolist()
    long = np.concatenate([waves[1]] * 6)[:500000]                            # longer than 30 s: cut to 30 s, as the feature extractor does
    assert tr.transcribe([long]) == tr.transcribe([long[:480000]])

    class Tok:
        def decode(self, ids, skip_special_tokens=True):
            return " ".join(f"t{i}" for i in ids)
    assert tr.texts(waves, Tok()) == [" ".join(f"t{i}" for i in w) for w in want]


# ---------------------------------------------------------------------------------------------------------------- score_from_wav(transcribe=True)
def test_score_from_wav_with_its_own_transcripts(fx, tmp_path, capsys):
    """bin/predict_cat_from_wav.py --transcribe: the Whisper stream's own transcripts feed the text stream.  It equals score_from_wav fed the
    table preprocessing/transcribe_whisper.py wrote for the same files, byte for byte (both routes make the same launches); without
    vocabulary files a transcript is its ids as decimal numbers, and a stub tokenizer turns that text into RoBERTa ids."""
    import wave
    import pandas as pd
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as T
    from interspeech_ser_amd.predictor import score_from_wav
    from oracle.fusion_head import seeded_head_weights
    import fusion_ref
    gold, geo, sd, spec, _ = fx
    tgeo, max_len = Cfg.TINY_ROBERTA, 16
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    seconds = (0.3, 2.0, 0.71, 1.2, 0.5)
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(len(seconds))]
    for i, (name, s) in enumerate(zip(names, seconds)):
        with wave.open(str(wav_dir / name), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(synth_wave(20 + i, int(16000 * s)) * 32767.0).astype("<i2").tobytes())
    pd.DataFrame({"FileName": names}).to_csv(tmp_path / "test.csv", index=False)

    def stub_tokenize(batch):
        ids = torch.full((len(batch), max_len), tgeo.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((len(batch), max_len), dtype=torch.int64)
        for i, t in enumerate(batch):
            toks = ([0] + [3 + int(w) % (tgeo.vocab_size - 4) for w in t.split()])[: max_len - 1] + [2]
            ids[i, : len(toks)] = torch.tensor(toks)
            mask[i, : len(toks)] = 1
        return ids, mask

    head_sd = seeded_head_weights(fusion_ref.head_shapes(128, 128, h=64), 31)
    cfgs = []
    for tag in ("table", "transcribe"):
        cfg = {"wav_dir": str(wav_dir), "feat1_dim": 128, "feat2_dim": 128, "model_path": str(tmp_path / f"exp_{tag}")}
        if tag == "table":                                                    # the transcribe config has no txt_dir at all
            cfg["txt_dir"] = str(tmp_path / "whisper_transcripts.csv")
        os.makedirs(cfg["model_path"])
        torch.save(head_sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
        cfgs.append(cfg)
    Cfg._REGISTRY["tiny-whisper-dec-from-wav"], Cfg._REGISTRY["tiny-roberta-for-transcripts"] = geo, tgeo
    try:
        assert T.run(["--ssl_type", "tiny-whisper-dec-from-wav", "--wav_dir", str(wav_dir), "--out_csv", cfgs[0]["txt_dir"], "--synthetic_weights",
                      "--seed", "7", "--mode", "f16x"], spec=spec) == 0
        table = T.read_table(cfgs[0]["txt_dir"])
        assert sorted(table) == names and all(all(w.isdigit() for w in t.split()) and t for t in table.values()), table
        common = dict(test_csv=str(tmp_path / "test.csv"), mode="f16x", text_mode="f16x", head_mode="f16x", batch_size=16, max_len=max_len,
                      synthetic_weights=True, seed=7, tokenize=stub_tokenize)
        encs = ["tiny-whisper-dec-from-wav", "tiny-roberta-for-transcripts"]
        capsys.readouterr()
        a = score_from_wav(cfgs[0], encs, **common)
        b = score_from_wav(cfgs[1], encs, transcribe=True, spec=spec, **common)
        log = capsys.readouterr().out
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-dec-from-wav")
        Cfg._REGISTRY.pop("tiny-roberta-for-transcripts")
    assert a["n"] == b["n"] == 5 and a["failed"] == b["failed"] == 0, log
    assert open(a["csv"], "rb").read() == open(b["csv"], "rb").read()
    assert "txt_dir" not in cfgs[1] and len(open(b["csv"]).read().splitlines()) == 6


def test_failed_transcription_leaves_no_stale_guard_bit(fx):
    """A decode that fails inside FusionPredictor raises before predict() reads the encoder's fp16 range-guard word: the word must be taken
    and cleared there, or the file-by-file retry's first forward fails on the stale bit.  WhisperDecoder.begin() clears its own word."""
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd._lib import SerHipError
    from interspeech_ser_amd.engine import DecodeResult, TextEncoder, WhisperEncoder
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, TextStream
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle.fusion_head import seeded_head_weights
    import fusion_ref
    gold, geo, sd, spec, _ = fx
    enc = WhisperEncoder(geo, synthetic_state_dict(Cfg.TINY_WHISPER, 14), DEV, "f16x")
    txt = TextEncoder(Cfg.TINY_ROBERTA, synthetic_state_dict(Cfg.TINY_ROBERTA, 15), DEV, "f16x")
    pred = FusionPredictor([AudioStream(enc), TextStream(txt)], seeded_head_weights(fusion_ref.head_shapes(128, 128, h=64), 31), "f16x")
    seen = {}

    class FailingDecoder:
        def generate(self, last_state, B, spec_):
            seen["flag"] = next(iter(enc._cache.values()))["range_flag"]
            seen["flag"].fill_(3)                                             # as if the forward had saturated an fp16 plane
            return DecodeResult(np.zeros((B, 4), np.int64), np.zeros(B, np.int64), [[] for _ in range(B)], np.zeros((B, 3), np.float32), 0, 1)

    def tokenize(texts):
        ids = torch.full((len(texts), 8), Cfg.TINY_ROBERTA.pad_token_id, dtype=torch.int64)
        ids[:, 0], ids[:, 1] = 0, 2
        mask = torch.zeros((len(texts), 8), dtype=torch.int64)
        mask[:, :2] = 1
        return ids, mask
    pred.transcribe_with(FailingDecoder(), spec, tokenize)
    with pytest.raises(SerHipError, match="transcription failed"):
        pred.predict([synth_wave(3, 8000), synth_wave(4, 12000)])
    assert int(seen["flag"].item()) == 0
    dec = decoder("f16x")
    pl = dec.begin(1, spec)
    pl["range_flag"].fill_(3)
    assert int(dec.begin(1, spec)["range_flag"].item()) == 0
