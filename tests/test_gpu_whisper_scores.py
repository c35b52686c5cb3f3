"""GPU: Whisper transcript scores (csrc/whisper_score.hip, include/ser_hip.h "a38").

A. ser_dec_select_score_v against the rule (tests/whisper_score_ref.py) on scripted logits, no model, both plans (rule 0 / 1), V = 9, 522
   and 51 866: token, margin, ts_gap, ids, finished, tickets, *pos and *unfinished bit for bit those of ser_dec_select_v /
   ser_dec_select_ts_v launched on the same inputs; logprob and no_speech within ``score_bound`` of the rule; the error bits; a row alone
   against the same row in a batch, bit for bit.
B. The engine: the scored plans give the unscored plans' tokens, margins and ts_gaps bit for bit and leave the default plans' command
   lists alone; in every mode the rule fed the device's own logits reproduces the device's log-probabilities, no-speech probabilities and
   average; the refusals.
C. WhisperTranscriber: scores of a batch equal the per-file ones; the long-form queue skips on the device's own scores, the same at
   batch 2 and 16; the command line.
D. tests/golden/tiny_whisper_score_d128h2.npz (HF's long-form loop under thresholds, a skipped middle window): tokens, seeks, segments,
   skip decisions and needs_fallback equal HF's for every file, alone and through the queue at batch 2 and 16, in f16x and fp32x; every
   token's log-probability within 2 g of HF's float64 value, the no-speech probability within expm1(2 g) relatively.
Lines that start with "SCORES" carry the measured figures.
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import whisper_dec_ref as R
import whisper_long_ref as LR
import whisper_score_ref as QR
import whisper_seg_ref as SR
from interspeech_ser_amd._lib import DecSelectScoreArgs                       # the feature's binding: the module needs it
from test_gpu_whisper_decoder import enc_dev, stream, synth_wave
from test_gpu_whisper_segments import LAYOUTS, MAXPOS, P, steady_script

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def score_bound(V, value):
    """|device - numpy| of a log-probability or a no-speech probability computed from the same fp32 values, u = 2^-53.  Both sides form
    (x[tok] - w) - log S around the row's maximum w, S = sum exp(x_v - w) over at most V terms in (0, 1]: each exp within 1 ulp = 2 u, added
    in some order: S (1 + d), |d| <= (V + 1) u; the device joins its two partial sums with one exp, one product and one addition more
    (4 u); log S moves by |d| absolutely plus its own ulp, 2 u |log S|; the subtraction rounds once.  One side: u ((V + 5) + 3 |value|) <=
    u (V + 8) max(1, |value|); two sides: 2^-52 (V + 8) max(1, |value|) -- ts_gap's bound (tests/test_gpu_whisper_segments.gap_bound) with
    the value itself as the only magnitude, because the maximum is taken off before anything is rounded.  A probability p = e / S is
    bounded the same way relatively, and p <= 1."""
    return 2.0 ** -52 * (V + 8) * max(1.0, abs(float(value)))


# ---------------------------------------------------------------------------------------------------------------- one launch
def launch(kind, lay, logits, ids, *, pos, forced=None, phase=None, finished=None, mask=None, max_initial=-1, pad=0, begin_index=P,
           no_speech_token=None, mutate=None):
    """One launch of ``kind``: "plain" (ser_dec_select_v), "ts" (ser_dec_select_ts_v), "score0" / "score1" (ser_dec_select_score_v with
    rule 0 / 1) on fresh device copies of the same inputs.  logits fp32 [B, V] (host; the padded columns hold NaN: a kernel that read one
    would fail the batch), ids [B, <= MAXPOS] the rows so far.  Returns the whole state afterwards (host), canaries checked."""
    from interspeech_ser_amd import _lib
    B, V = logits.shape[0], lay.V
    z = np.full((B, lay.ld), np.nan, dtype=np.float32)
    z[:, :V] = logits
    lg = torch.from_numpy(z).to(DEV)
    mk = torch.zeros((3, V), dtype=torch.float32, device=DEV) if mask is None else torch.from_numpy(mask.astype(np.float32)).to(DEV)
    ph = torch.zeros(MAXPOS, dtype=torch.int32, device=DEV) if phase is None else torch.tensor(phase, dtype=torch.int32, device=DEV)
    fo = torch.full((MAXPOS,), -1, dtype=torch.int32, device=DEV) if forced is None else torch.tensor(forced, dtype=torch.int32, device=DEV)
    host_ids = np.full((B + 2, MAXPOS), -9, dtype=np.int32)
    for b, row in enumerate(ids):
        host_ids[b + 1, : len(row)] = row
    idt = torch.from_numpy(host_ids).to(DEV)
    fin = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    fin[B] = -9
    if finished is not None:
        fin[:B] = torch.tensor(finished, dtype=torch.int32)
    margin = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float32, device=DEV)
    gap = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float64, device=DEV)
    lp = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float64, device=DEV)
    ns = torch.full((B + 2,), -9.0, dtype=torch.float64, device=DEV)
    word = torch.tensor([pos, -9, 0, 0, 0, -9], dtype=torch.int32, device=DEV)            # pos, unfinished, work[2], err, canary
    q = DecSelectScoreArgs()
    x = q.ts
    a = x.base
    a.logits, a.ldl, a.mask, a.ldm, a.phase, a.forced = lg.data_ptr(), lay.ld, mk.data_ptr(), V, ph.data_ptr(), fo.data_ptr()
    a.ids, a.ld_ids, a.finished = idt.data_ptr() + MAXPOS * 4, MAXPOS, fin.data_ptr()
    a.margin, a.ld_margin = margin.data_ptr() + MAXPOS * 4, MAXPOS
    a.pos, a.unfinished, a.work, a.err = word.data_ptr(), word.data_ptr() + 4, word.data_ptr() + 8, word.data_ptr() + 16
    a.B, a.V, a.eos, a.pad, a.max_pos = B, V, lay.eos, pad, MAXPOS
    if kind in ("ts", "score1"):
        x.ts_gap, x.ld_gap = gap.data_ptr() + MAXPOS * 8, MAXPOS
        x.ts_begin, x.no_ts, x.begin_index, x.max_initial = lay.tsb, lay.no_ts, begin_index, max_initial
    q.logprob, q.ld_logprob, q.no_speech = lp.data_ptr() + MAXPOS * 8, MAXPOS, ns.data_ptr() + 8
    q.no_speech_token, q.rule = lay.no_ts - 1 if no_speech_token is None else no_speech_token, 1 if kind == "score1" else 0
    fn = {"plain": _lib.lib.ser_dec_select_v, "ts": _lib.lib.ser_dec_select_ts_v}.get(kind, _lib.lib.ser_dec_select_score_v)
    arg = {"plain": a, "ts": x}.get(kind, q)
    if mutate is not None:
        mutate(q)
        return fn(C.byref(arg), stream())
    _lib.check(fn(C.byref(arg), stream()), kind)
    torch.cuda.synchronize()
    ids_h, mg, gp, w, f = idt.cpu().numpy(), margin.cpu().numpy(), gap.cpu().numpy(), word.cpu().numpy(), fin.cpu().numpy()
    lp_h, ns_h = lp.cpu().numpy(), ns.cpu().numpy()
    for arr in (ids_h, mg, gp, lp_h):
        assert (arr[0] == -9).all() and (arr[B + 1] == -9).all(), "a canary row was written"
    assert f[B] == -9 and w[5] == -9 and ns_h[0] == -9 and ns_h[B + 1] == -9 and w[2] == 0 and w[3] == 0
    written = np.zeros_like(ids_h, dtype=bool)
    col = np.ones((B, MAXPOS), dtype=bool)
    if 0 <= pos < MAXPOS - 1:
        written[1: B + 1, pos + 1] = True
        col[:, pos] = False
    assert np.array_equal(ids_h[~written], host_ids[~written]), "ids changed outside column pos + 1"
    for arr in (mg, gp, lp_h):
        assert (arr[1: B + 1][col] == -9).all(), "margin / ts_gap / logprob changed outside column pos"
    if kind in ("plain", "score0"):
        assert (gp == -9).all(), "no ts_gap without the rule"
    if kind in ("plain", "ts"):
        assert (lp_h == -9).all() and (ns_h == -9).all()
    if pos != 0:
        assert (ns_h == -9).all(), "no_speech is written by the step at position 0 only"
    c = min(max(pos, 0), MAXPOS - 1)
    return dict(ids=ids_h[1: B + 1], token=ids_h[1: B + 1, min(pos + 1, MAXPOS - 1)], margin=mg[1: B + 1, c], gap=gp[1: B + 1, c],
                logprob=lp_h[1: B + 1, c], no_speech=ns_h[1: B + 1], finished=f[:B], pos=int(w[0]), unfinished=int(w[1]),
                err=int(w[4]) & 0xffffffff)


def same_bits(scored, base):
    """token choice, margin, ts_gap, ids, finished flags, position and count: bit for bit the unscored kernel's"""
    assert np.array_equal(scored["ids"], base["ids"]) and scored["margin"].tobytes() == base["margin"].tobytes()
    assert scored["gap"].tobytes() == base["gap"].tobytes() and scored["finished"].tolist() == base["finished"].tolist()
    assert (scored["pos"], scored["unfinished"]) == (base["pos"], base["unfinished"])


def check_logprobs(lay, got, want, decided):
    worst = 0.0
    for b, lp in enumerate(want):
        if not decided[b]:
            assert np.isinf(got[b]) and got[b] > 0, (b, got[b])
            continue
        bound = score_bound(lay.V, lp)
        worst = max(worst, abs(got[b] - lp) / bound)
        assert abs(got[b] - lp) <= bound, (b, got[b], lp, bound)
    return worst


def the_mask(lay):
    mask = np.zeros((3, lay.V))
    mask[0, 2] = mask[1, 2] = -np.inf                                         # a suppressed text token, everywhere
    mask[1, lay.ts(0)] = -np.inf
    mask[2] = -np.inf
    mask[2, [0, 1]] = 0.0                                                     # the language set
    return mask


PHASE = [2] + [0] * (P - 2) + [1] + [0] * (MAXPOS - P)


@pytest.mark.parametrize("name", ["V9", "V522", "V51866"])
def test_scored_select_with_the_rule(name):
    """every branch of whisper_seg_ref's script at n = 5 (a closed pair, an opening timestamp, the bound, the outweigh case, L == M, a
    -inf-masked neighbour of the winner, a finished row), then n = 0 with max_initial, n = 1, a forced step and the language step"""
    lay = LAYOUTS[name]
    mask = the_mask(lay)
    z, rows, names, ties = steady_script(lay, seed=4)
    z[names.index("text-text"), 3] = 49.0                                     # beside the winner (column 2 holds 50, and is masked): the runner-up wins
    pos = P + 4
    fin = [0] * len(rows)
    fin[4] = 1
    base = launch("ts", lay, z, rows, pos=pos, mask=mask, phase=PHASE, finished=fin, pad=1)
    got = launch("score1", lay, z, rows, pos=pos, mask=mask, phase=PHASE, finished=fin, pad=1)
    same_bits(got, base)
    assert got["err"] == base["err"] == 0
    want, fired = [], []
    for b, row in enumerate(rows):
        x, tok, _, gp, lp = QR.score_ts(z[b].astype(np.float64), mask[0], row[P: pos + 1], lay.tsb, lay.no_ts, lay.eos)
        assert gp >= 1e-3 or (gp == 0.0 and names[b] == "L-equals-M"), f"row {names[b]} decides its sum rule by {gp:.3e}: script it again"
        assert fin[b] or tok == got["token"][b]
        want.append(lp)
        fired.append(bool(np.isneginf(x[: lay.tsb]).all()))
    assert fired[names.index("sum-fires")] and got["token"][names.index("text-text")] == 3
    assert got["gap"][names.index("L-equals-M")] == 0.0 and not fired[names.index("L-equals-M")]
    worst = check_logprobs(lay, got["logprob"], want, [not f for f in fin])
    b = names.index("sum-fires")                                              # the outweigh case: the normaliser is the L of the sum rule
    x = SR.rule(z[b].astype(np.float64), mask[0], rows[b][P: pos + 1], lay.tsb, lay.no_ts, lay.eos)[0]
    assert abs(got["logprob"][b] - (x[got["token"][b]] - SR.logsumexp(x[lay.tsb:]))) <= 1e-9
    print(f"SCORES kernel rule=1 {name} B={len(rows)}: worst |logprob - rule| / bound {worst:.3f}")
    # B = 1 and 3: a row alone and in a batch, bit for bit
    three = launch("score1", lay, z[5:8], rows[5:8], pos=pos, mask=mask, phase=PHASE)
    for b in range(3):
        one = launch("score1", lay, z[5 + b: 6 + b], rows[5 + b: 6 + b], pos=pos, mask=mask, phase=PHASE)
        for k in ("token", "margin", "gap", "logprob"):
            assert one[k][:1].tobytes() == three[k][b: b + 1].tobytes() == got[k][5 + b: 6 + b].tobytes(), (k, b)
    # n == 0 (text masked, max_initial) and n == 1
    g = np.random.default_rng(5)
    z0 = (2.0 * g.standard_normal((3, lay.V))).astype(np.float32)
    z0[:, 1] = 40.0
    z0[1, lay.ts(3)] = 30.0
    rows0 = [[0, 0, 0]] * 3
    for mi in (None, 2):
        kw = dict(pos=P - 1, mask=mask, phase=PHASE, max_initial=-1 if mi is None else mi)
        s0, b0 = launch("score1", lay, z0, rows0, **kw), launch("ts", lay, z0, rows0, **kw)
        same_bits(s0, b0)
        want0 = [QR.score_ts(z0[b].astype(np.float64), mask[1], [], lay.tsb, lay.no_ts, lay.eos, mi)[4] for b in range(3)]
        check_logprobs(lay, s0["logprob"], want0, [True] * 3)
        assert s0["err"] == 0
    z1 = (2.0 * g.standard_normal((2, lay.V))).astype(np.float32)
    rows1 = [[0, 0, 0, lay.ts(0)], [0, 0, 0, 1]]
    s1, b1 = launch("score1", lay, z1, rows1, pos=P, mask=mask, phase=PHASE), launch("ts", lay, z1, rows1, pos=P, mask=mask, phase=PHASE)
    same_bits(s1, b1)
    check_logprobs(lay, s1["logprob"], [QR.score_ts(z1[b].astype(np.float64), mask[0], rows1[b][P:], lay.tsb, lay.no_ts, lay.eos)[4] for b in range(2)], [True] * 2)
    # a forced step reads no logits and scores nothing
    forced = [-1] * MAXPOS
    forced[1] = lay.eos - 1
    nan = np.full((2, lay.V), np.nan, dtype=np.float32)
    f = launch("score1", lay, nan, [[0, 0], [0, 0]], pos=1, mask=mask, phase=PHASE, forced=forced)
    same_bits(f, launch("ts", lay, nan, [[0, 0], [0, 0]], pos=1, mask=mask, phase=PHASE, forced=forced))
    assert f["err"] == 0 and np.isinf(f["logprob"]).all() and (f["logprob"] > 0).all()


@pytest.mark.parametrize("name", ["V9", "V522", "V51866"])
@pytest.mark.parametrize("kind", ["score0", "score1"])
def test_position_zero_writes_the_no_speech_probability(name, kind):
    """the step at position 0, language detected (phase 2) and language forced: softmax of the RAW row at the no-speech token whatever the
    mask and the rule do, next to the unscored kernel's bits; a NaN or an infinity in that row sets bit 0"""
    lay = LAYOUTS[name]
    mask = the_mask(lay)
    base_kind = "plain" if kind == "score0" else "ts"
    g = np.random.default_rng(17)
    B = 3
    z = (2.0 * g.standard_normal((B, lay.V))).astype(np.float32)
    z[0, lay.no_ts - 1] = 25.0                                                # silence: the no-speech token dominates, and the mask hides it
    z[1, lay.no_ts - 1] = -20.0
    rows = [[0]] * B
    for forced_lang in (None, 1):
        forced = [-1] * MAXPOS
        if forced_lang is not None:
            forced[0] = forced_lang
        got = launch(kind, lay, z, rows, pos=0, mask=mask, phase=PHASE, forced=forced)
        same_bits(got, launch(base_kind, lay, z, rows, pos=0, mask=mask, phase=PHASE, forced=forced))
        assert got["err"] == 0 and got["pos"] == 1
        worst = 0.0
        for b in range(B):
            want = QR.no_speech(z[b], lay.no_ts - 1)
            worst = max(worst, abs(got["no_speech"][b] - want) / score_bound(lay.V, want))
            assert abs(got["no_speech"][b] - want) <= score_bound(lay.V, want), (b, got["no_speech"][b], want)
            if forced_lang is None:
                x, tok, _, lp = QR.score_plain(z[b], mask[2])
                assert tok == got["token"][b] and abs(got["logprob"][b] - lp) <= score_bound(lay.V, lp)
            else:
                assert got["token"][b] == forced_lang and np.isinf(got["logprob"][b])
        assert got["no_speech"][0] > 0.9 and got["no_speech"][1] < 1e-6
        print(f"SCORES kernel {kind} {name} position 0 forced={forced_lang}: worst |no_speech - rule| / bound {worst:.3f}")
        alone = launch(kind, lay, z[2:3], rows[2:3], pos=0, mask=mask, phase=PHASE, forced=forced)
        assert alone["no_speech"][:1].tobytes() == got["no_speech"][2:3].tobytes() and alone["logprob"][:1].tobytes() == got["logprob"][2:3].tobytes()
    for bad in (np.nan, np.inf, -np.inf):
        zb = z.copy()
        zb[1, lay.V - 1] = bad                                                # masked at the language step: only the raw row sees it
        forced = [-1] * MAXPOS
        forced[0] = 1
        e = launch(kind, lay, zb, rows, pos=0, mask=mask, phase=PHASE, forced=forced)
        assert e["err"] & 1 and np.isnan(e["no_speech"][1]) and np.isfinite(e["no_speech"][[0, 2]]).all(), bad
        assert launch(base_kind, lay, zb, rows, pos=0, mask=mask, phase=PHASE, forced=forced)["err"] == 0, "the unscored kernel does not read a forced step's row"


@pytest.mark.parametrize("name", ["V9", "V522", "V51866"])
def test_scored_select_without_the_rule(name):
    """ser_dec_select_v's choice with scores: ties, a masked maximum beside the winner, a finished row, eos, and the error bits"""
    lay = LAYOUTS[name]
    V = lay.V
    g = np.random.default_rng(23)
    B = 6
    z = (2.0 * g.standard_normal((B, V))).astype(np.float32)
    mask = the_mask(lay)
    z[0, [3, V - 1]] = 19.0                                                   # a tie: the lowest index wins, margin 0
    z[1, 2], z[1, 3] = 50.0, 20.0                                             # the masked maximum's neighbour wins
    z[2, lay.eos] = 30.0                                                      # row 2 chooses eos
    pos = 5
    rows = [[0] * (pos + 1)] * B
    fin = [0] * B
    fin[4] = 1
    got = launch("score0", lay, z, rows, pos=pos, mask=mask, finished=fin, pad=1)
    same_bits(got, launch("plain", lay, z, rows, pos=pos, mask=mask, finished=fin, pad=1))
    assert got["err"] == 0 and got["token"][:3].tolist() == [3, 3, lay.eos] and got["margin"][0] == 0.0 and got["finished"][2] == 1
    want = [QR.score_plain(z[b], mask[0])[3] for b in range(B)]
    worst = check_logprobs(lay, got["logprob"], want, [not f for f in fin])
    assert abs(got["logprob"][0] - (-np.log(2.0))) < 1e-3 or V > 9, "two equal maxima far above the rest: log 1/2"
    print(f"SCORES kernel rule=0 {name} B={B}: worst |logprob - rule| / bound {worst:.3f}")
    for b in range(min(B, 3)):
        one = launch("score0", lay, z[b: b + 1], rows[b: b + 1], pos=pos, mask=mask)
        for k in ("token", "margin", "logprob"):
            assert one[k][:1].tobytes() == got[k][b: b + 1].tobytes(), (k, b)
    bad = z.copy()
    bad[0, 4] = np.nan                                                        # a NaN wins and fails the batch, as in the unscored kernel
    e, e0 = launch("score0", lay, bad, rows, pos=pos, mask=mask), launch("plain", lay, bad, rows, pos=pos, mask=mask)
    same_bits(e, e0)
    assert e["err"] & 1 and e0["err"] & 1 and e["token"][0] == 4 and np.isnan(e["logprob"][0]) and np.isfinite(e["logprob"][1:]).all()
    dead = np.zeros((3, V))
    dead[0] = -np.inf                                                         # nothing is live: no finite winner, no finite normaliser
    assert launch("score0", lay, z, rows, pos=pos, mask=dead)["err"] & 1
    assert launch("score0", lay, bad, rows, pos=pos, mask=mask, finished=[1] + [0] * (B - 1))["err"] == 0, "a finished row's logits decide nothing"
    end = launch("score0", lay, z, [[0] * MAXPOS] * B, pos=MAXPOS - 1, mask=mask)
    assert end["err"] & 4 and end["pos"] == MAXPOS - 1


def test_scored_select_refuses_bad_arguments():
    lay = LAYOUTS["V9"]
    z = np.zeros((1, 9), dtype=np.float32)
    for what in (lambda q: setattr(q, "logprob", 0), lambda q: setattr(q, "no_speech", 0), lambda q: setattr(q, "ld_logprob", MAXPOS - 2),
                 lambda q: setattr(q, "no_speech_token", 9), lambda q: setattr(q, "no_speech_token", -1), lambda q: setattr(q, "rule", 2),
                 lambda q: setattr(q.ts, "ts_begin", 0), lambda q: setattr(q.ts, "ts_gap", 0), lambda q: setattr(q.ts.base, "V", 1)):
        assert launch("score1", lay, z, [[0, 0, 0]], pos=2, mutate=what) != 0
    assert launch("score0", lay, z, [[0, 0, 0]], pos=2, mutate=lambda q: setattr(q.ts, "ts_gap", 0)) == 0, "rule 0 reads no ts_gap"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the engine
@functools.lru_cache(maxsize=None)
def fixtures():
    return R.load_fixture(GOLDEN), SR.load_fixture(GOLDEN)


@functools.lru_cache(maxsize=None)
def decoders(mode):
    from interspeech_ser_amd.engine import WhisperDecoder
    (_, geo, sd, spec, _), (_, sgeo, ssd, sspec, _) = fixtures()
    return WhisperDecoder(geo, sd, DEV, mode, spec), WhisperDecoder(sgeo, ssd, DEV, mode, sspec)


def tape_bytes(pl):
    return C.string_at(C.addressof(pl["tape"].cmds), pl["tape"].n * C.sizeof(type(pl["tape"].cmds[0])))


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_engine_scored_plans_give_the_unscored_tokens_and_the_rule_on_their_own_logits(mode):
    """both scored plans against the unscored ones (bit for bit: sequences, margins, ts_gaps, segments), the default plans' command
    lists before and after, and the scores against the numpy rule fed the device's own fp32 logits"""
    (_, geo, _, spec, enc), (_, sgeo, _, sspec, senc) = fixtures()
    dec, sdec = decoders(mode)
    V = geo.decoder_vocab_size
    m, sm = R.masks(spec, V), R.masks(sspec, sgeo.decoder_vocab_size)
    for d, e, sp, masks, ts in ((dec, enc, spec, m, False), (sdec, senc, sspec, sm, True)):
        B = e.shape[0]
        kw = dict(timestamps=True) if ts else {}
        plain = d.generate(enc_dev(e, slice(None)), B, **kw)
        pl = d._plan(B, 0, timestamps=ts)
        tape = tape_bytes(pl)
        got = d.generate(enc_dev(e, slice(None)), B, scores=True, keep_logits=True, **kw)
        again = d.generate(enc_dev(e, slice(None)), B, **kw)
        assert d._plan(B, 0, timestamps=ts) is pl and tape_bytes(pl) == tape, "the unscored plan's command list is what it was"
        assert not got.failed and not plain.failed
        for r in (got, again):
            assert np.array_equal(r.sequences, plain.sequences) and r.margins.tobytes() == plain.margins.tobytes() and r.lists == plain.lists
        if ts:
            assert got.ts_gaps.tobytes() == plain.ts_gaps.tobytes() and got.segments == plain.segments and got.next_seek.tolist() == plain.next_seek.tolist()
        assert plain.token_logprobs is None and plain.no_speech_prob is None and again.avg_logprob is None
        Pp = sp.prompt_len(ts)
        logits, first = got.step_logits.cpu().numpy(), got.first_logits.cpu().numpy()
        worst = 0.0
        for b in range(B):
            gen = got.sequences[b, Pp:].tolist()
            n = gen.index(sp.eos_token_id) + 1 if sp.eos_token_id in gen else len(gen)
            assert len(got.token_logprobs[b]) == n >= 1
            for s in range(n):
                row = masks[1 if s == 0 else 0]
                if ts:
                    _, tok, _, _, lp = QR.score_ts(logits[s, b], row, gen[:s], sp.timestamp_begin, sp.no_timestamps_token_id, sp.eos_token_id,
                                                   sp.max_initial_timestamp_index)
                else:
                    _, tok, _, lp = QR.score_plain(logits[s, b], row)
                assert tok == gen[s], (b, s)
                worst = max(worst, abs(got.token_logprobs[b][s] - lp) / score_bound(V, lp))
                assert abs(got.token_logprobs[b][s] - lp) <= score_bound(V, lp), (b, s, got.token_logprobs[b][s], lp)
            assert got.avg_logprob[b] == QR.avg_logprob(got.token_logprobs[b])
            ns = QR.no_speech(first[b], sp.no_speech_token)
            assert abs(got.no_speech_prob[b] - ns) <= score_bound(V, ns), (b, got.no_speech_prob[b], ns)
        # a file alone gives the same scores, bit for bit; and so does a forced language (the step at position 0 still computes its logits)
        one = d.generate(enc_dev(e, slice(1, 2)), 1, scores=True, **kw)
        assert one.token_logprobs[0].tobytes() == got.token_logprobs[1].tobytes() and one.no_speech_prob[0] == got.no_speech_prob[1]
        lang = d.generate(enc_dev(e, slice(1, 2)), 1, scores=True, language=int(got.languages[1]), **kw)
        assert lang.token_logprobs[0].tobytes() == got.token_logprobs[1].tobytes() and lang.no_speech_prob[0] == got.no_speech_prob[1]
        print(f"SCORES engine {mode} {'timestamps' if ts else 'greedy'}: worst |logprob - rule on own logits| / bound {worst:.3f}; avg_logprob "
              f"{np.array2string(got.avg_logprob, precision=4)}, no_speech_prob {np.array2string(got.no_speech_prob, precision=3)}")


def test_engine_refusals():
    (_, geo, _, spec, enc), _ = fixtures()
    dec, _ = decoders("f16x")
    with pytest.raises(ValueError, match="scores=True with num_beams > 1"):
        dec.generate(enc_dev(enc, slice(None)), 3, scores=True, num_beams=2)
    with pytest.raises(ValueError, match="scores=True with token_times"):
        dec.generate(enc_dev(enc, slice(None)), 3, scores=True, token_times=True, lengths=[16000] * 3)


# ---------------------------------------------------------------------------------------------------------------- the transcriber
@functools.lru_cache(maxsize=None)
def long_transcriber(mode="f16x"):
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperDecoder, WhisperEncoder
    gold, geo, sd, spec, waves = LR.load_fixture(GOLDEN)
    return TR.WhisperTranscriber(WhisperEncoder(geo, sd, DEV, mode), WhisperDecoder(geo, sd, DEV, mode, spec), spec), waves


def _tokens_with_eos(tr, ids, entry, kw):
    """a greedy file's generated tokens as the rule counts them: its ids and, when one was generated, the closing eos"""
    return list(ids) + [tr.spec.eos_token_id] * (len(entry["token_logprobs"]) - len(ids))


def test_transcriber_scores_alone_and_batched():
    tr, _ = long_transcriber()
    waves = [synth_wave(3000, 16000), synth_wave(3013, 100000), synth_wave(3021, 48000)]
    for kw in ({}, dict(timestamps=True)):
        plain = tr.transcribe(waves, **kw)
        assert tr.scores == [None] * 3
        both = tr.transcribe(waves, scores=True, **kw)
        scores = list(tr.scores)
        assert both == plain and all(s is not None for s in scores)
        V = tr.dec.geo.decoder_vocab_size
        for i, w in enumerate(waves):
            assert tr.transcribe([w], scores=True, **kw) == [both[i]] and tr.scores == [scores[i]], "a file alone: the same bits"
            s = scores[i]
            assert sorted(s) == ["avg_logprob", "compression_ratio", "needs_fallback", "no_speech_prob", "skipped", "token_logprobs"]
            assert s["avg_logprob"] == QR.avg_logprob(s["token_logprobs"]) < 0.0 <= s["no_speech_prob"] <= 1.0
            assert not s["needs_fallback"] and not s["skipped"], "no threshold is set"
            assert len(s["token_logprobs"]) >= len(both[i]), "one log-probability per generated token, the eos included"
            assert s["compression_ratio"] == QR.compression_ratio(_tokens_with_eos(tr, both[i], s, kw), V) if not kw else s["compression_ratio"] > 0.0


def test_long_form_queue_skips_on_the_devices_own_scores():
    """thresholds chosen between the scores the device itself gives the windows of the fixture's files: the queue then skips exactly
    the windows HF's rule names, a skipped window advances by its nf and contributes nothing, and batch 2 and 16 agree"""
    import dataclasses
    from interspeech_ser_amd import transcribe as TR
    tr, waves = long_transcriber()
    items = [(f"f{k}.wav", w) for k, w in enumerate(waves)] + [("short.wav", synth_wave(3013, 100000))]
    base = tr.transcribe_long(iter(items), batch=16)
    plain_windows = [list(w) for w in tr.windows]
    assert all(len(w) == 3 for wins in plain_windows for w in wins)
    scored = tr.transcribe_long(iter(items), batch=16, scores=True)
    assert scored == base and [[w[:3] for w in wins] for wins in tr.windows] == plain_windows, "scores alone change nothing"
    entries = [w[3] for wins in tr.windows for w in wins]
    assert len(entries) >= 6 and not any(e["skipped"] or e["needs_fallback"] for e in entries)
    # the target: the first window (its scores do not depend on what was skipped before it) with the lowest average; the thresholds lie
    # halfway to the next window's values, so the target is skipped and every other first window is kept
    first = [wins[0][3] for wins in tr.windows]
    target = min(first, key=lambda e: e["avg_logprob"])
    above = [e["avg_logprob"] for e in entries if e["avg_logprob"] > target["avg_logprob"]]
    below = [e["no_speech_prob"] for e in entries if e["no_speech_prob"] < target["no_speech_prob"]]
    limits = dict(logprob_threshold=0.5 * (target["avg_logprob"] + min(above)),
                  no_speech_threshold=0.5 * (target["no_speech_prob"] + max(below)) if below else 0.5 * target["no_speech_prob"])
    expect_first = [e["avg_logprob"] < limits["logprob_threshold"] and e["no_speech_prob"] > limits["no_speech_threshold"] for e in first]
    spec = tr.spec
    try:
        tr.spec = dataclasses.replace(spec, **limits)
        runs = []
        for batch in (2, 16):
            ids = tr.transcribe_long(iter(items), batch=batch)
            assert tr.failed == [] and all(i is not None for i in ids)
            runs.append((ids, [list(w) for w in tr.windows], list(tr.next_seek), [list(s) for s in tr.segments]))
            for i, (name, w) in enumerate(items):
                F, at, nseg = len(w) // 160, 0, 0
                assert tr.windows[i][0][3]["skipped"] == expect_first[i], "the first window is the one the unthresholded run scored"
                for seek, nf, adv, e in tr.windows[i]:
                    assert seek == at and nf == min(3000, F - seek)
                    assert e["skipped"] == (e["avg_logprob"] < limits["logprob_threshold"] and e["no_speech_prob"] > limits["no_speech_threshold"])
                    assert e["needs_fallback"] == (e["avg_logprob"] < limits["logprob_threshold"] and not e["skipped"])
                    assert adv == nf if e["skipped"] else adv > 0
                    at += adv
                assert at == tr.next_seek[i] >= min(F, 3000)
                kept = [(seek, nf) for seek, nf, adv, e in tr.windows[i] if not e["skipped"]]
                # a segment starts at its window's offset plus a timestamp token's time (up to 30 s, whatever nf is), and every kept
                # window yields at least one segment
                assert all(any(seek * 0.01 - 1e-9 <= a <= seek * 0.01 + 30.0 + 1e-9 for seek, nf in kept) for a, b, _ in tr.segments[i])
                assert len(tr.segments[i]) >= len(kept)
                if not kept:
                    assert ids[i] == [] and tr.segments[i] == []
        assert runs[0] == runs[1], "batch 2 and batch 16"
        flat = [e for wins in runs[1][1] for *_, e in wins]
        print(f"SCORES queue: thresholds {limits}; {sum(e['skipped'] for e in flat)} of {len(flat)} windows skipped, "
              f"{sum(e['needs_fallback'] for e in flat)} flagged for fallback")
        assert any(e["skipped"] for e in flat) and any(not e["skipped"] for e in flat)
    finally:
        tr.spec = spec
    assert tr.transcribe_long(iter(items), batch=16) == base and [list(w) for w in tr.windows] == plain_windows, "the unscored queue afterwards"


def test_command_line_scores_json(tmp_path, capsys):
    """--scores_json on the greedy path, with --segments_json and with --long_form (+ thresholds); without the new flags the CSV and the
    segments file are byte for byte what they were"""
    import wave
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as TR
    gold, geo, sd, spec, _ = LR.load_fixture(GOLDEN)
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    for i, s in enumerate((0.4, 1.5, 31.0)):
        with wave.open(str(wav_dir / f"f{i}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(synth_wave(70 + i, int(16000 * s)) * 32767.0).astype("<i2").tobytes())
    Cfg._REGISTRY["tiny-whisper-scores"] = geo
    p = lambda n: str(tmp_path / n)
    try:
        common = ["--ssl_type", "tiny-whisper-scores", "--wav_dir", str(wav_dir), "--synthetic_weights", "--seed", "7", "--mode", "f16x"]
        assert TR.run(common + ["--out_csv", p("a.csv")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("a_seg.csv"), "--segments_json", p("a_seg.json")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("q.csv"), "--scores_json", p("q.json")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("q_seg.csv"), "--segments_json", p("q_seg.json"), "--scores_json", p("q_seg_scores.json")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("l.csv"), "--long_form", "--segments_json", p("l_seg.json")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("lq.csv"), "--long_form", "--segments_json", p("lq_seg.json"), "--scores_json", p("lq.json")], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("skip.csv"), "--long_form", "--scores_json", p("skip.json"), "--logprob_threshold", "0.0",
                                "--no_speech_threshold", "-1.0"], spec=spec) == 0
        assert TR.run(common + ["--out_csv", p("b.csv")], spec=spec) == 0
        capsys.readouterr()
        with pytest.raises(SystemExit):
            TR.run(common + ["--out_csv", p("x.csv"), "--logprob_threshold", "-1"], spec=spec)
        assert "--long_form" in capsys.readouterr().err
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-scores")
    read = lambda n: open(p(n), "rb").read()
    assert read("a.csv") == read("b.csv") == read("q.csv") and read("a_seg.csv") == read("q_seg.csv")
    assert read("a_seg.json") == read("q_seg.json") and read("l.csv") == read("lq.csv") and read("l_seg.json") == read("lq_seg.json")
    for name in ("q.json", "q_seg_scores.json"):
        q = json.load(open(p(name)))
        assert sorted(q) == ["f0.wav", "f1.wav", "f2.wav"]
        for e in q.values():
            assert sorted(e) == ["avg_logprob", "compression_ratio", "needs_fallback", "no_speech_prob", "token_logprobs"]
            assert e["avg_logprob"] < 0.0 <= e["no_speech_prob"] <= 1.0 and e["needs_fallback"] is False and len(e["token_logprobs"]) >= 1
            assert abs(e["avg_logprob"] - QR.avg_logprob(e["token_logprobs"])) < 1e-12
    lq = json.load(open(p("lq.json")))
    assert sorted(lq) == ["f0.wav", "f1.wav", "f2.wav"] and len(lq["f2.wav"]["windows"]) >= 2 and len(lq["f0.wav"]["windows"]) == 1
    for e in lq.values():
        for w in e["windows"]:
            assert sorted(w) == ["avg_logprob", "compression_ratio", "needs_fallback", "nf", "no_speech_prob", "seek_s", "skipped"] and w["skipped"] is False
    # logprob_threshold 0 and no_speech_threshold -1: every window is below the one and above the other, so every window of every file is skipped
    skip = json.load(open(p("skip.json")))
    assert all(w["skipped"] and not w["needs_fallback"] for e in skip.values() for w in e["windows"])
    assert [len(e["windows"]) for e in skip.values()] == [1, 1, 2] and skip["f2.wav"]["windows"][1]["seek_s"] == 30.0
    table = TR.read_table(p("skip.csv"))
    assert sorted(table) == ["f0.wav", "f1.wav", "f2.wav"] and all(t == "nan" for t in table.values()), "every file: a row with empty text, no failure"


# ---------------------------------------------------------------------------------------------------------------- HF's fixture
@functools.lru_cache(maxsize=None)
def score_fixture():
    return QR.load_fixture(GOLDEN)


@functools.lru_cache(maxsize=None)
def score_transcriber(mode):
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperDecoder, WhisperEncoder
    gold, geo, sd, spec, waves = score_fixture()
    return TR.WhisperTranscriber(WhisperEncoder(geo, sd, DEV, mode), WhisperDecoder(geo, sd, DEV, mode, spec), spec)


def hf_file(gold, i):
    wins = [tuple(int(x) for x in w) for w in gold[f"f{i}_windows"]]
    skipped, needs = gold[f"f{i}_skipped"].tolist(), gold[f"f{i}_needs_fallback"].tolist()
    times, lens, seq = gold[f"f{i}_seg_times"], gold[f"f{i}_seg_lens"].tolist(), gold[f"f{i}_sequence"].tolist()
    segs, at = [], 0
    for (a, b), n in zip(times, lens):
        segs.append((float(a), float(b), seq[at: at + n]))
        at += n
    return wins, skipped, needs, segs, seq


@pytest.mark.parametrize("mode", ["f16x", "fp32x"])
def test_fixture_equals_hf_alone_and_through_the_queue(mode):
    """tests/golden/tiny_whisper_score_d128h2.npz (tools/make_whisper_scores_golden.py): tokens, seeks, segments, skip decisions and
    needs_fallback equal HF's for every file, alone and through the queue at batch 2 and 16; every token's log-probability within 2 g of
    HF's float64 value and the no-speech probability within expm1(2 g) relatively"""
    gold, geo, sd, spec, waves = score_fixture()
    tr = score_transcriber(mode)
    g = float(gold["g"])
    items = [(f"f{i}.wav", w) for i, w in enumerate(waves)]
    worst_lp, worst_ns = 0.0, 0.0
    for picked, batch in [([it], 16) for it in items] + [(items, 2), (items, 16), (items[::-1], 16)]:
        ids = tr.transcribe_long(iter(picked), batch=batch)
        assert tr.failed == []
        for k, (name, _) in enumerate(picked):
            i = int(name[1:-4])
            wins, skipped, needs, segs, seq = hf_file(gold, i)
            assert [w[:3] for w in tr.windows[k]] == wins and [w[3]["skipped"] for w in tr.windows[k]] == skipped, (mode, batch, name)
            assert [w[3]["needs_fallback"] for w in tr.windows[k]] == needs
            assert tr.sequences[k] == seq and ids[k] == [t for t in seq if t < spec.timestamp_begin] and tr.next_seek[k] == int(gold[f"f{i}_seek"])
            assert [(a, b, list(t)) for a, b, t in tr.segments[k]] == segs and tr.last_languages[k] == int(gold[f"f{i}_language"])
            for w, avg, ns in zip(tr.windows[k], gold[f"f{i}_avg_logprob"], gold[f"f{i}_no_speech_prob"]):
                assert abs(w[3]["avg_logprob"] - avg) <= 2 * g and abs(w[3]["no_speech_prob"] / ns - 1.0) <= math.expm1(2 * g)
                worst_ns = max(worst_ns, abs(w[3]["no_speech_prob"] / ns - 1.0))
    # every token's log-probability, window by window through the engine
    for i, w in enumerate(waves):
        wins = hf_file(gold, i)[0]
        handle = tr.enc.log_mel_long(tr.enc.upload([w], 0), [len(w)])
        at, lang = 0, None
        want = gold[f"f{i}_token_logprobs"]
        for seek, nf, _ in wins:
            hs = tr.enc.forward_windows(handle, [(0, seek, nf)], 0)
            res = tr.dec.generate(hs.states[-1], 1, spec, language=lang, timestamps=True, num_frames=[nf], scores=True)
            lang = int(res.languages[0])
            got = res.token_logprobs[0]
            assert np.abs(got - want[at: at + len(got)]).max() <= 2 * g
            worst_lp = max(worst_lp, float(np.abs(got - want[at: at + len(got)]).max()))
            at += len(got)
        assert at == len(want)
    print(f"SCORES fixture {mode}: g {g:.3e}; worst |token logprob - HF| {worst_lp:.3e} (bound 2 g = {2 * g:.3e}); worst relative distance of "
          f"no_speech_prob {worst_ns:.3e} (bound {math.expm1(2 * g):.3e})")
