"""GPU: Whisper beam search (csrc/beam.hip, include/ser_hip.h "a34").

B. ser_beam_select_v against the rule (tests/whisper_beam_ref.py) on scripted logits, no model: parents, tokens, running order, finished
   handles, flags, done step and error word equal; scores within the float64 bound derived at ``score_bound``.
C. ser_dec_attn_beam_v: the identity table equals ser_dec_attn_v bit for bit; random tables equal the float64 reference over the gathered
   rows; the shared cross cache; and through the engine on the decoder fixture: the logits of every (step, beam) row equal the
   teacher-forced path's bit for bit (a wrong ancestor changes bits), and the rule fed the device's own logits reproduces the device's
   result exactly, in all three modes.
E. Waveforms to ids through WhisperTranscriber and the command line.

Scripted logits are drawn so that every comparison that decides a step has a gap of at least 1e-3 or is an exact tie (checked on the
rule, on the CPU, before anything is launched): the device's scores differ from the rule's by ~1e-15 and decide alike.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import whisper_beam_ref as BR
import whisper_dec_ref as R
from test_gpu_whisper_decoder import (BF16, FP16X, FP32X, GARBAGE, attn_reference, decoder, enc_dev, planes_value, stream, synth_wave,
                                      teacher_forced_device, unit_roundoff)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, P, EOS, PAD = 16, 4, 1, 0                      # positions of the scripted runs, prompt length, eos and pad ids
MIN_GAP = 1e-3


def score_bound(V, *magnitudes):
    """|device - numpy| of one step's score from the same fp32 logits and the same running score, u = 2^-53:
    S = sum_v exp(z_v - M) has V terms in (0, 1], each exp within 1 ulp = 2 u relative, added in some order: S (1 + d), |d| <= (V + 1) u;
    log S moves by |d| absolutely (d log S = dS / S) plus its own ulp, 2 u |log S|; lse = M + log S, logp = z - lse and score = logp + run
    add one rounding each, u times their magnitude.  One side: u ((V + 1) + 2 |log S| + |lse| + |logp| + |score|) <= u (V + 8) m with m
    the largest magnitude involved (>= 1; log S <= ln V is counted in |lse|'s scale).  Two sides: 2^-52 (V + 8) m."""
    return 2.0 ** -52 * (V + 8) * max(1.0, *[float(abs(x)) for x in magnitudes])


class DeviceBeam:
    """The device state of a scripted run of ser_beam_select_v: B utterances of K beams over V tokens, canary rows around ids."""

    def __init__(self, B, K, V, max_length, lp=1.0, banned=None, first_banned=None, pos0=P - 1):
        from interspeech_ser_amd import _lib
        from interspeech_ser_amd.beam import lenpow_table
        self.B, self.K, self.V, self.R, self.max_length = B, K, V, B * K, max_length
        self.ldl = (V + 7) // 8 * 8 + 8
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=DEV)
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)
        mask = np.zeros((3, V), dtype=np.float32)
        if banned is not None:
            mask[0, banned] = mask[1, banned] = -np.inf
        if first_banned is not None:
            mask[1, first_banned] = -np.inf
        self.mask = torch.from_numpy(mask).to(DEV)
        phase = np.zeros(T, dtype=np.int32)
        phase[P - 1] = 1
        self.phase = torch.from_numpy(phase).to(DEV)
        self.lenpow = torch.from_numpy(lenpow_table(T + 1, lp)).to(DEV)
        self.ids = torch.full((self.R + 2, T), -9, dtype=torch.int32, device=DEV)
        self.src = torch.arange(self.R, dtype=torch.int32, device=DEV).view(1, self.R, 1).expand(2, self.R, T).contiguous()
        run = np.full((B, K), -np.inf)
        run[:, 0] = 0.0
        self.run, self.fin_score, self.fin_handle, self.state = torch.from_numpy(run).to(DEV), f64(B, K), i32(B, K, 2), i32(B, 4)
        self.state[:, 1] = 1
        self.trace_run, self.trace_cand = torch.full((T, B, K, 2), -7, dtype=torch.int32, device=DEV), torch.full((T, B, 2 * K, 2), -7, dtype=torch.int32, device=DEV)
        self.cand_score, self.gaps = f64(T, B, 2 * K), torch.full((T, B), np.inf, dtype=torch.float64, device=DEV)
        self.word = torch.tensor([pos0, -9, 0, 0, 0, -9], dtype=torch.int32, device=DEV)          # pos, unfinished, ticket[2], err, canary
        nbytes = int(_lib.lib.ser_beam_work_bytes(B, K, V))
        assert nbytes > 0
        self.work = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
        self.work[-1] = -9
        a = self.args = _lib.BeamSelectArgs()
        a.ldl, a.mask, a.ldm, a.phase, a.lenpow = self.ldl, self.mask.data_ptr(), V, self.phase.data_ptr(), self.lenpow.data_ptr()
        a.ids, a.ld_ids = self.ids.data_ptr() + T * 4, T
        a.src, a.src_parity_stride, a.ld_src = self.src.data_ptr(), self.R * T, T
        a.run, a.fin_score, a.fin_handle, a.state = self.run.data_ptr(), self.fin_score.data_ptr(), self.fin_handle.data_ptr(), self.state.data_ptr()
        a.trace_run, a.trace_cand, a.cand_score, a.gaps = self.trace_run.data_ptr(), self.trace_cand.data_ptr(), self.cand_score.data_ptr(), self.gaps.data_ptr()
        a.work, a.work_bytes = self.work.data_ptr(), nbytes
        w = self.word.data_ptr()
        a.pos, a.unfinished, a.ticket, a.err = w, w + 4, w + 8, w + 16
        a.B, a.K, a.V, a.eos, a.pad, a.max_pos, a.max_length, a.prompt_len = B, K, V, EOS, PAD, T, max_length, P

    def step(self, logits):
        """logits fp32 [B K, V] (host); the padded columns hold the largest value and are never read"""
        from interspeech_ser_amd import _lib
        z = np.full((self.R, self.ldl), 1.0e4, dtype=np.float32)
        z[:, : self.V] = logits
        self.z = torch.from_numpy(z).to(DEV)
        self.args.logits = self.z.data_ptr()
        _lib.check(_lib.lib.ser_beam_select_v(C.byref(self.args), stream()), "ser_beam_select_v")
        torch.cuda.synchronize()
        w = self.word.cpu().numpy()
        assert w[2] == 0 and w[3] == 0 and w[5] == -9 and int(self.work[-1].item()) == -9, "ticket words left zero, canaries intact"
        ids = self.ids.cpu().numpy()
        assert (ids[0] == -9).all() and (ids[-1] == -9).all(), "ids canary rows"
        return dict(pos=int(w[0]), unfinished=int(w[1]), err=int(w[4]) & 0xffffffff, ids=ids[1:-1], state=self.state.cpu().numpy(),
                    run=self.run.cpu().numpy(), fin_score=self.fin_score.cpu().numpy(), fin_handle=self.fin_handle.cpu().numpy(),
                    trace_run=self.trace_run.cpu().numpy(), trace_cand=self.trace_cand.cpu().numpy(), cand_score=self.cand_score.cpu().numpy(),
                    gaps=self.gaps.cpu().numpy(), src=self.src.cpu().numpy())


def rule_run(script, B, K, V, max_length, lp, banned=None, first_banned=None):
    """The rule over a script [steps][B K, V]: one Beam per utterance, and the smallest deciding gap that is not an exact tie."""
    ban = np.zeros(V, dtype=bool)
    if banned is not None:
        ban[banned] = True
    ban1 = ban.copy()
    if first_banned is not None:
        ban1[first_banned] = True
    beams = [BR.Beam(K, V, EOS, PAD, P, max_length, lp) for _ in range(B)]
    worst = np.inf
    for s, z in enumerate(script):
        for b, bm in enumerate(beams):
            bm.step(z[b * K: (b + 1) * K], P + s, ban1 if s == 0 else ban)
            st = bm.steps[-1]
            if st is not None and st["gap"] > 0:
                worst = min(worst, st["gap"])
    return beams, worst


def check_against_rule(script, B, K, V, max_length, lp=1.0, banned=None, first_banned=None):
    """Run the script through the device and the rule, compare after every step.  Returns (beams, last device state, DeviceBeam)."""
    beams, worst = rule_run(script, B, K, V, max_length, lp, banned, first_banned)
    assert worst >= MIN_GAP, f"the script decides a step by {worst:.3e}: draw again"
    dev = DeviceBeam(B, K, V, max_length, lp, banned, first_banned)
    table = np.tile(np.arange(B * K, dtype=np.int32)[None, :, None], (2, 1, T))          # the ancestor table, simulated on the host
    run_prev = dev.run.cpu().numpy().copy()
    lenpow = dev.lenpow.cpu().numpy()
    worst_ratio = 0.0
    for s, z in enumerate(script):
        p = P - 1 + s
        d = dev.step(z)
        assert d["pos"] == p + 1
        written = np.zeros_like(d["ids"], dtype=bool)
        written[:, P: p + 2] = True
        assert (d["ids"][~written] == -9).all(), "ids changed outside the generated columns"
        lp64 = BR.log_softmax64(z)
        for b, bm in enumerate(beams):
            st = bm.steps[s] if s < len(bm.steps) else None
            failed = bm.err != 0
            if failed:
                continue                                                      # after an error bit only the error word is specified
            rows = slice(b * K, (b + 1) * K)
            if st is None:                                                    # frozen: identity parents, pad, state as it was
                assert (d["trace_run"][p, b, :, 0] == -1).all() and (d["ids"][rows, p + 1] == PAD).all()
                parents = np.arange(K)
            else:
                assert d["trace_cand"][p, b].tolist() == [list(c) for c in st["cand"]], (s, b, "candidates")
                assert d["trace_run"][p, b].tolist() == [list(c) for c in st["run"]], (s, b, "running rows")
                assert d["ids"][rows, p + 1].tolist() == [t for _, t in st["run"]]
                parents = np.array([q for q, _ in st["run"]])
                for j, (q, t) in enumerate(st["cand"]):                       # each score from the device's own previous running score
                    want = lp64[b * K + q, t] + run_prev[b, q]
                    bound = score_bound(V, want, lp64[b * K + q, t], run_prev[b, q], float(z[b * K + q, t]) - lp64[b * K + q, t])
                    err = abs(d["cand_score"][p, b, j] - want)
                    worst_ratio = max(worst_ratio, err / bound)
                    assert err <= bound, (s, b, j, err, bound)
                    assert abs(d["cand_score"][p, b, j] - st["cand_scores"][j]) <= 1e-9
                alive = np.isfinite(st["run_scores"])
                assert np.array_equal(np.isfinite(d["run"][b]), alive)
                assert np.abs(d["run"][b][alive] - st["run_scores"][alive]).max(initial=0.0) <= 1e-9
                if np.isfinite(st["gap"]):
                    assert abs(d["gaps"][p, b] - st["gap"]) <= 1e-9 * max(1.0, st["gap"])
                else:
                    assert np.isinf(d["gaps"][p, b])
            cur = table[p & 1]
            nxt = table[(p + 1) & 1]
            for r in range(K):
                nxt[b * K + r, :p] = cur[b * K + parents[r], :p]
                nxt[b * K + r, p] = b * K + parents[r]
            assert np.array_equal(d["src"][(p + 1) & 1, rows, : p + 1], nxt[rows, : p + 1]), (s, b, "ancestor table")
            n_steps = min(s + 1, len(bm.steps))
            fin_now = [f for f in _finished_after(bm, n_steps)]
            assert int(d["state"][b, 0]) == len(fin_now)
            assert [tuple(h) for h in d["fin_handle"][b, : len(fin_now)].tolist()] == [(P - 1 + h[0], h[1]) for _, h in fin_now], (s, b, "finished handles")
            for k, (sc, (hs, hr)) in enumerate(fin_now):
                assert abs(d["fin_score"][b, k] - sc) <= 1e-9
                assert d["fin_score"][b, k] == d["cand_score"][P - 1 + hs, b, hr] / lenpow[hs + 1], "one IEEE division of the device's own score"
        run_prev = d["run"].copy()
    for b, bm in enumerate(beams):
        if bm.err:
            continue
        assert bool(d["state"][b, 1]) == bm.flag and bool(d["state"][b, 2]) == bm.done, (b, "flags")
        if bm.done:
            assert int(d["state"][b, 3]) == P - 1 + bm.done_step, (b, "done step")
    want_err = 0
    for bm in beams:
        want_err |= bm.err
    assert d["err"] == want_err, (d["err"], want_err)
    assert d["unfinished"] == sum(not bm.done for bm in beams)
    print(f"BEAMSEL B {B} K {K} V {V}: worst score err / bound {worst_ratio:.3f}, smallest deciding gap {worst:.3e}")
    return beams, d, dev


def _finished_after(bm, n_steps):
    """the finished set of a rule run as it stood after its first ``n_steps`` steps: replayed from the recorded steps"""
    fin = []
    flag = True
    for s in range(n_steps):
        st = bm.steps[s]
        if st is None:
            continue
        K = bm.K
        den = bm.lenpow(st["cur"] + 1 - bm.P)
        at_max = st["cur"] + 1 >= bm.max_length
        if flag:
            for j in range(K):
                if st["cand"][j][1] == bm.eos or at_max:
                    sc = st["cand_scores"][j] / den
                    at = len(fin)
                    while at > 0 and sc > fin[at - 1][0]:
                        at -= 1
                    fin.insert(at, (sc, (s, j)))
                    del fin[K:]
        if len(fin) == K and not st["run_scores"][0] / den > fin[-1][0]:
            flag = False
    return fin


def draw_script(seed, steps, B, K, V, max_length, lp=1.0, eos_boost=2.0, banned=None, first_banned=None, edit=None):
    """A random script whose deciding gaps are all >= MIN_GAP (or exact ties): redrawn, on the CPU, until the rule says so."""
    for k in range(200):
        rng = np.random.default_rng(seed + 1000 * k)
        script = [(3.0 * rng.standard_normal((B * K, V))).astype(np.float32) for _ in range(steps)]
        for z in script:
            z[:, EOS] += np.float32(eos_boost)
        if edit is not None:
            edit(script)
        beams, worst = rule_run(script, B, K, V, max_length, lp, banned, first_banned)
        if worst >= MIN_GAP:
            return script
    raise AssertionError("no script with gaps above MIN_GAP")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", ["2K", 63, 64, 65, 522])
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_beam_select_equals_the_rule(K, V, B):
    """random scripts to max_length: step 0 with only beam 0 alive, eos hits, every candidate hitting at max_length"""
    V = 2 * K if V == "2K" else V
    max_length = P + 6
    lp = (0.0, 1.0, 2.0)[(K + B) % 3]
    script = draw_script(7 * K + V + B, max_length - P, B, K, V, max_length, lp, eos_boost=1.0 if V > 2 * K else 0.0)
    for z in script[:1]:
        z[1::K] += np.float32(50.0)                                           # dead beams with the largest logits decide nothing at step 0
    beams, d, dev = check_against_rule(script, B, K, V, max_length, lp)
    for b, bm in enumerate(beams):
        assert all(q == 0 for q, _ in bm.steps[0]["cand"]) and bm.done and len(bm.finished) >= 1
        assert (d["trace_cand"][P - 1, b, :, 0] == 0).all()


def test_beam_select_large_vocabulary():
    """V = 51 866 (13 chunks of 4 096 columns), K = 5, B = 2"""
    K, V, B, max_length = 5, 51866, 2, P + 3
    script = draw_script(99, 3, B, K, V, max_length, 1.0, eos_boost=6.0)
    script[1][0, 51865] = np.float32(40.0)                                    # winners in the first and in the last chunk
    script[1][1, 0] = np.float32(39.0)
    beams, worst = rule_run(script, B, K, V, max_length, 1.0)
    assert worst >= MIN_GAP
    beams, d, dev = check_against_rule(script, B, K, V, max_length, 1.0)
    assert any(t == 51865 for _, t in beams[0].steps[1]["cand"])


def test_beam_select_entry_boundary_and_many_eos():
    """eos at rank K - 1 enters the finished set, eos at rank K does not; K eos candidates in one step; two survivors of one parent"""
    K, V, B, max_length = 3, 64, 2, P + 5

    def edit(script):
        z = script[1]
        z[:] = np.float32(-4.0)                                               # beams 1, 2: flat rows, log-probability -log 64 everywhere
        # utterance 0: beam 0 carries all six candidates (log-probability ~ -1.8 each): tokens 10, 11 (ranks 0, 1), eos (rank 2 = K - 1), ..
        z[0, [10, 11, EOS, 12, 13, 14]] = np.array([9.0, 8.9, 8.8, 8.7, 8.6, 8.5], dtype=np.float32)
        # utterance 1: eos at rank 3 = K
        z[3, [10, 11, 12, EOS, 13, 14]] = np.array([9.0, 8.9, 8.8, 8.7, 8.6, 8.5], dtype=np.float32)
        script[2][:, EOS] = np.float32(30.0)                                  # every beam's best token is eos: K eos candidates at once
    script = draw_script(5, max_length - P, B, K, V, max_length, 1.0, eos_boost=-20.0, edit=edit)
    beams, d, dev = check_against_rule(script, B, K, V, max_length, 1.0)
    s1 = [bm.steps[1] for bm in beams]
    assert s1[0]["cand"][K - 1][1] == EOS and s1[1]["cand"][K][1] == EOS
    assert [h for _, h in _finished_after(beams[0], 2)] == [(1, K - 1)] and _finished_after(beams[1], 2) == []
    assert len({q for q, _ in s1[0]["run"]}) == 1                             # the survivors share one parent
    assert sum(t == EOS for _, t in beams[0].steps[2]["cand"][:K]) == K and len(_finished_after(beams[0], 3)) == K


def test_beam_select_heuristic_freezes_one_utterance():
    """utterance 0 finishes K strong hypotheses, its flag drops and it is frozen while its batch mate runs on: nothing enters afterwards"""
    K, V, B, max_length = 2, 65, 2, P + 8

    def edit(script):
        for z in script[:2]:
            z[0:K, EOS] = np.float32(25.0)                                    # utterance 0: eos with probability ~1 twice
        for z in script[2:]:
            z[0:K, EOS] = np.float32(25.0)                                    # and it would go on finishing, were it not frozen
    script = draw_script(11, max_length - P, B, K, V, max_length, 1.0, eos_boost=-20.0, edit=edit)
    beams, d, dev = check_against_rule(script, B, K, V, max_length, 1.0)
    assert beams[0].done and not beams[0].flag and beams[0].done_step <= 2 and beams[1].done_step == max_length - P - 1
    assert all(h[0] <= beams[0].done_step for _, h in beams[0].finished)
    assert (d["trace_run"][P - 1 + beams[0].done_step + 1:, 0, :, 0][: 3] == -1).all()


def test_beam_select_three_way_tie_across_beams():
    """three candidates of different beams with the same float64 score: the lower flat index wins"""
    K, V, B, max_length = 3, 63, 1, P + 3
    script = draw_script(21, 3, B, K, V, max_length, 1.0, eos_boost=-20.0)
    z0 = script[0]
    z0[:] = np.float32(0.0)
    z0[0, [20, 30, 40]] = np.float32(8.0)                                     # three tokens tie at step 0: running scores equal bit for bit
    z0[0, [50, 51, 52]] = np.array([3.0, 2.0, 1.0], dtype=np.float32)
    script[1][:] = script[1][0]                                               # identical rows: every token ties three ways across the beams
    beams, worst = rule_run(script, B, K, V, max_length, 1.0)
    assert worst >= MIN_GAP
    beams, d, dev = check_against_rule(script, B, K, V, max_length, 1.0)
    st = beams[0].steps[1]
    assert st["cand_scores"][0] == st["cand_scores"][1] == st["cand_scores"][2] and [q for q, _ in st["cand"][:3]] == [0, 1, 2]
    assert len({t for _, t in st["cand"][:3]}) == 1


def test_beam_select_suppressed_winner_counts_in_the_normaliser():
    K, V, B, max_length = 2, 64, 1, P + 3
    banned, first = [7, 9], [11]

    def edit(script):
        for z in script:
            z[:, 7] = np.float32(15.0)                                        # the suppressed token would win everywhere
        script[0][:, 11] = np.float32(11.0)                                   # and the begin-suppressed one at the first position
    script = draw_script(31, 3, B, K, V, max_length, 1.0, banned=banned, first_banned=first, edit=edit)
    beams, d, dev = check_against_rule(script, B, K, V, max_length, 1.0, banned=banned, first_banned=first)
    toks = {t for st in beams[0].steps for _, t in st["cand"]}
    assert 7 not in toks and 9 not in toks and 11 not in {t for _, t in beams[0].steps[0]["cand"]}
    assert beams[0].steps[0]["cand_scores"][0] < -3.0                         # the winner's log-probability carries the suppressed mass


def test_beam_select_errors():
    """fewer than 2K finite candidates: the new error bit, nothing out of range; a NaN logit: bit 0; the position at the end: bit 2"""
    K, V, B, max_length = 3, 64, 2, P + 3
    script = draw_script(41, 1, B, K, V, max_length)
    first = [t for t in range(V) if t >= 2 * K - 1]                           # 2K - 1 tokens stay at the first position
    dev = DeviceBeam(B, K, V, max_length, first_banned=first)
    d = dev.step(script[0])
    assert d["err"] == BR.ERR_CANDIDATES and d["pos"] == P
    assert (d["ids"][:, P] >= 0).all() and (d["ids"][:, P] < V).all()
    assert ((d["trace_run"][P - 1, :, :, 0] >= 0) & (d["trace_run"][P - 1, :, :, 0] < K)).all()
    assert ((d["src"] >= 0) & (d["src"] < B * K)).all()
    bm, _ = rule_run(script, B, K, V, max_length, 1.0, first_banned=first)
    assert bm[0].err == BR.ERR_CANDIDATES
    bad = script[0].copy()
    bad[K, 17] = np.nan                                                       # utterance 1, beam 0
    dev = DeviceBeam(B, K, V, max_length)
    d = dev.step(bad)
    assert d["err"] == BR.ERR_NONFINITE
    assert rule_run([bad], B, K, V, max_length, 1.0)[0][1].err & BR.ERR_NONFINITE
    dead = script[0].copy()
    dead[1, 17] = np.nan                                                      # a dead beam's logits decide nothing
    dev = DeviceBeam(B, K, V, max_length)
    assert dev.step(dead)["err"] == 0
    end = DeviceBeam(B, K, V, T, pos0=T - 1)
    d = end.step(script[0])
    assert d["err"] == BR.ERR_POSITION and d["pos"] == T - 1 and (d["ids"] == -9).all() and (d["trace_run"] == -7).all()


def test_beam_select_alone_equals_batched_bit_for_bit():
    K, V, max_length = 5, 522, P + 5
    script = draw_script(51, max_length - P, 3, K, V, max_length, 2.0)
    batch = DeviceBeam(3, K, V, max_length, 2.0)
    for z in script:
        d3 = batch.step(z)
    for b in range(3):
        alone = DeviceBeam(1, K, V, max_length, 2.0)
        for z in script:
            d1 = alone.step(z[b * K: (b + 1) * K])
        for name in ("run", "fin_score", "fin_handle", "state"):
            assert np.array_equal(d1[name][0].view(np.uint8), d3[name][b].view(np.uint8)), (b, name)
        for name in ("trace_run", "trace_cand", "cand_score", "gaps"):
            assert np.array_equal(np.ascontiguousarray(d1[name][:, 0]).view(np.uint8), np.ascontiguousarray(d3[name][:, b]).view(np.uint8)), (b, name)
        assert np.array_equal(d1["ids"], d3["ids"][b * K: (b + 1) * K])


def test_beam_select_refuses_bad_arguments():
    from interspeech_ser_amd import _lib
    dev = DeviceBeam(1, 2, 64, P + 3)
    dev.args.logits = dev.mask.data_ptr()
    for field, value, text in (("K", 9, b"K=9"), ("K", 1, b"K=1"), ("V", 3, b"V=3"), ("max_length", T + 1, b"max_length"), ("work_bytes", 8, b"work_bytes")):
        keep = getattr(dev.args, field)
        setattr(dev.args, field, value)
        assert _lib.lib.ser_beam_select_v(C.byref(dev.args), None) < 0 and text in _lib.lib.ser_last_error(), field
        setattr(dev.args, field, keep)
    assert _lib.lib.ser_beam_work_bytes(1, 2, 60000) == -1 and _lib.lib.ser_beam_work_bytes(1, 9, 64) == -1


# ---------------------------------------------------------------------------------------------------------------- ser_dec_attn_beam_v
MAXL = 64


def launch_attn_beam(q, kc, vc, length, H, mode, *, src=None, row_div=1, new=None, beam=True):
    """One launch over caches [rows, MAXL, D] (device tensors, written by an append).  Returns the output words (host) [P, B, D]."""
    from interspeech_ser_amd import _lib
    B, D = q.shape
    planes = 1 if mode == BF16 else 2
    out = torch.full((planes, B + 2, D), GARBAGE, dtype=torch.int16, device=DEV)
    qd = torch.from_numpy(q).to(DEV)
    ld = torch.tensor([length - 1], dtype=torch.int32, device=DEV)
    x = _lib.DecAttnBeamArgs()
    a = x.base if beam else _lib.DecAttnArgs()
    a.q, a.ldq = qd.data_ptr(), D
    keep = [qd, ld]
    if new is not None:
        kn, vn = torch.from_numpy(new[0]).to(DEV), torch.from_numpy(new[1]).to(DEV)
        keep += [kn, vn]
        a.k_new, a.v_new, a.ld_new = kn.data_ptr(), vn.data_ptr(), D
    a.kcache, a.vcache, a.ldc, a.batch_stride = kc.data_ptr(), vc.data_ptr(), D, MAXL * D
    a.lens, a.lens_stride, a.len_add = ld.data_ptr(), 0, 1
    a.out_act, a.ldo_act, a.out_plane_stride = out.data_ptr() + D * 2, D, (B + 2) * D
    a.scale, a.B, a.H, a.dh, a.max_len, a.mode = 0.125, B, H, 64, MAXL, mode
    if beam:
        if src is not None:
            keep.append(src)
            x.src, x.src_parity_stride, x.ld_src = src.data_ptr(), src.stride(0), src.shape[2]
        x.row_div = row_div
        _lib.check(_lib.lib.ser_dec_attn_beam_v(C.byref(x), stream()), "ser_dec_attn_beam_v")
    else:
        _lib.check(_lib.lib.ser_dec_attn_v(C.byref(a), stream()), "ser_dec_attn_v")
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool((o[:, 0] == GARBAGE).all()) and bool((o[:, B + 1] == GARBAGE).all())
    return o[:, 1: B + 1]


@functools.lru_cache(maxsize=None)
def beam_attn_case(H, rows):
    D = 64 * H
    rng = np.random.default_rng(7 * H + rows)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(rows, D), f(rows, MAXL, D), (1.5 * f(rows, MAXL, D) + np.float32(0.25)), f(rows, D), f(rows, D)


@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("rows", [1, 6])
@pytest.mark.parametrize("H", [2, 20])
def test_attn_beam_identity_table_equals_dec_attn_bit_for_bit(H, rows, mode, append):
    q, k, v, kn, vn = beam_attn_case(H, rows)
    ident = torch.arange(rows, dtype=torch.int32, device=DEV).view(1, rows, 1).expand(2, rows, MAXL).contiguous()
    for length in (1, 16, 17, 63, 64):
        new = (kn, vn) if append else None
        caches = [[torch.from_numpy(t).to(DEV) for t in (k, v)] for _ in range(2)]
        want = launch_attn_beam(q, *caches[0], length, H, mode, new=new, beam=False)
        got = launch_attn_beam(q, *caches[1], length, H, mode, src=ident, new=new)
        assert torch.equal(want, got), (length, "the identity table changes bits")
        assert torch.equal(caches[0][0], caches[1][0]) and torch.equal(caches[0][1], caches[1][1]), (length, "the append differs")


@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
def test_attn_beam_random_tables_equal_float64(mode):
    """scripted reorder steps on the host build the table a beam run would; the output equals the float64 reference over the gathered rows
    within test_gpu_whisper_decoder's bound; the appended row lands in the row's own physical cache"""
    H, rows = 2, 6
    D = 64 * H
    q, k, v, kn, vn = beam_attn_case(H, rows)
    u, eta = unit_roundoff(mode)
    rng = np.random.default_rng(3)
    table = np.tile(np.arange(rows, dtype=np.int32)[None, :, None], (2, 1, MAXL))
    for p in range(1, 40):                                                    # the select's update, K = 3 beams of 2 utterances
        cur, nxt = table[p & 1], table[(p + 1) & 1]
        for b in range(2):
            par = rng.integers(0, 3, 3) + 3 * b
            for r in range(3):
                nxt[3 * b + r, :p] = cur[par[r], :p]
                nxt[3 * b + r, p] = par[r]
    for length in (17, 40):
        src = torch.from_numpy(table).to(DEV)
        kc, vc = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
        out = launch_attn_beam(q, kc, vc, length, H, mode, src=src, new=(kn, vn))
        val = planes_value(out.contiguous(), mode)
        t = table[(length - 1) & 1]
        for r in range(rows):
            kk = np.stack([k[t[r, j], j] for j in range(length - 1)] + [kn[r]])
            vv = np.stack([v[t[r, j], j] for j in range(length - 1)] + [vn[r]])
            ref, ref32, floor = attn_reference(q[r], kk, vv, 0.125, H)
            tol = 2 * np.abs(ref32.astype(np.float64) - ref).max() + floor + u * np.abs(ref) + eta
            assert (np.abs(val[r] - ref) <= tol).all(), (length, r)
        kh, vh = kc.cpu().numpy(), vc.cpu().numpy()
        want_k, want_v = k.copy(), v.copy()
        want_k[np.arange(rows), length - 1], want_v[np.arange(rows), length - 1] = kn, vn
        assert np.array_equal(kh, want_k) and np.array_equal(vh, want_v)


@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
def test_attn_beam_shared_cross_cache(mode):
    """3 rows per cache: row r reads cache r / 3, bit for bit what ser_dec_attn_v gives over a cache copied three times"""
    H, caches = 2, 2
    q, _, _, _, _ = beam_attn_case(H, 6)
    _, k, v, _, _ = beam_attn_case(H, caches)
    kc, vc = torch.from_numpy(k).to(DEV), torch.from_numpy(v).to(DEV)
    k3, v3 = torch.from_numpy(np.repeat(k, 3, 0)).to(DEV), torch.from_numpy(np.repeat(v, 3, 0)).to(DEV)
    for length in (1, 33, 64):
        got = launch_attn_beam(q, kc, vc, length, H, mode, row_div=3)
        want = launch_attn_beam(q, k3, v3, length, H, mode, beam=False)
        assert torch.equal(got, want), length


def test_attn_beam_refuses_bad_arguments():
    from interspeech_ser_amd import _lib
    x = _lib.DecAttnBeamArgs()
    a = x.base
    a.q = a.kcache = a.vcache = a.out_act = 256
    a.ldq = a.ldc = a.ldo_act = 128
    a.B, a.H, a.dh, a.max_len, a.mode, a.len_add = 1, 2, 64, 8, FP16X, 1
    assert _lib.lib.ser_dec_attn_beam_v(C.byref(x), None) < 0 and b"row_div=0" in _lib.lib.ser_last_error()
    x.src, x.ld_src = 256, 4
    assert _lib.lib.ser_dec_attn_beam_v(C.byref(x), None) < 0 and b"ld_src=4" in _lib.lib.ser_last_error()


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir)


def rule_on_device_logits(res, spec, V, K, lp, n_max):
    """The rule fed the device's own kept logits: one Beam per utterance."""
    first = res.beam_trace["first"]
    logits = res.beam_logits.cpu().numpy()
    ban = np.zeros(V, dtype=bool)
    ban[list(spec.suppress_tokens)] = True
    ban1 = ban.copy()
    ban1[list(spec.begin_suppress_tokens)] = True
    B = logits.shape[1] // K
    beams = [BR.Beam(K, V, spec.eos_token_id, spec.pad_token_id, spec.PROMPT_LEN, n_max, lp) for _ in range(B)]
    for s in range(logits.shape[0]):
        for b, bm in enumerate(beams):
            bm.step(logits[s, b * K: (b + 1) * K], first + 1 + s, ban1 if s == 0 else ban)
    return beams


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_engine_beam_run_is_the_rule_on_its_own_logits(fx, mode):
    """sequences, trace, finished sets and nbest of the device equal the rule fed the device's own logits; a second generate on the same
    plan gives the same bits; every (step, beam) row's logits equal the teacher-forced path's bit for bit"""
    from interspeech_ser_amd import beam as BM
    gold, geo, sd, spec, enc = fx
    dec = decoder(mode)
    V, K, lp = geo.decoder_vocab_size, 3, 1.0
    res = dec.generate(enc_dev(enc, slice(None)), 3, num_beams=K, length_penalty=lp, keep_logits=True)
    assert not res.failed and res.err == 0
    first = res.beam_trace["first"]
    beams = rule_on_device_logits(res, spec, V, K, lp, min(spec.max_length, geo.max_target_positions))
    tr = res.beam_trace
    for b, bm in enumerate(beams):
        assert bm.err == 0 and bm.done
        for s, st in enumerate(bm.steps):
            if st is None:
                assert (tr["run"][first + s, b, :, 0] == -1).all()
                continue
            assert tr["cand"][first + s, b].tolist() == [list(c) for c in st["cand"]], (b, s)
            assert tr["run"][first + s, b].tolist() == [list(c) for c in st["run"]], (b, s)
        assert int(tr["n_fin"][b]) == len(bm.finished) and int(tr["done_step"][b]) == first + bm.done_step
        assert [tuple(h) for h in tr["fin_handles"][b, : len(bm.finished)].tolist()] == [(first + h[0], h[1]) for _, h in bm.finished]
        want = bm.nbest()
        assert [ids for ids, _ in res.nbest[b]] == [ids for ids, _ in want]
        assert np.abs(np.array([s for _, s in res.nbest[b]]) - np.array([s for _, s in want])).max() <= 1e-9
        assert all(res.nbest[b][i][1] >= res.nbest[b][i + 1][1] for i in range(len(want) - 1))
        best = want[0][0]
        assert res.sequences[b, spec.PROMPT_LEN: spec.PROMPT_LEN + len(best)].tolist() == best
        assert (res.sequences[b, spec.PROMPT_LEN + len(best):] == spec.pad_token_id).all()
        assert res.lists[b] == (best[: best.index(spec.eos_token_id)] if spec.eos_token_id in best else best)
        assert res.beam_scores[b] == res.nbest[b][0][1]
    again = dec.generate(enc_dev(enc, slice(None)), 3, num_beams=K, length_penalty=lp, keep_logits=True)
    assert np.array_equal(again.sequences, res.sequences) and torch.equal(again.beam_logits, res.beam_logits)
    for name in ("run", "cand", "cand_scores", "fin_scores", "fin_handles"):
        assert np.array_equal(again.beam_trace[name].view(np.uint8), tr[name].view(np.uint8)), name
    # the ancestor table: the logits of running row r at step s are those of its own history, teacher-forced alone
    logits = res.beam_logits.cpu().numpy()
    prompt = res.sequences[:, : spec.PROMPT_LEN]
    checked = 0
    for b, bm in enumerate(beams):
        n = len([st for st in bm.steps if st is not None])
        hist = {}
        for s in range(1, n):
            for r in range(K):
                if np.isfinite(bm.steps[s - 1]["run_scores"][r]):
                    hist[tuple(BM.running_history(tr["run"], b, first + s - 1, r, first))] = None
        maximal = [h for h in hist if not any(o != h and o[: len(h)] == h for o in hist)]
        forced = {h: teacher_forced_device(dec, enc[b], list(prompt[b]) + list(h), spec) for h in maximal}
        for s in range(n):
            for r in range(K):
                if s > 0 and not np.isfinite(bm.steps[s - 1]["run_scores"][r]):
                    continue
                h = tuple(BM.running_history(tr["run"], b, first + s - 1, r, first)) if s > 0 else ()
                full = next(m for m in maximal if m[: len(h)] == h)
                want = forced[full][spec.PROMPT_LEN - 1 + len(h)].astype(np.float32)
                assert np.array_equal(logits[s, b * K + r].view(np.uint32), want.view(np.uint32)), (b, s, r, "a wrong ancestor changes bits")
                checked += 1
    assert checked >= 3 * K
    print(f"BEAMENGINE {mode}: {checked} (step, beam) rows equal the teacher-forced logits; best {[nb[0] for nb in res.nbest]}")


def test_greedy_after_a_beam_run_equals_the_fixture(fx):
    gold, geo, sd, spec, enc = fx
    dec = decoder("f16x")
    beam = dec.generate(enc_dev(enc, slice(None)), 3, num_beams=2)
    assert not beam.failed and beam.nbest is not None
    res = dec.generate(enc_dev(enc, slice(None)), 3)
    assert np.array_equal(res.sequences, gold["a_sequences"]) and res.nbest is None
    one = dec.generate(enc_dev(enc, slice(0, 1)), 1, num_beams=2)
    n = min(one.sequences.shape[1], beam.sequences.shape[1])
    assert np.array_equal(one.sequences[0, :n], beam.sequences[0, :n]) and one.nbest[0] == beam.nbest[0]      # alone == batched
    with pytest.raises(ValueError, match="not built"):
        dec.generate(enc_dev(enc, slice(None)), 3, num_beams=2, token_times=True, lengths=[16000] * 3)
    with pytest.raises(ValueError, match="num_beams"):
        dec.generate(enc_dev(enc, slice(None)), 3, num_beams=9)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_transcriber_and_command_line_with_beams(fx, tmp_path, capsys):
    """two ragged waveforms: the batch equals the per-file runs; the command line writes the table; --num_beams 1 and no flag write the
    same bytes; a file that trips the guard fails as today"""
    import wave
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    gold, geo, sd, spec, _ = fx
    enc = WhisperEncoder(geo, synthetic_state_dict(Cfg.TINY_WHISPER, int(gold["b_encoder_weight_seed"])), DEV, "f16x")
    waves = [synth_wave(int(s), int(n)) for s, n in zip(gold["b_wave_seeds"], gold["b_lengths"])]
    tr = TR.WhisperTranscriber(enc, decoder("f16x"), spec)
    both = tr.transcribe(waves, num_beams=3)
    scores = list(tr.last_scores)
    assert all(ids is not None for ids in both) and all(s is not None for s in scores)
    for i, w in enumerate(waves):
        assert tr.transcribe([w], num_beams=3) == [both[i]] and tr.last_scores == [scores[i]]
    assert tr.transcribe(waves) == tr.transcribe(waves, num_beams=1)
    bad = waves[0][:15000]                                                    # this file's encoder states get a NaN: its logits are NaN in every beam
    forward = enc.forward

    def poisoned(wav, lengths, **kw):
        hs = forward(wav, lengths, **kw)
        for i, n in enumerate(lengths):
            if n == len(bad):
                hs.states[-1].view(len(lengths), -1, geo.hidden)[i, 7, 3] = float("nan")
        return hs
    enc.forward = poisoned
    try:
        assert tr.transcribe([bad, waves[1]], ["bad.wav", "good.wav"], num_beams=3) == [None, both[1]] and tr.failed == ["bad.wav"]
    finally:
        enc.forward = forward
    assert "Failed to process bad.wav: decoder error word" in capsys.readouterr().out    # error word or guard bits, as for a greedy batch
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    for i, s in enumerate((0.4, 1.5, 0.9)):
        with wave.open(str(wav_dir / f"f{i}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(synth_wave(60 + i, int(16000 * s)) * 32767.0).astype("<i2").tobytes())
    Cfg._REGISTRY["tiny-whisper-dec-beams"] = geo
    try:
        common = ["--ssl_type", "tiny-whisper-dec-beams", "--wav_dir", str(wav_dir), "--synthetic_weights", "--seed", "7", "--mode", "f16x"]
        out = {}
        for tag, extra in (("none", []), ("one", ["--num_beams", "1"]), ("three", ["--num_beams", "3", "--length_penalty", "0.5"])):
            path = tmp_path / f"{tag}.csv"
            assert TR.run(common + ["--out_csv", str(path)] + extra, spec=spec) == 0
            out[tag] = open(path, "rb").read()
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-dec-beams")
    assert out["none"] == out["one"]
    table = TR.read_table(str(tmp_path / "three.csv"))
    assert sorted(table) == ["f0.wav", "f1.wav", "f2.wav"] and all(all(w.isdigit() for w in t.split()) for t in table.values())


# ---------------------------------------------------------------------------------------------------------------- against HF directly
# E = worst |device - HF| over the fixture's (step, beam) logit rows through the teacher-forced path, measured on the first run on the
# MI355X (profiles/whisper_beams.txt, 2026-10-20); the fixture's r is recorded in the file itself
E_MEASURED = {"f16x": 1.907e-06, "fp32x": 3.201e-05, "bf16": 1.567e-02}       # r = 2.241e-03, g = 4.057e-03: 4 E / r = 0.003, 0.057, 28


@functools.lru_cache(maxsize=None)
def beam_fixture():
    """(gold, geometry, state dict, spec, encoder states [3, S, D]) of tests/golden/tiny_whisper_beam_d128h2.npz: weights and encoder states
    regenerated from the recorded seeds and checked against the recorded digest"""
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd.weights import state_dict_digest, synthetic_decoder_state_dict
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_whisper_beam_d128h2.npz"))
    geo = Cfg.TINY_WHISPER_DEC
    sd = synthetic_decoder_state_dict(geo, int(gold["decoder_seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    spec = Cfg.GenerationSpec(
        decoder_start_token_id=int(gold["start"]), eos_token_id=int(gold["eos"]), pad_token_id=int(gold["pad"]),
        suppress_tokens=tuple(int(t) for t in gold["suppress"]), begin_suppress_tokens=tuple(int(t) for t in gold["begin_suppress"]),
        no_timestamps_token_id=int(gold["no_timestamps"]), lang_ids=tuple(int(t) for t in gold["lang_ids"]), task_id=int(gold["task"]),
        max_length=int(gold["max_length"]))
    enc = np.concatenate([R.enc_states(int(e), 1, geo.max_source_positions, geo.hidden) for e in gold["enc_seeds"]])
    return gold, geo, sd, spec, enc


def hf_running_history(gold, b, step, row):
    """the generated tokens HF's running row ``row`` of utterance ``b`` holds after step ``step``"""
    out = []
    for s in range(step, -1, -1):
        out.append(int(gold["run_tokens"][s, b, row]))
        row = int(gold["run_parents"][s, b, row])
    return out[::-1]


@functools.lru_cache(maxsize=None)
def measured_E(mode):
    """(E, g): worst |device - HF| over every live (step, beam) row up to each utterance's own stop, and the project's gate over them"""
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = beam_fixture()
    dec = WhisperDecoder(geo, sd, DEV, mode, spec)
    K, logits = int(gold["K"]), gold["logits"].astype(np.float64)
    prompt = [[int(gold["start"]), int(l), int(gold["task"]), int(gold["no_timestamps"])] for l in gold["languages"]]
    worst, top = 0.0, 0.0
    for b in range(3):
        n = int(gold["done_steps"][b]) + 1
        hist = {(): [(0, r) for r in range(K)]}                               # history -> the (step, row) pairs whose logits it feeds
        for s in range(1, n):
            for r in range(K):
                if gold["run_scores"][s - 1, b, r] > -1e8:
                    hist.setdefault(tuple(hf_running_history(gold, b, s - 1, r)), []).append((s, r))
        maximal = [h for h in hist if not any(o != h and o[: len(h)] == h for o in hist)]
        forced = {h: teacher_forced_device(dec, enc[b], prompt[b] + list(h), spec) for h in maximal}
        for h, where in hist.items():
            full = next(m for m in maximal if m[: len(h)] == h)
            got = forced[full][spec.PROMPT_LEN - 1 + len(h)]
            for s, r in where:
                worst = max(worst, float(np.abs(got - logits[s, b * K + r]).max()))
                top = max(top, float(np.abs(logits[s, b * K + r]).max()))
    return worst, 1e-3 * max(1.0, top), dec


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_beam_result_equals_hf_where_the_margins_allow(mode):
    """E <= g over the fixture's rows (f16x, fp32x).  A hypothesis' score after n decided steps is off by at most 2 E n (E from the logit,
    at most E from the normaliser), two hypotheses differ by at most 4 E n: where 4 E <= r -- r the fixture's smallest gap / (step + 1)
    over every comparison that changes the rule's state -- the device's beam result must equal HF's exactly, alone and batched.  f16x must
    meet 4 E <= r; fp32x is pinned when it meets it and reported otherwise; bf16 is measured and never pinned."""
    gold, geo, sd, spec, enc = beam_fixture()
    E, g, dec = measured_E(mode)
    r, K = float(gold["r"]), int(gold["K"])
    print(f"BEAMHF {mode}: E {E:.3e}, g {g:.3e}, r {r:.3e}, 4 E / r {4 * E / r:.3f} (recorded E {E_MEASURED[mode]})")
    if mode == "bf16":
        return
    assert E <= g, (E, g)
    if mode == "f16x":
        assert 4 * E <= r, (E, r)
    if 4 * E > r:
        return
    first = spec.PROMPT_LEN - 1
    runs = [(dec.generate(enc_dev(enc, slice(None)), 3, num_beams=K, length_penalty=float(gold["length_penalty"])), [0, 1, 2])]
    runs += [(dec.generate(enc_dev(enc, slice(b, b + 1)), 1, num_beams=K, length_penalty=float(gold["length_penalty"])), [b]) for b in range(3)]
    for res, which in runs:
        assert not res.failed
        for i, b in enumerate(which):
            n = int(gold["lengths"][b])
            assert res.sequences[i, :n].tolist() == gold["sequences"][b, :n].tolist() and (res.sequences[i, n:] == spec.pad_token_id).all()
            assert abs(res.beam_scores[i] - gold["scores"][b]) <= 2 * E * (n - spec.PROMPT_LEN) + 1e-9
            tr = res.beam_trace
            assert int(tr["done_step"][i]) == first + int(gold["done_steps"][b])
            for s in range(int(gold["done_steps"][b]) + 1):
                assert tr["cand"][first + s, i, :, 0].tolist() == gold["cand_parents"][s, b].tolist(), (b, s)
                assert tr["cand"][first + s, i, :, 1].tolist() == gold["cand_tokens"][s, b].tolist(), (b, s)
                live = gold["run_scores"][s, b] > -1e8
                assert tr["run"][first + s, i, live, 0].tolist() == gold["run_parents"][s, b][live].tolist(), (b, s)
                assert tr["run"][first + s, i, live, 1].tolist() == gold["run_tokens"][s, b][live].tolist(), (b, s)
            fin = int(gold["fin_mask"][b].sum())
            assert int(tr["n_fin"][i]) == fin == len(res.nbest[i])
            for k, (ids, score) in enumerate(res.nbest[i]):
                assert gold["fin_sequences"][b, k, spec.PROMPT_LEN: spec.PROMPT_LEN + len(ids)].tolist() == ids, (b, k)
                assert abs(score - gold["fin_scores"][b, k]) <= 2 * E * len(ids) + 1e-9
