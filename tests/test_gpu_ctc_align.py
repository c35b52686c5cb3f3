"""GPU: CTC forced alignment -- ser_ctc_align_v against the numpy rule (tests/ctc_align_ref.py) bit for bit on synthetic logits, its ties,
status words and refusals, engine.CTCHead.forward_align / ctc.CTCAligner against HF's char offsets of the fixtures and against the rule on
the device's own logits, and the command line.

Bounds.  alpha is float64 over raw fp32 logits: one max of exact values and one addition per cell, so pos, starts, ends, status and
path_logit (its 64 bits) are compared for EQUALITY.  frame_score = fp32(z - lse64) goes against the float64 statement with
2^-23 max(1, |score64|): one rounding of the result (2^-24 relative) and as much again for the device library's double exp / log.
tok_score must be within one fp32 ulp of the numpy mean of the DEVICE's frame scores (the same float64 sum in frame order).
End to end (f16x, fp32x): the logits are within g of HF's and every fixture margin is at least 4 g, so the device's per-frame winners are
HF's and aligning the greedy ids gives HF's offsets exactly; for a non-greedy target the device must equal the rule on ITS OWN logits, and
its path_logit is within T g of the best float64 path over HF's logits (every path's sum moves by at most T times the logit error)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import ctc_align_ref as A
import ctc_ref as R
from test_gpu_ctc import _fixture, _snapshot, _write_pcm16, sticky_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = -777


def run_kernel(z, offs, targets, V, blank, optional=True, max_tokens=None):
    """ser_ctc_align_v on host logits z [rows, ldz] (fp32) -> dict of host arrays; every output buffer starts as POISON"""
    from interspeech_ser_amd import _lib
    z = np.ascontiguousarray(z, dtype=np.float32)
    rows, ldz = z.shape
    B = len(offs) - 1
    Tm = max(int(offs[b + 1] - offs[b]) for b in range(B))
    Lm = max(len(y) for y in targets) if max_tokens is None else max_tokens
    Lp = max(Lm, 1)
    toffs = np.concatenate([[0], np.cumsum([len(y) for y in targets])]).astype(np.int32)
    flat = np.array([v for y in targets for v in y] + [0], dtype=np.int32)
    zd = torch.from_numpy(z).to(DEV)
    od = torch.tensor([int(o) for o in offs], dtype=torch.int32, device=DEV)
    td, tod = torch.from_numpy(flat).to(DEV), torch.from_numpy(toffs).to(DEV)
    wb = int(_lib.lib.ser_ctc_align_work_bytes(rows, B, Tm, Lm))
    assert wb > 0
    work = torch.zeros((wb + 7) // 8, dtype=torch.int64, device=DEV)
    i32 = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device=DEV)                   # noqa: E731
    f32 = lambda *shape: torch.full(shape, float(POISON), dtype=torch.float32, device=DEV)          # noqa: E731
    out = dict(starts=i32(B, Lp), ends=i32(B, Lp), tok_score=f32(B, Lp), status=i32(B),
               path_logit=torch.full((B,), float(POISON), dtype=torch.float64, device=DEV), pos=i32(rows), frame_score=f32(rows))
    a = _lib.CtcAlignArgs()
    a.z, a.ldz, a.frame_offs, a.targets, a.tgt_offs = zd.data_ptr(), ldz, od.data_ptr(), td.data_ptr(), tod.data_ptr()
    a.work, a.work_bytes = work.data_ptr(), wb
    a.starts, a.ends, a.tok_score, a.ld_tok = out["starts"].data_ptr(), out["ends"].data_ptr(), out["tok_score"].data_ptr(), Lp
    a.status, a.path_logit = out["status"].data_ptr(), out["path_logit"].data_ptr()
    if optional:
        a.pos, a.frame_score = out["pos"].data_ptr(), out["frame_score"].data_ptr()
    a.B, a.V, a.rows, a.blank, a.max_frames, a.max_tokens, a.n_targets = B, V, rows, blank, Tm, Lm, len(flat) - 1
    _lib.check(_lib.lib.ser_ctc_align_v(ctypes.byref(a), None), "ser_ctc_align_v")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def within_one_ulp(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)))


def check_against_rule(got, z, offs, targets, V, blank, max_tokens=1023):
    """every utterance's outputs against the numpy rule's; returns the rule's results"""
    wants = []
    for b, y in enumerate(targets):
        r0, r1, L = int(offs[b]), int(offs[b + 1]), len(y)
        want = A.align(z[r0:r1], y, V, blank, max_tokens)
        wants.append(want)
        assert int(got["status"][b]) == want["status"], (b, got["status"][b], want["status"])
        if want["status"]:
            continue
        assert bits64(got["path_logit"][b: b + 1])[0] == bits64([want["path_logit"]])[0], b
        assert np.array_equal(got["pos"][r0:r1], want["pos"]), b
        assert np.array_equal(got["starts"][b, :L], want["starts"]) and np.array_equal(got["ends"][b, :L], want["ends"]), b
        for k in ("starts", "ends"):
            assert (got[k][b, L:] == POISON).all(), (k, b)
        assert (got["tok_score"][b, L:] == float(POISON)).all(), b
        fs, fs64 = got["frame_score"][r0:r1].astype(np.float64), want["frame_score64"]
        err = np.abs(fs - fs64)
        bound = 2.0 ** -23 * np.maximum(1.0, np.abs(fs64))
        assert (err <= bound).all(), (b, float((err / bound).max()))
        assert within_one_ulp(got["tok_score"][b, :L], A.token_means(got["frame_score"][r0:r1], want["starts"], want["ends"])), b
    return wants


def same_utterance(one, i, ro, whole, b, r0, L, T):
    """utterance i of ``one`` (rows from ro) is bit-equal to utterance b of ``whole`` (rows from r0)"""
    assert int(one["status"][i]) == int(whole["status"][b])
    assert bits64(one["path_logit"][i: i + 1])[0] == bits64(whole["path_logit"][b: b + 1])[0]
    for k in ("starts", "ends"):
        assert np.array_equal(one[k][i, :L], whole[k][b, :L]), k
    assert np.array_equal(bits32(one["tok_score"][i, :L]), bits32(whole["tok_score"][b, :L]))
    assert np.array_equal(one["pos"][ro: ro + T], whole["pos"][r0: r0 + T])
    assert np.array_equal(bits32(one["frame_score"][ro: ro + T]), bits32(whole["frame_score"][r0: r0 + T]))


# ------------------------------------------------------------------------------- 1. the kernel against the numpy rule
def _batch(V, blank, rng):
    """targets and frame counts on each side of every state-count threshold of the kernel (a wave's 64 states per ballot, the block's
    threads, twice the block's threads), each at T = L + rep (one path), L + rep + 1 and about 3 L; an empty target, T = 1 with one token,
    and one token repeated"""
    from interspeech_ser_amd import _lib
    targets, lengths = [], []
    for S_edge in (_lib.WAVE, _lib.CTC_ALIGN_THREADS, 2 * _lib.CTC_ALIGN_THREADS):
        for L in (S_edge // 2 - 1, S_edge // 2):                              # S = 2 L + 1 = edge - 1 and edge + 1
            y = A.sticky_targets(rng, L, V, blank)
            need = L + A.n_repeats(y)
            for T in (need, need + 1, max(3 * L, need + 2)):
                targets.append(y)
                lengths.append(T)
    targets += [[], A.sticky_targets(rng, 1, V, blank), [(blank + 1) % V] * 9]
    lengths += [5, 1, 20]
    return targets, lengths


@pytest.mark.parametrize("V, ldz, blank", [(2, 4, 0), (12, 16, 5), (32, 32, 0), (67, 68, 66), (1000, 1000, 3)])
def test_kernel_equals_the_rule_bit_for_bit(V, ldz, blank):
    rng = np.random.default_rng(300 + V)
    targets, lengths = _batch(V, blank, rng)
    offs = np.concatenate([[0], np.cumsum(lengths)])
    z = sticky_logits(rng, lengths, V, ldz, blank, 1e30)                       # a padding column would win every frame if read
    got = run_kernel(z, offs, targets, V, blank)
    wants = check_against_rule(got, z, offs, targets, V, blank)
    assert all(w["status"] == 0 for w in wants)
    # two utterances alone, and the batch reversed: bit-equal outputs
    for b in (5, 14):
        alone = run_kernel(z[offs[b]: offs[b + 1]], [0, lengths[b]], [targets[b]], V, blank)
        same_utterance(alone, 0, 0, got, b, int(offs[b]), len(targets[b]), lengths[b])
    order = list(range(len(lengths)))[::-1]
    roffs = np.concatenate([[0], np.cumsum([lengths[b] for b in order])])
    rev = run_kernel(np.concatenate([z[offs[b]: offs[b + 1]] for b in order]), roffs, [targets[b] for b in order], V, blank)
    for i, b in enumerate(order):
        same_utterance(rev, i, int(roffs[i]), got, b, int(offs[b]), len(targets[b]), lengths[b])
    # NULL optional outputs: the rest does not move, the skipped buffers keep their poison
    bare = run_kernel(z, offs, targets, V, blank, optional=False)
    assert (bare["pos"] == POISON).all() and (bare["frame_score"] == float(POISON)).all()
    for k in ("status", "starts", "ends"):
        assert np.array_equal(bare[k], got[k]), k
    assert np.array_equal(bits32(bare["tok_score"]), bits32(got["tok_score"])) and np.array_equal(bits64(bare["path_logit"]), bits64(got["path_logit"]))


# ------------------------------------------------------------------------------- 2. ties
def _states(got, r0, T, y):
    """the state sequence of an utterance from pos and the span table (a blank frame's state from the tokens around it)"""
    pos = got["pos"][r0: r0 + T]
    out, last = [], -1
    for t in range(T):
        if pos[t] >= 0:
            last = int(pos[t])
            out.append(2 * last + 1)
        else:
            out.append(2 * (last + 1))
    return out


def test_ties_stay_over_step_over_skip_and_the_end_rule():
    V, y = 4, [1, 2, 3]
    zero = np.zeros((7, V), dtype=np.float32)                                  # every path ties: end in S - 2, stay while reachable
    blank_last = zero.copy()
    blank_last[6, 0] = 1.0                                                     # S - 1 strictly better: ends in the blank, and stays there while reachable
    onehot = np.zeros((7, V), dtype=np.float32)
    for t, c in enumerate([0, 1, 1, 2, 0, 3, 0]):                              # one path is strictly best: blank A A B blank C blank
        onehot[t, c] = 5.0
    step_or_skip = np.zeros((3, V), dtype=np.float32)                          # T = 3 = L: one path, all skips
    rep = np.zeros((6, V), dtype=np.float32)                                   # [1, 1, 3]: no skip across the blank between the repeats
    cases = [(zero, y, [1, 3, 5, 5, 5, 5, 5]), (blank_last, y, [1, 3, 5, 6, 6, 6, 6]), (onehot, y, [0, 1, 1, 3, 4, 5, 6]),
             (step_or_skip, y, [1, 3, 5]), (rep, [1, 1, 3], [1, 2, 3, 5, 5, 5])]
    lengths = [c[0].shape[0] for c in cases]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    z = np.concatenate([c[0] for c in cases])
    targets = [c[1] for c in cases]
    got = run_kernel(z, offs, targets, V, 0)
    check_against_rule(got, z, offs, targets, V, 0)
    for b, (_, yb, want_states) in enumerate(cases):
        assert int(got["status"][b]) == 0 and _states(got, int(offs[b]), lengths[b], yb) == want_states, b
    assert got["path_logit"].tolist() == [0.0, 1.0, 35.0, 0.0, 0.0]


# ------------------------------------------------------------------------------- 3. status
STATUS_CASES = ["too few frames", "nan read", "+inf read", "nan unread", "blank -inf, needed", "blank in target", "id == V"]


@pytest.mark.parametrize("case", STATUS_CASES)
def test_status_is_per_utterance(case):
    """the middle utterance of three is spoilt; the other two are bit-equal to the clean run.  Nothing here faults: each is a value the
    kernel checks before it indexes with it."""
    from interspeech_ser_amd import _lib
    V, ldz, blank = 12, 12, 0
    rng = np.random.default_rng(11)
    targets = [A.sticky_targets(rng, 40, V, blank), [3, 4, 4, 5, 6, 3], A.sticky_targets(rng, 70, V, blank)]
    lengths = [100, 30, 200]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    z = sticky_logits(rng, lengths, V, ldz, blank, 0.0)
    z[:, 7] = -3.0                                                             # column 7 is in no target and wins no frame
    targets = [[v if v != 7 else 8 for v in y] for y in targets]
    clean = run_kernel(z, offs, targets, V, blank)
    assert (clean["status"] == 0).all()
    r0, t_bad = int(offs[1]), 13
    zz, tg, want = z.copy(), [list(y) for y in targets], None
    if case == "too few frames":
        lengths2 = [100, 6, 200]                                               # 6 tokens and one repeat need 7 frames
        offs2 = np.concatenate([[0], np.cumsum(lengths2)])
        zz = np.concatenate([z[: offs[1] + 6], z[offs[2]:]])
        got = run_kernel(zz, offs2, tg, V, blank)
        assert int(got["status"][1]) == _lib.CTC_ALIGN_INFEASIBLE
        same_utterance(got, 0, 0, clean, 0, 0, 40, 100)
        same_utterance(got, 2, int(offs2[2]), clean, 2, int(offs[2]), 70, 200)
        return
    if case == "nan read":
        zz[r0 + t_bad, 4], want = np.nan, _lib.CTC_ALIGN_NONFINITE
    elif case == "+inf read":
        zz[r0 + t_bad, 0], want = np.inf, _lib.CTC_ALIGN_NONFINITE
    elif case == "nan unread":
        zz[r0 + t_bad, 7], want = np.nan, 0
    elif case == "blank -inf, needed":
        zz[r0: r0 + 30, 0], want = -np.inf, _lib.CTC_ALIGN_NONFINITE           # [.., 4, 4, ..] needs a blank between: the best score is -inf
    elif case == "blank in target":
        tg[1][2], want = blank, _lib.CTC_ALIGN_BAD_TARGET
    elif case == "id == V":
        tg[1][5], want = V, _lib.CTC_ALIGN_BAD_TARGET
    got = run_kernel(zz, offs, tg, V, blank)
    assert int(got["status"][1]) == want == A.align(zz[r0: r0 + 30], tg[1], V, blank)["status"]
    same_utterance(got, 0, 0, clean, 0, 0, 40, 100)
    same_utterance(got, 2, int(offs[2]), clean, 2, int(offs[2]), 70, 200)
    if case == "nan unread":
        # a NaN outside {blank} U y sets no status and cannot move the path; that frame's lse64 is NaN, and with it the frame's score and
        # the mean of the token the frame belongs to (none when the frame is blank)
        assert np.array_equal(got["pos"][r0: r0 + 30], clean["pos"][r0: r0 + 30]) and np.array_equal(got["starts"][1], clean["starts"][1])
        assert np.array_equal(got["ends"][1], clean["ends"][1]) and bits64(got["path_logit"][1:2])[0] == bits64(clean["path_logit"][1:2])[0]
        fs, cs = got["frame_score"][r0: r0 + 30], clean["frame_score"][r0: r0 + 30]
        keep = np.arange(30) != t_bad
        assert np.isnan(fs[t_bad]) and np.array_equal(bits32(fs[keep]), bits32(cs[keep]))
        j = int(clean["pos"][r0 + t_bad])
        for k in range(6):
            if k == j:
                assert np.isnan(got["tok_score"][1, k])
            else:
                assert bits32(got["tok_score"][1, k: k + 1])[0] == bits32(clean["tok_score"][1, k: k + 1])[0]


# ------------------------------------------------------------------------------- 4. refusals (return codes only: no launch)
def test_refusals_on_device_buffers():
    from interspeech_ser_amd import _lib
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()

    def args(**kw):
        a = _lib.CtcAlignArgs()
        a.z, a.ldz, a.frame_offs, a.targets, a.tgt_offs, a.work, a.work_bytes = p, 12, p, p, p, p, 8 * buf.numel()
        a.starts, a.ends, a.tok_score, a.ld_tok, a.status, a.path_logit = p, p, p, 8, p, p
        a.B, a.V, a.rows, a.blank, a.max_frames, a.max_tokens, a.n_targets = 2, 12, 40, 0, 20, 8, 10
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    need = int(_lib.lib.ser_ctc_align_work_bytes(40, 2, 20, 8))
    for kw, rc in ((dict(status=None), -1), (dict(targets=None), -1), (dict(work_bytes=need - 1), -2), (dict(B=0), -2), (dict(B=65536), -2),
                   (dict(max_tokens=_lib.CTC_ALIGN_MAX_TOKENS + 1), -2), (dict(blank=12), -2), (dict(ldz=11), -3), (dict(ld_tok=7), -3),
                   (dict(work=p + 4), -3), (dict(z=p + 2), -3)):
        assert _lib.lib.ser_ctc_align_v(ctypes.byref(args(**kw)), None) == rc, kw
        assert b"ser_ctc_align" in _lib.lib.ser_last_error()
    torch.cuda.synchronize()
    assert int(buf.abs().sum().item()) == 0                                    # nothing ran


# ------------------------------------------------------------------------------- 5. end to end on the fixtures
_AL = {}


def _aligner(name, mode):
    from interspeech_ser_amd.ctc import CTCAligner
    from interspeech_ser_amd.weights import CTC_HEAD_PREFIXES, normalize_names
    if (name, mode) not in _AL:
        fx, waves, sd = _fixture(name)
        _AL[(name, mode)] = CTCAligner(fx.geometry(), fx.spec(), normalize_names(sd, keep=CTC_HEAD_PREFIXES), DEV, mode, batch_size=16,
                                       normalize=bool(fx.preprocessor.get("do_normalize", True)))
    return _AL[(name, mode)]


def _thinned(ids):
    return [t for k, t in enumerate(ids) if k % 3 != 2]


@pytest.mark.parametrize("mode", ["f16x", "fp32x"])
@pytest.mark.parametrize("name", R.FIXTURES)
def test_aligner_equals_hf_offsets_and_the_rule_on_its_own_logits(name, mode):
    fx, waves, _ = _fixture(name)
    al = _aligner(name, mode)
    got = al.align(waves, fx.ids)                                              # one ragged batch through the slot pipeline
    assert al.failed == []
    for j, r in enumerate(got):
        assert r.ids == fx.ids[j] and r.spans == fx.offsets[j], j
        assert len(r.tok_scores) == len(fx.ids[j]) and all(s <= 0 for s in r.tok_scores) and r.score <= 0
    # a non-greedy target: every third greedy id dropped
    targets = [_thinned(i) for i in fx.ids]
    res = al.extract(waves, targets)
    z = al.head.logits(0).cpu().numpy()
    g, r0, agree, total = fx.gate(), 0, 0, 0
    for j, (y, r) in enumerate(zip(targets, res)):
        T = fx.logits64[j].shape[0]
        want = A.align(z[r0: r0 + T], y, fx.V, fx.blank)
        if want["status"]:
            assert isinstance(r, Exception) and r.status == want["status"], j
        else:
            assert r.spans == list(zip(want["starts"].tolist(), want["ends"].tolist())) and np.array_equal(r.pos, want["pos"]), j
            assert bits64([r.path_logit])[0] == bits64([want["path_logit"]])[0], j
            best64, states64 = A.trellis(fx.logits64[j], y, fx.blank, dtype=np.float64)
            print(f"CTC_ALIGN {name} {mode} utt {j}: |path_logit - best64| {abs(r.path_logit - best64):.3e} (T g = {T * g:.3e})")
            assert abs(r.path_logit - float(best64)) <= T * g, j
            agree += int(np.array_equal(want["states"], states64))
            total += 1
        r0 += T
    print(f"CTC_ALIGN_PATHS {name} {mode}: {agree} of {total} non-greedy paths equal the float64 path over HF's logits (not asserted)")


@pytest.mark.parametrize("name", R.FIXTURES)
def test_aligner_bf16_agreement_is_recorded(name):
    """bf16 operands: no span is pinned; the agreement with HF's offsets is printed for the profile"""
    fx, waves, _ = _fixture(name)
    got = _aligner(name, "bf16").align(waves, fx.ids)
    same = sum(int(r is not None and r.spans == fx.offsets[j]) for j, r in enumerate(got))
    spans = sum(int(a == b) for j, r in enumerate(got) if r is not None for a, b in zip(r.spans, fx.offsets[j]))
    print(f"CTC_ALIGN_BF16 {name}: {same} of {len(got)} utterances, {spans} of {sum(len(o) for o in fx.offsets)} spans equal HF's offsets")
    assert all(r is not None and r.ids == fx.ids[j] for j, r in enumerate(got))


def test_an_infeasible_item_fails_alone_in_the_pipeline(capsys):
    name = "tiny_ctc_wavlm"
    fx, waves, _ = _fixture(name)
    al = _aligner(name, "f16x")
    targets = [list(i) for i in fx.ids]
    targets[3] = [1, 1, 1]                                                     # one frame cannot hold three tokens
    got = al.align(waves, targets)
    assert got[3] is None and [i for i, _ in al.failed] == [3] and "1 frames are too few for a target of 3 tokens" in capsys.readouterr().out
    for j in range(3):
        assert got[j].spans == fx.offsets[j]


# ------------------------------------------------------------------------------- 6. the command line
def test_command_line(tmp_path, capsys):
    from interspeech_ser_amd import ctc as CT
    from interspeech_ser_amd.transcribe import write_table
    name = "tiny_ctc_wavlm_base"
    fx, waves, _ = _fixture(name)
    snap = _snapshot(tmp_path, name)
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    files = {f"u{j}.wav": _write_pcm16(wav_dir / f"u{j}.wav", waves[j]) for j in (0, 1, 2)}
    texts = {"u0.wav": "Ab c, a!", "u1.wav": "b 7 d", "u2.wav": "2024 ..."}   # u2: nothing the vocabulary can spell
    table = tmp_path / "t.csv"
    write_table(str(table), list(texts), list(texts.values()))
    vocab = CT.CTCVocab(R.tiny_vocab(fx.V, fx.blank))
    al = _aligner(name, "f16x")
    good = ["u0.wav", "u1.wav"]
    want = al.align([files[n] for n in good], [texts[n] for n in good], vocab=vocab)
    out_json = tmp_path / "a.json"
    assert CT.run_align(["--model", str(snap), "--wav_dir", str(wav_dir), "--df_path", str(table), "--out_json", str(out_json), "--chars"]) == 0
    out = capsys.readouterr().out
    assert f"Failed to process {wav_dir / 'u2.wav'}" in out and "has no word the vocabulary can spell" in out and "Wrote 2 of 3 alignments" in out
    got = json.loads(out_json.read_text())
    sec = al.hop / 16000.0
    assert sorted(got) == good
    for n, w in zip(good, want):
        ws = CT.words(w, vocab.encode_words(texts[n]))
        assert got[n]["score"] == w.score
        assert got[n]["words"] == [[x, None if s is None else s * sec, None if e is None else e * sec, sc] for x, s, e, sc in ws]
        ch, offs = vocab.chars(w.ids, w.spans)
        assert got[n]["chars"] == [[c, s * sec, e * sec, sc] for c, (s, e), sc in zip(ch, offs, w.tok_scores)]
    assert [x[0] for x in got["u1.wav"]["words"]] == ["b", "7", "d"] and got["u1.wav"]["words"][1][1:] == [None, None, None]
