"""Generate tests/golden/tiny_whisper_ts_d128h2.npz: HF's token timestamps (``WhisperGenerationMixin._extract_token_timestamps``) for
three utterances, EACH GIVEN ALONE, on the decoder fixture's geometry, seeded weights and encoder states
(tools/make_whisper_decoder_golden.py, tests/golden/tiny_whisper_dec_d128h2.npz).  Run once on the CPU; the output is committed.
TEST INFRASTRUCTURE ONLY (needs ``transformers``).

    python tools/make_whisper_timestamps_golden.py

How HF is driven.  As for the decoder fixture, ``generate`` cannot be driven offline on a hand-made generation config, so HF's own pieces
are called in ``generate``'s order: the greedy loop of the decoder fixture's tool with batch 1 (max_length 12: at most 8 generated
tokens), then ONE forward of the float64 model (eager attention, ``output_attentions=True``) over the sequence without its last token --
causal, so its cross-attention rows are the rows the incremental steps see --, wrapped as the ``cross_attentions`` of a generate output,
and HF's ``_extract_token_timestamps(outputs, alignment_heads, num_frames=len // 160, num_input_ids=4)``.  The float64 matrix is what
that function hands to ``_dynamic_time_warping`` (recorded through a wrapper around it, negated back).

Edge cases settled here against HF, each asserted below: one generated token gives zeros; two give one row whose z-score is NaN and the
time 0; at most 3 frames leave the median filter's input as it is.

The fixture rule: token-time equality must be a CONSEQUENCE of the matrix gate.  Per item, mu = (the cost of the best path whose jump
times differ from the optimum's) - (the optimum), by a forward and a backward DP in float64 over -matrix: a path first enters row i at
frame j exactly when it steps from row i - 1 into cell (i, j), so best(i, j) = min(fwd[i-1][j-1], fwd[i-1][j]) + bwd[i][j], and mu is
its minimum over rows i >= 2 and frames j other than the optimum's.  A matrix within g = 1e-3 max(1, max|matrix|) of HF's, entry by
entry, moves the cost of any path of at most N + M - 1 cells by at most (N + M - 1) g, and the fp32 cost table adds at most
(N + M) 2^-24 max|cost| per path: with mu above twice their sum the device's path has HF's jump times.  The sequences are the decoder
fixture's own (its margins hold), so what is searched is what they do not depend on: the alignment-head list (every list over the 2 x 2
heads with both layers and two heads of one layer) and the three frame counts (6 .. 24 frames, pairwise different).  No item is left out.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from interspeech_ser_amd import config as C                                                     # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_decoder_state_dict         # noqa: E402
import make_whisper_decoder_golden as D                                                         # noqa: E402
import whisper_dec_ref as R                                                                     # noqa: E402
import whisper_ts_ref as TS                                                                     # noqa: E402

GEO = C.TINY_WHISPER_DEC
OUT = os.path.join(ROOT, "tests", "golden", "tiny_whisper_ts_d128h2.npz")
DEC_GOLDEN = os.path.join(ROOT, "tests", "golden", "tiny_whisper_dec_d128h2.npz")
MAX_LENGTH = 12                                   # prompt 4 + at most 8 generated tokens: N <= 7 token rows
MAX_FRAMES = 24
P = 4


def margin(m64: np.ndarray, first: np.ndarray) -> float:
    """mu of the module docstring for the float64 matrix m64 [N, M] and the optimum's first frames."""
    c = -m64
    N, M = c.shape
    fwd = np.full((N + 1, M + 1), np.inf)
    fwd[0, 0] = 0.0
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            fwd[i, j] = c[i - 1, j - 1] + min(fwd[i - 1, j - 1], fwd[i - 1, j], fwd[i, j - 1])
    bwd = np.full((N + 2, M + 2), np.inf)           # bwd[i][j]: cell (i, j) to (N, M), both included
    for i in range(N, 0, -1):
        for j in range(M, 0, -1):
            nxt = 0.0 if (i == N and j == M) else min(bwd[i + 1, j + 1], bwd[i + 1, j], bwd[i, j + 1])
            bwd[i, j] = c[i - 1, j - 1] + nxt
    opt = fwd[N, M]
    mu = np.inf
    for i in range(2, N + 1):
        for j in range(1, M + 1):
            if j - 1 == int(first[i - 1]):
                continue
            mu = min(mu, min(fwd[i - 1, j - 1], fwd[i - 1, j]) + bwd[i, j] - opt)
    return float(mu)


def needed(m64: np.ndarray):
    N, M = m64.shape
    g = 1e-3 * max(1.0, float(np.abs(m64).max()))
    slack = (N + M) * 2.0 ** -24 * (N + M) * float(np.abs(m64).max())
    return g, 2 * ((N + M - 1) * g + slack)


@torch.no_grad()
def hf_token_timestamps(model, seq: torch.Tensor, enc: torch.Tensor, heads, num_frames: int):
    """(token_timestamps fp32 [len], the float64 matrix HF's DTW received, or None when it was not called)."""
    import transformers.models.whisper.generation_whisper as gw
    from transformers.generation.utils import GenerateEncoderDecoderOutput
    from transformers.modeling_outputs import BaseModelOutput
    out = model(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=seq[:, :-1], use_cache=False, output_attentions=True)
    assert out.cross_attentions is not None and out.cross_attentions[0].shape[2] == seq.shape[1] - 1
    go = GenerateEncoderDecoderOutput(sequences=seq, cross_attentions=(tuple(out.cross_attentions),))
    seen = []
    orig = gw._dynamic_time_warping

    def spy(neg):
        seen.append(-np.array(neg, dtype=np.float64))
        return orig(neg)

    gw._dynamic_time_warping = spy
    try:
        with np.errstate(invalid="ignore"):
            ts = model._extract_token_timestamps(go, [list(h) for h in heads], num_frames=int(num_frames), num_input_ids=P)
    finally:
        gw._dynamic_time_warping = orig
    assert ts.shape == (1, seq.shape[1]) and ts.dtype == torch.float32 and float(ts[0, :P].abs().max()) == 0.0
    return ts[0].numpy(), (seen[0] if seen else None)


def main():
    torch.set_num_threads(8)
    gold = np.load(DEC_GOLDEN)
    seed, enc_seed = int(gold["decoder_seed"]), int(gold["enc_seed"])
    sd = synthetic_decoder_state_dict(GEO, seed)
    assert state_dict_digest(sd) == str(gold["digest"])
    model = D.hf_model(sd)
    model.config._attn_implementation = "eager"
    model.model.config._attn_implementation = "eager"
    spec = C.GenerationSpec(decoder_start_token_id=D.START, eos_token_id=int(gold["eos"]), pad_token_id=D.PAD, suppress_tokens=D.SUPPRESS,
                            begin_suppress_tokens=tuple(int(t) for t in gold["begin_suppress"]), no_timestamps_token_id=D.NO_TS,
                            lang_ids=tuple(sorted(D.LANGS.values())), task_id=D.TASK, max_length=MAX_LENGTH)
    assert tuple(int(t) for t in gold["suppress"]) == tuple(D.SUPPRESS)
    enc = torch.from_numpy(R.enc_states(enc_seed, 3, GEO.max_source_positions, GEO.hidden)).double()
    seqs = []
    for b in range(3):
        s, lang = D.hf_greedy(model, spec, enc[b:b + 1])
        ref = gold["a_sequences"][b, :MAX_LENGTH]
        got = s[0].numpy()
        assert int(lang[0]) == int(gold["a_languages"][b]) and np.array_equal(got, ref[: len(got)]), (b, got, ref)
        seqs.append(s)
    n_tok = [int(s.shape[1]) - P for s in seqs]
    print("generated tokens per item:", n_tok)
    assert max(n_tok) <= 8 and len(set(n_tok)) >= 2

    # ---- the edge cases, against HF
    e1, m1 = hf_token_timestamps(model, seqs[1][:, : P + 1], enc[1:2], [(0, 0), (1, 1)], 20)
    assert m1 is None and np.all(e1 == 0), "one generated token: zeros, no DTW"
    e2, m2 = hf_token_timestamps(model, seqs[1][:, : P + 2], enc[1:2], [(0, 0), (1, 1)], 20)
    assert m2.shape == (1, 10) and np.isnan(m2).all() and np.all(e2 == 0), "two generated tokens: a NaN row and time 0"
    t2, i2, _ = TS.dtw(m2.astype(np.float32))
    assert np.array_equal(TS.token_times(TS.first_frames(t2, i2), 2), e2[P:])
    e3, m3 = hf_token_timestamps(model, seqs[1], enc[1:2], [(0, 0)], 6)
    import transformers.models.whisper.generation_whisper as gw
    z3 = torch.from_numpy(m3)[None]
    assert m3.shape[1] == 3 and torch.equal(gw._median_filter(z3, 7), z3), "three frames: the median filter returns its input"
    print("edge cases agree with HF: n = 1 zeros, n = 2 NaN row -> 0, F = 3 unfiltered")

    # ---- the search: head lists x frame counts
    all_heads = [(l, h) for l in range(GEO.decoder_layers) for h in range(GEO.decoder_attention_heads)]
    lists = [hs for k in (3, 4) for hs in itertools.combinations(all_heads, k)
             if len({l for l, _ in hs}) >= 2 and max(sum(1 for l, _ in hs if l == q) for q in range(GEO.decoder_layers)) >= 2]
    rng = np.random.default_rng(0)
    found = None
    tried = 0
    for heads in lists:
        for _ in range(40):
            frames = sorted(rng.choice(np.arange(6, MAX_FRAMES + 1), size=3, replace=False).tolist(), reverse=True)
            tried += 1
            items = []
            for b in range(3):
                ts, m = hf_token_timestamps(model, seqs[b], enc[b:b + 1], heads, 2 * frames[b])
                if not np.isfinite(m).all():
                    break
                text, time, _ = TS.dtw(m.astype(np.float32))
                first = TS.first_frames(text, time)
                assert np.array_equal(TS.token_times(first, n_tok[b]), ts[P:]), "the numpy rule and HF disagree"
                mu = margin(m, first)
                g, need = needed(m)
                items.append(dict(ts=ts, m=m, mu=mu, g=g, need=need, first=first))
                if mu < need:
                    break
            if len(items) == 3 and all(it["mu"] >= it["need"] for it in items):
                found = (heads, frames, items)
                break
        if found:
            break
    if not found:
        raise SystemExit(f"no head list and frame counts among {tried} meet the margin: shrink N or M, do not drop an item")
    heads, frames, items = found
    for b, it in enumerate(items):
        assert it["mu"] >= it["need"]
        print(f"item {b}: n = {n_tok[b]} tokens, F = {frames[b]} frames, mu = {it['mu']:.4f} >= {it['need']:.4f} (g = {it['g']:.3e}), "
              f"first frames {it['first'].tolist()}")
    N = max(n_tok)
    mats = np.full((3, N - 1, MAX_FRAMES), np.nan)
    tst = np.zeros((3, P + N), dtype=np.float32)
    sq = np.zeros((3, P + N), dtype=np.int64)
    for b, it in enumerate(items):
        mats[b, : n_tok[b] - 1, : frames[b]] = it["m"]
        tst[b, : P + n_tok[b]] = it["ts"]
        sq[b, : P + n_tok[b]] = seqs[b][0].numpy()
    np.savez_compressed(
        OUT, decoder_seed=np.array(seed), enc_seed=np.array(enc_seed), digest=state_dict_digest(sd), max_length=np.array(MAX_LENGTH),
        eos=np.array(spec.eos_token_id), begin_suppress=np.array(spec.begin_suppress_tokens), alignment_heads=np.array(heads),
        lengths=np.array([320 * f + 7 * b for b, f in enumerate(frames)]), frames=np.array(frames), n_tokens=np.array(n_tok),
        sequences=sq, matrix=mats, token_timestamps=tst, mu=np.array([it["mu"] for it in items]), g=np.array([it["g"] for it in items]),
        needed=np.array([it["need"] for it in items]))
    print(f"heads {heads}, frames {frames} after {tried} tries; {os.path.getsize(OUT)} bytes -> {OUT}")


if __name__ == "__main__":
    main()
