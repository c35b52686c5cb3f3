"""Generate tests/golden/tiny_whisper_seg_d128h2.npz: HF's greedy decoding WITH segment timestamps on the tiny decoder geometry
(config.TINY_WHISPER_DEC).  Run once on the CPU; the output is committed.  TEST INFRASTRUCTURE ONLY (needs ``transformers``).

    python tools/make_whisper_segments_golden.py [--seeds 300]

How HF is driven.  ``generate`` cannot be driven offline on a hand-made tiny config (tools/make_whisper_decoder_golden.py says why), so
``hf_timestamps`` calls HF's own pieces in ``generate``'s order around the float64 model's forward: ``detect_language``, then per position
``SuppressTokensAtBeginLogitsProcessor(begin_index=3)``, ``SuppressTokensLogitsProcessor``, ``WhisperTimeStampLogitsProcessor(
begin_index=3)``, argmax, pad for finished rows, stop on all-finished or max_length.  The prompt is ``[start, language, task]``.

The token layout is a real checkpoint's order on V = 522: text 0 .. 469 < eos 470 < start 471, languages 472 .. 475, translate 476,
transcribe 477, three further specials < no_timestamps 481 < 40 timestamp tokens 482 .. 521 (<|0.00|> .. <|0.78|>); pad = eos.

What is stored.  Seeds, a digest, ONE scalar (``ts_scale``, put on the timestamp rows of embed_tokens -- the tied output projection --
so that the sum rule neither always nor never fires), HF's sequences and HF's float64 logits of the decided rows as fp32.

The search.  Decoder seeds (at most ``--seeds``, at most 300) x ``ts_scale`` in SCALES; per pair a pool of 40 encoder-state seeds, each one
utterance.  Three utterances are picked, one per role -- at least 2 closed segments; ends on a single timestamp before eos; cut by
max_length -- that are pairwise different, with the largest smallest (margin, ts_gap) / g.  Asserted here and again in
tests/test_whisper_segments_host.py: the roles; step 5 changes the winner at some step and stays silent at some step where timestamps
were allowed; with g = 1e-3 max(1, max|logits|) every decided step has margin >= 4 g and ts_gap >= 4 g; the numpy rule
(tests/whisper_seg_ref.py) fed HF's logits gives HF's tokens.  The first pair that meets them is stored.
"""
from __future__ import annotations

import argparse
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
from interspeech_ser_amd.weights import state_dict_digest                                       # noqa: E402
import make_whisper_decoder_golden as G                                                         # noqa: E402
import whisper_dec_ref as R                                                                     # noqa: E402
import whisper_seg_ref as SR                                                                    # noqa: E402

GEO = C.TINY_WHISPER_DEC
OUT = os.path.join(ROOT, "tests", "golden", "tiny_whisper_seg_d128h2.npz")
V = GEO.decoder_vocab_size
EOS, START, TRANSLATE, TASK, NO_TS = 470, 471, 476, 477, 481
LANGS = {"<|en|>": 472, "<|de|>": 473, "<|fr|>": 474, "<|es|>": 475}
TS_BEGIN = NO_TS + 1
PAD = EOS
SUPPRESS = tuple(range(30, 70)) + (START, TRANSLATE, TASK, 478, 479, 480) + tuple(LANGS.values())
BEGIN_SUPPRESS = (220, EOS)                      # Whisper's: the space token and eos
MAX_LENGTH = 24
MAX_INITIAL = 25                                 # <|0.50|>: inside the 40 timestamp tokens, so that the bound is live
SCALES = (1.0, 0.75, 1.25, 0.5, 1.5)
POOL = 40
P = SR.P


def make_spec() -> C.GenerationSpec:
    return C.GenerationSpec(decoder_start_token_id=START, eos_token_id=EOS, pad_token_id=PAD, suppress_tokens=SUPPRESS,
                            begin_suppress_tokens=BEGIN_SUPPRESS, no_timestamps_token_id=NO_TS, lang_ids=tuple(sorted(LANGS.values())),
                            task_id=TASK, max_length=MAX_LENGTH, max_initial_timestamp_index=MAX_INITIAL)


def hf_generation_config(spec):
    import transformers as tf
    return tf.GenerationConfig(decoder_start_token_id=START, eos_token_id=EOS, pad_token_id=PAD, bos_token_id=START,
                               suppress_tokens=list(spec.suppress_tokens), begin_suppress_tokens=list(spec.begin_suppress_tokens),
                               no_timestamps_token_id=NO_TS, lang_to_id=dict(LANGS), task_to_id={"transcribe": TASK, "translate": TRANSLATE},
                               is_multilingual=True, max_length=spec.max_length, return_timestamps=True,
                               max_initial_timestamp_index=spec.max_initial_timestamp_index)


@torch.no_grad()
def hf_timestamps(model, spec, enc):
    """HF's pieces in ``generate``'s order (module docstring).  Returns (sequences [B, n], languages [B])."""
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=enc)
    B = enc.shape[0]
    gc = hf_generation_config(spec)
    langs = model.detect_language(encoder_outputs=eo, generation_config=gc)
    ids = torch.tensor([[START, 0, TASK]] * B, dtype=torch.long)
    ids[:, 1] = langs
    procs = [SuppressTokensAtBeginLogitsProcessor(list(spec.begin_suppress_tokens), begin_index=P),
             SuppressTokensLogitsProcessor(list(spec.suppress_tokens)),
             WhisperTimeStampLogitsProcessor(gc, begin_index=P)]
    assert procs[2].max_initial_timestamp_index == spec.max_initial_timestamp_index and procs[2].timestamp_begin == TS_BEGIN
    unfinished = torch.ones(B, dtype=torch.long)
    while ids.shape[1] < spec.max_length and int(unfinished.max()) > 0:
        scores = model(encoder_outputs=eo, decoder_input_ids=ids, use_cache=False).logits[:, -1].clone()
        for p in procs:
            scores = p(ids, scores)
        nxt = scores.argmax(-1) * unfinished + PAD * (1 - unfinished)
        ids = torch.cat([ids, nxt[:, None]], 1)
        unfinished = unfinished * (nxt != spec.eos_token_id).long()
    return ids, langs


def decided(seq_row, spec):
    """positions of one row whose logits decide a token: from P - 1 to the one that emits eos (or the last)"""
    out = []
    for p in range(P - 1, len(seq_row) - 1):
        out.append(p)
        if seq_row[p + 1] == spec.eos_token_id:
            break
    return out


def analyse(spec, seq_row, logits_row):
    """The numpy rule on HF's logits of one utterance: dict(ok = the rule gives HF's tokens, margin, gap (the smallest), zmax, changed =
    step 5 changed the winner somewhere, silent = it stayed silent somewhere with a live timestamp column, pairs, single_end, cut)."""
    m = R.masks(spec, V)
    ok, margin, gap, zmax, changed, silent = True, np.inf, np.inf, 0.0, False, False
    for p in decided(seq_row, spec):
        z = logits_row[p]
        gen = [int(t) for t in seq_row[P: p + 1]]
        _, tok, mg, gp, fired, before = SR.rule(z, m[1 if p == P - 1 else 0], gen, TS_BEGIN, NO_TS, EOS, spec.max_initial_timestamp_index)
        ok &= tok == int(seq_row[p + 1])
        margin, gap, zmax = min(margin, mg), min(gap, gp), max(zmax, float(np.abs(z).max()))
        changed |= fired and before != tok
        silent |= (not fired) and np.isfinite(gp)           # a finite gap: a timestamp column and a text column were both live
    gen = [int(t) for t in seq_row[P:]]
    cut = EOS not in gen
    body = gen if cut else gen[: gen.index(EOS)]
    ts = [t >= TS_BEGIN for t in body]
    pairs = sum(1 for i in range(len(body) - 1) if ts[i] and ts[i + 1])
    return dict(ok=bool(ok), margin=margin, gap=gap, zmax=zmax, changed=changed, silent=silent, pairs=pairs,
                single_end=(not cut) and ts[-2:] == [False, True], cut=cut, body=body)


def search(seed: int, scale: float):
    """None, or the record of (decoder seed, ts_scale): the three picked utterances of the pool."""
    spec = make_spec()
    sd = SR.fixture_state_dict(GEO, seed, TS_BEGIN, scale)
    model = G.hf_model(sd)
    enc_seeds = [2000 + e for e in range(POOL)]
    encs = torch.from_numpy(np.concatenate([R.enc_states(e, 1, GEO.max_source_positions, GEO.hidden) for e in enc_seeds])).double()
    seq, langs = hf_timestamps(model, spec, encs)
    logits = G.hf_logits(model, encs, seq).numpy()
    seq = seq.numpy()
    info = [analyse(spec, seq[b], logits[b]) for b in range(POOL)]
    g = 1e-3 * max(1.0, max(i["zmax"] for i in info))
    good = [b for b in range(POOL) if info[b]["ok"] and min(info[b]["margin"], info[b]["gap"]) >= 4 * g]
    roles = ([b for b in good if info[b]["pairs"] >= 2], [b for b in good if info[b]["single_end"]], [b for b in good if info[b]["cut"]])
    best = None
    for pick in itertools.product(*roles):
        if len(set(pick)) < 3 or len({tuple(info[b]["body"]) for b in pick}) < 3:
            continue
        if not (any(info[b]["changed"] for b in pick) and any(info[b]["silent"] for b in pick)):
            continue
        r = min(min(info[b]["margin"], info[b]["gap"]) for b in pick)
        if best is None or r > best[0]:
            best = (r, pick)
    if best is None:
        return None, (f"roles {[len(r) for r in roles]} of {len(good)} good utterances, changed "
                      f"{sum(i['changed'] for i in info)}, silent {sum(i['silent'] for i in info)}")
    pick = list(best[1])
    return dict(seed=seed, scale=scale, sd=sd, model=model, spec=spec, enc_seeds=[enc_seeds[b] for b in pick]), ""


def record(case) -> None:
    """Run HF on the three picked utterances alone (a batch of 3), assert the conditions on that run, and store it."""
    spec, model = case["spec"], case["model"]
    encs = torch.from_numpy(np.concatenate([R.enc_states(e, 1, GEO.max_source_positions, GEO.hidden) for e in case["enc_seeds"]])).double()
    seq, langs = hf_timestamps(model, spec, encs)
    logits = G.hf_logits(model, encs, seq).numpy()
    seq = seq.numpy()
    info = [analyse(spec, seq[b], logits[b]) for b in range(3)]
    g = 1e-3 * max(1.0, max(i["zmax"] for i in info))
    assert all(i["ok"] for i in info), "the numpy rule does not give HF's tokens"
    assert min(i["margin"] for i in info) >= 4 * g and min(i["gap"] for i in info) >= 4 * g, (g, info)
    assert info[0]["pairs"] >= 2 and info[1]["single_end"] and info[2]["cut"]
    assert any(i["changed"] for i in info) and any(i["silent"] for i in info)
    assert len({tuple(i["body"]) for i in info}) == 3
    n = seq.shape[1]
    keep = np.zeros((3, n), dtype=bool)                                       # the decided rows: only their logits are stored
    for b in range(3):
        keep[b, decided(seq[b], spec)] = True
    np.savez_compressed(
        OUT, decoder_seed=np.array(case["seed"]), ts_scale=np.array(case["scale"]), digest=state_dict_digest(case["sd"]),
        enc_seeds=np.array(case["enc_seeds"]), max_length=np.array(spec.max_length), max_initial=np.array(spec.max_initial_timestamp_index),
        eos=np.array(EOS), start=np.array(START), pad=np.array(PAD), task=np.array(TASK), no_timestamps=np.array(NO_TS),
        ts_begin=np.array(TS_BEGIN), lang_ids=np.array(spec.lang_ids), suppress=np.array(spec.suppress_tokens),
        begin_suppress=np.array(spec.begin_suppress_tokens), languages=langs.numpy(), sequences=seq, decided=keep,
        logits=logits[keep].astype(np.float32), g=np.array(g), min_margin=np.array(min(i["margin"] for i in info)),
        min_gap=np.array(min(i["gap"] for i in info)))
    print(f"seed {case['seed']} ts_scale {case['scale']} utterances {case['enc_seeds']}: g {g:.3e} margin {min(i['margin'] for i in info):.3e} "
          f"gap {min(i['gap'] for i in info):.3e}\n  rows {[list(r) for r in seq]}\n  {os.path.getsize(OUT)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300, help="decoder seeds 0 .. seeds - 1 are searched (at most 300)")
    ap.add_argument("--only", type=int, default=None, help="search this decoder seed alone")
    args = ap.parse_args()
    torch.set_num_threads(8)
    for seed in (range(min(args.seeds, 300)) if args.only is None else [args.only]):
        for scale in SCALES:
            case, why = search(seed, scale)
            print(f"seed {seed} ts_scale {scale}: " + ("found" if case else why), flush=True)
            if case is not None:
                record(case)
                return
    raise SystemExit("no decoder seed meets the conditions")


if __name__ == "__main__":
    main()
