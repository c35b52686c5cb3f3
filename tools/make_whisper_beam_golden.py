"""Generate tests/golden/tiny_whisper_beam_d128h2.npz: HF's beam search on the tiny decoder geometry (config.TINY_WHISPER_DEC), with the
margins that say where a device may be held to it token for token.  Run once on the CPU; the output is committed.  TEST INFRASTRUCTURE
ONLY (needs ``transformers``).

    python tools/make_whisper_beam_golden.py [--seeds 300]

How HF is driven.  ``GenerationMixin._beam_search`` itself could not be driven for this purpose: it creates its running and finished
scores as ``torch.float`` whatever the model's dtype, so its sums of log-probabilities are fp32 sums, and Whisper's ``generate`` cannot be
driven offline on the hand-made generation config at all (tools/make_whisper_decoder_golden.py says why).  ``hf_beam`` therefore calls
``_beam_search``'s OWN helper functions -- ``_get_top_k_continuations``, ``_get_running_beams_for_next_iteration``,
``_update_finished_beams``, ``_check_early_stop_heuristic``, ``_beam_search_has_unfinished_sequences``, ``_flatten_beam_dim`` /
``_unflatten_beam_dim`` -- in ``_beam_search``'s order around the float64 model's forward, with its initial values ([0, -1e9, ...] running
scores, -1e9 finished scores), the two suppress processors and the max-length and eos stopping criteria, on float64 tensors: the logits
are cast to fp32 as ``_beam_search`` casts them, the log-softmax and every sum behind it run in float64.

The search (issue D).  Decoder seeds (at most ``--seeds``), K in {2, 3}, max_length in {12, 20}.  For a decoder seed every encoder-state seed
of a pool of 40 is one utterance; its r is the smallest gap / (step + 1) over every comparison that changes the rule's state (the gaps of
tests/whisper_beam_ref.py, and best against second-best finished at the end).  The 3 utterances of largest r are taken, r of the case is
their smallest.  Required: the beam result differs from the greedy one for at least one utterance, two survivors share a parent at
some step, one hypothesis is finished by eos before max_length, one utterance stops at least 3 steps before another.  The case of
largest r over the search is stored: HF's sequences, trace and scores, r, and HF's float64 logits of every (step, beam) row as fp32.
The committed file is the best of decoder seeds 0 .. 39 (``--seeds 40``: seed 26, K = 2, max_length 12, r = 2.24e-3; ``--only 26`` writes
it again): r already lies 300 times above four times the f16x logit error, so the search was not widened further.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_whisper_decoder_golden as G                                                          # noqa: E402
import whisper_beam_ref as BR                                                                   # noqa: E402
import whisper_dec_ref as R                                                                     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tiny_whisper_beam_d128h2.npz")
P = 4


@torch.no_grad()
def hf_beam(model, spec, enc, langs, K: int, length_penalty: float, max_length: int):
    """HF's helpers in ``_beam_search``'s order (module docstring) for a batch of encoder states [B, S, D] (float64) and the language ids
    of the prompt.  Returns dict: sequences (list of B id lists, prompt included, cut to the hypothesis' own length), scores [B],
    stop_step (the number of steps taken), and per step: logits fp32 [B K, V], cand (parents, tokens, scores [B, 2K]), run (parents,
    tokens, scores [B, K]), finished (scores [B, K], mask [B, K], sequences [B, K, max_length]), flag [B]."""
    from transformers.generation.logits_process import LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor
    from transformers.generation.stopping_criteria import EosTokenCriteria, MaxLengthCriteria, StoppingCriteriaList
    from transformers.modeling_outputs import BaseModelOutput
    B, V = enc.shape[0], model.config.vocab_size
    eo = BaseModelOutput(last_hidden_state=enc.repeat_interleave(K, dim=0))
    ids = torch.tensor([[G.START, int(l), G.TASK, G.NO_TS] for l in langs], dtype=torch.long).repeat_interleave(K, dim=0)
    procs = LogitsProcessorList([SuppressTokensLogitsProcessor(list(spec.suppress_tokens)),
                                 SuppressTokensAtBeginLogitsProcessor(list(spec.begin_suppress_tokens), begin_index=P)])
    crit = StoppingCriteriaList([MaxLengthCriteria(max_length=max_length), EosTokenCriteria(eos_token_id=spec.eos_token_id)])
    cur_len, keep = P, 2 * K
    top_mask = torch.cat((torch.ones(K, dtype=torch.bool), torch.zeros(keep - K, dtype=torch.bool)))
    running_sequences = torch.full((B, K, max_length), spec.pad_token_id, dtype=torch.int64)
    running_sequences[:, :, :cur_len] = model._unflatten_beam_dim(ids, B, K)
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((B, K), dtype=torch.float64)
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, K), -1e9, dtype=torch.float64)
    is_sent_finished = torch.zeros((B, K), dtype=torch.bool)
    flag = torch.ones((B, 1), dtype=torch.bool)
    running_beam_indices = torch.full((B, K, max_length - cur_len), -1, dtype=torch.int32)
    beam_indices = running_beam_indices.clone()
    offset = (torch.arange(B) * K).view(-1, 1)
    steps = []
    finished = False
    while not finished:
        flat = model._flatten_beam_dim(running_sequences[:, :, :cur_len])
        logits = model(encoder_outputs=eo, decoder_input_ids=flat, use_cache=False).logits[:, -1, :].to(dtype=torch.float32)
        log_probs = torch.nn.functional.log_softmax(logits.double(), dim=-1)
        log_probs = procs(flat, log_probs)
        log_probs = model._unflatten_beam_dim(log_probs, B, K) + running_beam_scores[:, :, None]
        log_probs = torch.reshape(log_probs, (B, K * V))
        topk_log_probs, topk_running_sequences, topk_running_beam_indices = model._get_top_k_continuations(
            accumulated_log_probs=log_probs, running_sequences=running_sequences, running_beam_indices=running_beam_indices, cur_len=cur_len,
            decoder_prompt_len=P, do_sample=False, beams_to_keep=keep, num_beams=K, vocab_size=V, batch_size=B)
        hits = crit(model._flatten_beam_dim(topk_running_sequences[:, :, : cur_len + 1]), None)
        hits = model._unflatten_beam_dim(hits, B, keep)
        cand = ((topk_running_beam_indices[:, :, cur_len - P] - offset).numpy().copy(), topk_running_sequences[:, :, cur_len].numpy().copy(),
                topk_log_probs.numpy().copy())
        running_sequences, running_beam_scores, running_beam_indices = model._get_running_beams_for_next_iteration(
            topk_log_probs=topk_log_probs, topk_running_sequences=topk_running_sequences, topk_running_beam_indices=topk_running_beam_indices,
            next_token_hits_stopping_criteria=hits, num_beams=K)
        sequences, beam_scores, beam_indices, is_sent_finished = model._update_finished_beams(
            sequences=sequences, topk_running_sequences=topk_running_sequences, beam_scores=beam_scores, topk_log_probs=topk_log_probs,
            beam_indices=beam_indices, topk_running_beam_indices=topk_running_beam_indices, is_early_stop_heuristic_unsatisfied=flag,
            is_sent_finished=is_sent_finished, next_token_hits_stopping_criteria=hits, top_num_beam_mask=top_mask, num_beams=K, cur_len=cur_len,
            decoder_prompt_len=P, length_penalty=length_penalty, early_stopping=False)
        run = ((running_beam_indices[:, :, cur_len - P] - offset).numpy().copy(), running_sequences[:, :, cur_len].numpy().copy(),
               running_beam_scores.numpy().copy())
        cur_len += 1
        flag = model._check_early_stop_heuristic(
            is_early_stop_heuristic_unsatisfied=flag, running_beam_scores=running_beam_scores, beam_scores=beam_scores,
            is_sent_finished=is_sent_finished, cur_len=cur_len, max_length=max_length, decoder_prompt_len=P, early_stopping=False,
            length_penalty=length_penalty)
        finished = not bool(model._beam_search_has_unfinished_sequences(flag, is_sent_finished, hits, False))
        steps.append(dict(logits=logits.numpy().copy(), cand=cand, run=run, flag=flag[:, 0].numpy().copy(),
                          finished=(beam_scores.numpy().copy(), is_sent_finished.numpy().copy(), sequences.numpy().copy(),
                                    beam_indices.numpy().copy())))
    best_idx = beam_indices[:, 0, :]
    lengths = P + ((best_idx + 1).bool()).sum(dim=1)                          # the hypothesis' own length (``_beam_search``'s crop, per row)
    return dict(sequences=[sequences[b, 0, : int(lengths[b])].tolist() for b in range(B)], scores=beam_scores[:, 0].numpy().copy(),
                stop_step=len(steps), steps=steps)


def rule_on(hf, b: int, K: int, V: int, spec, length_penalty: float, max_length: int) -> BR.Beam:
    """The rule fed HF's logits of utterance ``b``, for as long as the rule runs (a done utterance is frozen while HF's batch goes on)."""
    ban = np.zeros(V, dtype=bool)
    ban[list(spec.suppress_tokens)] = True
    ban1 = ban.copy()
    ban1[list(spec.begin_suppress_tokens)] = True
    bm = BR.Beam(K, V, spec.eos_token_id, spec.pad_token_id, P, max_length, length_penalty)
    for s, st in enumerate(hf["steps"]):
        bm.step(st["logits"][b * K: (b + 1) * K], P + s, ban1 if s == 0 else ban)
    return bm


def utterance_r(bm: BR.Beam) -> float:
    """the smallest gap / (step + 1) over every comparison that changed the rule's state, the final best-against-second included"""
    r = min([st["gap"] / (s + 1) for s, st in enumerate(bm.steps) if st is not None] + [np.inf])
    n = len([st for st in bm.steps if st is not None])
    return float(min(r, bm.final_gap() / max(n, 1)))


def greedy_of(model, spec, enc, max_length):
    import dataclasses
    seq, langs = G.hf_greedy(model, dataclasses.replace(spec, max_length=max_length), enc)
    return seq.numpy(), langs.numpy()


def search_seed(seed: int, pool: int = 40):
    """The best case of one decoder seed over K and max_length: (r, record) or (0, why)."""
    rec, why = G.case_a(seed)                                                 # the greedy fixture's own choice of eos and begin-suppress for this seed
    if rec is None:
        return 0.0, why
    model, spec = rec["model"], rec["spec"]
    V = G.GEO.decoder_vocab_size
    encs = torch.from_numpy(np.concatenate([R.enc_states(1000 + e, 1, G.GEO.max_source_positions, G.GEO.hidden) for e in range(pool)])).double()
    best = (0.0, "no case meets the structural conditions")
    for max_length in (12, 20):
        gseq, langs = greedy_of(model, spec, encs, max_length)
        for K in (2, 3):
            hf = hf_beam(model, spec, encs, langs, K, 1.0, max_length)
            beams = [rule_on(hf, b, K, V, spec, 1.0, max_length) for b in range(pool)]
            rs = np.array([utterance_r(bm) if bm.err == 0 else 0.0 for bm in beams])
            order = np.argsort(-rs)
            # the three of largest r that also meet the structural conditions together: try the top few combinations
            import itertools
            for pick in itertools.islice(itertools.combinations(order[:8].tolist(), 3), 56):
                bs = [beams[b] for b in pick]
                r = float(min(rs[list(pick)]))
                if r <= best[0]:
                    continue
                differs = any(gseq[b, : len(hf["sequences"][b])].tolist() != hf["sequences"][b] for b in pick)
                shared = any(len({q for (q, _), sc in zip(st["run"], st["run_scores"]) if np.isfinite(sc)}) < int(np.isfinite(st["run_scores"]).sum())
                             for bm in bs for st in bm.steps if st is not None)
                by_eos = any(bm.steps[h[0]]["cand"][h[1]][1] == spec.eos_token_id and P + h[0] + 1 < max_length for bm in bs for _, h in bm.finished)
                stops = sorted(bm.done_step for bm in bs)
                if differs and shared and by_eos and stops[-1] - stops[0] >= 3:
                    best = (r, dict(seed=seed, K=K, max_length=max_length, pick=list(pick), spec=spec, model=model, rec=rec, r=r))
    return best


def record(case) -> None:
    """Run HF on the three picked utterances alone (a batch of 3) and store it."""
    from interspeech_ser_amd.weights import state_dict_digest
    spec, model, K, max_length = case["spec"], case["model"], case["K"], case["max_length"]
    V = G.GEO.decoder_vocab_size
    enc_seeds = [1000 + e for e in case["pick"]]
    encs = torch.from_numpy(np.concatenate([R.enc_states(e, 1, G.GEO.max_source_positions, G.GEO.hidden) for e in enc_seeds])).double()
    gseq, langs = greedy_of(model, spec, encs, max_length)
    hf = hf_beam(model, spec, encs, langs, K, 1.0, max_length)
    beams = [rule_on(hf, b, K, V, spec, 1.0, max_length) for b in range(3)]
    r = min(utterance_r(bm) for bm in beams)
    n = hf["stop_step"]
    width = max(len(s) for s in hf["sequences"])
    seqs = np.full((3, width), spec.pad_token_id, dtype=np.int64)
    for b, s in enumerate(hf["sequences"]):
        seqs[b, : len(s)] = s
    np.savez_compressed(
        OUT, decoder_seed=np.array(case["seed"]), digest=state_dict_digest(case["rec"]["sd"]), enc_seeds=np.array(enc_seeds), K=np.array(K),
        max_length=np.array(max_length), length_penalty=np.array(1.0), eos=np.array(spec.eos_token_id),
        start=np.array(spec.decoder_start_token_id), pad=np.array(spec.pad_token_id), task=np.array(spec.task_id),
        no_timestamps=np.array(spec.no_timestamps_token_id), lang_ids=np.array(spec.lang_ids), suppress=np.array(spec.suppress_tokens),
        begin_suppress=np.array(spec.begin_suppress_tokens), languages=langs, greedy_sequences=gseq, r=np.array(r),
        sequences=seqs, lengths=np.array([len(s) for s in hf["sequences"]]), scores=hf["scores"], stop_step=np.array(n),
        done_steps=np.array([bm.done_step for bm in beams]),
        cand_parents=np.stack([st["cand"][0] for st in hf["steps"]]), cand_tokens=np.stack([st["cand"][1] for st in hf["steps"]]),
        cand_scores=np.stack([st["cand"][2] for st in hf["steps"]]),
        run_parents=np.stack([st["run"][0] for st in hf["steps"]]), run_tokens=np.stack([st["run"][1] for st in hf["steps"]]),
        run_scores=np.stack([st["run"][2] for st in hf["steps"]]),
        fin_scores=hf["steps"][-1]["finished"][0], fin_mask=hf["steps"][-1]["finished"][1], fin_sequences=hf["steps"][-1]["finished"][2],
        logits=np.stack([st["logits"] for st in hf["steps"]]).astype(np.float32))
    print(f"seed {case['seed']} K {K} max_length {max_length} utterances {enc_seeds}: r {r:.4e}; {os.path.getsize(OUT)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=300, help="decoder seeds 0 .. seeds - 1 are searched (at most 300)")
    ap.add_argument("--only", type=int, default=None, help="search this decoder seed alone")
    args = ap.parse_args()
    torch.set_num_threads(8)
    best = (0.0, None)
    for seed in (range(min(args.seeds, 300)) if args.only is None else [args.only]):
        r, case = search_seed(seed)
        print(f"seed {seed}: " + (f"r {r:.4e} K {case['K']} max_length {case['max_length']}" if r > 0 else str(case)), flush=True)
        if r > best[0]:
            best = (r, case)
    if best[1] is None:
        raise SystemExit("no decoder seed meets the conditions")
    record(best[1])


if __name__ == "__main__":
    main()
