"""Generate tests/golden/tiny_whisper_score_d128h2.npz: HF's long-form transcription WITH its thresholds (``logprob_threshold``,
``no_speech_threshold``: the skip of a silent window) on the tiny encoder + the tiny decoder of the long-form fixture.  Run once on the
CPU; the output is committed.  TEST INFRASTRUCTURE ONLY (needs ``transformers``).

    python tools/make_whisper_scores_golden.py [--start 0] [--seeds 40] [--waves 12]

How HF is driven.  tools/make_whisper_longform_golden.py's way -- HF's own pieces in ``generate``'s order around the float64 model -- with
what the thresholds add: ``WhisperNoSpeechDetection`` in front of the three logits processors (its forward over the whole prompt is the
float64 model itself), the processed scores of every step kept as ``generate(output_scores=True)`` keeps them, and per window
``_need_fallback`` itself -- which calls ``_retrieve_avg_logprobs`` and reads the detector -- on the sequence with its closing eos; a
window it marks ``should_skip`` advances the seek by its whole ``seek_num_frames`` and retrieves nothing (generation_whisper.py's seek
loop).  One temperature: ``needs_fallback`` is recorded and acts on nothing.

The search.  Decoder seeds x ``ts_scale`` x seeded waves (the long-form fixture's own first).  A file is first run without thresholds; then
thresholds are chosen FROM ITS DATA, halfway between neighbouring windows' values, so that a middle window is skipped, and the file is run
again with them.  A main file is kept when that second run has at least three windows, a skipped middle window and a kept one, and
  * every decided step has margin and ts_gap >= 4 g, g = 1e-3 max(1, max|logits|) (the existing gate),
  * every window's average log-probability lies at least 4 x 2 g from ``logprob_threshold`` and its no-speech probability at least
    4 x expm1(2 g) from ``no_speech_threshold`` relatively: a log-softmax moves by at most twice the largest logit error.
A second file of the same weights that meets the gates under the same thresholds rides along for the queue.  Stored: seeds, thresholds,
HF's windows, skip and fallback decisions, sequences, segments, languages, and per window HF's average (fp32 log-softmax inside HF), the
float64 log-probability of every generated token and the no-speech probability.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from interspeech_ser_amd import config as C                                                     # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict                 # noqa: E402
import make_whisper_longform_golden as LG                                                       # noqa: E402
import whisper_long_ref as LR                                                                   # noqa: E402
import whisper_seg_ref as SR                                                                    # noqa: E402

FIXTURE = "tiny_whisper_score_d128h2.npz"
OUT = os.path.join(ROOT, "tests", "golden", FIXTURE)
P = SR.P
NO_SPEECH = LR.NO_TS - 1


@torch.no_grad()
def hf_scored_window(model, spec, gc, segment_input, language):
    """one window: (sequence with the prompt, language, teacher-forced logits [n, V], the processed scores of every generated step, the
    detector)"""
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperNoSpeechDetection, WhisperTimeStampLogitsProcessor)
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=model.model.encoder(segment_input).last_hidden_state)
    if language is None:
        language = int(model.detect_language(encoder_outputs=eo, generation_config=gc)[0])
    ids = torch.tensor([[LR.START, language, LR.TASK]], dtype=torch.long)
    det = WhisperNoSpeechDetection(no_speech_token=gc.no_timestamps_token_id - 1, begin_index=P, scores_is_logprobs=False)
    det.model = lambda **kw: model(encoder_outputs=eo, decoder_input_ids=ids[:, :P], use_cache=False)   # its forward over the whole prompt
    det.inputs = {}
    procs = [det, SuppressTokensAtBeginLogitsProcessor(list(spec.begin_suppress_tokens), begin_index=P),
             SuppressTokensLogitsProcessor(list(spec.suppress_tokens)), WhisperTimeStampLogitsProcessor(gc, begin_index=P)]
    kept = []
    while ids.shape[1] < spec.max_length:
        scores = model(encoder_outputs=eo, decoder_input_ids=ids, use_cache=False).logits[:, -1].clone()
        for p in procs:
            scores = p(ids, scores)
        kept.append(scores)
        nxt = scores.argmax(-1)
        ids = torch.cat([ids, nxt[:, None]], 1)
        if int(nxt[0]) == spec.eos_token_id:
            break
    logits = model(encoder_outputs=eo, decoder_input_ids=ids, use_cache=False).logits[0]
    return ids[0], language, logits.numpy(), tuple(s[0] for s in kept), det     # per item [V] rows, as _postprocess_outputs splits them


@torch.no_grad()
def hf_long_form_scored(model, spec, wave, limits, max_windows=12):
    """HF's pieces in ``generate``'s order on one file under ``limits`` (dict of the three thresholds, None = absent).  Returns LG.hf_long_form's
    dict plus per window: skipped, needs_fallback, avg (HF's own), ns (the detector's), logprobs (float64, per generated token);
    None when a kept window makes no progress or the loop does not end."""
    import transformers as tf
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    fe = tf.WhisperFeatureExtractor(feature_size=LG.GEO.n_mels)
    feats = fe(wave, sampling_rate=16000, truncation=False, padding="longest", return_tensors="pt")["input_features"].double()
    F = feats.shape[-1]
    gc = LG.hf_generation_config(spec)
    for k, v in limits.items():
        setattr(gc, k, v)
    me = types.SimpleNamespace(_retrieve_compression_ratio=M._retrieve_compression_ratio, _retrieve_avg_logprobs=M._retrieve_avg_logprobs)
    max_frames, seek = M._retrieve_max_frames_and_seek(batch_size=1, attention_mask=None, total_input_frames=F, is_shortform=False)
    cur_bsz, batch_idx_map = 1, [0]
    out = dict(windows=[], rows=[], logits=[], language=None, segments=[], frames=F, skipped=[], needs_fallback=[], avg=[], ns=[], logprobs=[])
    while (seek < max_frames).any():
        if len(out["windows"]) >= max_windows:
            return None
        feats, cur_bsz, batch_idx_map = M._maybe_reduce_batch(input_features=feats, seek=seek, max_frames=max_frames, cur_bsz=cur_bsz,
                                                              batch_idx_map=batch_idx_map)
        time_offset = seek.to(torch.float64) * 0.02 / 2
        seek_num_frames = (max_frames - seek).clamp(max=3000)
        seg_in = M._get_input_segment(input_features=feats, seek=seek, seek_num_frames=seek_num_frames, num_segment_frames=3000,
                                      cur_bsz=cur_bsz, batch_idx_map=batch_idx_map)
        row, lang, logits, scores, det = hf_scored_window(model, spec, gc, seg_in, out["language"])
        out["language"] = lang
        seq = row[P:]                                                          # the closing eos stays: _need_fallback counts it
        tokens = seq.tolist()
        lp = torch.log_softmax(torch.stack(scores), dim=-1)                      # float64 [n, V]
        out["logprobs"].append(np.array([float(lp[i, t]) for i, t in enumerate(tokens)]))
        out["avg"].append(float(M._retrieve_avg_logprobs(scores, seq, 0.0)))
        out["ns"].append(float(det.no_speech_prob[0]))
        if limits.get("logprob_threshold") is None and limits.get("no_speech_threshold") is None and limits.get("compression_ratio_threshold") is None:
            needs, skip = False, False
        else:
            needs, skip = M._need_fallback(me, seq, [{"scores": scores}], 0, [det], gc, LR.V, 0.0)
        out["needs_fallback"].append(bool(needs))
        out["skipped"].append(bool(skip))
        out["rows"].append(row.numpy())
        out["logits"].append(logits)
        if skip:
            out["windows"].append((int(seek[0]), int(seek_num_frames[0]), int(seek_num_frames[0])))
            seek[0] += seek_num_frames[0]
            continue
        body = tokens[: tokens.index(spec.eos_token_id)] if spec.eos_token_id in tokens else tokens
        if not body:
            return None
        segs, off = M._retrieve_segment(seek_sequence=torch.tensor(body, dtype=torch.long), seek_outputs=[{}], time_offset=time_offset,
                                        timestamp_begin=LR.TS_BEGIN, seek_num_frames=seek_num_frames, time_precision=0.02,
                                        time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0, return_token_timestamps=False,
                                        decoder_input_ids=torch.zeros((1, P), dtype=torch.long))
        out["windows"].append((int(seek[0]), int(seek_num_frames[0]), int(off)))
        if int(off) <= 0:
            return None
        out["segments"] += [(float(s["start"]), float(s["end"]), [int(t) for t in s["tokens"]]) for s in segs]
        seek[0] += off
    out["sequence"] = [t for _, _, ids in out["segments"] for t in ids]
    out["seek"] = int(seek[0])
    return out


def score_gate(run, limits, g):
    """the smallest distance of a window's scores from the thresholds, in units of the gate (>= 4 wanted)"""
    lt, nt = limits["logprob_threshold"], limits["no_speech_threshold"]
    a = min(abs(v - lt) for v in run["avg"]) / (2.0 * g)
    b = min(abs(v / nt - 1.0) for v in run["ns"]) / math.expm1(2.0 * g)
    return min(a, b)


def choose_limits(run):
    """candidate thresholds from a file's own windows: for every middle window j, a logprob_threshold halfway between its average and the
    next higher one and a no_speech_threshold halfway between its probability and the next lower one"""
    out = []
    n = len(run["windows"])
    for j in range(1, n - 1):
        above = [v for v in run["avg"] if v > run["avg"][j]]
        below = [v for v in run["ns"] if v < run["ns"][j]]
        if not above:
            continue
        out.append(dict(logprob_threshold=0.5 * (run["avg"][j] + min(above)),
                        no_speech_threshold=0.5 * (run["ns"][j] + max(below)) if below else 0.5 * run["ns"][j], compression_ratio_threshold=None))
    return out


def passes(spec, run, limits):
    if run is None:
        return None
    info = LG.analyse(spec, run)
    g, worst = LG.gate(info)
    if not info["ok"] or worst < 4 * g or score_gate(run, limits, g) < 4.0:
        return None
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40, help="decoder seeds start .. seeds - 1 are searched")
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--waves", type=int, default=12)
    ap.add_argument("--out", type=str, default=OUT)
    args = ap.parse_args()
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "8")))
    spec = LR.fixture_spec()
    enc_sd = synthetic_state_dict(C.TINY_WHISPER, LR.ENCODER_WEIGHT_SEED)
    long_gold = np.load(os.path.join(ROOT, "tests", "golden", LR.FIXTURE))
    rng = np.random.default_rng(2024)
    pool = [(int(s), int(n)) for s, n in zip(long_gold["wave_seeds"], long_gold["wave_lengths"])]
    pool += [(5000 + j, int(16000 * rng.uniform(65.0, 80.0)) + int(rng.integers(1, 160))) for j in range(args.waves)]
    pool += [(6000 + j, int(16000 * rng.uniform(95.0, 125.0)) + int(rng.integers(1, 160))) for j in range(args.waves)]     # four and five windows
    tries = [(int(long_gold["decoder_seed"]), float(long_gold["ts_scale"]))] + [(s, sc) for s in range(args.start, args.seeds) for sc in LG.SCALES]
    none = dict(logprob_threshold=None, no_speech_threshold=None, compression_ratio_threshold=None)
    for seed, scale in tries:
        dec_sd = SR.fixture_state_dict(LG.GEO, seed, LR.TS_BEGIN, scale)
        sd = dict(enc_sd)
        sd.update(dec_sd)
        model = LG.hf_model(sd)
        first = {}
        for wseed, n in pool:
            run = hf_long_form_scored(model, spec, LR.fixture_wave(wseed, n), none)
            if run is not None and len(run["windows"]) >= 3:
                first[(wseed, n)] = run
        print(f"seed {seed} ts_scale {scale}: {len(first)} files of three windows or more", flush=True)
        for (wseed, n), run in first.items():
            for limits in choose_limits(run):
                main_run = hf_long_form_scored(model, spec, LR.fixture_wave(wseed, n), limits)
                info = passes(spec, main_run, limits)
                if info is None:
                    continue
                sk = main_run["skipped"]
                if len(sk) < 3 or not any(sk[1:-1]) or all(sk):
                    continue
                for (wseed2, n2) in pool:
                    if (wseed2, n2) == (wseed, n):
                        continue
                    other = hf_long_form_scored(model, spec, LR.fixture_wave(wseed2, n2), limits)
                    info2 = passes(spec, other, limits)
                    if info2 is None:
                        continue
                    files = [(wseed, n, main_run, info), (wseed2, n2, other, info2)]
                    g = 1e-3 * max(1.0, max(f[3]["zmax"] for f in files))
                    if min(LG.gate(f[3])[1] for f in files) < 4 * g or min(score_gate(f[2], limits, g) for f in files) < 4.0:
                        continue
                    record(seed, scale, dec_sd, limits, files, g, args.out)
                    return
    raise SystemExit("no (decoder seed, ts_scale, file, thresholds) meets the conditions")


def record(seed, scale, dec_sd, limits, files, g, out=OUT):
    store = {}
    for i, (wseed, n, run, info) in enumerate(files):
        width = max(len(r) for r in run["rows"])
        rows = np.full((len(run["rows"]), width), -1, dtype=np.int64)
        for k, r in enumerate(run["rows"]):
            rows[k, : len(r)] = r
        store[f"f{i}_windows"] = np.array(run["windows"], dtype=np.int64)
        store[f"f{i}_rows"] = rows
        store[f"f{i}_skipped"] = np.array(run["skipped"])
        store[f"f{i}_needs_fallback"] = np.array(run["needs_fallback"])
        store[f"f{i}_avg_logprob"] = np.array(run["avg"], dtype=np.float64)
        store[f"f{i}_no_speech_prob"] = np.array(run["ns"], dtype=np.float64)
        store[f"f{i}_token_logprobs"] = np.concatenate(run["logprobs"])
        store[f"f{i}_language"] = np.array(run["language"])
        store[f"f{i}_sequence"] = np.array(run["sequence"], dtype=np.int64)
        store[f"f{i}_seek"] = np.array(run["seek"])
        store[f"f{i}_seg_times"] = np.array([(a, b) for a, b, _ in run["segments"]], dtype=np.float64).reshape(-1, 2)
        store[f"f{i}_seg_lens"] = np.array([len(t) for _, _, t in run["segments"]], dtype=np.int64)
        store[f"f{i}_margins"] = np.concatenate(info["margins"])
        store[f"f{i}_gaps"] = np.concatenate(info["gaps"])
        store[f"f{i}_lang_margin"] = np.array(info["lang_margin"])
    np.savez_compressed(out, decoder_seed=np.array(seed), ts_scale=np.array(scale), digest=state_dict_digest(dec_sd),
                        encoder_seed=np.array(LR.ENCODER_WEIGHT_SEED), wave_seeds=np.array([f[0] for f in files]),
                        wave_lengths=np.array([f[1] for f in files]), g=np.array(g),
                        logprob_threshold=np.array(limits["logprob_threshold"]), no_speech_threshold=np.array(limits["no_speech_threshold"]),
                        no_speech_token=np.array(NO_SPEECH), min_margin=np.array(min(LG.gate(f[3])[1] for f in files)),
                        score_gate=np.array(min(score_gate(f[2], limits, g) for f in files)), **store)
    size = os.path.getsize(out)
    assert size < 1024 * 1024, size
    print(f"seed {seed} ts_scale {scale}: g {g:.3e}, thresholds {limits}, smallest margin / gap {min(LG.gate(f[3])[1] for f in files):.3e}, "
          f"score distance / gate {min(score_gate(f[2], limits, g) for f in files):.2f}")
    for wseed, n, run, info in files:
        print(f"  wave {wseed} ({n} samples): windows {run['windows']} skipped {run['skipped']} fallback {run['needs_fallback']} "
              f"avg {np.round(run['avg'], 4).tolist()} no_speech {np.round(run['ns'], 5).tolist()}")
    print(f"  {size} bytes")


if __name__ == "__main__":
    main()
