"""Generate tests/golden/tiny_whisper_long_d128h2.npz: HF's long-form transcription (``generate`` on input over 30 s with
``return_timestamps=True``, greedy, every file given alone) on the tiny encoder + a tiny decoder with 1 501 timestamp tokens.  Run once on
the CPU; the output is committed.  TEST INFRASTRUCTURE ONLY (needs ``transformers``).

    python tools/make_whisper_longform_golden.py [--seeds 40] [--waves 12]

How HF is driven.  ``generate`` cannot be driven offline on a hand-made tiny config (tools/make_whisper_decoder_golden.py says why), so
``hf_long_form`` calls HF's own pieces in ``generate``'s order (generation_whisper.py:649-903) around the float64 model:
``WhisperFeatureExtractor(truncation=False, padding="longest")`` over the whole file, ``_retrieve_max_frames_and_seek``, then per window
``_maybe_reduce_batch``, the time offset, ``_get_input_segment``, the encoder, on the first window ``detect_language`` (later windows are
forced to it), per position the three logits processors of tools/make_whisper_segments_golden.py and the argmax, and
``_retrieve_segment``; the sequence is the concatenation of the segments' tokens.

The search.  Decoder seeds x ``ts_scale`` x seeded waves of 65 to 80 s (tests/whisper_long_ref.fixture_wave: noise whose level changes
every few seconds).  A main file is kept when it has at least 3 windows, one window ended by a closed pair whose advance is no multiple of
3000, one window consumed whole, a last window of fewer than 3000 frames, no zero advance, and every decided step (the language step
included) has margin and ts_gap >= 4 g, g = 1e-3 max(1, max|logits|); a second file of the same weights that meets the gate rides along
for the queue.  Stored: seeds, scalars, HF's windows, sequences, segments and languages, every decided row's margin and gap, and HF's
float64 logits of the main file's decided rows as fp32.  Asserted: the file is under 1 MiB, and the numpy rule (tests/whisper_seg_ref.py)
fed HF's logits gives HF's tokens.
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

from interspeech_ser_amd import config as C                                                     # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict                 # noqa: E402
import whisper_dec_ref as R                                                                     # noqa: E402
import whisper_long_ref as LR                                                                   # noqa: E402
import whisper_seg_ref as SR                                                                    # noqa: E402

GEO = LR.fixture_geo()
OUT = os.path.join(ROOT, "tests", "golden", LR.FIXTURE)
LANGS = {"<|en|>": 472, "<|de|>": 473, "<|fr|>": 474, "<|es|>": 475}
SCALES = (1.0, 0.75, 1.25, 0.5, 1.5)
P = SR.P


def hf_generation_config(spec):
    import transformers as tf
    return tf.GenerationConfig(decoder_start_token_id=LR.START, eos_token_id=LR.EOS, pad_token_id=LR.EOS, bos_token_id=LR.START,
                               suppress_tokens=list(spec.suppress_tokens), begin_suppress_tokens=list(spec.begin_suppress_tokens),
                               no_timestamps_token_id=LR.NO_TS, lang_to_id=dict(LANGS), task_to_id={"transcribe": LR.TASK, "translate": LR.TRANSLATE},
                               is_multilingual=True, max_length=spec.max_length, return_timestamps=True,
                               max_initial_timestamp_index=spec.max_initial_timestamp_index)


def hf_model(sd):
    import transformers as tf
    cfg = tf.WhisperConfig(num_mel_bins=GEO.n_mels, d_model=GEO.hidden, encoder_layers=GEO.num_layers, encoder_attention_heads=GEO.heads,
                           encoder_ffn_dim=GEO.ffn, decoder_layers=GEO.decoder_layers, decoder_attention_heads=GEO.decoder_attention_heads,
                           decoder_ffn_dim=GEO.decoder_ffn_dim, max_source_positions=GEO.max_source_positions,
                           max_target_positions=GEO.max_target_positions, vocab_size=GEO.decoder_vocab_size, pad_token_id=LR.EOS,
                           bos_token_id=LR.START, eos_token_id=LR.EOS, decoder_start_token_id=LR.START, activation_function="gelu")
    model = tf.WhisperForConditionalGeneration(cfg).eval()
    res = model.model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and not res.missing_keys, (res.unexpected_keys, res.missing_keys)
    model.tie_weights()
    assert model.proj_out.weight.data_ptr() == model.model.decoder.embed_tokens.weight.data_ptr()
    return model.double()


@torch.no_grad()
def hf_window(model, spec, gc, segment_input, language):
    """one window: (sequence [n] with the prompt, language, logits [n, V] float64 teacher-forced on that sequence)"""
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    from transformers.modeling_outputs import BaseModelOutput
    eo = BaseModelOutput(last_hidden_state=model.model.encoder(segment_input).last_hidden_state)
    if language is None:
        language = int(model.detect_language(encoder_outputs=eo, generation_config=gc)[0])
    ids = torch.tensor([[LR.START, language, LR.TASK]], dtype=torch.long)
    procs = [SuppressTokensAtBeginLogitsProcessor(list(spec.begin_suppress_tokens), begin_index=P),
             SuppressTokensLogitsProcessor(list(spec.suppress_tokens)), WhisperTimeStampLogitsProcessor(gc, begin_index=P)]
    assert procs[2].max_initial_timestamp_index == spec.max_initial_timestamp_index and procs[2].timestamp_begin == LR.TS_BEGIN
    while ids.shape[1] < spec.max_length:
        scores = model(encoder_outputs=eo, decoder_input_ids=ids, use_cache=False).logits[:, -1].clone()
        for p in procs:
            scores = p(ids, scores)
        nxt = scores.argmax(-1)
        ids = torch.cat([ids, nxt[:, None]], 1)
        if int(nxt[0]) == spec.eos_token_id:
            break
    logits = model(encoder_outputs=eo, decoder_input_ids=ids, use_cache=False).logits[0]
    return ids[0], language, logits.numpy()


@torch.no_grad()
def hf_long_form(model, spec, wave, max_windows=12):
    """HF's pieces in ``generate``'s order (module docstring) on one file.  Returns dict(windows [(seek, nf, advance)], rows (per window the
    sequence with its prompt), logits (per window [n, V]), language, segments [(start, end, ids)], sequence, seek); None when a window
    makes no progress or the loop does not end within ``max_windows``."""
    import transformers as tf
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    fe = tf.WhisperFeatureExtractor(feature_size=GEO.n_mels)
    feats = fe(wave, sampling_rate=16000, truncation=False, padding="longest", return_tensors="pt")["input_features"].double()
    F = feats.shape[-1]
    assert F == len(wave) // 160
    gc = hf_generation_config(spec)
    max_frames, seek = M._retrieve_max_frames_and_seek(batch_size=1, attention_mask=None, total_input_frames=F, is_shortform=False)
    cur_bsz, batch_idx_map = 1, [0]
    out = dict(windows=[], rows=[], logits=[], language=None, segments=[], frames=F)
    while (seek < max_frames).any():
        if len(out["windows"]) >= max_windows:
            return None
        feats, cur_bsz, batch_idx_map = M._maybe_reduce_batch(input_features=feats, seek=seek, max_frames=max_frames, cur_bsz=cur_bsz,
                                                              batch_idx_map=batch_idx_map)
        time_offset = seek.to(torch.float64) * 0.02 / 2
        seek_num_frames = (max_frames - seek).clamp(max=3000)
        seg_in = M._get_input_segment(input_features=feats, seek=seek, seek_num_frames=seek_num_frames, num_segment_frames=3000,
                                      cur_bsz=cur_bsz, batch_idx_map=batch_idx_map)
        row, lang, logits = hf_window(model, spec, gc, seg_in, out["language"])
        out["language"] = lang
        gen = row[P:].tolist()
        body = gen[: gen.index(spec.eos_token_id)] if spec.eos_token_id in gen else gen
        if not body:
            return None
        segs, off = M._retrieve_segment(seek_sequence=torch.tensor(body, dtype=torch.long), seek_outputs=[{}], time_offset=time_offset,
                                        timestamp_begin=LR.TS_BEGIN, seek_num_frames=seek_num_frames, time_precision=0.02,
                                        time_precision_features=0.01, input_stride=2, prev_idx=0, idx=0, return_token_timestamps=False,
                                        decoder_input_ids=torch.zeros((1, P), dtype=torch.long))
        out["windows"].append((int(seek[0]), int(seek_num_frames[0]), int(off)))
        out["rows"].append(row.numpy())
        out["logits"].append(logits)
        if int(off) <= 0:
            return None
        out["segments"] += [(float(s["start"]), float(s["end"]), [int(t) for t in s["tokens"]]) for s in segs]
        seek[0] += off
    out["sequence"] = [t for _, _, ids in out["segments"] for t in ids]
    out["seek"] = int(seek[0])
    return out


def analyse(spec, run):
    """per window the decided positions with the numpy rule on HF's logits: dict(ok, margins, gaps (per window arrays over positions
    P - 1 ..), lang_margin, zmax, kinds per window: 'pair' (a closed pair, partial advance), 'whole')"""
    m = R.masks(spec, LR.V)
    ok, zmax, margins, gaps, kinds = True, 0.0, [], [], []
    for k, (row, logits, (seek, nf, adv)) in enumerate(zip(run["rows"], run["logits"], run["windows"])):
        mg, gp = [], []
        for p in range(P - 1, len(row) - 1):
            z = logits[p]
            _, tok, a, b, _, _ = SR.rule(z, m[1 if p == P - 1 else 0], row[P: p + 1], LR.TS_BEGIN, LR.NO_TS, LR.EOS, spec.max_initial_timestamp_index)
            ok &= tok == int(row[p + 1])
            mg.append(a)
            gp.append(b)
            zmax = max(zmax, float(np.abs(z).max()))
        margins.append(np.array(mg))
        gaps.append(np.array(gp))
        body = [t for t in row[P:].tolist() if t != LR.EOS]
        ts = [t >= LR.TS_BEGIN for t in body]
        pair = any(ts[i] and ts[i + 1] for i in range(len(body) - 1))
        kinds.append("pair" if pair and ts[-2:] != [False, True] else "whole")
    z0 = run["logits"][0][0]
    lang_margin = R.top2_margin(z0 + m[2])
    zmax = max(zmax, float(np.abs(z0).max()))
    return dict(ok=bool(ok), margins=margins, gaps=gaps, kinds=kinds, lang_margin=lang_margin, zmax=zmax)


def gate(info):
    g = 1e-3 * max(1.0, info["zmax"])
    worst = min([info["lang_margin"]] + [float(a.min()) for a in info["margins"]] + [float(b.min()) for b in info["gaps"]])
    return g, worst


def wanted(run, info):
    w = run["windows"]
    return (len(w) >= 3 and any(k == "pair" and adv % 3000 != 0 for k, (_, _, adv) in zip(info["kinds"], w))
            and any(adv == nf for _, nf, adv in w) and w[-1][1] < 3000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40, help="decoder seeds 0 .. seeds - 1 are searched")
    ap.add_argument("--waves", type=int, default=12, help="waves per (seed, ts_scale)")
    ap.add_argument("--out", type=str, default=OUT)
    ap.add_argument("--only", type=int, default=None, help="search this decoder seed alone")
    args = ap.parse_args()
    torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "8")))
    spec = LR.fixture_spec()
    enc_sd = synthetic_state_dict(C.TINY_WHISPER, LR.ENCODER_WEIGHT_SEED)
    rng = np.random.default_rng(2024)
    pool = [(5000 + j, int(16000 * rng.uniform(65.0, 80.0)) + int(rng.integers(1, 160))) for j in range(args.waves)]
    for seed in (range(args.seeds) if args.only is None else [args.only]):
        for scale in SCALES:
            dec_sd = SR.fixture_state_dict(GEO, seed, LR.TS_BEGIN, scale)
            sd = dict(enc_sd)
            sd.update(dec_sd)
            model = hf_model(sd)
            good, main_file = [], None
            for wseed, n in pool:
                run = hf_long_form(model, spec, LR.fixture_wave(wseed, n))
                if run is None:
                    continue
                info = analyse(spec, run)
                g, worst = gate(info)
                if not info["ok"] or worst < 4 * g:
                    continue
                if main_file is None and wanted(run, info):
                    main_file = (wseed, n, run, info)
                else:
                    good.append((wseed, n, run, info))
                if main_file is not None and good:
                    break
            print(f"seed {seed} ts_scale {scale}: main {'found' if main_file else 'none'}, {len(good)} further files pass the gate"
                  + "".join(f"; {f[2]['windows']}" for f in good[:3]), flush=True)
            if main_file is None or not good:
                continue
            both = [main_file, good[0]]
            if min(gate(f[3])[1] for f in both) < 4e-3 * max(1.0, max(f[3]["zmax"] for f in both)):
                continue                                    # the gate of the two files together: the larger g
            record(seed, scale, dec_sd, spec, both, args.out)
            return
    raise SystemExit("no (decoder seed, ts_scale) meets the conditions")


def record(seed, scale, dec_sd, spec, files, out=OUT):
    zmax = max(f[3]["zmax"] for f in files)
    g = 1e-3 * max(1.0, zmax)
    store = {}
    for i, (wseed, n, run, info) in enumerate(files):
        assert info["ok"], "the numpy rule does not give HF's tokens"
        assert gate(info)[1] >= 4 * g, (g, gate(info))
        width = max(len(r) for r in run["rows"])
        rows = np.full((len(run["rows"]), width), -1, dtype=np.int64)
        for k, r in enumerate(run["rows"]):
            rows[k, : len(r)] = r
        store[f"f{i}_windows"] = np.array(run["windows"], dtype=np.int64)
        store[f"f{i}_rows"] = rows
        store[f"f{i}_language"] = np.array(run["language"])
        store[f"f{i}_sequence"] = np.array(run["sequence"], dtype=np.int64)
        store[f"f{i}_seek"] = np.array(run["seek"])
        store[f"f{i}_seg_times"] = np.array([(a, b) for a, b, _ in run["segments"]], dtype=np.float64)
        store[f"f{i}_seg_lens"] = np.array([len(t) for _, _, t in run["segments"]], dtype=np.int64)
        store[f"f{i}_margins"] = np.concatenate(info["margins"])
        store[f"f{i}_gaps"] = np.concatenate(info["gaps"])
        store[f"f{i}_lang_margin"] = np.array(info["lang_margin"])
    run, info = files[0][2], files[0][3]
    assert wanted(run, info)
    store["f0_logits"] = np.concatenate([lg[P - 1: len(r) - 1] for lg, r in zip(run["logits"], run["rows"])]).astype(np.float32)
    store["f0_lang_logits"] = run["logits"][0][0].astype(np.float32)
    np.savez_compressed(out, decoder_seed=np.array(seed), ts_scale=np.array(scale), digest=state_dict_digest(dec_sd),
                        encoder_seed=np.array(LR.ENCODER_WEIGHT_SEED), wave_seeds=np.array([f[0] for f in files]),
                        wave_lengths=np.array([f[1] for f in files]), g=np.array(g),
                        min_margin=np.array(min(gate(f[3])[1] for f in files)), **store)
    size = os.path.getsize(out)
    assert size < 1024 * 1024, size
    print(f"seed {seed} ts_scale {scale}: g {g:.3e}, smallest margin / gap {min(gate(f[3])[1] for f in files):.3e}")
    for wseed, n, run, info in files:
        print(f"  wave {wseed} ({n} samples, {run['frames']} frames): windows {run['windows']} kinds {info['kinds']} language {run['language']}")
    print(f"  {size} bytes")


if __name__ == "__main__":
    main()
