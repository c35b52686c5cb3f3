"""Writes tests/golden/tiny_ctc_<family>.npz (CPU, needs `transformers`): the HF CTC classes (*ForCTC) on seeded weights.

TEST INFRASTRUCTURE ONLY.  Per fixture: the class's config as JSON text, a preprocessor_config, the encoder's weights as the seed and digest
of weights.synthetic_state_dict (tests/ctc_ref.py rebuilds the full state dict under HF names), lm_head drawn from N(0, 0.5) with 2 added
to the blank's bias -- random weights almost never repeat a token or emit the blank otherwise --, four waveforms as seeds and lengths,
three ragged ones up to 1 s and the shortest the stem admits (one frame); and per waveform HF's logits at batch size 1 without padding
and without an attention mask, the model in .double(), their argmax per frame, and what Wav2Vec2CTCTokenizer.decode(...,
output_char_offsets=True) makes of those ids: the collapsed ids and the char offsets in frames.

The head's seed is SEARCHED, upwards from the case's first, until
  (a) every frame's float64 margin top1 - top2 is at least 4 g, g = 1e-3 * max(1, max|logits|) over the fixture: a device whose logits are
      within g of HF's (the project's gate) then cannot choose another token, so the tests compare every frame's token; and
  (b) the fixture holds at least 3 blank frames and at least 3 repeated non-blank frames, so that both collapse rules are exercised.
The hidden states do not depend on the head, so the search costs one encoder forward per waveform and a matrix product per seed.

Three geometries; V = 12 (the GEMM's padding columns exist) with the blank first, in the middle and last.

    python tools/make_golden_ctc.py
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict  # noqa: E402
import ctc_ref as R                                                               # noqa: E402
from make_golden_audio_cls import front_end                                      # noqa: E402
from make_golden_xvector import length_with_frames                               # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
RAGGED = (16000, 12345, 6007)
MAX_SEEDS = 400
# tag, geometry, encoder seed, first head seed, vocab_size, blank
CASES = (
    ("tiny_ctc_wavlm", C.TINY_WAVLM, 61, 6100, 12, 0),
    ("tiny_ctc_wavlm_base", C.TINY_WAVLM_BASE, 62, 6200, 12, 5),
    ("tiny_ctc_w2v_bert", C.TINY_W2V_BERT, 63, 6300, 12, 11),
)


def hf_model(geo, V, blank):
    import transformers as tf
    head = dict(vocab_size=V, pad_token_id=blank, add_adapter=False)
    if geo.family == C.FAMILY_W2V_BERT:
        cfg = tf.Wav2Vec2BertConfig(
            hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
            feature_projection_input_dim=geo.fbank_dim, conv_depthwise_kernel_size=geo.conv_depthwise_kernel,
            left_max_position_embeddings=geo.left_max_positions, right_max_position_embeddings=geo.right_max_positions,
            layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False, **head)
        return tf.Wav2Vec2BertForCTC(cfg).eval()
    assert geo.family == C.FAMILY_WAVLM
    common = dict(hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                  intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel),
                  conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias, feat_extract_norm=geo.feat_extract_norm,
                  do_stable_layer_norm=geo.stable_layer_norm, num_conv_pos_embeddings=geo.pos_conv_kernel,
                  num_conv_pos_embedding_groups=geo.pos_conv_groups, layer_norm_eps=geo.layer_norm_eps,
                  hidden_act="gelu", feat_extract_activation="gelu", apply_spec_augment=False, **head)
    return tf.WavLMForCTC(tf.WavLMConfig(num_buckets=geo.num_buckets, max_bucket_distance=geo.max_bucket_distance, **common)).eval()


def draw_head(D: int, V: int, blank: int, seed: int) -> dict:
    g = np.random.default_rng(seed)
    w = (g.standard_normal((V, D)) * 0.5).astype(np.float32)
    b = (g.standard_normal(V) * 0.5).astype(np.float32)
    b[blank] += np.float32(2.0)
    return {"lm_head.weight": w, "lm_head.bias": b}


def conditions(logits, blank: int):
    """(smallest margin / g, blank frames, repeated non-blank frames) over a fixture's list of float64 logits"""
    g = max(R.gate(l) for l in logits)
    worst = min(float(R.margins64(l).min()) for l in logits if l.shape[0])
    blanks = repeats = 0
    for l in logits:
        ids = np.argmax(l, axis=1)
        blanks += int((ids == blank).sum())
        repeats += int(((ids[1:] == ids[:-1]) & (ids[1:] != blank)).sum())
    return worst / g, blanks, repeats


def hf_tokenizer(V: int, blank: int, tmp: str):
    import transformers as tf
    path = os.path.join(tmp, "vocab.json")
    with open(path, "w") as f:
        json.dump(R.tiny_vocab(V, blank), f)
    return tf.Wav2Vec2CTCTokenizer(path)


def make_case(tag, geo, seed, head_seed0, V, blank):
    torch.manual_seed(0)
    model = hf_model(geo, V, blank)
    enc = synthetic_state_dict(geo, seed)
    fe, pre = front_end(geo)
    lengths = RAGGED + (length_with_frames(geo, 1),)
    wave_seeds = [9000 + 10 * seed + j for j in range(len(lengths))]
    cfg = model.config.to_dict()
    cfg["architectures"] = [type(model).__name__]
    sd = {R.WRAPPER[geo.family] + k: v for k, v in enc.items()}
    res = model.float().load_state_dict(sd, strict=False)
    extra = [k for k in res.missing_keys if "masked_spec_embed" not in k and not k.startswith("lm_head.")]
    assert not res.unexpected_keys and not extra, res
    model.double()
    feeds, hidden = [], []
    for ws, ln in zip(wave_seeds, lengths):
        inputs = fe(R.synth_wave(ws, ln), sampling_rate=16000, return_tensors="pt")
        if geo.family == C.FAMILY_W2V_BERT:              # batch size 1 without padding: the frames the mask keeps, and no mask
            inputs = {"input_features": inputs["input_features"][:, inputs["attention_mask"][0].bool()]}
        else:
            inputs = {"input_values": inputs["input_values"]}
        inputs = {k: v.double() for k, v in inputs.items()}
        with torch.no_grad():
            out = model(**inputs, output_hidden_states=True)
        hs = out.hidden_states[-1][0].numpy()
        assert hs.shape == (geo.frames_for(ln), geo.hidden), (hs.shape, geo.frames_for(ln))
        feeds.append(inputs)
        hidden.append(hs)
    assert hidden[-1].shape[0] == 1
    met = 0
    for head_seed in range(head_seed0, head_seed0 + MAX_SEEDS):
        head = draw_head(geo.hidden, V, blank, head_seed)
        w, b = head["lm_head.weight"].astype(np.float64), head["lm_head.bias"].astype(np.float64)
        ratio, blanks, repeats = conditions([h @ w.T + b for h in hidden], blank)
        met += ratio >= 4.0
        if ratio >= 4.0 and blanks >= 3 and repeats >= 3:
            break
    else:
        raise SystemExit(f"{tag}: no head seed in {head_seed0}..{head_seed0 + MAX_SEEDS - 1} meets the margin and collapse conditions")
    model.float().load_state_dict({k: torch.from_numpy(v) for k, v in head.items()}, strict=False)
    model.double()
    rec = {"config": np.array(json.dumps(cfg, sort_keys=True)), "preprocessor": np.array(json.dumps(pre, sort_keys=True)),
           "seed": np.array(seed), "head_seed": np.array(head_seed), "digest": np.array(state_dict_digest(enc)),
           "lengths": np.array(lengths, dtype=np.int64), "wave_seeds": np.array(wave_seeds, dtype=np.int64)}
    rec.update({"head." + k: v for k, v in head.items()})
    logits = []
    with tempfile.TemporaryDirectory() as tmp:
        tok = hf_tokenizer(V, blank, tmp)
        assert tok.pad_token_id == blank
        for j, inputs in enumerate(feeds):
            with torch.no_grad():
                z = model(**inputs).logits[0]
            fid = torch.argmax(z, dim=-1)
            dec = tok.decode(fid, output_char_offsets=True)
            offs = [(int(o["start_offset"]), int(o["end_offset"])) for o in dec.char_offsets]
            ids = [int(fid[s]) for s, _ in offs]                      # the id of each kept group: the token at its first frame
            assert np.abs(z.numpy() - (hidden[j] @ w.T + b)).max() < 1e-9
            logits.append(z.numpy())
            rec[f"logits64_{j}"], rec[f"frame_ids_{j}"] = z.numpy(), fid.numpy().astype(np.int32)
            rec[f"ids_{j}"], rec[f"offsets_{j}"] = np.array(ids, dtype=np.int32), np.array(offs, dtype=np.int32).reshape(-1, 2)
    ratio, blanks, repeats = conditions(logits, blank)
    assert ratio >= 4.0 and blanks >= 3 and repeats >= 3
    print(f"{tag}: lengths {lengths}, head seed {head_seed} ({head_seed - head_seed0 + 1} tried, {met} met the margin rule), smallest margin "
          f"{ratio:.2f} g, {blanks} blank frames, {repeats} repeated frames, {sum(len(rec[f'ids_{j}']) for j in range(len(lengths)))} tokens")
    return rec


def main(out_dir: str = OUT) -> None:
    torch.set_num_threads(1)           # one summation order for the CPU convolutions: regenerating gives the same arrays
    for case in CASES:
        rec = make_case(*case)
        path = os.path.join(out_dir, case[0] + ".npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
