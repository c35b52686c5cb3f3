"""Writes tests/golden/tiny_cls_<family>.npz (CPU, needs `transformers`): the HF audio-classification classes on seeded weights.

TEST INFRASTRUCTURE ONLY.  Per fixture: the class's config as JSON text, a preprocessor_config, the encoder's weights as the seed and digest
of weights.synthetic_state_dict (the tensors themselves would not fit the 1 MiB a committed file may have; tests/audio_cls_ref.py rebuilds
the full state dict under HF names), the five head tensors -- layer_weights, projector and classifier redrawn from a normal distribution,
because the default init makes the layer weights uniform and the logits tiny --, three waveforms (16 000 samples, 23 457 samples, the
family's shortest legal input) as seeds, and per waveform HF's logits at batch size 1 in fp32 and, with the model in .double(), in float64,
with the float64 hidden states (Whisper: their mean over the 1 500 rows and max|hs|).

The head's seed is the first for which the fixture has the property the GPU test relies on: for at least two of the three waveforms HF's
top-two margin exceeds twice the logit bound of the f16x and fp32x modes (eps 1e-3, tests/test_gpu_audio_cls.py; the bf16 bound, eps 3e-2, is wider than any margin here).

    python tools/make_golden_audio_cls.py [output directory [one fixture's tag]]
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict  # noqa: E402
import audio_cls_ref as R                                                         # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
EPS = (1e-3,)
EMOTIONS = ("angry", "happy", "neutral", "sad", "surprised")
TINY_WAV2VEC2_H3 = C.tiny_geometry(C.FAMILY_WAV2VEC2, hidden=192, heads=3, ffn=256, pos_groups=3)
# tag, geometry, encoder seed, use_weighted_layer_sum, classifier_proj_size, labels (None: LABEL_i), shortest input
CASES = (
    ("tiny_cls_wavlm", C.TINY_WAVLM, 41, True, 48, EMOTIONS, 400),
    ("tiny_cls_wav2vec2", TINY_WAV2VEC2_H3, 42, False, 256, 3, 400),
    ("tiny_cls_wavlm_base", C.TINY_WAVLM_BASE, 43, True, 64, 4, 400),
    ("tiny_cls_w2v_bert", C.TINY_W2V_BERT, 44, True, 32, 130, 560),
    ("tiny_cls_whisper", C.TINY_WHISPER, 45, True, 40, 1, 400),
    ("tiny_cls_w2v_conformer", C.TINY_W2V_CONFORMER_ROPE, 46, True, 48, EMOTIONS, 400),
)
# the prefix the HF class puts in front of its encoder's parameter names (tests/audio_cls_ref.py's, and the conformer family's)
WRAPPER = dict(R.WRAPPER, **{C.FAMILY_W2V_CONFORMER: "wav2vec2_conformer."})


def hf_model(geo, weighted: bool, proj: int, labels):
    import transformers as tf
    n = len(labels) if not isinstance(labels, int) else labels
    head = dict(use_weighted_layer_sum=weighted, classifier_proj_size=proj, num_labels=n)
    if not isinstance(labels, int):
        head.update(id2label={i: l for i, l in enumerate(labels)}, label2id={l: i for i, l in enumerate(labels)})
    if geo.family == C.FAMILY_WHISPER:
        cfg = tf.WhisperConfig(d_model=geo.hidden, encoder_layers=geo.num_layers, encoder_attention_heads=geo.heads, encoder_ffn_dim=geo.ffn,
                               num_mel_bins=geo.n_mels, max_source_positions=geo.max_source_positions, decoder_layers=1,
                               decoder_attention_heads=geo.heads, decoder_ffn_dim=64, vocab_size=64, max_target_positions=16,
                               pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1, apply_spec_augment=False, **head)
        return tf.WhisperForAudioClassification(cfg).eval()
    if geo.family == C.FAMILY_W2V_BERT:
        cfg = tf.Wav2Vec2BertConfig(
            hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
            feature_projection_input_dim=geo.fbank_dim, conv_depthwise_kernel_size=geo.conv_depthwise_kernel,
            left_max_position_embeddings=geo.left_max_positions, right_max_position_embeddings=geo.right_max_positions,
            layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False, **head)
        return tf.Wav2Vec2BertForSequenceClassification(cfg).eval()
    if geo.family == C.FAMILY_W2V_CONFORMER:
        cfg = tf.Wav2Vec2ConformerConfig(
            hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
            conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel), conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias,
            feat_extract_norm="layer", feat_extract_activation="gelu", hidden_act="swish", position_embeddings_type=geo.position_type,
            rotary_embedding_base=geo.rotary_base, max_source_positions=geo.max_source_positions,
            conv_depthwise_kernel_size=geo.conv_depthwise_kernel, layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False,
            vocab_size=32, **head)
        return tf.Wav2Vec2ConformerForSequenceClassification(cfg).eval()
    common = dict(hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                  intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel),
                  conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias, feat_extract_norm=geo.feat_extract_norm,
                  do_stable_layer_norm=geo.stable_layer_norm, num_conv_pos_embeddings=geo.pos_conv_kernel,
                  num_conv_pos_embedding_groups=geo.pos_conv_groups, layer_norm_eps=geo.layer_norm_eps,
                  hidden_act="gelu", feat_extract_activation="gelu", vocab_size=32, apply_spec_augment=False, **head)
    if geo.family == C.FAMILY_WAVLM:
        return tf.WavLMForSequenceClassification(
            tf.WavLMConfig(num_buckets=geo.num_buckets, max_bucket_distance=geo.max_bucket_distance, **common)).eval()
    assert geo.family == C.FAMILY_WAV2VEC2
    return tf.Wav2Vec2ForSequenceClassification(tf.Wav2Vec2Config(**common)).eval()


def front_end(geo):
    """(feature extractor, its preprocessor_config as a dict)"""
    import transformers as tf
    if geo.family == C.FAMILY_WHISPER:
        fe = tf.WhisperFeatureExtractor(feature_size=geo.n_mels)
    elif geo.family == C.FAMILY_W2V_BERT:
        fe = tf.SeamlessM4TFeatureExtractor()
    else:
        fe = tf.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=True)
    pre = {k: v for k, v in fe.to_dict().items() if isinstance(v, (int, float, str, bool)) or v is None}     # drops the mel filter tables
    return fe, pre


def draw_head(D: int, L1: int, proj: int, n: int, weighted: bool, seed: int) -> dict:
    g = np.random.default_rng(seed)
    f = lambda *shape, std=1.0: (g.standard_normal(shape) * std).astype(np.float32)           # noqa: E731
    head = {"projector.weight": f(proj, D, std=1.0 / np.sqrt(D)), "projector.bias": f(proj, std=0.5),
            "classifier.weight": f(n, proj, std=1.0 / np.sqrt(proj)), "classifier.bias": f(n, std=0.5)}
    if weighted:
        head["layer_weights"] = f(L1)
    return head


def forget_cached_positions(model) -> None:
    """HF's rotary module keeps its cos / sin by sequence length alone: a table made in fp32 would serve the float64 run"""
    for m in model.modules():
        if hasattr(m, "cached_sequence_length"):
            m.cached_sequence_length = None


def make_case(tag, geo, seed, weighted, proj, labels, shortest):
    torch.manual_seed(0)
    model = hf_model(geo, weighted, proj, labels)
    n = model.config.num_labels
    enc = synthetic_state_dict(geo, seed)
    fe, pre = front_end(geo)
    lengths = (16000, 23457, shortest)
    wave_seeds = [7000 + 10 * seed + j for j in range(3)]
    cfg = model.config.to_dict()
    cfg["architectures"] = [type(model).__name__]
    for head_seed in range(seed * 100, seed * 100 + 50):
        head = draw_head(geo.hidden, geo.num_layers + 1, proj, n, weighted, head_seed)
        sd = {WRAPPER[geo.family] + k: v for k, v in enc.items()}
        sd.update({k: torch.from_numpy(v) for k, v in head.items()})
        res = model.float().load_state_dict(sd, strict=False)
        # off the encoder's path: the mask embedding; for the conformer family the positional convolution HF builds and never calls,
        # BatchNorm's step counter and the rotary buffer HF computes at construction
        extra = [k for k in res.missing_keys if "masked_spec_embed" not in k and not (
            geo.family == C.FAMILY_W2V_CONFORMER and ("pos_conv_embed." in k or k.endswith(("num_batches_tracked", "inv_freq"))))]
        assert not res.unexpected_keys and not extra, res
        rec = {"config": np.array(json.dumps(cfg, sort_keys=True)), "preprocessor": np.array(json.dumps(pre, sort_keys=True)),
               "seed": np.array(seed), "head_seed": np.array(head_seed), "digest": np.array(state_dict_digest(enc)),
               "lengths": np.array(lengths, dtype=np.int64), "wave_seeds": np.array(wave_seeds, dtype=np.int64)}
        rec.update({"head." + k: v for k, v in head.items()})
        cp = np.abs(head["classifier.weight"].astype(np.float64) @ head["projector.weight"].astype(np.float64)).sum(axis=1)
        wide, worst_id = 0, 0.0
        for j, (ws, ln) in enumerate(zip(wave_seeds, lengths)):
            wave = R.synth_wave(ws, ln)
            inputs = fe(wave, sampling_rate=16000, return_tensors="pt")
            mask = inputs["attention_mask"][0].bool() if geo.family == C.FAMILY_W2V_BERT else None
            if geo.family == C.FAMILY_WHISPER:
                inputs = {"input_features": inputs["input_features"]}
            with torch.no_grad():
                out32 = model.float()(**inputs, output_hidden_states=True)
                in64 = {k: (v.double() if v.is_floating_point() else v) for k, v in inputs.items()}
                forget_cached_positions(model)
                out64 = model.double()(**in64, output_hidden_states=True)
            model.float()
            forget_cached_positions(model)
            hs = torch.stack([h[0] for h in out64.hidden_states])
            if mask is not None:
                hs = hs[:, mask]
            hs = hs.numpy()
            assert hs.shape[0] == geo.num_layers + 1 and hs.dtype == np.float64
            if geo.family != C.FAMILY_WHISPER:
                assert hs.shape[1] == geo.frames_for(ln), (hs.shape, geo.frames_for(ln))
            l64 = out64.logits[0].numpy()
            ours = R.head_logits(hs, head, weighted)
            worst_id = max(worst_id, float(np.abs(ours - l64).max() / max(1e-300, np.abs(l64).max())))
            absmax = float(np.abs(hs).max())
            rec[f"logits32_{j}"] = out32.logits[0].numpy().astype(np.float32)
            rec[f"logits64_{j}"] = l64
            rec[f"states64_{j}"] = hs.mean(axis=1, keepdims=True) if geo.family == C.FAMILY_WHISPER else hs
            rec[f"hs_absmax_{j}"] = np.array(absmax)
            if n > 1:
                top = np.sort(l64)[::-1]
                wide += all(top[0] - top[1] > 2 * (e * max(1.0, absmax) * cp).max() for e in EPS)
        assert worst_id < 1e-10, worst_id
        if n == 1 or wide >= 2:
            print(f"{tag}: head seed {head_seed}, pool-first statement vs HF float64 {worst_id:.1e}, {wide} of 3 margins beyond twice the bound")
            return rec
    raise AssertionError(f"{tag}: no head seed gives two wide margins")


def main(out_dir: str = OUT, only: str = "") -> None:
    torch.set_num_threads(1)           # one summation order for the CPU convolutions: regenerating gives the same arrays
    for case in CASES:
        if only and case[0] != only:
            continue
        rec = make_case(*case)
        path = os.path.join(out_dir, case[0] + ".npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT, sys.argv[2] if len(sys.argv) > 2 else "")
