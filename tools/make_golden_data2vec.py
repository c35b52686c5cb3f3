"""Generate tests/golden/tiny_data2vec_audio_*.npz -- the data2vec-audio fixtures (layer-norm stem, post-LN encoder, LayerNorm'd
positional conv stack).

TEST INFRASTRUCTURE ONLY, CPU.  Seeded synthetic weights (weights.synthetic_state_dict of config.TINY_DATA2VEC_AUDIO /
TINY_DATA2VEC_AUDIO_G48) are loaded strictly into ``transformers.Data2VecAudioModel`` -- the class the reference's ``AutoModel``
resolves to for facebook/data2vec-audio-* -- and driven batch-of-one with ``output_hidden_states=True`` after
``Wav2Vec2FeatureExtractor(do_normalize=True)`` (preprocess_speech.py:43-50).  Three ragged waveforms per geometry: one near the
400-sample receptive field, about 1 s, and several seconds.  tests/data2vec_oracle.py is checked against the HF states here and again
by tests/test_data2vec_host.py.

    python tools/make_golden_data2vec.py            # writes tests/golden/
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict, state_dict_digest  # noqa: E402
import data2vec_oracle as DO                                                      # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CASES = (("tiny_data2vec_audio_d128h2", "TINY_DATA2VEC_AUDIO", 31), ("tiny_data2vec_audio_d192h3g48", "TINY_DATA2VEC_AUDIO_G48", 32))
LENGTHS = (430, 16400, 52000)          # 0.03 s (1 frame), ~1 s, 3.25 s


def hf_model(geo):
    import transformers as tf
    cfg = tf.Data2VecAudioConfig(
        hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
        conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel), conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias,
        conv_pos_kernel_size=geo.pos_conv_kernel, num_conv_pos_embeddings=geo.pos_conv_layers,
        num_conv_pos_embedding_groups=geo.pos_conv_groups, layer_norm_eps=geo.layer_norm_eps, hidden_act="gelu",
        feat_extract_activation="gelu", vocab_size=32)
    assert C.geometry_from_config(cfg.to_dict(), name=geo.name) == geo
    return tf.Data2VecAudioModel(cfg).eval()


def make_case(geo, seed: int):
    """-> dict of arrays (the fixture) and the restatement's worst relative error against HF."""
    import transformers as tf
    torch.manual_seed(0)
    sd = synthetic_state_dict(geo, seed)
    model = hf_model(geo)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["masked_spec_embed"], res        # masked_spec_embed: training only
    fe = tf.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True,
                                     return_attention_mask=True)
    rec = {"seed": np.array(seed), "digest": np.array(state_dict_digest(sd)), "lengths": np.array(LENGTHS, dtype=np.int64),
           "do_normalize": np.array(True)}
    worst = 0.0
    for j, n in enumerate(LENGTHS):
        wseed = 3000 + 31 * j + seed
        wave = DO.synth_wave(wseed, n)
        inputs = fe(wave, sampling_rate=16000, return_tensors="pt")
        with torch.no_grad():
            hs = [h.squeeze(0) for h in model(**inputs, output_hidden_states=True).hidden_states]
        x = DO.normalize_wave(wave)
        assert np.abs(x - inputs["input_values"][0].numpy()).max() == 0.0
        with torch.no_grad():
            ours = DO.hidden_states(geo, sd, torch.from_numpy(x))
        assert len(ours) == len(hs) == geo.num_layers + 1 and hs[0].shape[0] == geo.frames_for(n)
        for a, b in zip(ours, hs):
            worst = max(worst, float((a - b).abs().max() / max(1.0, float(b.abs().max()))))
        rec[f"wave_seed_{j}"] = np.array(wseed)
        rec[f"states_{j}"] = torch.stack(hs).numpy().astype(np.float32)          # [L+1, T, D]
    return rec, worst


def main(out_dir: str = OUT) -> None:
    os.makedirs(out_dir, exist_ok=True)
    torch.set_num_threads(1)           # one summation order for the CPU convolutions: regenerating gives the same arrays
    for tag, geo_name, seed in CASES:
        rec, worst = make_case(getattr(C, geo_name), seed)
        print(f"{tag}: restatement vs HF rel-max err {worst:.2e}")
        assert worst < 2e-5, worst
        np.savez_compressed(os.path.join(out_dir, f"{tag}.npz"), **rec)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
