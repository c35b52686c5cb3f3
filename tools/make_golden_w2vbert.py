"""Writes tests/golden/tiny_w2v_bert_d128h2.npz and tiny_w2v_bert_d192h3.npz (CPU, needs `transformers`): HF's SeamlessM4TFeatureExtractor
and Wav2Vec2BertModel on seeded synthetic weights at two tiny geometries.  No weights are stored: the seed, the state dict's digest, HF's
stacked fbank rows and HF's fp32 hidden states at the rows whose attention_mask is 1.

    python tools/make_golden_w2vbert.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = (560, 16160, 52000)          # one row; 99 frames (the odd case); a few 64-key tiles
CASES = (("tiny_w2v_bert_d128h2", "TINY_W2V_BERT", 11), ("tiny_w2v_bert_d192h3", "TINY_W2V_BERT_H3", 12))


def main() -> None:
    import transformers as tf
    import w2vbert_ref as R
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict

    torch.manual_seed(0)
    fe = tf.SeamlessM4TFeatureExtractor()
    for tag, gname, seed in CASES:
        geo = getattr(C, gname)
        sd = synthetic_state_dict(geo, seed)
        cfg = tf.Wav2Vec2BertConfig(
            hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
            feature_projection_input_dim=geo.fbank_dim, conv_depthwise_kernel_size=geo.conv_depthwise_kernel,
            left_max_position_embeddings=geo.left_max_positions, right_max_position_embeddings=geo.right_max_positions,
            layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False)
        model = tf.Wav2Vec2BertModel(cfg).eval()
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and res.missing_keys == ["masked_spec_embed"], res
        out = dict(seed=np.int64(seed), digest=np.array(state_dict_digest(sd)), lengths=np.array(LENGTHS, dtype=np.int64))
        for j, n in enumerate(LENGTHS):
            wseed = 100 * seed + j
            wave = R.synth_wave(wseed, n)
            inputs = fe(wave, sampling_rate=16000, return_tensors="pt")
            mask = inputs["attention_mask"][0].bool()
            assert int(mask.sum()) == geo.frames_for(n), (n, int(mask.sum()))
            with torch.no_grad():
                hs = model(**inputs, output_hidden_states=True).hidden_states
            assert len(hs) == geo.num_layers + 1
            out[f"wave_seed_{j}"] = np.int64(wseed)
            out[f"fbank_{j}"] = inputs["input_features"][0][mask].numpy().astype(np.float32)
            out[f"states_{j}"] = torch.stack([h[0][mask] for h in hs]).numpy().astype(np.float32)
        path = os.path.join(ROOT, "tests", "golden", tag + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
