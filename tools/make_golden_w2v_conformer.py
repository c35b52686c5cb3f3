"""Writes tests/golden/tiny_w2v_conformer_rope.npz and tiny_w2v_conformer_rel.npz (CPU, needs `transformers`): HF's
Wav2Vec2ConformerModel(...).double().eval() on seeded synthetic weights at the two tiny geometries, one per position type, each utterance
at batch size 1 with no padding and no attention mask.  No weights are stored: the seed, the state dict's digest, the lengths, the
waveform seeds and HF's float64 hidden states cast to fp32.

    python tools/make_golden_w2v_conformer.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LENGTHS = (400, 5500, 32000, 52000)          # 1, 16, 99 and 162 frames: one row; a conformer-conv tile edge; odd; a few 64-key tiles
CASES = (("tiny_w2v_conformer_rope", "TINY_W2V_CONFORMER_ROPE", 21), ("tiny_w2v_conformer_rel", "TINY_W2V_CONFORMER_REL", 22))


def hf_config(geo, **extra):
    import transformers as tf
    return tf.Wav2Vec2ConformerConfig(
        hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
        conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel), conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias,
        feat_extract_norm="layer", feat_extract_activation="gelu", hidden_act="swish", position_embeddings_type=geo.position_type,
        rotary_embedding_base=geo.rotary_base, max_source_positions=geo.max_source_positions,
        conv_depthwise_kernel_size=geo.conv_depthwise_kernel, layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False,
        vocab_size=32, **extra)


# what HF's module tree holds and the synthetic state dict does not: the mask embedding, the positional convolution HF builds and never
# calls, BatchNorm's step counter and the rotary buffer (computed by HF at construction; the encoder computes the same expression)
def off_path(key: str) -> bool:
    return key.startswith(("masked_spec_embed", "encoder.pos_conv_embed.")) or key.endswith(("num_batches_tracked", "embed_positions.inv_freq"))


def main() -> None:
    import transformers as tf
    import w2vconf_ref as R
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict

    torch.manual_seed(0)
    torch.set_num_threads(1)
    for tag, gname, seed in CASES:
        geo = getattr(C, gname)
        sd = synthetic_state_dict(geo, seed)
        model = tf.Wav2Vec2ConformerModel(hf_config(geo))
        res = model.load_state_dict(sd, strict=False)
        assert not res.unexpected_keys and all(off_path(k) for k in res.missing_keys), res
        model = model.double().eval()
        out = dict(seed=np.int64(seed), digest=np.array(state_dict_digest(sd)), lengths=np.array(LENGTHS, dtype=np.int64))
        for j, n in enumerate(LENGTHS):
            wseed = 100 * seed + j
            wave = R.synth_wave(wseed, n)
            with torch.no_grad():
                hs = model(R.normalize_wave(wave)[None], output_hidden_states=True).hidden_states
            assert len(hs) == geo.num_layers + 1 and hs[0].shape[1] == geo.frames_for(n), (n, hs[0].shape)
            out[f"wave_seed_{j}"] = np.int64(wseed)
            out[f"states_{j}"] = torch.stack([h[0] for h in hs]).numpy().astype(np.float32)
        path = os.path.join(ROOT, "tests", "golden", tag + ".npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
