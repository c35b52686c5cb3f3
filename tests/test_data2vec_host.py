"""CPU: the data2vec-audio speech checkpoints (layer-norm conv stem, post-LayerNorm encoder, a stack of LayerNorm'd positional convs) --
geometry from config.json and the registry, names, the synthetic state dict against the HF class, and the restatement
tests/data2vec_oracle.py against the HF fixtures."""
import os

import numpy as np
import pytest
import torch

import data2vec_oracle as DO

CASES = (("tiny_data2vec_audio_d128h2", "TINY_DATA2VEC_AUDIO"), ("tiny_data2vec_audio_d192h3g48", "TINY_DATA2VEC_AUDIO_G48"))


def _config(**kw) -> dict:
    """A data2vec-audio config.json as the hub ships it (transformers' Data2VecAudioConfig keys and defaults)."""
    d = dict(model_type="data2vec-audio", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
             conv_dim=[512] * 7, conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_bias=False,
             conv_pos_kernel_size=19, num_conv_pos_embeddings=5, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
             add_adapter=False, feat_extract_activation="gelu", hidden_act="gelu")
    d.update(kw)
    return d


def test_geometry_from_base_and_large_configs():
    from interspeech_ser_amd import config as C
    base = C.geometry_from_config(_config(), name="facebook/data2vec-audio-base")
    large = C.geometry_from_config(_config(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096),
                                   name="facebook/data2vec-audio-large")
    for geo, dims in ((base, (12, 768, 12, 3072)), (large, (24, 1024, 16, 4096))):
        assert geo.family == C.FAMILY_DATA2VEC_AUDIO
        assert (geo.num_layers, geo.hidden, geo.heads, geo.ffn) == dims
        # the kernel is conv_pos_kernel_size; num_conv_pos_embeddings counts the LAYERS here (it is the kernel in wav2vec2 configs)
        assert (geo.pos_conv_kernel, geo.pos_conv_layers, geo.pos_conv_groups, geo.pos_conv_norm) == (19, 5, 16, "layer")
        assert geo.feat_extract_norm == "layer" and not geo.stable_layer_norm and not geo.conv_bias
    assert base == C.DATA2VEC_AUDIO_BASE and large == C.DATA2VEC_AUDIO_LARGE
    odd = C.geometry_from_config(_config(conv_bias=True, layer_norm_eps=1e-6, conv_pos_kernel_size=5, num_conv_pos_embeddings=3,
                                         num_conv_pos_embedding_groups=8, conv_dim=[256] * 7))
    assert (odd.conv_bias, odd.layer_norm_eps, odd.pos_conv_kernel, odd.pos_conv_layers, odd.pos_conv_groups, odd.conv_dim) == \
        (True, 1e-6, 5, 3, 8, (256,) * 7)


def test_geometry_from_the_transformers_default_config():
    tf = pytest.importorskip("transformers")
    from interspeech_ser_amd import config as C
    assert C.geometry_from_config(tf.Data2VecAudioConfig().to_dict(), name="facebook/data2vec-audio-base") == C.DATA2VEC_AUDIO_BASE


def test_adapter_and_even_kernel_are_refused():
    from interspeech_ser_amd import config as C
    with pytest.raises(OSError, match="add_adapter"):
        C.geometry_from_config(_config(add_adapter=True))
    with pytest.raises(OSError, match="even"):
        C.geometry_from_config(_config(conv_pos_kernel_size=16))


def test_other_families_keep_their_pos_conv_and_refusals():
    from interspeech_ser_amd import config as C
    for geo in (C.WAVLM_LARGE, C.XLSR_2B, C.HUBERT_XLARGE, C.WAVLM_BASE, C.TINY_WAVLM, C.TINY_HUBERT_BASE):
        assert (geo.pos_conv_layers, geo.pos_conv_norm) == (1, "weight")
    wav2vec2 = dict(model_type="wav2vec2", hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                    num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
    assert C.geometry_from_config(dict(wav2vec2, feat_extract_norm="group")).pos_conv_kernel == 128
    with pytest.raises(OSError, match="post-LayerNorm"):
        C.geometry_from_config(dict(wav2vec2, feat_extract_norm="layer", do_stable_layer_norm=False))


@pytest.mark.parametrize("name,layers", [("facebook/data2vec-audio-base", 12), ("facebook/data2vec-audio-base-960h", 12),
                                         ("facebook/data2vec-audio-large", 24), ("facebook/data2vec-audio-large-960h", 24),
                                         ("data2vec-audio-large", 24), ("DATA2VEC-AUDIO-BASE-960H", 12)])
def test_registry_names_resolve(name, layers):
    from interspeech_ser_amd import config as C
    geo = C.geometry_for(name)
    assert geo.family == C.FAMILY_DATA2VEC_AUDIO and geo.num_layers == layers and geo.pos_conv_layers == 5
    assert C.resolve_geometry(name) == geo


def test_normalize_names_strips_the_ctc_wrapper():
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import normalize_names, synthetic_state_dict
    sd = synthetic_state_dict(C.TINY_DATA2VEC_AUDIO, 2)
    wrapped = {"data2vec_audio." + k: v for k, v in sd.items()}
    wrapped["lm_head.weight"] = torch.zeros(32, 128)
    wrapped["data2vec_audio.masked_spec_embed"] = torch.zeros(128)
    out = normalize_names(wrapped)
    assert sorted(out) == sorted(sd)


@pytest.mark.parametrize("gname", ["TINY_DATA2VEC_AUDIO", "TINY_DATA2VEC_AUDIO_G48", "DATA2VEC_AUDIO_BASE"])
def test_synthetic_state_dict_loads_strictly(gname):
    tf = pytest.importorskip("transformers")
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, gname)
    if geo.num_layers > 2:
        from dataclasses import replace
        geo = replace(geo, num_layers=1)             # the full stem and positional stack, one layer: keeps the test fast
    sd = synthetic_state_dict(geo, 3)
    assert not any("parametrizations" in k or "weight_g" in k for k in sd)
    assert sorted(k for k in sd if k.startswith("encoder.pos_conv_embed.")) == sorted(
        f"encoder.pos_conv_embed.layers.{j}.conv.{leaf}" for j in range(5) for leaf in ("weight", "bias"))
    cfg = tf.Data2VecAudioConfig(hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                                 intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), conv_bias=geo.conv_bias,
                                 num_conv_pos_embedding_groups=geo.pos_conv_groups)
    model = tf.Data2VecAudioModel(cfg)
    res = model.load_state_dict(sd, strict=False)
    # strict except masked_spec_embed, a training-time parameter the encoder path never reads (weights.normalize_names drops it)
    assert not res.unexpected_keys and res.missing_keys == ["masked_spec_embed"], res


@pytest.mark.parametrize("case", [0, 1])
def test_oracle_matches_hf_fixture(golden_dir, case):
    """tests/data2vec_oracle.py reproduces every hidden state of the HF fixture within 2e-5 (relative to max(1, max|ref|))."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict, state_dict_digest
    tag, gname = CASES[case]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    sd = synthetic_state_dict(geo, int(gold["seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    for j, n in enumerate(int(x) for x in gold["lengths"]):
        ref = torch.from_numpy(gold[f"states_{j}"])
        with torch.no_grad():
            ours = DO.hidden_states(geo, sd, torch.from_numpy(DO.normalize_wave(DO.synth_wave(int(gold[f"wave_seed_{j}"]), n))))
        assert len(ours) == ref.shape[0] == geo.num_layers + 1 and ref.shape[1] == geo.frames_for(n)
        for layer, r in enumerate(ref):
            err = float((ours[layer] - r).abs().max() / max(1.0, float(r.abs().max())))
            assert err < 2e-5, (j, layer, err)
