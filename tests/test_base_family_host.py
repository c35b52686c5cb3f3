"""CPU: the *-base speech checkpoints (GroupNorm feature extractor + post-LayerNorm encoder: wavlm-base, wav2vec2-base,
hubert-base) -- geometry from config.json and the registry, the synthetic state dict against the HF classes, do_normalize from
preprocessor_config.json, the restatement tests/base_oracle.py against the HF fixtures, and the fixture generator's determinism."""
import json
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import base_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("tiny_wavlm_base_d128h2", "TINY_WAVLM_BASE"), ("tiny_wav2vec2_base_d128h2", "TINY_WAV2VEC2_BASE"),
         ("tiny_hubert_base_d128h2", "TINY_HUBERT_BASE"))


def _hf_configs():
    import transformers as tf
    return (("microsoft/wavlm-base", tf.WavLMConfig()), ("facebook/wav2vec2-base", tf.Wav2Vec2Config()),
            ("facebook/hubert-base-ls960", tf.HubertConfig()))


def test_geometry_from_default_configs_equals_registry():
    from interspeech_ser_amd import config as C
    for name, cfg in _hf_configs():
        geo = C.geometry_from_config(cfg.to_dict(), name=name)
        assert geo == C.geometry_for(name), name
        assert geo.feat_extract_norm == "group" and not geo.stable_layer_norm
        assert (geo.num_layers, geo.hidden, geo.heads, geo.ffn, geo.conv_bias) == (12, 768, 12, 3072, False)


def test_mixed_norm_combinations_stay_refused():
    from interspeech_ser_amd import config as C
    for _, cfg in _hf_configs():
        d = cfg.to_dict()
        with pytest.raises(OSError, match="GroupNorm"):
            C.geometry_from_config(dict(d, feat_extract_norm="group", do_stable_layer_norm=True))
        with pytest.raises(OSError, match="post-LayerNorm"):
            C.geometry_from_config(dict(d, feat_extract_norm="layer", do_stable_layer_norm=False))


def test_large_geometries_are_unchanged():
    from interspeech_ser_amd import config as C
    for geo in (C.WAVLM_LARGE, C.XLSR_2B, C.HUBERT_XLARGE, C.TINY_WAVLM, C.TINY_WAV2VEC2, C.TINY_HUBERT):
        assert geo.feat_extract_norm == "layer" and geo.stable_layer_norm


@pytest.mark.parametrize("name", ["wavlm-base", "microsoft/wavlm-base", "microsoft/wavlm-base-plus", "facebook/wav2vec2-base",
                                  "facebook/hubert-base-ls960", "wavlm-base-plus"])
def test_base_names_resolve(name):
    from interspeech_ser_amd import config as C
    geo = C.geometry_for(name)
    assert geo.num_layers == 12 and geo.hidden == 768 and not geo.stable_layer_norm
    assert C.geometry_for("wavlm-base").name == "microsoft/wavlm-base"


@pytest.mark.parametrize("case", [0, 1, 2])
def test_synthetic_base_state_dict_loads_into_hf(case):
    import transformers as tf
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, CASES[case][1])
    sd = synthetic_state_dict(geo, 3)
    assert sd["feature_extractor.conv_layers.0.layer_norm.weight"].shape == (geo.conv_dim[0],)
    assert not any(f"conv_layers.{i}.layer_norm" in k for k in sd for i in range(1, 7))
    cls = {C.FAMILY_WAVLM: (tf.WavLMConfig, tf.WavLMModel), C.FAMILY_WAV2VEC2: (tf.Wav2Vec2Config, tf.Wav2Vec2Model),
           C.FAMILY_HUBERT: (tf.HubertConfig, tf.HubertModel)}[geo.family]
    model = cls[1](cls[0](hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                          intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), num_conv_pos_embedding_groups=geo.pos_conv_groups))
    # strict except masked_spec_embed, a training-time parameter the encoder path never reads (weights.normalize_names drops it)
    model.load_state_dict(dict(sd, masked_spec_embed=model.masked_spec_embed.detach()), strict=True)


def test_do_normalize_read_from_preprocessor_config(tmp_path, monkeypatch):
    from interspeech_ser_amd import config as C
    monkeypatch.setenv("HF_HOME", str(tmp_path / "hf"))
    snap = tmp_path / "hf" / "hub" / "models--microsoft--wavlm-base" / "snapshots" / "abc"
    snap.mkdir(parents=True)
    (snap / "config.json").write_text(json.dumps(dict(_hf_configs()[0][1].to_dict())))
    assert C.resolve_do_normalize("microsoft/wavlm-base") is True               # no preprocessor_config.json: normalise
    (snap / "preprocessor_config.json").write_text(json.dumps({"do_normalize": False, "feature_size": 1}))
    assert C.resolve_do_normalize("microsoft/wavlm-base") is False
    (snap / "preprocessor_config.json").write_text(json.dumps({"do_normalize": True}))
    assert C.resolve_do_normalize("microsoft/wavlm-base") is True
    ck = tmp_path / "ck"
    ck.mkdir()
    (ck / "config.json").write_text("{}")
    (ck / "preprocessor_config.json").write_text(json.dumps({"do_normalize": False}))
    assert C.resolve_do_normalize("anything", str(ck)) is False
    assert C.resolve_do_normalize("microsoft/wavlm-large") is True


@pytest.mark.parametrize("case", [0, 1, 2])
def test_restatement_matches_hf_fixtures(golden_dir, case):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict, state_dict_digest
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden_base import synth_wave
    tag, gname = CASES[case]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    sd = synthetic_state_dict(geo, int(gold["seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    for j, n in enumerate(gold["lengths"]):
        wave = synth_wave(int(gold[f"wave_seed_{j}"]), int(n))
        with torch.no_grad():
            ours = BO.hidden_states(geo, sd, torch.from_numpy(BO.normalize_wave(wave)))
        ref = torch.from_numpy(gold[f"states_{j}"])
        assert len(ours) == ref.shape[0] == geo.num_layers + 1
        for a, b in zip(ours, ref):
            assert a.shape == b.shape
            assert float((a - b).abs().max() / max(1.0, float(b.abs().max()))) <= 2e-5


def test_fixture_generator_is_deterministic(golden_dir, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_base as G
    G.main(str(tmp_path))
    for tag, _, _ in G.CASES:
        a, b = np.load(os.path.join(golden_dir, tag + ".npz")), np.load(str(tmp_path / (tag + ".npz")))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (tag, k)
