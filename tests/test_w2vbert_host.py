"""CPU: w2v-BERT 2.0 (HF Wav2Vec2BertModel) -- geometry from config.json, the refusals, the synthetic state dict's names, the frame rule,
the front end's host tables, and the float64 statement tests/w2vbert_ref.py against the HF fixtures of tools/make_golden_w2vbert.py."""
import json
import os

import numpy as np
import pytest
import torch

import w2vbert_ref as R

CASES = (("tiny_w2v_bert_d128h2", "TINY_W2V_BERT"), ("tiny_w2v_bert_d192h3", "TINY_W2V_BERT_H3"))
LENGTHS = (560, 16160, 52000)


def _config(**kw) -> dict:
    """A wav2vec2-bert config.json as the hub ships it (transformers' Wav2Vec2BertConfig keys and defaults)."""
    d = dict(model_type="wav2vec2-bert", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
             feature_projection_input_dim=160, hidden_act="swish", layer_norm_eps=1e-5, position_embeddings_type="relative_key",
             left_max_position_embeddings=64, right_max_position_embeddings=8, conv_depthwise_kernel_size=31, add_adapter=False)
    d.update(kw)
    return d


def test_geometry_from_config_and_registry():
    from interspeech_ser_amd import config as C
    geo = C.geometry_from_config(_config(), name="facebook/w2v-bert-2.0")
    assert geo == C.W2V_BERT_2 == C.geometry_for("facebook/w2v-bert-2.0") == C.geometry_for("w2v-bert-2.0")
    assert geo.family == C.FAMILY_W2V_BERT and (geo.num_layers, geo.hidden, geo.heads, geo.ffn, geo.head_dim) == (24, 1024, 16, 4096, 64)
    assert (geo.fbank_dim, geo.conv_depthwise_kernel, geo.left_max_positions, geo.right_max_positions, geo.distance_positions) == (160, 31, 64, 8, 73)
    odd = C.geometry_from_config(_config(conv_depthwise_kernel_size=7, left_max_position_embeddings=5, right_max_position_embeddings=3,
                                         layer_norm_eps=1e-6, hidden_size=192, num_attention_heads=3))
    assert (odd.conv_depthwise_kernel, odd.left_max_positions, odd.right_max_positions, odd.layer_norm_eps, odd.head_dim) == (7, 5, 3, 1e-6, 64)


def test_geometry_round_trips_the_transformers_default_config():
    tf = pytest.importorskip("transformers")
    from interspeech_ser_amd import config as C
    assert C.geometry_from_config(tf.Wav2Vec2BertConfig().to_dict(), name="facebook/w2v-bert-2.0") == C.W2V_BERT_2


@pytest.mark.parametrize("kw,match", [(dict(position_embeddings_type="rotary"), "position_embeddings_type"),
                                      (dict(position_embeddings_type="relative"), "position_embeddings_type"),
                                      (dict(add_adapter=True), "add_adapter"), (dict(hidden_act="gelu"), "hidden_act"),
                                      (dict(conv_depthwise_kernel_size=32), "even"),
                                      (dict(left_max_position_embeddings=120, right_max_position_embeddings=8), "128")])
def test_refusals(kw, match):
    from interspeech_ser_amd import config as C
    with pytest.raises(OSError, match=match):
        C.geometry_from_config(_config(**kw), name="acme/w2v-bert-x")


def test_front_end_settings_come_from_the_preprocessor_config(tmp_path):
    from interspeech_ser_amd import config as C
    snap = tmp_path / "snap"
    snap.mkdir()
    (snap / "config.json").write_text(json.dumps(_config(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)))
    geo = C.resolve_fbank(C.resolve_geometry(str(snap)), str(snap))
    assert (geo.fbank_mels, geo.fbank_stride) == (80, 2)                   # no file: 80 and 2
    (snap / "preprocessor_config.json").write_text(json.dumps(dict(feature_extractor_type="SeamlessM4TFeatureExtractor", num_mel_bins=40,
                                                                   stride=4, sampling_rate=16000)))
    geo = C.resolve_fbank(C.resolve_geometry(str(snap)), str(snap))
    assert (geo.fbank_mels, geo.fbank_stride, geo.fbank_dim) == (40, 4, 160)
    (snap / "preprocessor_config.json").write_text(json.dumps(dict(num_mel_bins=80, stride=3)))
    with pytest.raises(OSError, match="feature projection"):
        C.resolve_fbank(C.resolve_geometry(str(snap)), str(snap))
    assert C.resolve_fbank(C.WAVLM_LARGE, "microsoft/wavlm-large") is C.WAVLM_LARGE


def test_frames_equal_hf_mask_sum():
    """frames(n) = (1 + (n - 400) // 160) // 2 is the number of rows HF marks valid, for every n in 400 .. 1200 and the fixture lengths."""
    tf = pytest.importorskip("transformers")
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.frontend import w2vbert_frames
    fe = tf.SeamlessM4TFeatureExtractor()
    x = np.random.default_rng(0).standard_normal(52000).astype(np.float32) * 0.1
    for n in list(range(400, 1201)) + list(LENGTHS):
        want = (1 + (n - 400) // 160) // 2
        assert C.W2V_BERT_2.frames_for(n) == w2vbert_frames(n) == R.frames(n) == want, n
        with np.errstate(all="ignore"):                                       # (one frame: HF divides by the variance of a single value)
            mask = fe(x[:n], sampling_rate=16000, return_tensors="np")["attention_mask"]
        assert int(mask.sum()) == want, n
    assert C.W2V_BERT_2.frames_for(399) == 0 and C.W2V_BERT_2.frames_for(559) == 0 and C.W2V_BERT_2.frames_for(560) == 1


def test_host_tables_restate_the_statement():
    from interspeech_ser_amd.frontend import w2vbert_dft_table, w2vbert_mel_filters
    w, rng = w2vbert_mel_filters(80)
    assert np.abs(w.T - R.mel_filters(80)).max() < 1e-15
    for m in range(80):
        assert rng[m, 0] < rng[m, 1] <= 257 and not w[m, : rng[m, 0]].any() and not w[m, rng[m, 1]:].any()
    t = w2vbert_dft_table()
    z = np.random.default_rng(1).standard_normal(400)
    spec = np.fft.rfft(z * np.hanning(400) ** 0.85, 512)
    got = (z[:, None, None] * t).sum(0)
    assert t.shape == (400, 257, 2) and np.abs(got[:, 0] - spec.real).max() < 1e-10 and np.abs(got[:, 1] - spec.imag).max() < 1e-10


def test_synthetic_keys_are_hf_names():
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import normalize_names, synthetic_state_dict
    geo = C.TINY_W2V_BERT_H3
    sd = synthetic_state_dict(geo, 3)
    want = {"feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias", "feature_projection.projection.weight",
            "feature_projection.projection.bias"}
    for i in range(geo.num_layers):
        p = f"encoder.layers.{i}."
        for ln in ("ffn1_layer_norm", "self_attn_layer_norm", "conv_module.layer_norm", "conv_module.depthwise_layer_norm", "ffn2_layer_norm",
                   "final_layer_norm"):
            want |= {p + ln + ".weight", p + ln + ".bias"}
        for lin in ("ffn1.intermediate_dense", "ffn1.output_dense", "ffn2.intermediate_dense", "ffn2.output_dense", "self_attn.linear_q",
                    "self_attn.linear_k", "self_attn.linear_v", "self_attn.linear_out"):
            want |= {p + lin + ".weight", p + lin + ".bias"}
        want |= {p + "self_attn.distance_embedding.weight", p + "conv_module.pointwise_conv1.weight", p + "conv_module.depthwise_conv.weight",
                 p + "conv_module.pointwise_conv2.weight"}
    assert set(sd) == want
    assert tuple(sd["encoder.layers.0.self_attn.distance_embedding.weight"].shape) == (9, 64)
    assert tuple(sd["encoder.layers.1.conv_module.depthwise_conv.weight"].shape) == (192, 1, 7)
    wrapped = {"wav2vec2_bert." + k: v for k, v in sd.items()}
    wrapped["wav2vec2_bert.masked_spec_embed"] = torch.zeros(192)
    wrapped["lm_head.weight"] = torch.zeros(32, 192)
    assert sorted(normalize_names(wrapped)) == sorted(sd)


@pytest.mark.parametrize("gname", ["TINY_W2V_BERT", "TINY_W2V_BERT_H3"])
def test_synthetic_state_dict_loads_strictly(gname):
    tf = pytest.importorskip("transformers")
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, gname)
    cfg = tf.Wav2Vec2BertConfig(hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                                intermediate_size=geo.ffn, feature_projection_input_dim=geo.fbank_dim,
                                conv_depthwise_kernel_size=geo.conv_depthwise_kernel, left_max_position_embeddings=geo.left_max_positions,
                                right_max_position_embeddings=geo.right_max_positions)
    res = tf.Wav2Vec2BertModel(cfg).load_state_dict(synthetic_state_dict(geo, 3), strict=False)
    assert not res.unexpected_keys and res.missing_keys == ["masked_spec_embed"], res


def test_ffn_fold_moves_no_rounding():
    from interspeech_ser_amd.weights import fold_w2v_bert_ffn
    w, b = torch.randn(8, 16), torch.randn(8)
    fw, fb = fold_w2v_bert_ffn(w, b)
    x = torch.randn(5, 16)
    assert torch.equal(x @ fw.T + fb, 0.5 * (x @ w.T + b))


@pytest.mark.parametrize("case", [0, 1])
def test_statement_matches_hf_fixture(golden_dir, case):
    """tests/w2vbert_ref.py reproduces HF's stacked fbank rows and every hidden state within 2e-5 (relative to max(1, max|ref|))."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
    tag, gname = CASES[case]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    assert os.path.getsize(os.path.join(golden_dir, tag + ".npz")) < (1 << 20)
    sd = synthetic_state_dict(geo, int(gold["seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    assert tuple(int(x) for x in gold["lengths"]) == LENGTHS
    for j, n in enumerate(LENGTHS):
        rows = R.fbank_rows(R.synth_wave(int(gold[f"wave_seed_{j}"]), n))
        fb = gold[f"fbank_{j}"].astype(np.float64)
        assert rows.shape == fb.shape == (geo.frames_for(n), 160)
        err = float(np.abs(rows - fb).max() / max(1.0, float(np.abs(fb).max())))
        assert err < 2e-5, (j, "fbank", err)
        ref = torch.from_numpy(gold[f"states_{j}"]).double()
        with torch.no_grad():
            ours = R.hidden_states(geo, sd, torch.from_numpy(rows))
        assert len(ours) == ref.shape[0] == geo.num_layers + 1 and ref.shape[1] == geo.frames_for(n)
        for layer, r in enumerate(ref):
            err = float((ours[layer] - r).abs().max() / max(1.0, float(r.abs().max())))
            assert err < 2e-5, (j, layer, err)
