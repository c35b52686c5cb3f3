"""CPU: the wav2vec2-conformer family's host side -- the float64 statement (tests/w2vconf_ref.py) against HF's fixtures, the geometry and
its refusals, the load-time folds and the position tables."""
import os

import numpy as np
import pytest
import torch

import w2vconf_ref as R
from interspeech_ser_amd import config as C
from interspeech_ser_amd import weights as W

CASES = (("tiny_w2v_conformer_rope", "TINY_W2V_CONFORMER_ROPE"), ("tiny_w2v_conformer_rel", "TINY_W2V_CONFORMER_REL"))
LARGE = dict(model_type="wav2vec2-conformer", hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
             feat_extract_norm="layer", hidden_act="swish", conv_depthwise_kernel_size=31, conv_bias=True, conv_dim=[512] * 7,
             conv_kernel=[10, 3, 3, 3, 3, 2, 2], conv_stride=[5, 2, 2, 2, 2, 2, 2], max_source_positions=5000,
             rotary_embedding_base=10000, layer_norm_eps=1e-5, add_adapter=False)


@pytest.mark.parametrize("tag, gname", CASES)
def test_statement_equals_hf_fixture(golden_dir, tag, gname):
    """HF's float64 states: the i - j index of the relative term, the u / v split, the BatchNorm fold and the rotation in front of the
    projections all sit in this comparison (2e-5 relative, tests/test_oracle_golden.py's gate; the fixture itself is fp32)"""
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    sd = W.synthetic_state_dict(geo, int(gold["seed"]))
    assert W.state_dict_digest(sd) == str(gold["digest"])
    assert [int(n) for n in gold["lengths"]] == [400, 5500, 32000, 52000]
    for j, n in enumerate(gold["lengths"]):
        ref = torch.from_numpy(gold[f"states_{j}"]).double()
        got = torch.stack(R.forward(geo, sd, R.synth_wave(int(gold[f"wave_seed_{j}"]), int(n))))
        assert got.shape == ref.shape == (geo.num_layers + 1, geo.frames_for(int(n)), geo.hidden)
        err = float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))
        print(f"W2VCONF statement vs HF {tag} {int(n)} samples: {err:.3e}")
        assert err < 2e-5, (tag, int(n), err)


def test_fixture_frames():
    assert [C.TINY_W2V_CONFORMER_ROPE.frames_for(n) for n in (400, 5500, 32000, 52000)] == [1, 16, 99, 162]


@pytest.mark.parametrize("pos", ["rotary", "relative"])
def test_geometry_of_the_published_large_configuration(pos):
    geo = C.geometry_from_config(dict(LARGE, position_embeddings_type=pos), name="facebook/wav2vec2-conformer-large")
    assert (geo.family, geo.num_layers, geo.hidden, geo.heads, geo.ffn) == (C.FAMILY_W2V_CONFORMER, 24, 1024, 16, 4096)
    assert geo.family == "wav2vec2-conformer" and geo.position_type == pos and geo.head_dim == 64 and geo.conv_depthwise_kernel == 31
    assert geo.rotary_base == 10000 and geo.max_source_positions == 5000 and geo.feat_extract_norm == "layer" and geo.conv_bias
    assert geo.frames_for(160000) == 499


def test_new_geometry_fields_leave_the_other_geometries_equal():
    assert C.WAVLM_LARGE.position_type == "" and C.WAVLM_LARGE.rotary_base == 10000 and C.WAVLM_LARGE.max_source_positions == 1500
    assert C.TINY_W2V_CONFORMER_ROPE.position_type == "rotary" and C.TINY_W2V_CONFORMER_REL.position_type == "relative"
    assert (C.TINY_W2V_CONFORMER_ROPE.hidden, C.TINY_W2V_CONFORMER_ROPE.heads) == (128, 2)
    assert (C.TINY_W2V_CONFORMER_REL.hidden, C.TINY_W2V_CONFORMER_REL.heads) == (192, 3)
    for g in (C.TINY_W2V_CONFORMER_ROPE, C.TINY_W2V_CONFORMER_REL):
        assert g.num_layers == 2 and g.conv_depthwise_kernel == 31 and int(np.prod(g.conv_stride)) == 320


@pytest.mark.parametrize("edit, what", [
    (dict(add_adapter=True), "add_adapter"),
    (dict(feat_extract_norm="group"), "feat_extract_norm='group'"),
    (dict(hidden_act="gelu"), "hidden_act='gelu'"),
    (dict(hidden_act=None), "hidden_act='gelu'"),                       # a missing key: the class default
    (dict(feat_extract_norm=None), "feat_extract_norm='group'"),
    (dict(conv_depthwise_kernel_size=32), "conv_depthwise_kernel_size"),
    (dict(conv_depthwise_kernel_size=33), "conv_depthwise_kernel_size"),
    (dict(num_attention_heads=8), "head dim"),
    (dict(position_embeddings_type="relative_key"), "position_embeddings_type='relative_key'"),
])
def test_refusals_are_one_oserror_each_by_name(edit, what):
    cfg = dict(LARGE, position_embeddings_type="rotary")
    for k, v in edit.items():
        if v is None:
            cfg.pop(k)
        else:
            cfg[k] = v
    with pytest.raises(OSError, match=what.replace("(", r"\(")) as e:
        C.geometry_from_config(cfg, name="x/y")
    assert "x/y" in str(e.value)


def test_w2v_bert_still_refuses_the_other_position_types():
    for pos in ("rotary", "relative"):
        with pytest.raises(OSError, match="position_embeddings_type"):
            C.geometry_from_config(dict(model_type="wav2vec2-bert", hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                                        intermediate_size=256, position_embeddings_type=pos), name="x")


def test_the_heads_that_are_not_built_stay_refused_and_the_classifier_is_accepted():
    with pytest.raises(OSError, match="Wav2Vec2ConformerForCTC"):
        C.CTCSpec.from_config({"architectures": ["Wav2Vec2ConformerForCTC"], "vocab_size": 32, "pad_token_id": 0}, name="x/y")
    with pytest.raises(OSError, match="Wav2Vec2ConformerForXVector"):
        C.XVectorSpec.from_config({"architectures": ["Wav2Vec2ConformerForXVector"]}, name="x/y")
    spec = C.ClassifierSpec.from_config(dict(LARGE, architectures=["Wav2Vec2ConformerForSequenceClassification"], num_labels=3,
                                             classifier_proj_size=48, use_weighted_layer_sum=True))
    assert spec is not None and spec.architecture == "Wav2Vec2ConformerForSequenceClassification"
    assert (spec.num_labels, spec.classifier_proj_size, spec.use_weighted_layer_sum) == (3, 48, True)


def test_batch_norm_fold_equals_torch_eval_in_float64():
    geo = C.TINY_W2V_CONFORMER_REL
    sd = W.synthetic_state_dict(geo, 5)
    p = "encoder.layers.1.conv_module.batch_norm"
    var, mean = sd[p + ".running_var"], sd[p + ".running_mean"]
    assert float(var.min()) >= 0.25 and float(var.max()) <= 4.0 and float(mean.abs().max()) > 0.1        # the fold is exercised, and cannot amplify
    bn = torch.nn.BatchNorm1d(geo.hidden).double().eval()
    bn.load_state_dict({k: sd[f"{p}.{k}"].double() for k in ("weight", "bias", "running_mean", "running_var")}, strict=False)
    x = torch.randn(7, geo.hidden, 11, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    # the fold itself in float64 (the statement's), then the fp32 pair the kernel reads: one rounding of each number
    s64, h64 = R.batch_norm_affine({k: v.double() for k, v in sd.items()}, p)
    with torch.no_grad():
        ref = bn(x)
    assert float((x * s64[None, :, None] + h64[None, :, None] - ref).abs().max()) < 1e-12
    s32, h32 = W.fold_batch_norm(sd[p + ".weight"], sd[p + ".bias"], mean, var, 1e-5)
    assert s32.dtype == h32.dtype == torch.float32
    assert torch.equal(s32, s64.float()) and torch.equal(h32, h64.float())


def test_pos_bias_u_fold():
    bq, u = torch.randn(128), torch.randn(2, 64)
    got = W.fold_pos_bias_u(bq, u)
    assert got.dtype == torch.float32 and torch.equal(got, (bq.double() + u.double().reshape(-1)).float())


def half_ulp32(ref64: np.ndarray) -> np.ndarray:
    return 0.5 * np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def test_rotary_tables_equal_hf_modules_buffers():
    import transformers as tf
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerRotaryPositionalEmbedding as Rot
    cfg = tf.Wav2Vec2ConformerConfig(hidden_size=128, num_attention_heads=2, rotary_embedding_base=10000)
    mod = Rot(cfg)
    inv = W.rotary_inv_freq(64, 10000)
    assert torch.equal(inv, mod.inv_freq)                                # HF's own fp32 expression
    T = 530
    hf = mod.double()(torch.zeros(1, T, 128, dtype=torch.float64))       # [2, T, 1, 1, dh] float64 from the fp32 inv_freq
    cos, sin = W.rotary_tables(T, inv)
    for mine, ref in ((cos, hf[0, :, 0, 0]), (sin, hf[1, :, 0, 0])):
        assert mine.dtype == torch.float32 and tuple(mine.shape) == (T, 64)
        assert bool((np.abs(mine.numpy().astype(np.float64) - ref.numpy()) <= half_ulp32(ref.numpy())).all())
    # a row is the same bits for any table length
    c2, s2 = W.rotary_tables(37, inv)
    assert torch.equal(c2, cos[:37]) and torch.equal(s2, sin[:37])


def test_relative_pe_rows_equal_hf_modules_buffer():
    """HF builds pe in fp32 (torch's sin / cos of the fp32 product r div) at construction; the host's rows repeat that arithmetic a row at
    a time.  Two fp32 numbers within half an ulp of each other are the same number."""
    import transformers as tf
    from transformers.models.wav2vec2_conformer.modeling_wav2vec2_conformer import Wav2Vec2ConformerRelPositionalEmbedding as Rel
    D, T = 192, 300
    mod = Rel(tf.Wav2Vec2ConformerConfig(hidden_size=D, num_attention_heads=3, max_source_positions=T))
    hf = mod(torch.zeros(1, T, D))[0]
    assert tuple(hf.shape) == (2 * T - 1, D)
    hf_by_r = torch.flip(hf, [0]).numpy().astype(np.float64)             # HF's row 0 is r = T - 1: positive distances first
    mine = W.relpos_pe(T, D)                                             # row T - 1 + r
    assert mine.dtype == torch.float32 and tuple(mine.shape) == (2 * T - 1, D)
    assert bool((np.abs(mine.numpy().astype(np.float64) - hf_by_r) <= half_ulp32(hf_by_r)).all())
    # a row for distance r is the same bits for any table length
    small = W.relpos_pe(41, D)
    assert torch.equal(small, mine[T - 41: T + 40])
    # ... and the statement's float64 rows are the exact functions of the same fp32 arguments: within torch's fp32 function error (1 ulp)
    exact = R.relpos_pe(T, D).numpy()
    ulp = np.spacing(np.maximum(np.abs(exact), 1e-30).astype(np.float32)).astype(np.float64)
    assert bool((np.abs(mine.numpy().astype(np.float64) - exact) <= ulp).all())


def test_key_normalisation_drops_what_lies_off_the_encoder_path():
    geo = C.TINY_W2V_CONFORMER_ROPE
    sd = W.synthetic_state_dict(geo, 3)
    wrapped = {"wav2vec2_conformer." + k: v for k, v in sd.items()}
    wrapped.update({"wav2vec2_conformer.masked_spec_embed": torch.zeros(4), "quantizer.codevectors": torch.zeros(4),
                    "project_hid.weight": torch.zeros(4), "project_q.weight": torch.zeros(4), "lm_head.weight": torch.zeros(4)})
    out = W.normalize_names(wrapped)
    assert sorted(out) == sorted(sd)


def test_synthetic_state_dict_has_hf_names(golden_dir):
    """every tensor of the synthetic dict is one HF's module tree holds, with its shape (what load_state_dict checked when the fixtures
    were made), and the relative type adds linear_pos and the two biases"""
    rope, rel = (W.synthetic_state_dict(g, 1) for g in (C.TINY_W2V_CONFORMER_ROPE, C.TINY_W2V_CONFORMER_REL))
    a = "encoder.layers.0.self_attn."
    assert a + "linear_pos.weight" not in rope and tuple(rel[a + "linear_pos.weight"].shape) == (192, 192)
    assert tuple(rel[a + "pos_bias_u"].shape) == tuple(rel[a + "pos_bias_v"].shape) == (3, 64)
    assert tuple(rope["encoder.layers.1.conv_module.depthwise_conv.weight"].shape) == (128, 1, 31)
    assert not any("pos_conv_embed" in k for k in rope)
