"""Writes tests/golden/tiny_xvec_<family>.npz (CPU, needs `transformers`): the HF x-vector classes (*ForXVector) on seeded weights.

TEST INFRASTRUCTURE ONLY.  Per fixture: the class's config as JSON text, a preprocessor_config, the encoder's weights as the seed and digest
of weights.synthetic_state_dict (tests/xvector_ref.py rebuilds the full state dict under HF names), the head tensors -- layer_weights,
projector, TDNN kernels, feature_extractor and classifier redrawn from normal distributions (He-scaled in front of the ReLUs), because the
default init makes the layer weights uniform and the embeddings tiny; objective.weight, the AMSoftmax training weight, as HF drew it --,
six waveforms as seeds and lengths: one whose TDNN output has exactly two rows, one with a single row (no expected output: it has no
unbiased std and must fail alone), four ragged ones up to 1 s; and per waveform with an output HF's `embeddings` and `logits` at batch
size 1 without padding and without an attention mask, the model in .double(), with the float64 hidden states.

Three geometries chosen so that no constant of one survives in another (TDNN widths 100 / 96, 72 / 128: the output-column and the
K padding live; kernels 5, 3, 1 / 3, 2 / 2; dilations 1, 2, 3 / 2 / 3; weighted sum on / off / on).

`gain_emb_<mode>` / `gain_logits_<mode>`: with eps the family's hidden-state gate for the mode (the tables at the top of
tests/test_gpu_audio_cls.py), the largest error by max|a - b| / max(1, max|b|) over the fixture's waveforms and 8 seeded sign-pattern
perturbations of the hidden states of size eps * max(1, max|hs|), pushed through tests/xvector_ref.py in float64.

    python tools/make_golden_xvector.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict  # noqa: E402
import xvector_ref as R                                                           # noqa: E402
from make_golden_audio_cls import front_end                                      # noqa: E402
from test_gpu_audio_cls import EPS_OTHER, EPS_SPEECH                             # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
RAGGED = (16000, 12345, 9000, 6007)
# tag, geometry, encoder seed, use_weighted_layer_sum, tdnn_dim, tdnn_kernel, tdnn_dilation, xvector_output_dim, num_labels, eps table
CASES = (
    ("tiny_xvec_wavlm", C.TINY_WAVLM, 51, True, (64, 64, 64, 64, 100), (5, 3, 3, 1, 1), (1, 2, 3, 1, 1), 24, 5, EPS_SPEECH),
    ("tiny_xvec_wavlm_base", C.TINY_WAVLM_BASE, 52, False, (96, 64, 72), (3, 2, 1), (2, 1, 1), 40, 3, EPS_SPEECH),
    ("tiny_xvec_w2v_bert", C.TINY_W2V_BERT, 53, True, (64, 128), (2, 1), (3, 1), 16, 7, EPS_OTHER),
)


def hf_model(geo, weighted, dims, kernel, dilation, out_dim, labels):
    import transformers as tf
    head = dict(use_weighted_layer_sum=weighted, tdnn_dim=list(dims), tdnn_kernel=list(kernel), tdnn_dilation=list(dilation),
                xvector_output_dim=out_dim, num_labels=labels)
    if geo.family == C.FAMILY_W2V_BERT:
        cfg = tf.Wav2Vec2BertConfig(
            hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads, intermediate_size=geo.ffn,
            feature_projection_input_dim=geo.fbank_dim, conv_depthwise_kernel_size=geo.conv_depthwise_kernel,
            left_max_position_embeddings=geo.left_max_positions, right_max_position_embeddings=geo.right_max_positions,
            layer_norm_eps=geo.layer_norm_eps, apply_spec_augment=False, **head)
        return tf.Wav2Vec2BertForXVector(cfg).eval()
    assert geo.family == C.FAMILY_WAVLM
    common = dict(hidden_size=geo.hidden, num_hidden_layers=geo.num_layers, num_attention_heads=geo.heads,
                  intermediate_size=geo.ffn, conv_dim=list(geo.conv_dim), conv_kernel=list(geo.conv_kernel),
                  conv_stride=list(geo.conv_stride), conv_bias=geo.conv_bias, feat_extract_norm=geo.feat_extract_norm,
                  do_stable_layer_norm=geo.stable_layer_norm, num_conv_pos_embeddings=geo.pos_conv_kernel,
                  num_conv_pos_embedding_groups=geo.pos_conv_groups, layer_norm_eps=geo.layer_norm_eps,
                  hidden_act="gelu", feat_extract_activation="gelu", vocab_size=32, apply_spec_augment=False, **head)
    return tf.WavLMForXVector(tf.WavLMConfig(num_buckets=geo.num_buckets, max_bucket_distance=geo.max_bucket_distance, **common)).eval()


def draw_head(D, L1, dims, kernel, out_dim, labels, weighted, seed) -> dict:
    g = np.random.default_rng(seed)
    f = lambda *shape, std=1.0: (g.standard_normal(shape) * std).astype(np.float32)           # noqa: E731
    head = {"projector.weight": f(dims[0], D, std=1.0 / np.sqrt(D)), "projector.bias": f(dims[0], std=0.5)}
    for i, k in enumerate(kernel):
        d_in = dims[i - 1] if i else dims[0]
        head[f"tdnn.{i}.kernel.weight"] = f(dims[i], k * d_in, std=np.sqrt(2.0 / (k * d_in)))
        head[f"tdnn.{i}.kernel.bias"] = f(dims[i], std=0.3)
    head["feature_extractor.weight"] = f(out_dim, 2 * dims[-1], std=1.0 / np.sqrt(2 * dims[-1]))
    head["feature_extractor.bias"] = f(out_dim, std=0.5)
    # HF: classifier = Linear(xvector_output_dim, xvector_output_dim); the label count only sizes objective.weight
    head["classifier.weight"] = f(out_dim, out_dim, std=1.0 / np.sqrt(out_dim))
    head["classifier.bias"] = f(out_dim, std=0.5)
    if weighted:
        head["layer_weights"] = f(L1)
    return head


def length_with_frames(geo, frames: int) -> int:
    """the shortest waveform the encoder turns into exactly ``frames`` rows"""
    n = 400
    while geo.frames_for(n) < frames:
        n += 1
    assert geo.frames_for(n) == frames
    return n


def make_case(tag, geo, seed, weighted, dims, kernel, dilation, out_dim, labels, eps_table):
    torch.manual_seed(0)
    model = hf_model(geo, weighted, dims, kernel, dilation, out_dim, labels)
    spec = C.XVectorSpec.from_config(dict(model.config.to_dict(), architectures=[type(model).__name__]))
    enc = synthetic_state_dict(geo, seed)
    fe, pre = front_end(geo)
    two, one = len(RAGGED), len(RAGGED) + 1
    lengths = RAGGED + (length_with_frames(geo, spec.min_frames), length_with_frames(geo, spec.min_frames - 1))
    wave_seeds = [8000 + 10 * seed + j for j in range(len(lengths))]
    cfg = model.config.to_dict()
    cfg["architectures"] = [type(model).__name__]
    head = draw_head(geo.hidden, geo.num_layers + 1, dims, kernel, out_dim, labels, weighted, seed * 100)
    head["objective.weight"] = model.objective.weight.detach().numpy().astype(np.float32).copy()
    sd = {R.WRAPPER[geo.family] + k: v for k, v in enc.items()}
    sd.update({k: torch.from_numpy(v) for k, v in head.items()})
    res = model.float().load_state_dict(sd, strict=False)
    extra = [k for k in res.missing_keys if "masked_spec_embed" not in k]
    assert not res.unexpected_keys and not extra, res
    rec = {"config": np.array(json.dumps(cfg, sort_keys=True)), "preprocessor": np.array(json.dumps(pre, sort_keys=True)),
           "seed": np.array(seed), "digest": np.array(state_dict_digest(enc)), "two": np.array(two), "one": np.array(one),
           "lengths": np.array(lengths, dtype=np.int64), "wave_seeds": np.array(wave_seeds, dtype=np.int64)}
    rec.update({"head." + k: v for k, v in head.items()})
    worst_id = 0.0
    gain = {m: [0.0, 0.0] for m in R.MODES}
    model.double()
    for j, (ws, ln) in enumerate(zip(wave_seeds, lengths)):
        if j == one:
            continue
        wave = R.synth_wave(ws, ln)
        inputs = fe(wave, sampling_rate=16000, return_tensors="pt")
        if geo.family == C.FAMILY_W2V_BERT:              # batch size 1 without padding: the frames the mask keeps, and no mask
            inputs = {"input_features": inputs["input_features"][:, inputs["attention_mask"][0].bool()]}
        else:
            inputs = {"input_values": inputs["input_values"]}
        with torch.no_grad():
            out = model(**{k: v.double() for k, v in inputs.items()}, output_hidden_states=True)
        hs = torch.stack([h[0] for h in out.hidden_states]).numpy()
        assert hs.dtype == np.float64 and hs.shape == (geo.num_layers + 1, geo.frames_for(ln), geo.hidden), (hs.shape, geo.frames_for(ln))
        e64, l64 = out.embeddings[0].numpy(), out.logits[0].numpy()
        e, l = R.head_outputs(hs, head, weighted, kernel, dilation)
        worst_id = max(worst_id, float(np.abs(e - e64).max() / np.abs(e64).max()), float(np.abs(l - l64).max() / np.abs(l64).max()))
        rec[f"emb64_{j}"], rec[f"logits64_{j}"], rec[f"states64_{j}"] = e64, l64, hs
        for m in R.MODES:
            ge, gl = R.gains(hs, head, weighted, kernel, dilation, eps_table[m], seed=1000 * seed + j)
            gain[m] = [max(gain[m][0], ge), max(gain[m][1], gl)]
    assert worst_id < 1e-10, worst_id
    assert hs.shape[1] - spec.context == 2                               # the last waveform with an output is the T' = 2 one
    for m in R.MODES:
        rec[f"gain_emb_{m}"], rec[f"gain_logits_{m}"] = np.array(gain[m][0]), np.array(gain[m][1])
    print(f"{tag}: lengths {lengths}, float64 statement vs HF float64 {worst_id:.1e}, gains " +
          ", ".join(f"{m} {gain[m][0]:.2e} / {gain[m][1]:.2e}" for m in R.MODES))
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
