"""Frozen-encoder weights: HuggingFace state-dict names in, plain fp32 tensors out.

The reference obtains weights with ``AutoModel.from_pretrained(--ssl_type)``
(preprocess_speech.py:112, preprocess_whisper.py:120).  There is no network in
the build or benchmark environment, so two sources are supported:

* ``load_checkpoint(path)``   -- a local ``*.safetensors`` / ``pytorch_model.bin``
  (file or HF snapshot directory) using the hub's parameter names, so a real
  checkpoint drops in unchanged;
* ``synthetic_state_dict(geo, seed)`` -- seeded random tensors of the same names
  and shapes (benchmarks, parity tests).  Scales are chosen so that every code
  path carries signal: non-unit LayerNorm affine, peaky attention, non-trivial
  relative-position bias and gate.
"""
from __future__ import annotations

import math
import os
from typing import Dict

import numpy as np
import torch

from .config import (EncoderGeometry, FAMILY_DEBERTA, FAMILY_ROBERTA, FAMILY_W2V_BERT, FAMILY_W2V_CONFORMER, FAMILY_WAVLM,
                     FAMILY_WHISPER)

StateDict = Dict[str, torch.Tensor]


class _Rng:
    """numpy PCG64 stream: unlike torch's CPU ``randn`` (whose vectorised fill depends on the
    host's SIMD width) it yields the same numbers in the build container and on the GPU box."""

    def __init__(self, seed: int, fast: bool = False):
        self.g = np.random.default_rng(int(seed))
        # fast: torch's vectorised CPU generator (several GB/s instead of numpy's ~0.3) for throughput-only runs of the multi-billion
        # parameter geometries (bench.py other_encoders); NOT stable across hosts, so never used where a digest or an oracle compares
        self.t = torch.Generator().manual_seed(int(seed)) if fast else None

    def normal(self, *shape, std=1.0, mean=0.0):
        if self.t is not None:
            return torch.randn(*shape, generator=self.t) * std + mean
        x = self.g.standard_normal(size=shape, dtype=np.float32)
        return torch.from_numpy(x) * std + mean


def _linear(sd, r, name, out_f, in_f, gain=0.7, bias=True):
    sd[name + ".weight"] = r.normal(out_f, in_f, std=gain / math.sqrt(in_f))
    if bias:
        sd[name + ".bias"] = r.normal(out_f, std=0.05)


def _layer_norm(sd, r, name, dim):
    sd[name + ".weight"] = r.normal(dim, std=0.1, mean=1.0)
    sd[name + ".bias"] = r.normal(dim, std=0.1)


def whisper_sinusoids(length: int, channels: int) -> torch.Tensor:
    """Whisper's frozen position table at init (HF modeling_whisper.py:55-64)."""
    inc = math.log(10000.0) / (channels // 2 - 1)
    inv = np.exp(-inc * np.arange(channels // 2, dtype=np.float64))
    t = np.arange(length, dtype=np.float64)[:, None] * inv[None, :]
    # float64 then one rounding: bit-identical on every host (fixture digests depend on it)
    return torch.from_numpy(np.concatenate([np.sin(t), np.cos(t)], axis=1).astype(np.float32))


def synthetic_decoder_state_dict(geo: EncoderGeometry, seed: int = 0, fast: bool = False) -> StateDict:
    """Seeded ``decoder.*`` tensors of a Whisper checkpoint (HF names and shapes; ``proj_out`` is tied to ``embed_tokens``, so it has no
    tensor).  Scales chosen so that greedy decoding carries signal: token embeddings of N(0, 0.08) and learned positions of N(0, 1), so
    that a step's output follows the position and the attended context rather than repeating the token it was fed (tied embeddings make
    a large E[t] . E[t] win the next argmax); q / k projections at gain 1.6 (peaky attention), v / out projections at 0.7 in both
    attentions."""
    r = _Rng(seed, fast)
    sd: StateDict = {}
    D, Fd = geo.hidden, geo.decoder_ffn_dim
    sd["decoder.embed_tokens.weight"] = r.normal(geo.decoder_vocab_size, D, std=0.08)
    sd["decoder.embed_positions.weight"] = r.normal(geo.max_target_positions, D, std=1.0)
    for i in range(geo.decoder_layers):
        p = f"decoder.layers.{i}"
        for a in (".self_attn", ".encoder_attn"):
            _layer_norm(sd, r, p + a + "_layer_norm", D)
            _linear(sd, r, p + a + ".q_proj", D, D, gain=1.6)
            _linear(sd, r, p + a + ".k_proj", D, D, gain=1.6, bias=False)
            _linear(sd, r, p + a + ".v_proj", D, D)
            _linear(sd, r, p + a + ".out_proj", D, D)
        _layer_norm(sd, r, p + ".final_layer_norm", D)
        _linear(sd, r, p + ".fc1", Fd, D)
        _linear(sd, r, p + ".fc2", D, Fd)
    _layer_norm(sd, r, "decoder.layer_norm", D)
    return sd


def synthetic_state_dict(geo: EncoderGeometry, seed: int = 0, fast: bool = False) -> StateDict:
    r = _Rng(seed, fast)
    sd: StateDict = {}
    D, H, Fd, dh = geo.hidden, geo.heads, geo.ffn, geo.head_dim
    if geo.family == FAMILY_ROBERTA:
        sd["embeddings.word_embeddings.weight"] = r.normal(geo.vocab_size, D, std=0.5)
        sd["embeddings.position_embeddings.weight"] = r.normal(geo.max_positions, D, std=0.3)
        sd["embeddings.token_type_embeddings.weight"] = r.normal(geo.type_vocab_size, D, std=0.2)
        _layer_norm(sd, r, "embeddings.LayerNorm", D)
        for i in range(geo.num_layers):
            p = f"encoder.layer.{i}"
            _linear(sd, r, p + ".attention.self.query", D, D, gain=1.6)
            _linear(sd, r, p + ".attention.self.key", D, D, gain=1.6)
            _linear(sd, r, p + ".attention.self.value", D, D)
            _linear(sd, r, p + ".attention.output.dense", D, D)
            _layer_norm(sd, r, p + ".attention.output.LayerNorm", D)
            _linear(sd, r, p + ".intermediate.dense", Fd, D)
            _linear(sd, r, p + ".output.dense", D, Fd)
            _layer_norm(sd, r, p + ".output.LayerNorm", D)
        return sd
    if geo.family == FAMILY_DEBERTA:       # HF DebertaV2Model names (v3 settings: shared q/k position projections)
        sd["embeddings.word_embeddings.weight"] = r.normal(geo.vocab_size, D, std=0.5)
        _layer_norm(sd, r, "embeddings.LayerNorm", D)
        sd["encoder.rel_embeddings.weight"] = r.normal(2 * geo.position_buckets, D, std=0.4)
        _layer_norm(sd, r, "encoder.LayerNorm", D)
        if geo.text_conv_kernel:           # DebertaV2Encoder.conv (ConvLayer): Conv1d(D, D, k) over tokens + its LayerNorm
            k = geo.text_conv_kernel
            sd["encoder.conv.conv.weight"] = r.normal(D, D, k, std=0.7 / math.sqrt(D * k))
            sd["encoder.conv.conv.bias"] = r.normal(D, std=0.05)
            _layer_norm(sd, r, "encoder.conv.LayerNorm", D)
        for i in range(geo.num_layers):
            p = f"encoder.layer.{i}"
            _linear(sd, r, p + ".attention.self.query_proj", D, D, gain=1.6)
            _linear(sd, r, p + ".attention.self.key_proj", D, D, gain=1.6)
            _linear(sd, r, p + ".attention.self.value_proj", D, D)
            _linear(sd, r, p + ".attention.output.dense", D, D)
            _layer_norm(sd, r, p + ".attention.output.LayerNorm", D)
            _linear(sd, r, p + ".intermediate.dense", Fd, D)
            _linear(sd, r, p + ".output.dense", D, Fd)
            _layer_norm(sd, r, p + ".output.LayerNorm", D)
        return sd
    if geo.family == FAMILY_WHISPER:
        sd["encoder.conv1.weight"] = r.normal(D, geo.n_mels, 3, std=math.sqrt(2.0 / (geo.n_mels * 3)))
        sd["encoder.conv1.bias"] = r.normal(D, std=0.05)
        sd["encoder.conv2.weight"] = r.normal(D, D, 3, std=math.sqrt(2.0 / (D * 3)))
        sd["encoder.conv2.bias"] = r.normal(D, std=0.05)
        sd["encoder.embed_positions.weight"] = whisper_sinusoids(geo.max_source_positions, D)
        for i in range(geo.num_layers):
            p = f"encoder.layers.{i}"
            _layer_norm(sd, r, p + ".self_attn_layer_norm", D)
            _linear(sd, r, p + ".self_attn.q_proj", D, D, gain=1.6)
            _linear(sd, r, p + ".self_attn.k_proj", D, D, gain=1.6, bias=False)
            _linear(sd, r, p + ".self_attn.v_proj", D, D)
            _linear(sd, r, p + ".self_attn.out_proj", D, D)
            _layer_norm(sd, r, p + ".final_layer_norm", D)
            _linear(sd, r, p + ".fc1", Fd, D)
            _linear(sd, r, p + ".fc2", D, Fd)
        _layer_norm(sd, r, "encoder.layer_norm", D)
        return sd

    if geo.family == FAMILY_W2V_BERT:      # HF Wav2Vec2BertModel names; a branch of its own, the other families' streams stay as they were
        K, P = geo.conv_depthwise_kernel, geo.distance_positions
        _layer_norm(sd, r, "feature_projection.layer_norm", geo.fbank_dim)
        _linear(sd, r, "feature_projection.projection", D, geo.fbank_dim)
        for i in range(geo.num_layers):
            p = f"encoder.layers.{i}"
            for f in ("ffn1", "ffn2"):
                _layer_norm(sd, r, f"{p}.{f}_layer_norm", D)
                _linear(sd, r, f"{p}.{f}.intermediate_dense", Fd, D)
                _linear(sd, r, f"{p}.{f}.output_dense", D, Fd)
            _layer_norm(sd, r, p + ".self_attn_layer_norm", D)
            _linear(sd, r, p + ".self_attn.linear_q", D, D, gain=1.6)
            _linear(sd, r, p + ".self_attn.linear_k", D, D, gain=1.6)
            _linear(sd, r, p + ".self_attn.linear_v", D, D)
            _linear(sd, r, p + ".self_attn.linear_out", D, D)
            # q rows have |q| ~ 1.6 sqrt(dh) / ... ; N(0, 0.3) entries make the bias a logit term of the size of q . k's spread
            sd[p + ".self_attn.distance_embedding.weight"] = r.normal(P, dh, std=0.3)
            c = p + ".conv_module"
            _layer_norm(sd, r, c + ".layer_norm", D)
            sd[c + ".pointwise_conv1.weight"] = r.normal(2 * D, D, 1, std=1.0 / math.sqrt(D))
            sd[c + ".depthwise_conv.weight"] = r.normal(D, 1, K, std=1.0 / math.sqrt(K))
            _layer_norm(sd, r, c + ".depthwise_layer_norm", D)
            sd[c + ".pointwise_conv2.weight"] = r.normal(D, D, 1, std=0.7 / math.sqrt(D))
            _layer_norm(sd, r, p + ".final_layer_norm", D)
        return sd

    cin = 1
    for i, (c, k) in enumerate(zip(geo.conv_dim, geo.conv_kernel)):
        p = f"feature_extractor.conv_layers.{i}"
        sd[p + ".conv.weight"] = r.normal(c, cin, k, std=math.sqrt(2.0 / (cin * k)))
        if geo.conv_bias:
            sd[p + ".conv.bias"] = r.normal(c, std=0.05)
        if geo.feat_extract_norm == "layer" or i == 0:     # "group": GroupNorm(C, C) on layer 0 only, same key names and [C] shapes
            _layer_norm(sd, r, p + ".layer_norm", c)
        cin = c
    if geo.feat_proj_layer_norm:
        _layer_norm(sd, r, "feature_projection.layer_norm", cin)
    _linear(sd, r, "feature_projection.projection", D, cin)

    if geo.family == FAMILY_W2V_CONFORMER:
        # HF Wav2Vec2ConformerModel names behind wav2vec2's stem and projection (above); no positional convolution (HF builds the module
        # and never calls it).  A branch of its own: the other families' streams stay as they were.
        K = geo.conv_depthwise_kernel
        _layer_norm(sd, r, "encoder.layer_norm", D)
        for i in range(geo.num_layers):
            p = f"encoder.layers.{i}"
            for f in ("ffn1", "ffn2"):
                _layer_norm(sd, r, f"{p}.{f}_layer_norm", D)
                _linear(sd, r, f"{p}.{f}.intermediate_dense", Fd, D)
                _linear(sd, r, f"{p}.{f}.output_dense", D, Fd)
            _layer_norm(sd, r, p + ".self_attn_layer_norm", D)
            _linear(sd, r, p + ".self_attn.linear_q", D, D, gain=1.6)
            _linear(sd, r, p + ".self_attn.linear_k", D, D, gain=1.6)
            _linear(sd, r, p + ".self_attn.linear_v", D, D)
            _linear(sd, r, p + ".self_attn.linear_out", D, D)
            if geo.position_type == "relative":
                # |P_h(r)| ~ 1.6 sqrt(dh / 2) like a key row, and u, v of the size of a query's entries: all four terms carry signal
                _linear(sd, r, p + ".self_attn.linear_pos", D, D, gain=1.6, bias=False)
                sd[p + ".self_attn.pos_bias_u"] = r.normal(H, dh, std=0.5)
                sd[p + ".self_attn.pos_bias_v"] = r.normal(H, dh, std=0.5)
            c = p + ".conv_module"
            _layer_norm(sd, r, c + ".layer_norm", D)
            sd[c + ".pointwise_conv1.weight"] = r.normal(2 * D, D, 1, std=1.0 / math.sqrt(D))
            sd[c + ".depthwise_conv.weight"] = r.normal(D, 1, K, std=1.0 / math.sqrt(K))
            _layer_norm(sd, r, c + ".batch_norm", D)
            sd[c + ".batch_norm.running_mean"] = r.normal(D, std=0.3)
            sd[c + ".batch_norm.running_var"] = torch.exp2(r.normal(D, std=1.0).clamp(-2.0, 2.0))      # in [0.25, 4]: the fold cannot amplify
            sd[c + ".pointwise_conv2.weight"] = r.normal(D, D, 1, std=0.7 / math.sqrt(D))
            _layer_norm(sd, r, p + ".final_layer_norm", D)
        return sd

    cg = D // geo.pos_conv_groups
    if geo.pos_conv_norm == "layer":
        # data2vec-audio: pos_conv_layers plain grouped convs (HF Data2VecAudioPositionalConvLayer; no weight norm, LayerNorm without
        # parameters).  A branch of its own: the other families' streams, and so their fixture digests, stay as they were.
        k = geo.pos_conv_kernel
        for j in range(geo.pos_conv_layers):
            p = f"encoder.pos_conv_embed.layers.{j}.conv"
            sd[p + ".weight"] = r.normal(D, cg, k, std=math.sqrt(2.0 / (cg * k)))
            sd[p + ".bias"] = r.normal(D, std=0.2)
        return _encoder_layers(sd, r, geo)
    v = r.normal(D, cg, geo.pos_conv_kernel, std=math.sqrt(2.0 / (cg * geo.pos_conv_kernel)))
    vnorm = np.sqrt((v.numpy().astype(np.float64) ** 2).sum(axis=(0, 1), keepdims=True)).astype(np.float32)
    g = torch.from_numpy(vnorm) * r.normal(1, 1, geo.pos_conv_kernel, std=0.1, mean=1.0)
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"] = g
    sd["encoder.pos_conv_embed.conv.parametrizations.weight.original1"] = v
    sd["encoder.pos_conv_embed.conv.bias"] = r.normal(D, std=0.05)
    return _encoder_layers(sd, r, geo)


def _encoder_layers(sd: StateDict, r: _Rng, geo: EncoderGeometry) -> StateDict:
    """encoder.layer_norm and the encoder layers of the wav2vec2-style families (after the positional embedding in the stream)."""
    D, H, Fd, dh = geo.hidden, geo.heads, geo.ffn, geo.head_dim
    _layer_norm(sd, r, "encoder.layer_norm", D)
    for i in range(geo.num_layers):
        p = f"encoder.layers.{i}"
        a = p + ".attention"
        _linear(sd, r, a + ".q_proj", D, D, gain=1.6)
        _linear(sd, r, a + ".k_proj", D, D, gain=1.6)
        _linear(sd, r, a + ".v_proj", D, D)
        _linear(sd, r, a + ".out_proj", D, D)
        if geo.family == FAMILY_WAVLM:
            sd[a + ".gru_rel_pos_const"] = r.normal(1, H, 1, 1, std=0.2, mean=1.0)
            sd[a + ".gru_rel_pos_linear.weight"] = r.normal(8, dh, std=0.3)
            sd[a + ".gru_rel_pos_linear.bias"] = r.normal(8, std=0.3)
            if i == 0:
                sd[a + ".rel_attn_embed.weight"] = r.normal(geo.num_buckets, H, std=1.0)
        _layer_norm(sd, r, p + ".layer_norm", D)
        _linear(sd, r, p + ".feed_forward.intermediate_dense", Fd, D)
        _linear(sd, r, p + ".feed_forward.output_dense", D, Fd)
        _layer_norm(sd, r, p + ".final_layer_norm", D)
    return sd


def apply_stress(sd: StateDict, geo: EncoderGeometry, kind: str) -> StateDict:
    """Deterministic edits of a synthetic wav2vec2-style state dict that reproduce what real checkpoints do to the
    residual stream and seeded Gaussian weights never do (fixtures ``tiny_*_outlier`` / ``tiny_*_rowmean``):

    * ``"outliers"``: two "massive activation" channels -- layer 0's feed-forward output writes +800 / -500 into them
      (1000x the other channels), their weight rows are 30x larger, and every later LayerNorm damps them with a
      small gamma, as trained models do;
    * ``"rowmean"``: a uniform offset on every channel (positional-conv bias +40, which passes its GELU unchanged; each
      feed-forward output bias +3; one attention LayerNorm bias x8), so that rows have |mean| >> std: the one-pass
      variance and the deferred-LayerNorm term ``acc - mean * colsum`` of csrc/gemm.hip cancel catastrophically
      unless the operands are stored shifted;
    * ``"sharp"``: q / k projections x4 (logits x16): near one-hot attention rows.
    """
    D = geo.hidden
    sd = {k: v.clone() for k, v in sd.items()}
    fc2 = "encoder.layers.{}.feed_forward.output_dense"
    if kind == "outliers":
        c1, c2 = 7, D - 5
        sd[fc2.format(0) + ".bias"][c1] += 800.0
        sd[fc2.format(0) + ".bias"][c2] -= 500.0
        sd[fc2.format(0) + ".weight"][c1] *= 30.0
        sd[fc2.format(0) + ".weight"][c2] *= 30.0
        for k in sd:
            if k.endswith("layer_norm.weight") and k.startswith("encoder."):
                sd[k][c1] = 0.05
                sd[k][c2] = -0.05
    elif kind == "rowmean":
        sd["encoder.pos_conv_embed.conv.bias"] += 40.0
        for i in range(geo.num_layers):
            sd[fc2.format(i) + ".bias"] += 3.0
        sd["encoder.layers.0.layer_norm.bias"] *= 8.0
    elif kind == "sharp":
        # sharp attention: query and key projections 4x larger -> logits 16x larger, softmax rows near one-hot -- what
        # trained checkpoints (and LoRA-scaled query projections) have and Gaussian weights do not.  A softmax weight moves
        # by (logit error) * ln 2, so this is the fixture that separates single-product q / k rounding from the fp32 reference.
        for i in range(geo.num_layers):
            for proj in ("q_proj", "k_proj"):
                for leaf in ("weight", "bias"):
                    sd[f"encoder.layers.{i}.attention.{proj}.{leaf}"] *= 4.0
    else:
        raise ValueError(f"unknown stress kind '{kind}'")
    return sd


_STRIP_PREFIXES = ("wavlm.", "wav2vec2_bert.", "wav2vec2_conformer.", "wav2vec2.", "hubert.", "data2vec_audio.", "model.", "roberta.", "deberta.")


def normalize_names(sd: StateDict, keep: tuple = ()) -> StateDict:
    """Strip task-head wrappers (``wav2vec2.`` / ``data2vec_audio.`` in *ForCTC checkpoints, ``model.``
    in WhisperForConditionalGeneration) and drop everything off the encoder path
    (decoder, lm_head, quantizer, masked_spec_embed).  ``keep``: name prefixes that stay all the same
    (``CTC_HEAD_PREFIXES`` for the CTC drivers, which read ``lm_head``)."""
    out: StateDict = {}
    for k, v in sd.items():
        for p in _STRIP_PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        if not (keep and k.startswith(tuple(keep))) and k.startswith(("decoder.", "lm_head", "proj_out", "quantizer", "project_", "masked_spec_embed", "pooler.",
                         "embeddings.position_ids")):
            continue
        out[k] = v.detach().to(torch.float32).contiguous()
    return out


CLASSIFIER_HEAD_KEYS = ("projector.weight", "projector.bias", "classifier.weight", "classifier.bias", "layer_weights")


def split_classifier_head(sd: StateDict):
    """(encoder tensors, head tensors) of a normalised state dict (``normalize_names`` / ``load_checkpoint``) of an audio-classification
    checkpoint.  The head's are the five of ``CLASSIFIER_HEAD_KEYS`` that are present (``layer_weights`` exists only with
    ``use_weighted_layer_sum``); every other tensor stays with the encoder, so a snapshot without a head comes back whole."""
    enc = {k: v for k, v in sd.items() if k not in CLASSIFIER_HEAD_KEYS}
    head = {k: sd[k] for k in CLASSIFIER_HEAD_KEYS if k in sd}
    return enc, head


def check_classifier_head(head_sd: StateDict, D: int, proj: int, num_labels: int, num_states: int, weighted: bool) -> None:
    """Names and shapes of the head tensors against the encoder width, ``classifier_proj_size``, the label count and L + 1."""
    want = {"projector.weight": (proj, D), "projector.bias": (proj,), "classifier.weight": (num_labels, proj),
            "classifier.bias": (num_labels,)}
    if weighted:
        want["layer_weights"] = (num_states,)
    for k, shape in want.items():
        if k not in head_sd:
            raise ValueError(f"{k} is missing from the checkpoint (an audio-classification head needs {', '.join(want)})")
        if tuple(head_sd[k].shape) != shape:
            raise ValueError(f"{k}: shape {tuple(head_sd[k].shape)}, expected {shape} (hidden width {D}, classifier_proj_size {proj}, "
                             f"{num_labels} labels, {num_states} hidden states)")


def xvector_head_keys(num_tdnn: int, weighted: bool) -> tuple:
    """the head tensors of an x-vector checkpoint under normalised names (HF *ForXVector; ``feature_extractor.weight`` is the head's
    Linear, not the encoder's ``feature_extractor.conv_layers.*``)"""
    keys = ["projector.weight", "projector.bias"]
    for i in range(num_tdnn):
        keys += [f"tdnn.{i}.kernel.weight", f"tdnn.{i}.kernel.bias"]
    keys += ["feature_extractor.weight", "feature_extractor.bias", "classifier.weight", "classifier.bias"]
    return tuple(keys + (["layer_weights"] if weighted else []))


def split_xvector_head(sd: StateDict):
    """(encoder tensors, head tensors) of a normalised state dict of an x-vector checkpoint.  ``objective.*`` (the AMSoftmax training
    weight) is dropped; a snapshot without a head comes back whole."""
    def is_head(k: str) -> bool:
        return k in ("projector.weight", "projector.bias", "feature_extractor.weight", "feature_extractor.bias", "classifier.weight",
                     "classifier.bias", "layer_weights") or (k.startswith("tdnn.") and ".kernel." in k)
    enc = {k: v for k, v in sd.items() if not is_head(k) and not k.startswith("objective.")}
    head = {k: v for k, v in sd.items() if is_head(k)}
    return enc, head


def check_xvector_head(head_sd: StateDict, D: int, spec, num_states: int) -> None:
    """Names and shapes of the head tensors against the encoder width, the TDNN lists, ``xvector_output_dim`` and L + 1; the label count
    is the classifier's own (``ValueError`` naming the key)."""
    dims, n = tuple(spec.tdnn_dim), len(spec.tdnn_dim)
    want = {"projector.weight": (dims[0], D), "projector.bias": (dims[0],)}
    for i in range(n):
        d_in = dims[i - 1] if i > 0 else dims[0]
        want[f"tdnn.{i}.kernel.weight"] = (dims[i], d_in * spec.tdnn_kernel[i])
        want[f"tdnn.{i}.kernel.bias"] = (dims[i],)
    want["feature_extractor.weight"] = (spec.xvector_output_dim, 2 * dims[-1])
    want["feature_extractor.bias"] = (spec.xvector_output_dim,)
    labels = int(head_sd["classifier.weight"].shape[0]) if "classifier.weight" in head_sd and head_sd["classifier.weight"].dim() == 2 else 0
    want["classifier.weight"] = (labels, spec.xvector_output_dim)
    want["classifier.bias"] = (labels,)
    if spec.use_weighted_layer_sum:
        want["layer_weights"] = (num_states,)
    for k, shape in want.items():
        if k not in head_sd:
            raise ValueError(f"{k} is missing from the checkpoint (an x-vector head needs {', '.join(want)})")
        if tuple(head_sd[k].shape) != shape or 0 in shape:
            raise ValueError(f"{k}: shape {tuple(head_sd[k].shape)}, expected {shape} (hidden width {D}, tdnn_dim {dims}, tdnn_kernel "
                             f"{tuple(spec.tdnn_kernel)}, xvector_output_dim {spec.xvector_output_dim}, {num_states} hidden states)")


CTC_HEAD_KEYS = ("lm_head.weight", "lm_head.bias")
CTC_HEAD_PREFIXES = ("lm_head.",)


def split_ctc_head(sd: StateDict):
    """(encoder tensors, head tensors) of a state dict of a CTC checkpoint normalised with ``keep=CTC_HEAD_PREFIXES`` (plain
    ``normalize_names`` drops ``lm_head``).  A snapshot without a head comes back whole."""
    enc = {k: v for k, v in sd.items() if k not in CTC_HEAD_KEYS}
    head = {k: sd[k] for k in CTC_HEAD_KEYS if k in sd}
    return enc, head


def check_ctc_head(head_sd: StateDict, D: int, vocab_size: int) -> None:
    """Names and shapes of the head tensors against the encoder width and ``vocab_size`` (``ValueError`` naming the key)."""
    want = {"lm_head.weight": (vocab_size, D), "lm_head.bias": (vocab_size,)}
    for k, shape in want.items():
        if k not in head_sd:
            raise ValueError(f"{k} is missing from the checkpoint (a CTC head needs {', '.join(want)})")
        if tuple(head_sd[k].shape) != shape:
            raise ValueError(f"{k}: shape {tuple(head_sd[k].shape)}, expected {shape} (hidden width {D}, vocab_size {vocab_size})")


def merge_lora(sd: StateDict, lora_alpha: float = 16.0) -> StateDict:
    """Fold PEFT LoRA adapters into their base weights (next row 8f-4).  The reference fine-tunes WavLM with
    ``LoraConfig(r=8, lora_alpha=16, target_modules=['q_proj','v_proj'])`` inside a classifier wrapper and extracts
    with ``ssl_model.wavlm.model`` in eval mode (preprocessing/preprocess_speech_pretrained.py:108-177): dropout is
    inactive, so every adapted Linear computes ``x W^T + (alpha/r) x A^T B^T`` = a plain Linear with
    ``W + (alpha/r) B A``.  Keys: ``<wrapper>.base_model.model.<name>.base_layer.weight|bias``,
    ``<name>.lora_A.<adapter>.weight`` [r, in], ``<name>.lora_B.<adapter>.weight`` [out, r]; the classifier head
    and anything else off the encoder are dropped later by ``normalize_names``.  ``alpha`` is not stored in a
    state dict (it lives in LoraConfig), hence the argument; r is read from A's shape.  A state dict without
    adapter keys is returned unchanged."""
    if not any(".lora_A." in k for k in sd):
        return sd
    out: StateDict = {}
    adapters = {}
    for k, v in sd.items():
        k2 = k
        for wrap in ("wavlm.base_model.model.", "whisper.base_model.model.", "base_model.model."):
            if k2.startswith(wrap):
                k2 = k2[len(wrap):]
                break
        if ".lora_A." in k2 or ".lora_B." in k2:
            mod, rest = k2.split(".lora_", 1)
            adapters.setdefault(mod, {})[rest[0]] = v.detach().to(torch.float64)
        elif ".lora_dropout" in k2 or ".lora_embedding" in k2 or k2.startswith("classifier."):
            continue
        else:
            out[k2.replace(".base_layer.", ".")] = v
    for mod, ab in adapters.items():
        if "A" not in ab or "B" not in ab or mod + ".weight" not in out:
            raise OSError(f"incomplete LoRA adapter for '{mod}'")
        a, b = ab["A"], ab["B"]
        scale = float(lora_alpha) / a.shape[0]
        out[mod + ".weight"] = (out[mod + ".weight"].detach().to(torch.float64) + scale * (b @ a)).to(torch.float32)
    return out


def load_checkpoint(path: str, lora_alpha: float = 16.0, keep: tuple = ()) -> StateDict:
    """Read a local checkpoint file or directory.  Raises ``OSError`` when nothing
    loadable is found -- the error class the reference's driver reports as
    "No pretrained model found" (preprocess_speech.py:115-117).  ``keep``: ``normalize_names``'s."""
    candidates = []
    if os.path.isdir(path):
        for fn in sorted(os.listdir(path)):
            if fn.endswith(".safetensors") or fn in ("pytorch_model.bin",):
                candidates.append(os.path.join(path, fn))
    elif os.path.isfile(path):
        candidates.append(path)
    if not candidates:
        raise OSError(f"no checkpoint (*.safetensors / pytorch_model.bin) under '{path}'")
    sd: StateDict = {}
    for fn in candidates:
        if fn.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd.update(load_file(fn, device="cpu"))
        else:
            sd.update(torch.load(fn, map_location="cpu", weights_only=True))
    return normalize_names(merge_lora(sd, lora_alpha), keep)


def fold_wavlm_gate(w8: torch.Tensor, b8: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, heads: int, head_dim: int):
    """Load-time fold of WavLM's GRU gate (HF modeling_wavlm.py:167-180: Linear(dh -> 8) on LayerNorm1(x) per head, the eight
    outputs summed in two fours) for ser_attention's in-kernel gate (ser_attention_args.gate_x): with the RAW layer input x of a
    row, its mean mu and rstd,
        pre_j[h] = rstd * (x_h . wg[2h + j] - mu * sum(wg[2h + j])) + t[h, j],      j = 0 (first four), 1 (last four)
    Returns (wg [2H, dh] = gamma-folded summed weights, t [H, 2] = beta . w_j + b_j), both float64.  The column sums the kernel
    subtracts are taken by the caller from the ROUNDED operand planes it uploads, like every deferred-LayerNorm GEMM's colsum."""
    w8, b8 = w8.detach().double(), b8.detach().double()
    wab = torch.stack([w8[:4].sum(0), w8[4:].sum(0)], 0)                               # [2, dh]
    gam, bet = gamma.detach().double().view(heads, 1, head_dim), beta.detach().double().view(heads, 1, head_dim)
    wg = (gam * wab[None]).reshape(2 * heads, head_dim)
    t = (bet * wab[None]).sum(2) + torch.stack([b8[:4].sum(), b8[4:].sum()])[None]
    return wg, t


def fold_w2v_bert_ffn(w: torch.Tensor, b: torch.Tensor):
    """The conformer layer adds HALF of each feed-forward block to the residual stream (HF Wav2Vec2BertEncoderLayer: ``x * 0.5 + residual``).
    The factor goes into the block's output Linear at load: 0.5 is a power of two, so every product and sum keeps its rounding."""
    return w.detach().to(torch.float32) * 0.5, b.detach().to(torch.float32) * 0.5


def fold_batch_norm(gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, eps: float = 1e-5):
    """``BatchNorm1d`` in eval is a per-channel affine: (scale, shift) with scale = gamma / sqrt(running_var + eps) and
    shift = beta - running_mean scale, in float64, each rounded to fp32 once (ser_conformer_conv_bn_v's operands)."""
    g, b, m, v = (t.detach().double() for t in (gamma, beta, mean, var))
    scale = g / torch.sqrt(v + float(eps))
    return scale.float(), (b - m * scale).float()


def fold_pos_bias_u(bq: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Transformer-XL's content bias into ``linear_q``'s bias: the projection emits q + u ([H, dh] flattened head-major, as the
    projection's columns are)."""
    return (bq.detach().double() + u.detach().double().reshape(-1)).float()


def rotary_inv_freq(head_dim: int, base: float = 10000.0) -> torch.Tensor:
    """HF's ``inv_freq`` buffer, by HF's own fp32 expression (Wav2Vec2ConformerRotaryPositionalEmbedding.__init__).  A checkpoint stores
    the buffer (``encoder.embed_positions.inv_freq``); where it does, the encoder reads that instead."""
    return 1.0 / (float(base) ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))


def rotary_tables(frames: int, inv_freq: torch.Tensor):
    """(cos, sin) fp32 [frames][dh] of HF's rotary embedding: cos / sin(t inv_freq) duplicated over the two halves, with the fp32
    ``inv_freq`` [dh / 2]; the products t inv_freq and the functions in float64 (numpy), rounded to fp32 once.  Row t depends on t alone:
    a longer table starts with the shorter one's bits."""
    inv = inv_freq.detach().to(torch.float32).cpu().numpy().astype(np.float64)
    ang = np.arange(int(frames), dtype=np.float64)[:, None] * inv[None, :]
    ang = np.concatenate([ang, ang], axis=1)
    return torch.from_numpy(np.cos(ang).astype(np.float32)), torch.from_numpy(np.sin(ang).astype(np.float32))


def relpos_div_term(hidden: int) -> torch.Tensor:
    """HF's fp32 ``div_term`` [D / 2], by HF's own expression (Wav2Vec2ConformerRelPositionalEmbedding.extend_pe)."""
    return torch.exp(torch.arange(0, hidden, 2, dtype=torch.int64).float() * -(math.log(10000.0) / hidden))


def relpos_pe(frames: int, hidden: int) -> torch.Tensor:
    """The sinusoid rows of Transformer-XL's relative positions, fp32 [2 frames - 1][D]: row ``frames - 1 + r`` is pe(r) for the distance
    r = i - j in -(frames - 1) .. frames - 1 (positive: the key is to the left), pe(r)[0::2] = sin(r div), pe(r)[1::2] = cos(r div).
    HF's arithmetic, statement for statement (fp32 position times the fp32 ``div_term``, torch's fp32 sin / cos), so that the rows are the
    bits of the buffer HF's module holds -- taken ONE ROW AT A TIME on a [D / 2] tensor: the row for r is then a function of r and D
    alone, the same bits whatever ``frames`` is (a vectorised function may treat the tail of a longer tensor differently)."""
    div = relpos_div_term(hidden)
    pe = torch.empty((2 * int(frames) - 1, hidden), dtype=torch.float32)
    for row, r in enumerate(range(-(int(frames) - 1), int(frames))):
        arg = torch.tensor(float(r), dtype=torch.float32) * div
        pe[row, 0::2] = torch.sin(arg)
        pe[row, 1::2] = torch.cos(arg)
    return pe


F16_MAX = 65504.0


def check_f16_weight(w: torch.Tensor, name: str) -> None:
    """Refuse, at load, a weight that fp16 operand planes cannot hold (the FP16 / FP16X / FP16M formats of the "f16*" modes).  The kernels
    saturate at +-65504 on the way in and the activations' range guard (ser_hip.h range_flag) never sees the weights, so a weight beyond
    that range, or a NaN / Inf, would be wrong in every output without a failure line.  ``w`` is the fp32 tensor actually split, e.g.
    after a LayerNorm gamma fold; ``name`` says which checkpoint tensor it came from."""
    w = w.detach()
    finite = torch.isfinite(w)
    if not bool(finite.all()):
        raise ValueError(f"{name}: {int((~finite).sum())} non-finite value(s); fp16 operand planes cannot hold them -- "
                         "use --mode fp32x to inspect the checkpoint")
    amax = float(w.abs().max()) if w.numel() else 0.0
    if amax > F16_MAX:
        raise ValueError(f"{name}: |value| up to {amax:.6g} exceeds the fp16 operand range ({F16_MAX:g}) and would saturate -- "
                         "use --mode fp32x (bf16 planes, fp32 range)")


def state_dict_digest(sd: StateDict) -> str:
    """Order-independent checksum of a state dict (fixtures record it so a drift of
    the RNG stream between containers is detected instead of silently compared)."""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]
