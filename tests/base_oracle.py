"""Independent fp32 restatement of the *-base speech forward (GroupNorm stem, post-LayerNorm encoder) -- test helper.

What ``WavLMModel`` / ``Wav2Vec2Model`` / ``HubertModel`` built from the transformers config defaults compute for ONE utterance
(the reference runs batch = 1, preprocess_speech.py:76-81), written with plain ``F.conv1d`` / ``F.group_norm`` / ``F.layer_norm``:

  conv layer 0:   Conv1d(1, C, 10, 5) -> GroupNorm(C groups = C channels, over time, eps 1e-5, affine) -> GELU
  conv layer 1-6: Conv1d -> GELU
  projection:     LayerNorm(C) -> Linear(C, D)
  encoder:        x = LN_enc(p + posconv(p))                 = hidden_states[0]
  layer i:        h = LN1(x + Attn(x));  x = LN2(h + FFN(h))  = hidden_states[i + 1]   (no final LayerNorm)

WavLM's attention adds the bucketed relative-position bias of layer 0, scaled per query by the GRU gate of the attention's input.
tests/test_base_family_host.py pins this file to the HF fixtures (tests/golden/tiny_*_base_*.npz); the GPU tests compare against it.
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

StateDict = Dict[str, torch.Tensor]


def normalize_wave(wave: np.ndarray) -> np.ndarray:
    """Wav2Vec2FeatureExtractor's do_normalize: (x - mean) / sqrt(var + 1e-7), numpy fp32."""
    x = np.asarray(wave, dtype=np.float32)
    return ((x - x.mean()) / np.sqrt(x.var() + 1e-7)).astype(np.float32)


def conv_stem(geo, sd: StateDict, x: torch.Tensor) -> torch.Tensor:
    """[L] samples -> [T, C] features of the GroupNorm feature encoder."""
    h = x.to(torch.float32)[None, None, :]
    for i, (k, s) in enumerate(zip(geo.conv_kernel, geo.conv_stride)):
        p = f"feature_extractor.conv_layers.{i}"
        h = F.conv1d(h, sd[p + ".conv.weight"], sd.get(p + ".conv.bias"), stride=s)
        if i == 0:
            h = F.group_norm(h, h.shape[1], sd[p + ".layer_norm.weight"], sd[p + ".layer_norm.bias"], eps=1e-5)
        h = F.gelu(h)
    return h[0].transpose(0, 1).contiguous()


def conv0_groupnorm_stats(geo, sd: StateDict, x: torch.Tensor):
    """fp64 per-channel (mean, rstd) of conv layer 0's output over the utterance: what GroupNorm(C, C) normalises with."""
    w = sd["feature_extractor.conv_layers.0.conv.weight"].double()
    b = sd.get("feature_extractor.conv_layers.0.conv.bias")
    y = F.conv1d(x.double()[None, None, :], w, None if b is None else b.double(), stride=geo.conv_stride[0])[0]   # [C, T]
    mean = y.mean(dim=1)
    var = y.var(dim=1, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def _pos_conv(geo, sd: StateDict, h: torch.Tensor) -> torch.Tensor:
    base = "encoder.pos_conv_embed.conv."
    if base + "parametrizations.weight.original0" in sd:
        g, v = sd[base + "parametrizations.weight.original0"], sd[base + "parametrizations.weight.original1"]
        w = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
    else:
        w = sd[base + "weight"]
    k = geo.pos_conv_kernel
    y = F.conv1d(h.transpose(0, 1)[None], w, sd[base + "bias"], padding=k // 2, groups=geo.pos_conv_groups)
    if k % 2 == 0:
        y = y[:, :, :-1]
    return F.gelu(y)[0].transpose(0, 1)


def _buckets(rel: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    nb = num_buckets // 2
    ret = (rel > 0).to(torch.long) * nb
    n = rel.abs()
    exact = nb // 2
    large = exact + (torch.log(n.float() / exact) / math.log(max_distance / exact) * (nb - exact)).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return ret + torch.where(n < exact, n, large)


def _attention(geo, sd: StateDict, a: str, x: torch.Tensor, bias: torch.Tensor = None) -> torch.Tensor:
    T, H = x.shape[0], geo.heads
    dh = geo.hidden // H

    def heads(t):
        return t.view(T, H, dh).permute(1, 0, 2)

    q = heads(F.linear(x, sd[a + ".q_proj.weight"], sd[a + ".q_proj.bias"]))
    k = heads(F.linear(x, sd[a + ".k_proj.weight"], sd[a + ".k_proj.bias"]))
    v = heads(F.linear(x, sd[a + ".v_proj.weight"], sd[a + ".v_proj.bias"]))
    scores = torch.matmul(q * dh ** -0.5, k.transpose(1, 2))
    if bias is not None:                                    # WavLM: gate(x) * relative-position bias, per head and query
        g = F.linear(heads(x), sd[a + ".gru_rel_pos_linear.weight"], sd[a + ".gru_rel_pos_linear.bias"]).view(H, T, 2, 4).sum(-1)
        ga, gb = torch.sigmoid(g).unbind(-1)
        gate = ga * (gb * sd[a + ".gru_rel_pos_const"].view(H, 1) - 1.0) + 2.0
        scores = scores + gate[:, :, None] * bias
    ctx = torch.matmul(torch.softmax(scores, dim=-1), v).permute(1, 0, 2).reshape(T, H * dh)
    return F.linear(ctx, sd[a + ".out_proj.weight"], sd[a + ".out_proj.bias"])


def hidden_states(geo, sd: StateDict, input_values: torch.Tensor) -> List[torch.Tensor]:
    """One (already normalised, when the checkpoint normalises) waveform [L] -> the L+1 hidden states [T, D]."""
    eps = geo.layer_norm_eps
    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)   # noqa: E731
    feats = conv_stem(geo, sd, input_values)
    if geo.feat_proj_layer_norm:
        feats = ln(feats, "feature_projection.layer_norm")
    p = F.linear(feats, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"])
    x = ln(p + _pos_conv(geo, sd, p), "encoder.layer_norm")
    T = x.shape[0]
    bias = None
    if geo.family == "wavlm":
        rel = torch.arange(T)[None, :] - torch.arange(T)[:, None]                     # key - query
        emb = sd["encoder.layers.0.attention.rel_attn_embed.weight"]
        bias = emb[_buckets(rel, geo.num_buckets, geo.max_bucket_distance)].permute(2, 0, 1)   # [H, T, T]
    states = [x]
    for i in range(geo.num_layers):
        pre = f"encoder.layers.{i}"
        h = ln(x + _attention(geo, sd, pre + ".attention", x, bias), pre + ".layer_norm")
        ff = F.linear(F.gelu(F.linear(h, sd[pre + ".feed_forward.intermediate_dense.weight"],
                                      sd[pre + ".feed_forward.intermediate_dense.bias"])),
                      sd[pre + ".feed_forward.output_dense.weight"], sd[pre + ".feed_forward.output_dense.bias"])
        x = ln(h + ff, pre + ".final_layer_norm")
        states.append(x)
    return states
