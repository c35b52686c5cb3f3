"""Independent fp32 restatement of the data2vec-audio speech forward -- test helper.

What ``Data2VecAudioModel`` (transformers, models/data2vec/modeling_data2vec_audio.py) computes for ONE utterance (the reference
runs batch = 1, preprocess_speech.py:76-81), written with plain ``F.conv1d`` / ``F.layer_norm``:

  conv layers 0-6: Conv1d -> LayerNorm(C, eps 1e-5, affine) -> GELU   (Data2VecAudioConvLayer: the *-large layer-norm stem,
                   oracle/ssl_oracle.conv_feature_encoder)
  projection:      LayerNorm(C) -> Linear(C, D)                        (Data2VecAudioFeatureProjection, ssl_oracle.feature_projection)
  positional:      pos = x; num_conv_pos_embeddings times
                       pos = GELU(LayerNorm_noaffine(Conv1d(D, D, k, pad k // 2, groups)(pos)))   (Data2VecAudioPositionalConvLayer,
                   the LayerNorm with nn's default eps 1e-5; an even k would drop the last frame, Data2VecAudioPadLayer)
  encoder:         x = LN_enc(x + pos)                                 = hidden_states[0]  (Data2VecAudioEncoder.forward)
  layer i:         h = LN1(x + Attn(x));  x = LN2(h + FFN(h))          = hidden_states[i + 1]  (Data2VecAudioEncoderLayer, post-LN;
                   no final LayerNorm: tests/base_oracle.py's layer)

tests/test_data2vec_host.py pins this file to the HF fixtures (tests/golden/tiny_data2vec_audio_*.npz); the GPU tests compare against it.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F

import base_oracle as BO
from oracle import ssl_oracle as O

StateDict = Dict[str, torch.Tensor]

normalize_wave = BO.normalize_wave


def synth_wave(seed: int, n: int) -> np.ndarray:
    """The fixtures' waveforms (tools/make_golden_base.py's recipe): 0.1*N(0,1) + 220 Hz sine at 0.2 + a DC offset of 0.05, fp32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.05 + 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def positional_stack(geo, sd: StateDict, x: torch.Tensor) -> torch.Tensor:
    """[T, D] projection output -> [T, D] positional embedding (before the residual add)."""
    k = geo.pos_conv_kernel
    h = x.transpose(0, 1)[None]
    for j in range(geo.pos_conv_layers):
        p = f"encoder.pos_conv_embed.layers.{j}.conv"
        h = F.conv1d(h, sd[p + ".weight"], sd[p + ".bias"], padding=k // 2, groups=geo.pos_conv_groups)
        if k % 2 == 0:
            h = h[:, :, :-1]
        h = F.gelu(F.layer_norm(h.transpose(1, 2), (h.shape[1],), eps=1e-5).transpose(1, 2))
    return h[0].transpose(0, 1)


def hidden_states(geo, sd: StateDict, input_values: torch.Tensor) -> List[torch.Tensor]:
    """One (already normalised, when the checkpoint normalises) waveform [L] -> the L+1 hidden states [T, D]."""
    eps = geo.layer_norm_eps
    ln = lambda t, p: F.layer_norm(t, (t.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)   # noqa: E731
    feats = O.conv_feature_encoder(geo, sd, input_values.to(torch.float32))
    p = O.feature_projection(geo, sd, feats)
    x = ln(p + positional_stack(geo, sd, p), "encoder.layer_norm")
    states = [x]
    for i in range(geo.num_layers):
        pre = f"encoder.layers.{i}"
        h = ln(x + BO._attention(geo, sd, pre + ".attention", x), pre + ".layer_norm")
        x = ln(h + O.feed_forward(sd, pre + ".feed_forward.intermediate_dense", pre + ".feed_forward.output_dense", h),
               pre + ".final_layer_norm")
        states.append(x)
    return states
