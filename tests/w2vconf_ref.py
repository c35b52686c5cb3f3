"""float64 statement of the wav2vec2-conformer encoders (HF Wav2Vec2ConformerModel, one utterance alone, no padding and no mask): the
wav2vec2 convolutional stem and feature projection, and the conformer layer with rotary or Transformer-XL relative positions and a
centred depthwise convolution behind a BatchNorm in eval.  Test infrastructure, like tests/w2vbert_ref.py: written from the formulas of
include/ser_hip.h a35, pinned to the HF class by the fixtures of tools/make_golden_w2v_conformer.py, and the reference the GPU tests compare
kernels with.  numpy / torch on the CPU only; HF's layer is not imported."""
import math

import numpy as np
import torch

from w2vbert_ref import synth_wave  # noqa: F401  (the fixtures' waveforms)

BN_EPS = 1e-5
LAYER_EPS = 1e-5           # nn.LayerNorm's default: the stem's and the layer's norms; encoder.layer_norm and the projection's read the config


def normalize_wave(wave: np.ndarray) -> torch.Tensor:
    """Wav2Vec2FeatureExtractor(do_normalize=True): zero mean, unit (population) variance, in float64"""
    x = torch.from_numpy(np.asarray(wave, dtype=np.float32)).double()
    return (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)


def _ln(x, sd, p, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p, bias=True):
    w = sd[p + ".weight"]
    y = x @ w.reshape(w.shape[0], -1).T
    return y + sd[p + ".bias"] if bias else y


def swish(x):
    return x * torch.sigmoid(x)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def stem(geo, sd, x: torch.Tensor) -> torch.Tensor:
    """normalised samples [n] -> projected rows [T, D]: per conv layer Conv1d (no padding) -> LayerNorm over channels -> GELU, then
    LayerNorm -> Linear"""
    h = x[:, None]                                                       # [n, C_in]
    for i, (k, s) in enumerate(zip(geo.conv_kernel, geo.conv_stride)):
        p = f"feature_extractor.conv_layers.{i}"
        w = sd[p + ".conv.weight"]                                       # [C_out, C_in, k]
        T = (h.shape[0] - k) // s + 1
        win = torch.stack([h[j: j + (T - 1) * s + 1: s] for j in range(k)], dim=2)       # [T, C_in, k]
        y = torch.einsum("tck,ock->to", win, w)
        if geo.conv_bias:
            y = y + sd[p + ".conv.bias"]
        h = gelu(_ln(y, sd, p + ".layer_norm", LAYER_EPS))
    return _lin(_ln(h, sd, "feature_projection.layer_norm", geo.layer_norm_eps), sd, "feature_projection.projection")


def rotary_tables(T: int, dh: int, base: float):
    """float64 cos / sin [T, dh] of t inv_freq over both halves; inv_freq is HF's fp32 buffer"""
    inv = (1.0 / (float(base) ** (torch.arange(0, dh, 2, dtype=torch.int64).float() / dh))).double()
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], dim=1)
    return torch.cos(ang), torch.sin(ang)


def rotate(x: torch.Tensor, heads: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [T, D] -> per head of dh channels x cos + cat(-x[dh / 2:], x[:dh / 2]) sin; cos / sin [T, dh]"""
    T, D = x.shape
    dh = D // heads
    xh = x.view(T, heads, dh)
    rot = torch.cat([-xh[..., dh // 2:], xh[..., : dh // 2]], dim=-1)
    return (xh * cos[:, None, :] + rot * sin[:, None, :]).reshape(T, D)


def relpos_pe(T: int, D: int) -> torch.Tensor:
    """float64 [2 T - 1, D]: row T - 1 + r is pe(r), r = i - j; the argument r div is HF's fp32 product with its fp32 div_term"""
    div = torch.exp(torch.arange(0, D, 2, dtype=torch.int64).float() * -(math.log(10000.0) / D))
    r = torch.arange(-(T - 1), T, dtype=torch.int64).float()
    arg = (r[:, None] * div[None, :]).double()
    pe = torch.zeros(2 * T - 1, D, dtype=torch.float64)
    pe[:, 0::2] = torch.sin(arg)
    pe[:, 1::2] = torch.cos(arg)
    return pe


def relpos_scores(q, k, P, u, v):
    """q, k [H, T, dh]; P [H, 2 T - 1, dh] with row T - 1 + r = P_h(r); u, v [H, dh] -> [H, T, T] before the 1 / sqrt(dh):
    (q_i + u) . k_j + (q_i + v) . P(i - j)"""
    T = q.shape[1]
    pos = torch.arange(T)
    idx = pos[:, None] - pos[None, :] + (T - 1)                          # [i, j] -> row of P
    ac = (q + u[:, None, :]) @ k.transpose(1, 2)
    bd = torch.einsum("hid,hijd->hij", q + v[:, None, :], P[:, idx])
    return ac + bd


def attention(geo, x, sd, p):
    T, D = x.shape
    H, dh = geo.heads, D // geo.heads
    split = lambda t: t.view(T, H, dh).transpose(0, 1)
    if geo.position_type == "rotary":
        cos, sin = rotary_tables(T, dh, geo.rotary_base)
        xr = rotate(x, H, cos, sin)
        q, k, v = split(_lin(xr, sd, p + ".linear_q")), split(_lin(xr, sd, p + ".linear_k")), split(_lin(x, sd, p + ".linear_v"))
        s = q @ k.transpose(1, 2)
    else:
        q, k, v = (split(_lin(x, sd, p + ".linear_" + n)) for n in "qkv")
        P = _lin(relpos_pe(T, D), sd, p + ".linear_pos", bias=False).view(2 * T - 1, H, dh).transpose(0, 1)
        s = relpos_scores(q, k, P, sd[p + ".pos_bias_u"], sd[p + ".pos_bias_v"])
    ctx = (torch.softmax(s / math.sqrt(dh), dim=-1) @ v).transpose(0, 1).reshape(T, D)
    return _lin(ctx, sd, p + ".linear_out")


def batch_norm_affine(sd, p, eps=BN_EPS):
    scale = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + eps)
    return scale, sd[p + ".bias"] - sd[p + ".running_mean"] * scale


def conv_mid(y, w, scale, shift):
    """GLU of y [T, 2 D] -> depthwise conv with the window t - (K - 1) / 2 .. t + (K - 1) / 2 (zeros outside the utterance), w [D, K] ->
    per-channel affine -> swish"""
    T, D = y.shape[0], y.shape[1] // 2
    K = w.shape[1]
    g = y[:, :D] * torch.sigmoid(y[:, D:])
    half = (K - 1) // 2
    z = torch.zeros(half, D, dtype=y.dtype)
    gp = torch.cat([z, g, z], 0)
    u = torch.zeros_like(g)
    for k in range(K):
        u = u + gp[k: k + T] * w[:, k][None, :]
    return swish(u * scale + shift)


def conv_module(x, sd, p, K):
    D = x.shape[1]
    y = _lin(_ln(x, sd, p + ".layer_norm", LAYER_EPS), sd, p + ".pointwise_conv1", bias=False)
    scale, shift = batch_norm_affine(sd, p + ".batch_norm")
    return _lin(conv_mid(y, sd[p + ".depthwise_conv.weight"].reshape(D, K), scale, shift), sd, p + ".pointwise_conv2", bias=False)


def ffn(x, sd, p):
    return _lin(swish(_lin(x, sd, p + ".intermediate_dense")), sd, p + ".output_dense")


def hidden_states(geo, sd, rows: torch.Tensor):
    """The L + 1 hidden states [T, D] (float64) of the projected rows: state i < L is layer i's input, state L is encoder.layer_norm of
    the last layer's output."""
    x = rows
    states = []
    for i in range(geo.num_layers):
        states.append(x)
        p = f"encoder.layers.{i}"
        x = x + 0.5 * ffn(_ln(x, sd, p + ".ffn1_layer_norm", LAYER_EPS), sd, p + ".ffn1")
        x = x + attention(geo, _ln(x, sd, p + ".self_attn_layer_norm", LAYER_EPS), sd, p + ".self_attn")
        x = x + conv_module(x, sd, p + ".conv_module", geo.conv_depthwise_kernel)
        x = x + 0.5 * ffn(_ln(x, sd, p + ".ffn2_layer_norm", LAYER_EPS), sd, p + ".ffn2")
        x = _ln(x, sd, p + ".final_layer_norm", LAYER_EPS)
    states.append(_ln(x, sd, "encoder.layer_norm", geo.layer_norm_eps))
    return states


def forward(geo, sd, wave: np.ndarray):
    sd = {k: v.double() for k, v in sd.items()}
    return hidden_states(geo, sd, stem(geo, sd, normalize_wave(wave)))
