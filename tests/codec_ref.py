"""Float64 statement of the speaker half of the reference's 512-wide third stream (preprocessing/preprocess_ns3_prosody_speaker.py:41-60),
one utterance at a time: FACodecEncoderV2.block -- weight-normed convolutions around anti-aliased SnakeBeta activations (src/ns3/facodec.py,
src/ns3/alias_free_torch) -- and FACodecDecoderV2.timbre_encoder behind it; ``result`` = cat(prosody rows, timbre rows).  Written from what
those files compute, on the checkpoints' own key names; nothing of the product's ``prosody.prepare_codec`` is used, so its folds (weight
norm, tap-major weights, e^alpha and 1 / (e^beta + 1e-9), the position-0 vector in the last convolution's bias) are checked against this.

Everything is channels-last: a level is a [T, C] array.  ``torch_twin`` is the same computation in fp32 torch.nn.functional calls, composed as
the reference composes them; its distance from the statement is the yardstick for the device kernels.
Error form as everywhere: max|a - b| / max(1, max|b|)."""
import math

import numpy as np
import torch

from prosody_ref import _f64, layer_norm, rel_err  # noqa: F401  (rel_err re-exported)

HOP = 200
TIMBRE = "timbre_encoder"
DILATIONS = (1, 3, 9)
GOLDEN_FILES = ("tiny_codec_ngf8.npz", "tiny_codec_ngf8_timbre.npz")


def frames(n: int) -> int:
    return n // HOP + 1


def padded_len(n: int) -> int:
    """the reference pads with 200 - n % 200 zeros: always 1..200 of them"""
    return n + HOP - n % HOP


def kaiser_sinc_taps(cutoff: float = 0.25, half_width: float = 0.3, k: int = 12) -> np.ndarray:
    """the 12 low-pass taps of both resamplers of an Activation1d, float64: a Kaiser window (beta from the stop-band formula) times a
    sinc at 2 * cutoff, normalised to sum 1"""
    half = k // 2
    A = 2.285 * (half - 1) * math.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    n = np.arange(k, dtype=np.float64)
    window = np.i0(beta * np.sqrt(1.0 - (2.0 * n / (k - 1) - 1.0) ** 2)) / np.i0(beta)
    time = (np.arange(-half, half) + 0.5) if k % 2 == 0 else (np.arange(k) - half).astype(np.float64)
    f = 2 * cutoff * window * np.sinc(2 * cutoff * time)
    return f / f.sum()


def weight_norm_conv(sd, p: str) -> np.ndarray:
    """[N, C, k]: g v / |v| with one norm per output channel over (C, k)"""
    g, v = sd[p + ".weight_g"], sd[p + ".weight_v"]
    return g.reshape(-1, 1, 1) * v / np.sqrt((v ** 2).sum(axis=(1, 2), keepdims=True))


def conv1d(x, w, b, stride: int = 1, pad: int = 0, dilation: int = 1) -> np.ndarray:
    """x [T, C], w [N, C, k] -> [T_out, N], zero padding"""
    T, C = x.shape
    N, _, k = w.shape
    xp = np.concatenate([np.zeros((pad, C)), x, np.zeros((pad, C))])
    T_out = (T + 2 * pad - dilation * (k - 1) - 1) // stride + 1
    out = np.tile(b, (T_out, 1)).astype(np.float64)
    for j in range(k):
        out += xp[j * dilation: j * dilation + (T_out - 1) * stride + 1: stride] @ w[:, :, j].T
    return out


def activation1d(x, alpha, beta, f_up, f_down) -> np.ndarray:
    """x [T, C]: replicate-pad 5, x2 transposed convolution (times 2, trimmed 15 a side), x + sin^2(x e^alpha) / (e^beta + 1e-9),
    replicate-pad (5, 6), the taps again at stride 2"""
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    return activation1d_folded(x, np.exp(alpha), 1.0 / (np.exp(beta) + 1e-9), f_up, f_down)


def activation1d_folded(x, ea, ib, f_up, f_down) -> np.ndarray:
    """``activation1d`` on e^alpha and 1 / (e^beta + 1e-9)"""
    T, C = x.shape
    xp = np.concatenate([np.repeat(x[:1], 5, 0), x, np.repeat(x[-1:], 5, 0)])
    y = np.zeros((2 * len(xp) + 10, C))
    for i in range(12):
        y[i: i + 2 * len(xp): 2] += xp * f_up[i]
    u = 2.0 * y[15: -15]
    assert len(u) == 2 * T
    s = u + np.sin(u * ea) ** 2 * ib
    sp = np.concatenate([np.repeat(s[:1], 5, 0), s, np.repeat(s[-1:], 6, 0)])
    return sum(sp[k: k + 2 * T: 2] * f_down[k] for k in range(12))


def _act(sd, p: str, x) -> np.ndarray:
    return activation1d(x, sd[p + ".act.alpha"], sd[p + ".act.beta"], sd[p + ".upsample.filter"].reshape(-1),
                        sd[p + ".downsample.lowpass.filter"].reshape(-1))


def strides_of(sd) -> tuple:
    out, i = [], 1
    while f"block.{i}.block.4.weight_v" in sd:
        out.append(sd[f"block.{i}.block.4.weight_v"].shape[2] // 2)
        i += 1
    return tuple(out)


def codec(sd, wave) -> dict:
    """``sd``: float64 arrays under FACodecEncoderV2's key names.  Returns conv_in [P, ngf], every unit's output u{level}_{j}, every
    level's down-convolution level_{i} (i = 1 ..) and encoded [P / hop, out]."""
    y = np.asarray(wave, dtype=np.float64)
    x = np.concatenate([y, np.zeros(padded_len(len(y)) - len(y))])[:, None]
    out = {}
    x = out["conv_in"] = conv1d(x, weight_norm_conv(sd, "block.0"), sd["block.0.bias"], pad=3)
    strides = strides_of(sd)
    for i, s in enumerate(strides, start=1):
        for j, d in enumerate(DILATIONS):
            p = f"block.{i}.block.{j}.block"
            h = conv1d(_act(sd, p + ".0", x), weight_norm_conv(sd, p + ".1"), sd[p + ".1.bias"], pad=3 * d, dilation=d)
            x = out[f"u{i}_{j}"] = x + conv1d(_act(sd, p + ".2", h), weight_norm_conv(sd, p + ".3"), sd[p + ".3.bias"])
        p = f"block.{i}.block"
        x = out[f"level_{i}"] = conv1d(_act(sd, p + ".3", x), weight_norm_conv(sd, p + ".4"), sd[p + ".4.bias"], stride=s, pad=s // 2 + s % 2)
    n = len(strides)
    out["encoded"] = conv1d(_act(sd, f"block.{n + 1}", x), weight_norm_conv(sd, f"block.{n + 2}"), sd[f"block.{n + 2}.bias"], pad=1)
    return out


def pre_ln_encoder(sd, prefix: str, x, heads: int) -> np.ndarray:
    """x [T, D] -> last_ln(layers(x + position 0)): src/ns3/transformer.py's TransformerEncoder as the reference calls it (the positional
    encoding receives (1, T, d) and so adds position 0 -- 0 on the even channels, 1 on the odd -- to every frame)"""
    x = np.array(x, dtype=np.float64)
    T, D = x.shape
    x[:, 1::2] += 1.0
    dh = D // heads
    L = 0
    while f"{prefix}.layers.{L}.ln_1.weight" in sd:
        L += 1
    for i in range(L):
        p = f"{prefix}.layers.{i}"
        y = layer_norm(x, sd[p + ".ln_1.weight"], sd[p + ".ln_1.bias"])
        qkv = y @ sd[p + ".self_attn.in_proj_weight"].T + sd[p + ".self_attn.in_proj_bias"]
        ctx = np.empty((T, D))
        for h in range(heads):
            q, k, v = (qkv[:, j * D + h * dh: j * D + (h + 1) * dh] for j in range(3))
            s = (q * dh ** -0.5) @ k.T
            s = np.exp(s - s.max(axis=1, keepdims=True))
            ctx[:, h * dh:(h + 1) * dh] = (s / s.sum(axis=1, keepdims=True)) @ v
        x = x + ctx @ sd[p + ".self_attn.out_proj.weight"].T + sd[p + ".self_attn.out_proj.bias"]
        y = layer_norm(x, sd[p + ".ln_2.weight"], sd[p + ".ln_2.bias"])
        w = sd[p + ".ffn.ffn_1.weight"]
        f = conv1d(y, w, sd[p + ".ffn.ffn_1.bias"], pad=w.shape[2] // 2)
        x = x + np.maximum(f, 0.0) @ sd[p + ".ffn.ffn_2.weight"].T + sd[p + ".ffn.ffn_2.bias"]
    return layer_norm(x, sd[prefix + ".last_ln.weight"], sd[prefix + ".last_ln.bias"])


def forward(enc_sd, dec_sd, wave, heads: int, prosody_rows=None) -> dict:
    """the codec's levels, ``timbre`` [T, D] and -- given the prosody half -- ``result`` [T, 2 D]"""
    out = codec(_f64(enc_sd), wave)
    out["timbre"] = pre_ln_encoder(_f64(dec_sd), TIMBRE, out["encoded"], heads)
    if prosody_rows is not None:
        out["result"] = np.concatenate([np.asarray(prosody_rows, dtype=np.float64), out["timbre"]], axis=1)
    return out


# ---------------------------------------------------------------------------------------------- the fp32 torch twin (reference-style)
def twin_activation1d(x, alpha, beta, f_up, f_down) -> torch.Tensor:
    """x [1, C, T] fp32, as Activation1d composes UpSample1d, SnakeBeta(alpha_logscale) and DownSample1d"""
    F = torch.nn.functional
    C = x.shape[1]
    x = F.pad(x, (5, 5), mode="replicate")
    x = 2 * F.conv_transpose1d(x, f_up.reshape(1, 1, -1).expand(C, -1, -1), stride=2, groups=C)
    x = x[..., 15:-15]
    a, b = torch.exp(alpha)[None, :, None], torch.exp(beta)[None, :, None]
    x = x + (1.0 / (b + 0.000000001)) * torch.pow(torch.sin(x * a), 2)
    x = F.pad(x, (5, 6), mode="replicate")
    return F.conv1d(x, f_down.reshape(1, 1, -1).expand(C, -1, -1), stride=2, groups=C)


def twin_unit(x, w7, b7, w1, b1, d: int, act1, act2) -> torch.Tensor:
    """one ResidualUnit on x [1, C, T]; w7 [C, C, 7] and w1 [C, C, 1] with weight norm applied; act = (alpha, beta, f_up, f_down)"""
    F = torch.nn.functional
    h = F.conv1d(twin_activation1d(x, *act1), w7, b7, dilation=d, padding=3 * d)
    return x + F.conv1d(twin_activation1d(h, *act2), w1, b1)


def torch_twin(enc_sd, wave) -> dict:
    """the codec's levels in fp32 torch ops, batch of one; arrays are channels-last like the statement's"""
    F = torch.nn.functional
    sd = {k: torch.as_tensor(np.asarray(v)).float() for k, v in enc_sd.items()}

    def wn(p):
        g, v = sd[p + ".weight_g"], sd[p + ".weight_v"]
        return g * v / v.pow(2).sum(dim=(1, 2), keepdim=True).sqrt()

    def act(p):
        return (sd[p + ".act.alpha"], sd[p + ".act.beta"], sd[p + ".upsample.filter"].reshape(-1), sd[p + ".downsample.lowpass.filter"].reshape(-1))

    y = torch.as_tensor(np.asarray(wave, dtype=np.float32))
    x = F.pad(y, (0, padded_len(len(y)) - len(y)))[None, None]
    out = {}
    x = F.conv1d(x, wn("block.0"), sd["block.0.bias"], padding=3)
    out["conv_in"] = x
    strides = strides_of(sd)
    for i, s in enumerate(strides, start=1):
        for j, d in enumerate(DILATIONS):
            p = f"block.{i}.block.{j}.block"
            x = out[f"u{i}_{j}"] = twin_unit(x, wn(p + ".1"), sd[p + ".1.bias"], wn(p + ".3"), sd[p + ".3.bias"], d, act(p + ".0"), act(p + ".2"))
        p = f"block.{i}.block"
        x = out[f"level_{i}"] = F.conv1d(twin_activation1d(x, *act(p + ".3")), wn(p + ".4"), sd[p + ".4.bias"], stride=s, padding=s // 2 + s % 2)
    n = len(strides)
    out["encoded"] = F.conv1d(twin_activation1d(x, *act(f"block.{n + 1}")), wn(f"block.{n + 2}"), sd[f"block.{n + 2}.bias"], padding=1)
    return {k: v[0].T.contiguous().numpy() for k, v in out.items()}


def load_golden(golden_dir: str) -> dict:
    """tests/golden/tiny_codec_ngf8.npz and tiny_codec_ngf8_timbre.npz (one fixture in two files, each under 1 MiB) beside
    tiny_prosody_d128h2.npz, whose five waves they were computed on: encoder / decoder state dicts of fp32 tensors, the prosody fixture's
    dict, and all arrays of both files as one dict ``g``"""
    import os
    import prosody_ref as R
    pg = R.load_golden(golden_dir)
    g = {}
    for name in GOLDEN_FILES:
        with np.load(os.path.join(golden_dir, name)) as part:
            g.update({k: part[k] for k in part.files})
    enc = {str(k): torch.from_numpy(g["e." + str(k)].astype(np.float32)) for k in g["enc_keys"]}
    dec = {str(k): torch.from_numpy(g["d." + str(k)].astype(np.float32)) for k in g["dec_keys"]}
    return dict(g=g, enc=enc, dec=dec, prosody=pg, waves=pg["waves"], offs=pg["offs"])
