"""Host side of the prosody stream: what is read off ``ns3_facodec_decoder_v2.bin`` and folded once at load.

The reference's third stream is ``preprocessing/preprocess_ns3_prosody.py``: of FACodecDecoderV2 it reaches ``melspec_linear``,
``melspec_encoder`` (pre-LayerNorm transformer layers with a k = 5 convolution as FC1) and the first quantizer
(``get_processed_style_embedding``); FACodecEncoderV2 contributes its mel transform only -- its convolutional output is computed and never
used.  Nothing here touches a device: ``engine.ProsodyEncoder`` uploads what ``prepare`` returns."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict

import numpy as np
import torch

NS3_PROSODY = "ns3-prosody"                                       # the encoder id of bin/predict_cat_from_wav.py --encoder3
NS3_PROSODY_SPEAKER = "ns3-prosody-speaker"                       # the 512-wide stream: prosody rows | timbre rows
CHECKPOINT_FILE = "ns3_facodec_decoder_v2.bin"
ENCODER_CHECKPOINT_FILE = "ns3_facodec_encoder_v2.bin"
DEFAULT_CHECKPOINT = os.path.join(".", "pretrained_models", "ns3", CHECKPOINT_FILE)   # the reference's path
ENC, VQ = "melspec_encoder", "quantizer.0.layers.0"
TIMBRE = "timbre_encoder"


@dataclass(frozen=True)
class ProsodySpec:
    """Geometry of the stream, from the checkpoint's shapes; ``heads`` is not in them (4 in the reference)."""
    hidden: int = 256
    num_layers: int = 4
    ffn: int = 1024
    kernel: int = 5
    heads: int = 4
    n_codes: int = 1024
    code_dim: int = 8
    n_mels: int = 20
    family: str = NS3_PROSODY

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads


TINY = ProsodySpec(hidden=128, num_layers=2, ffn=128, kernel=5, heads=2, n_codes=64, code_dim=8)   # tests/golden/tiny_prosody_d128h2.npz


def spec_from_state_dict(sd: Dict[str, torch.Tensor], heads: int = 4) -> ProsodySpec:
    try:
        D, n_mels = (int(v) for v in sd["melspec_linear.weight"].shape)
        L = 0
        while f"{ENC}.layers.{L}.ln_1.weight" in sd:
            L += 1
        F, d2, k = (int(v) for v in sd[f"{ENC}.layers.0.ffn.ffn_1.weight"].shape)
        n_codes, cd = (int(v) for v in sd[f"{VQ}._codebook.weight"].shape)
    except KeyError as e:
        raise KeyError(f"not a FACodec decoder state dict: {e.args[0]} is missing") from None
    if L < 1 or d2 != D or k % 2 != 1:
        raise ValueError(f"unsupported prosody encoder: {L} layers, FC1 weight {(F, d2, k)} at hidden size {D}")
    if heads < 1 or D % heads:
        raise ValueError(f"hidden size {D} does not divide into {heads} heads")
    if D % 64 or F % 64 or cd != 8:
        raise ValueError(f"unsupported prosody geometry: hidden {D}, filter {F} (multiples of 64), code dim {cd} (8)")
    return ProsodySpec(D, L, F, k, int(heads), n_codes, cd, n_mels)


def checkpoint_path(checkpoint: str) -> str:
    """``--checkpoint3 <dir or .bin>`` (empty: the reference's ./pretrained_models/ns3/...) -> the decoder's file"""
    p = checkpoint or DEFAULT_CHECKPOINT
    return os.path.join(p, CHECKPOINT_FILE) if os.path.isdir(p) else p


def load_state_dict(checkpoint: str) -> Dict[str, torch.Tensor]:
    path = checkpoint_path(checkpoint)
    if not os.path.isfile(path):
        raise OSError(f"no prosody checkpoint at {path} (--checkpoint: a directory holding {CHECKPOINT_FILE}, or the file)")
    return torch.load(path, map_location="cpu", weights_only=True)


def resolve_spec(checkpoint: str, synthetic: bool = False, heads: int = 4) -> ProsodySpec:
    """the geometry before any weight goes to a device: the reference's with ``synthetic``, else the checkpoint's shapes"""
    if synthetic and not checkpoint:
        return ProsodySpec(heads=heads)
    path = checkpoint_path(checkpoint)
    if not os.path.isfile(path):
        raise OSError(f"no prosody checkpoint at {path}")
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True, mmap=True)
    except (RuntimeError, ValueError):                            # a legacy (non-zip) file cannot be mapped
        sd = torch.load(path, map_location="cpu", weights_only=True)
    return spec_from_state_dict(sd, heads)


def weight_norm_linear(sd, prefix: str) -> torch.Tensor:
    """w = g * v / |v| with one norm per output row: torch.nn.utils.weight_norm's default (dim 0) on a Linear, float64"""
    if prefix + ".weight_g" in sd:
        g, v = sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]
    elif prefix + ".parametrizations.weight.original0" in sd:
        g, v = sd[prefix + ".parametrizations.weight.original0"], sd[prefix + ".parametrizations.weight.original1"]
    else:
        return sd[prefix + ".weight"].double()
    g, v = g.double(), v.double()
    return v * (g.reshape(-1, 1) / v.pow(2).sum(dim=1, keepdim=True).sqrt())


def position0(D: int) -> torch.Tensor:
    """What the reference adds to EVERY frame: PositionalEncoding is written for (T, B, d) input and receives (1, T, d), so
    ``pe[:x.size(0)]`` is the encoding of position 0 -- sin(0) = 0 on the even channels, cos(0) = 1 on the odd ones -- broadcast over
    the frames (src/ns3/transformer.py:44-46, facodec.py:1036-1037)."""
    pe = torch.zeros(D, dtype=torch.float64)
    pe[1::2] = 1.0
    return pe


def synthetic_state_dict(spec: ProsodySpec = ProsodySpec(), seed: int = 7) -> Dict[str, torch.Tensor]:
    """Seeded weights under the checkpoint's key names, drawn like PyTorch's default initialisation of the reference's modules
    (FC1 / FC2 weights N(0, 0.02) as TransformerFFNLayer sets them; weight_g = the row norms of weight_v)."""
    g = torch.Generator().manual_seed(seed)
    D, F, k = spec.hidden, spec.ffn, spec.kernel

    def uni(shape, fan_in):
        b = 1.0 / np.sqrt(fan_in)
        return (torch.rand(shape, generator=g) * 2 - 1) * b

    sd = {"melspec_linear.weight": uni((D, spec.n_mels), spec.n_mels), "melspec_linear.bias": uni((D,), spec.n_mels)}
    _synthetic_layers(sd, ENC, spec, g, uni)
    for name, (o, i) in (("in_proj", (spec.code_dim, D)), ("out_proj", (D, spec.code_dim))):
        v = uni((o, i), i)
        sd[f"{VQ}.{name}.weight_v"] = v
        sd[f"{VQ}.{name}.weight_g"] = v.norm(dim=1, keepdim=True) * (1.0 + 0.1 * torch.randn(o, 1, generator=g))
        sd[f"{VQ}.{name}.bias"] = uni((o,), i)
    sd[f"{VQ}._codebook.weight"] = torch.randn(spec.n_codes, spec.code_dim, generator=g)
    return sd


def _synthetic_layers(sd, prefix: str, spec, g, uni) -> None:
    """the pre-LayerNorm layers and last_ln of one TransformerEncoder under ``prefix`` (melspec_encoder, timbre_encoder)"""
    D, F, k = spec.hidden, spec.ffn, spec.kernel
    for i in range(spec.num_layers):
        p = f"{prefix}.layers.{i}"
        for ln in ("ln_1", "ln_2"):
            sd[f"{p}.{ln}.weight"] = 1.0 + 0.1 * torch.randn(D, generator=g)
            sd[f"{p}.{ln}.bias"] = 0.1 * torch.randn(D, generator=g)
        sd[f"{p}.self_attn.in_proj_weight"] = uni((3 * D, D), D) * np.sqrt(3.0)       # xavier_uniform of the packed matrix
        sd[f"{p}.self_attn.in_proj_bias"] = 0.02 * torch.randn(3 * D, generator=g)
        sd[f"{p}.self_attn.out_proj.weight"] = uni((D, D), D)
        sd[f"{p}.self_attn.out_proj.bias"] = 0.02 * torch.randn(D, generator=g)
        sd[f"{p}.ffn.ffn_1.weight"] = 0.02 * torch.randn(F, D, k, generator=g)
        sd[f"{p}.ffn.ffn_1.bias"] = uni((F,), D * k)
        sd[f"{p}.ffn.ffn_2.weight"] = 0.02 * torch.randn(D, F, generator=g)
        sd[f"{p}.ffn.ffn_2.bias"] = uni((D,), F)
    sd[f"{prefix}.last_ln.weight"] = 1.0 + 0.1 * torch.randn(D, generator=g)
    sd[f"{prefix}.last_ln.bias"] = 0.1 * torch.randn(D, generator=g)


def prepare(sd: Dict[str, torch.Tensor], heads: int = 4) -> dict:
    """Everything ``engine.ProsodyEncoder`` uploads, as fp32 CPU tensors (folds in float64, one rounding):
      lin_w [D, n_mels], lin_b [D] = melspec_linear's bias + ``position0``
      layers: ln1 / ln2 (weight, bias), qkv (in_proj_weight [3D, D], bias), out, fc1 ([F, k * D] with W[n][j * D + c] = w[n][c][j], bias), fc2
      last_ln; w_in [8, D], b_in [8] (weight norm folded); codes [N, 8] L2-normalised; table [N, D] = out_proj of the RAW codes."""
    spec = spec_from_state_dict(sd, heads)
    if spec.head_dim != 64:
        raise ValueError(f"hidden size {spec.hidden} with {heads} heads: this stream's attention runs heads of 64 (the reference's 256 / 4)")
    D = spec.hidden
    f32 = _f32
    out = dict(spec=spec, lin_w=f32(sd["melspec_linear.weight"]), lin_b=(sd["melspec_linear.bias"].double() + position0(D)).float())
    out["layers"], out["last_ln"] = _prepare_layers(sd, ENC, spec)
    out["w_in"] = weight_norm_linear(sd, VQ + ".in_proj").float().contiguous()
    out["b_in"] = f32(sd[VQ + ".in_proj.bias"])
    cb = sd[VQ + "._codebook.weight"].double()
    out["codes"] = (cb / cb.norm(dim=1, keepdim=True).clamp_min(1e-12)).float().contiguous()
    out["table"] = (cb @ weight_norm_linear(sd, VQ + ".out_proj").T + sd[VQ + ".out_proj.bias"].double()).float().contiguous()
    return out


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().double().float().contiguous()


def _prepare_layers(sd, prefix: str, spec):
    """(layers, last_ln) of the TransformerEncoder under ``prefix``, as ``prepare`` documents them"""
    D, F, k = spec.hidden, spec.ffn, spec.kernel
    f32 = _f32
    layers = []
    for i in range(spec.num_layers):
        p = f"{prefix}.layers.{i}"
        a = p + ".self_attn"
        layers.append(dict(
            ln1=(f32(sd[p + ".ln_1.weight"]), f32(sd[p + ".ln_1.bias"])), ln2=(f32(sd[p + ".ln_2.weight"]), f32(sd[p + ".ln_2.bias"])),
            qkv=(f32(sd[a + ".in_proj_weight"]), f32(sd[a + ".in_proj_bias"])),
            out=(f32(sd[a + ".out_proj.weight"]), f32(sd[a + ".out_proj.bias"])),
            fc1=(f32(sd[p + ".ffn.ffn_1.weight"]).permute(0, 2, 1).reshape(F, k * D).contiguous(), f32(sd[p + ".ffn.ffn_1.bias"])),
            fc2=(f32(sd[p + ".ffn.ffn_2.weight"]), f32(sd[p + ".ffn.ffn_2.bias"]))))
    return layers, (f32(sd[prefix + ".last_ln.weight"]), f32(sd[prefix + ".last_ln.bias"]))


# ------------------------------------------------------------------------------------------------------ the speaker half (512-wide stream)
# preprocessing/preprocess_ns3_prosody_speaker.py saves cat(prosody rows, timbre rows): FACodecEncoderV2.block -- conv_in, four
# EncoderBlocks of three ResidualUnits (dilation 1, 3, 9) and a strided convolution, a last activation and a k = 3 convolution, every
# activation an anti-aliased SnakeBeta (x2 up, x + sin^2(x e^alpha) / (e^beta + 1e-9), x2 down; 12 Kaiser-sinc taps) -- and behind it
# FACodecDecoderV2.timbre_encoder, a TransformerEncoder of melspec_encoder's shapes fed the encoder's output directly.
DILATIONS = (1, 3, 9)
ACT_TAPS = 12
ACT_HALO = 6                        # input rows an Activation1d output reaches on each side
NARROW_MAX = 32                     # widest level the fp32 kernels (ser_codec_unit_v / ser_codec_conv_v) take; wider ones are multiples of 64
WIDE_HALO = 27                      # zero rows around each utterance in a wide level's operand copy: 3 * 9 covers d = 9 and every strided pad


@dataclass(frozen=True)
class CodecSpec:
    """Geometry of FACodecEncoderV2.block (from its checkpoint's shapes) with the timbre encoder's (a ``ProsodySpec``; its hidden size is
    ``out_channels``)."""
    ngf: int = 32
    strides: tuple = (2, 4, 5, 5)
    out_channels: int = 256
    timbre: ProsodySpec = ProsodySpec()
    family: str = NS3_PROSODY_SPEAKER

    @property
    def hop(self) -> int:
        return int(np.prod(self.strides))

    @property
    def hidden(self) -> int:
        """width of the saved rows: prosody rows | timbre rows"""
        return 2 * self.out_channels

    @property
    def channels(self) -> tuple:
        """input channels of level 0 .. len(strides) (the last: what the final convolution reads)"""
        return tuple(self.ngf << i for i in range(len(self.strides) + 1))

    def level_lengths(self, n: int) -> tuple:
        """rows of level 0 .. len(strides) for a wave of n samples: the zero-padded length (1..hop zeros) and its exact quotients"""
        P = n + self.hop - n % self.hop
        out = [P]
        for s in self.strides:
            out.append(out[-1] // s)
        return tuple(out)

    @staticmethod
    def unit_halo(d: int) -> int:
        """input rows one ResidualUnit of dilation d reaches on each side of an output row: 3 d of the k = 7 convolution + two activations"""
        return 3 * d + 2 * ACT_HALO


TINY_CODEC = CodecSpec(ngf=8, out_channels=128, timbre=ProsodySpec(hidden=128, num_layers=2, ffn=64, kernel=5, heads=2))   # tests/golden/tiny_codec_ngf8.npz


def kaiser_sinc_taps(cutoff: float = 0.25, half_width: float = 0.3, k: int = ACT_TAPS) -> np.ndarray:
    """float64 restatement of alias_free_torch's kaiser_sinc_filter1d at Activation1d's setting (ratio 2): 2 cutoff * Kaiser window * sinc,
    normalised to sum 1"""
    half = k // 2
    A = 2.285 * (half - 1) * np.pi * 4 * half_width + 7.95
    beta = 0.1102 * (A - 8.7) if A > 50.0 else (0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0) if A >= 21.0 else 0.0)
    n = np.arange(k, dtype=np.float64)
    window = np.i0(beta * np.sqrt(1.0 - (2.0 * n / (k - 1) - 1.0) ** 2)) / np.i0(beta)
    time = np.arange(-half, half) + 0.5 if k % 2 == 0 else np.arange(k) - float(half)
    f = 2 * cutoff * window * np.sinc(2 * cutoff * time)
    return f / f.sum()


def _conv_keys(sd, prefix: str):
    if prefix + ".weight_g" in sd:
        return sd[prefix + ".weight_g"], sd[prefix + ".weight_v"]
    if prefix + ".parametrizations.weight.original0" in sd:
        return sd[prefix + ".parametrizations.weight.original0"], sd[prefix + ".parametrizations.weight.original1"]
    return None, sd[prefix + ".weight"]


def weight_norm_conv(sd, prefix: str) -> torch.Tensor:
    """[N, C_in, k] float64: g v / |v| with one norm per output channel over (C_in, k) -- weight_norm's default on a Conv1d; both key
    spellings, as ``weight_norm_linear``"""
    g, v = _conv_keys(sd, prefix)
    v = v.double()
    return v if g is None else v * (g.double().reshape(-1, 1, 1) / v.pow(2).sum(dim=(1, 2), keepdim=True).sqrt())


def codec_spec_from_state_dict(enc_sd, dec_sd, heads: int = 4) -> CodecSpec:
    try:
        ngf, cin, k0 = (int(v) for v in _conv_keys(enc_sd, "block.0")[1].shape)
        strides, i, C = [], 1, ngf
        while any(key.startswith(f"block.{i}.block.4.") for key in enc_sd):
            n, c, k = (int(v) for v in _conv_keys(enc_sd, f"block.{i}.block.4")[1].shape)
            if c != C or n != 2 * C or k % 2:
                raise ValueError(f"unsupported codec level {i}: down-convolution weight {(n, c, k)} behind {C} channels")
            for j in range(3):
                w7 = tuple(_conv_keys(enc_sd, f"block.{i}.block.{j}.block.1")[1].shape)
                w1 = tuple(_conv_keys(enc_sd, f"block.{i}.block.{j}.block.3")[1].shape)
                if w7 != (C, C, 7) or w1 != (C, C, 1):
                    raise ValueError(f"unsupported residual unit {i}.{j}: weights {w7}, {w1} at {C} channels")
            strides.append(k // 2)
            C, i = 2 * C, i + 1
        out, c, k = (int(v) for v in _conv_keys(enc_sd, f"block.{i + 1}")[1].shape)
        D = int(dec_sd[f"{TIMBRE}.last_ln.weight"].shape[0])
        L = 0
        while f"{TIMBRE}.layers.{L}.ln_1.weight" in dec_sd:
            L += 1
        F, d2, kt = (int(v) for v in dec_sd[f"{TIMBRE}.layers.0.ffn.ffn_1.weight"].shape)
    except KeyError as e:
        raise KeyError(f"not a FACodec encoder / decoder state dict pair: {e.args[0]} is missing") from None
    if cin != 1 or k0 != 7 or not strides or c != C or k != 3:
        raise ValueError(f"unsupported codec: conv_in {(ngf, cin, k0)}, {len(strides)} levels, last convolution {(out, c, k)} behind {C} channels")
    if ngf % 8 or ngf > NARROW_MAX:
        raise ValueError(f"unsupported codec width ngf = {ngf}: a multiple of 8, at most {NARROW_MAX}")
    for s in strides:
        if s < 1 or s > 8:
            raise ValueError(f"unsupported codec stride {s} (1..8)")
    widths = [ngf << i for i in range(len(strides) + 1)]
    if any(w > NARROW_MAX and w % 64 for w in widths) or widths[-1] % 64:
        raise ValueError(f"unsupported codec widths {widths}: a level is at most {NARROW_MAX} channels wide or a multiple of 64, the last a multiple of 64")
    if out % 64 or out != D or d2 != D or kt % 2 != 1 or F % 64 or L < 1:
        raise ValueError(f"unsupported timbre geometry: encoder output {out}, hidden {D}, FC1 weight {(F, d2, kt)}, {L} layers")
    if heads < 1 or D % heads or D // heads != 64:
        raise ValueError(f"hidden size {D} with {heads} heads: this stream's attention runs heads of 64 (the reference's 256 / 4)")
    return CodecSpec(ngf, tuple(strides), out, ProsodySpec(D, L, F, kt, int(heads)))


def synthetic_codec_state_dict(spec: CodecSpec = CodecSpec(), seed: int = 5) -> Dict[str, torch.Tensor]:
    """Seeded weights under FACodecEncoderV2's key names: weight_v ~ N(0, 1), weight_g = |v| sqrt(0.5 / fan_in), biases U(-0.1, 0.1), alpha and
    beta U(-0.5, 0.5), the filter buffers from ``kaiser_sinc_taps``.  Every level's output then stays at max|.| ~ 1-3 on speech-like input;
    the reference's own initialisation leaves max|encoded| ~ 0.03, under which a max(1, .) error form tests nothing."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    taps = torch.from_numpy(kaiser_sinc_taps()).float().reshape(1, 1, ACT_TAPS)

    def conv(p, n, c, k):
        v = torch.randn(n, c, k, generator=g)
        sd[p + ".weight_g"] = v.pow(2).sum(dim=(1, 2), keepdim=True).sqrt() * float(np.sqrt(0.5 / (c * k)))
        sd[p + ".weight_v"] = v
        sd[p + ".bias"] = (torch.rand(n, generator=g) * 2 - 1) * 0.1

    def act(p, c):
        sd[p + ".act.alpha"] = torch.rand(c, generator=g) - 0.5
        sd[p + ".act.beta"] = torch.rand(c, generator=g) - 0.5
        sd[p + ".upsample.filter"] = taps.clone()
        sd[p + ".downsample.lowpass.filter"] = taps.clone()

    conv("block.0", spec.ngf, 1, 7)
    C = spec.ngf
    for i, s in enumerate(spec.strides, start=1):
        for j in range(3):
            p = f"block.{i}.block.{j}.block"
            act(p + ".0", C)
            conv(p + ".1", C, C, 7)
            act(p + ".2", C)
            conv(p + ".3", C, C, 1)
        act(f"block.{i}.block.3", C)
        conv(f"block.{i}.block.4", 2 * C, C, 2 * s)
        C *= 2
    n = len(spec.strides)
    act(f"block.{n + 1}", C)
    conv(f"block.{n + 2}", spec.out_channels, C, 3)
    return sd


def synthetic_timbre_state_dict(spec: ProsodySpec = ProsodySpec(), seed: int = 11) -> Dict[str, torch.Tensor]:
    """seeded timbre_encoder weights under the decoder checkpoint's key names, drawn as ``synthetic_state_dict`` draws melspec_encoder's"""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    _synthetic_layers(sd, TIMBRE, spec, g, lambda shape, fan_in: (torch.rand(shape, generator=g) * 2 - 1) / np.sqrt(fan_in))
    return sd


def _tap_major(w: torch.Tensor) -> torch.Tensor:
    """[N, C_in, k] -> [N, k * C_in] with W[n][j * C_in + c] = w[n][c][j]"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


def prepare_codec(enc_sd, dec_sd, heads: int = 4) -> dict:
    """Everything ``engine.SpeakerProsodyEncoder`` uploads for the speaker half, as fp32 CPU tensors (folds in float64, one rounding):
      taps [12]; conv_in (w [ngf, 7], b); levels: C, stride, pad, units [(d, act1, w7 [C, 7 C], b7, act2, w1 [C, C], b1)], act, down (w [2 C, 2 s C], b);
      final: act, w [out, 3 C], b = the bias + ``position0`` (the timbre encoder adds it to every frame); timbre layers / last_ln as ``prepare``.
    An act is (e^alpha [C], 1 / (e^beta + 1e-9) [C]).  Weight norm is folded in float64, weights are tap-major."""
    return _prepare_codec(enc_sd, dec_sd, heads, lambda t: t.double().float().contiguous())


def prepare_codec_f64(enc_sd, dec_sd, heads: int = 4) -> dict:
    """``prepare_codec`` before its one rounding: the float64 folds themselves (tests)"""
    return _prepare_codec(enc_sd, dec_sd, heads, lambda t: t.double().contiguous())


def _prepare_codec(enc_sd, dec_sd, heads, cast) -> dict:
    spec = codec_spec_from_state_dict(enc_sd, dec_sd, heads)
    want = kaiser_sinc_taps()
    taps = None
    for key, buf in enc_sd.items():
        if key.endswith(".filter"):
            f = buf.detach().double().reshape(-1).numpy()
            if f.shape != (ACT_TAPS,) or np.abs(f - want).max() > 1e-6:
                raise ValueError(f"{key}: not the {ACT_TAPS}-tap Kaiser-sinc filter of an Activation1d (cutoff 0.25, half-width 0.3)")
            if taps is not None and not np.array_equal(f, taps):
                raise ValueError(f"{key}: the activations' filter buffers differ from each other")
            taps = f
    if taps is None:
        raise KeyError("not a FACodec encoder state dict: no activation filter buffer")

    def act(p):
        a, b = enc_sd[p + ".act.alpha"].detach().double(), enc_sd[p + ".act.beta"].detach().double()
        return cast(torch.exp(a)), cast(1.0 / (torch.exp(b) + 1e-9))

    def conv(p):
        return cast(_tap_major(weight_norm_conv(enc_sd, p))), cast(enc_sd[p + ".bias"].detach().double())

    out = dict(spec=spec, taps=cast(torch.from_numpy(taps)), conv_in=conv("block.0"))
    levels = []
    for i, s in enumerate(spec.strides, start=1):
        units = []
        for j, d in enumerate(DILATIONS):
            p = f"block.{i}.block.{j}.block"
            w7, b7 = conv(p + ".1")
            w1, b1 = conv(p + ".3")
            units.append(dict(d=d, act1=act(p + ".0"), w7=w7, b7=b7, act2=act(p + ".2"), w1=w1, b1=b1))
        levels.append(dict(C=spec.channels[i - 1], stride=s, pad=s // 2 + s % 2, units=units, act=act(f"block.{i}.block.3"),
                           down=conv(f"block.{i}.block.4")))
    out["levels"] = levels
    n = len(spec.strides)
    w, b = conv(f"block.{n + 2}")
    out["final"] = dict(act=act(f"block.{n + 1}"), w=w, b=cast(b.double() + position0(spec.out_channels)))
    out["layers"], out["last_ln"] = _prepare_layers(dec_sd, TIMBRE, spec.timbre)
    return out


def encoder_checkpoint_path(checkpoint: str, encoder_checkpoint: str = "") -> str:
    """``--encoder_checkpoint <dir or .bin>``, else ns3_facodec_encoder_v2.bin beside the decoder's file"""
    if encoder_checkpoint:
        return os.path.join(encoder_checkpoint, ENCODER_CHECKPOINT_FILE) if os.path.isdir(encoder_checkpoint) else encoder_checkpoint
    return os.path.join(os.path.dirname(checkpoint_path(checkpoint)), ENCODER_CHECKPOINT_FILE)


def resolve_codec_spec(checkpoint: str, synthetic: bool = False, heads: int = 4, encoder_checkpoint: str = "") -> CodecSpec:
    """``resolve_spec`` for the 512-wide stream: the reference's geometry with ``synthetic``, else both checkpoints' shapes"""
    if synthetic and not checkpoint:
        return CodecSpec(timbre=ProsodySpec(heads=heads))
    pspec = resolve_spec(checkpoint, False, heads)
    spec = codec_spec_from_state_dict(load_encoder_state_dict(checkpoint, encoder_checkpoint), load_state_dict(checkpoint), heads)
    if spec.out_channels != pspec.hidden:
        raise ValueError(f"prosody rows are {pspec.hidden} wide, timbre rows {spec.out_channels}: not the halves of one tensor")
    return spec


def load_encoder_state_dict(checkpoint: str, encoder_checkpoint: str = "") -> Dict[str, torch.Tensor]:
    path = encoder_checkpoint_path(checkpoint, encoder_checkpoint)
    if not os.path.isfile(path):
        raise OSError(f"no codec encoder checkpoint at {path} (--encoder_checkpoint: a directory holding {ENCODER_CHECKPOINT_FILE}, or the file)")
    return torch.load(path, map_location="cpu", weights_only=True)


# ------------------------------------------------------------------------------------------------------ the extraction driver
def build_parser(speaker: bool = False):
    """``speaker``: the command line of preprocess_ns3_prosody_speaker.py (adds ``--encoder_checkpoint``)"""
    import argparse
    p = argparse.ArgumentParser(description="prosody + speaker features of every file in --wav_dir (the reference's preprocess_ns3_prosody_speaker.py)"
                                if speaker else "prosody features of every file in --wav_dir (the reference's preprocess_ns3_prosody.py)")
    if speaker:
        p.add_argument("--encoder_checkpoint", type=str, default="",
                       help=f"a directory holding {ENCODER_CHECKPOINT_FILE}, or the file (default: beside the decoder's file)")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--save_path", type=str, default="./")
    p.add_argument("--wav_dir", type=str, default="./")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--checkpoint", type=str, default="", help=f"a directory holding {CHECKPOINT_FILE}, or the file (default: {DEFAULT_CHECKPOINT})")
    p.add_argument("--mode", type=str, default="f16x", choices=("f16x", "fp32x", "bf16"))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--synthetic_weights", action="store_true", help="seeded weights at the reference's geometry (no checkpoint)")
    return p


def run_speaker(argv=None, encoder=None) -> int:
    """``run`` for the 512-wide stream (preprocessing/preprocess_ns3_prosody_speaker.py): [len // 200 + 1, 2 D] rows, prosody | timbre"""
    return run(argv, encoder, speaker=True)


def run(argv=None, encoder=None, speaker: bool = False) -> int:
    """``<save_path>/<utterance>.pt`` -- a [len // 200 + 1, D] float32 tensor, what the reference's ``torch.save(feats, ...)`` leaves --
    for every file of ``--wav_dir``, on batchloop's loop and failure contract: a file that cannot be decoded, or is shorter than 400
    samples, is printed ("Failed to process ...") and costs only itself; a batch whose range guard or quantizer error word is set is
    run again file by file.  One GPU, 16 kHz input.  ``encoder``: a built ``engine.ProsodyEncoder`` (tests); with ``speaker`` an
    ``engine.SpeakerProsodyEncoder``, whose rows are 2 D wide."""
    from concurrent.futures import ThreadPoolExecutor
    from ._lib import SerHipError
    from .batchloop import make_batches, prefetch, run_or_each
    from .frontend import feature_path, load_wav_16k, save_feature
    args = build_parser(speaker).parse_args(argv)
    print(f"Using device = {'cuda' if torch.cuda.is_available() else 'cpu'}")
    os.makedirs(args.save_path, exist_ok=True)
    print(f"Save path = {args.save_path} created. It has {len(os.listdir(args.save_path))} files in it.")
    names = sorted(os.listdir(args.wav_dir))
    print(f"{len(names)} file are going to be processed...")
    print("Extracting prosody codes from NaturalSpeech3")
    if not torch.cuda.is_available():
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        return 0
    if encoder is None:
        from .engine import ProsodyEncoder, SpeakerProsodyEncoder
        try:
            if args.synthetic_weights and not args.checkpoint:
                sd = synthetic_state_dict(ProsodySpec(), args.seed)
                if speaker:
                    sd.update(synthetic_timbre_state_dict(ProsodySpec(), args.seed))
                    enc_sd = synthetic_codec_state_dict(CodecSpec(), args.seed)
            else:
                sd = load_state_dict(args.checkpoint)
                if speaker:
                    enc_sd = load_encoder_state_dict(args.checkpoint, args.encoder_checkpoint)
            encoder = SpeakerProsodyEncoder(sd, enc_sd, "cuda:0", args.mode) if speaker else ProsodyEncoder(sd, "cuda:0", args.mode)
        except OSError as e:
            print("Error: No pretrained model found with the name")
            print(f"  ({e})")
            print("Something went wrong, make sure everything is correct before running again!")
            return 0
    failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(args.wav_dir, name)}: {err}")

    def load(name):
        path = os.path.join(args.wav_dir, name)
        if not os.path.isfile(path):
            print(f"File {path} not found.")
            return name, None, None
        try:
            return name, load_wav_16k(path), None
        except Exception as e:                                              # noqa: BLE001  (per-file failure, as in the reference)
            return name, None, e

    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        writes = []

        def run_batch(items):
            out = encoder.forward([w for _, w in items])
            rows = out.rows.cpu()
            if out.take_range_bits() & 1:
                raise SerHipError("a value beyond the fp16 operand range, or a latent that is not finite, reached the quantizer "
                                  "(use --mode fp32x)")
            for b, (name, _) in enumerate(items):
                feats = rows[out.frame_offs[b]: out.frame_offs[b + 1]].clone()
                writes.append(pool.submit(save_feature, feats, feature_path(args.save_path, name)))

        for loaded in prefetch(make_batches(names, max(1, args.batch_size)), pool, load):
            items = []
            for name, wave, err in loaded:
                if err is not None:
                    fail(name, err)
                elif wave is not None:
                    items.append((name, wave))
            if items:
                run_or_each(items, run_batch, lambda it, e: fail(it[0], e))
        for w in writes:
            w.result()
    print(f"{len(names) - failed} files processed, {failed} failed")
    return 0
