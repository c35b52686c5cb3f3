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
CHECKPOINT_FILE = "ns3_facodec_decoder_v2.bin"
DEFAULT_CHECKPOINT = os.path.join(".", "pretrained_models", "ns3", CHECKPOINT_FILE)   # the reference's path
ENC, VQ = "melspec_encoder", "quantizer.0.layers.0"


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
    for i in range(spec.num_layers):
        p = f"{ENC}.layers.{i}"
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
    sd[f"{ENC}.last_ln.weight"] = 1.0 + 0.1 * torch.randn(D, generator=g)
    sd[f"{ENC}.last_ln.bias"] = 0.1 * torch.randn(D, generator=g)
    for name, (o, i) in (("in_proj", (spec.code_dim, D)), ("out_proj", (D, spec.code_dim))):
        v = uni((o, i), i)
        sd[f"{VQ}.{name}.weight_v"] = v
        sd[f"{VQ}.{name}.weight_g"] = v.norm(dim=1, keepdim=True) * (1.0 + 0.1 * torch.randn(o, 1, generator=g))
        sd[f"{VQ}.{name}.bias"] = uni((o,), i)
    sd[f"{VQ}._codebook.weight"] = torch.randn(spec.n_codes, spec.code_dim, generator=g)
    return sd


def prepare(sd: Dict[str, torch.Tensor], heads: int = 4) -> dict:
    """Everything ``engine.ProsodyEncoder`` uploads, as fp32 CPU tensors (folds in float64, one rounding):
      lin_w [D, n_mels], lin_b [D] = melspec_linear's bias + ``position0``
      layers: ln1 / ln2 (weight, bias), qkv (in_proj_weight [3D, D], bias), out, fc1 ([F, k * D] with W[n][j * D + c] = w[n][c][j], bias), fc2
      last_ln; w_in [8, D], b_in [8] (weight norm folded); codes [N, 8] L2-normalised; table [N, D] = out_proj of the RAW codes."""
    spec = spec_from_state_dict(sd, heads)
    if spec.head_dim != 64:
        raise ValueError(f"hidden size {spec.hidden} with {heads} heads: this stream's attention runs heads of 64 (the reference's 256 / 4)")
    D, F, k = spec.hidden, spec.ffn, spec.kernel
    f32 = lambda t: t.detach().double().float().contiguous()
    out = dict(spec=spec, lin_w=f32(sd["melspec_linear.weight"]), lin_b=(sd["melspec_linear.bias"].double() + position0(D)).float())
    layers = []
    for i in range(spec.num_layers):
        p = f"{ENC}.layers.{i}"
        a = p + ".self_attn"
        layers.append(dict(
            ln1=(f32(sd[p + ".ln_1.weight"]), f32(sd[p + ".ln_1.bias"])), ln2=(f32(sd[p + ".ln_2.weight"]), f32(sd[p + ".ln_2.bias"])),
            qkv=(f32(sd[a + ".in_proj_weight"]), f32(sd[a + ".in_proj_bias"])),
            out=(f32(sd[a + ".out_proj.weight"]), f32(sd[a + ".out_proj.bias"])),
            fc1=(f32(sd[p + ".ffn.ffn_1.weight"]).permute(0, 2, 1).reshape(F, k * D).contiguous(), f32(sd[p + ".ffn.ffn_1.bias"])),
            fc2=(f32(sd[p + ".ffn.ffn_2.weight"]), f32(sd[p + ".ffn.ffn_2.bias"]))))
    out["layers"] = layers
    out["last_ln"] = (f32(sd[ENC + ".last_ln.weight"]), f32(sd[ENC + ".last_ln.bias"]))
    out["w_in"] = weight_norm_linear(sd, VQ + ".in_proj").float().contiguous()
    out["b_in"] = f32(sd[VQ + ".in_proj.bias"])
    cb = sd[VQ + "._codebook.weight"].double()
    out["codes"] = (cb / cb.norm(dim=1, keepdim=True).clamp_min(1e-12)).float().contiguous()
    out["table"] = (cb @ weight_norm_linear(sd, VQ + ".out_proj").T + sd[VQ + ".out_proj.bias"].double()).float().contiguous()
    return out


# ------------------------------------------------------------------------------------------------------ the extraction driver
def build_parser():
    import argparse
    p = argparse.ArgumentParser(description="prosody features of every file in --wav_dir (the reference's preprocess_ns3_prosody.py)")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--save_path", type=str, default="./")
    p.add_argument("--wav_dir", type=str, default="./")
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--checkpoint", type=str, default="", help=f"a directory holding {CHECKPOINT_FILE}, or the file (default: {DEFAULT_CHECKPOINT})")
    p.add_argument("--mode", type=str, default="f16x", choices=("f16x", "fp32x", "bf16"))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--synthetic_weights", action="store_true", help="seeded weights at the reference's geometry (no checkpoint)")
    return p


def run(argv=None, encoder=None) -> int:
    """``<save_path>/<utterance>.pt`` -- a [len // 200 + 1, D] float32 tensor, what the reference's ``torch.save(feats, ...)`` leaves --
    for every file of ``--wav_dir``, on batchloop's loop and failure contract: a file that cannot be decoded, or is shorter than 400
    samples, is printed ("Failed to process ...") and costs only itself; a batch whose range guard or quantizer error word is set is
    run again file by file.  One GPU, 16 kHz input.  ``encoder``: a built ``engine.ProsodyEncoder`` (tests)."""
    from concurrent.futures import ThreadPoolExecutor
    from ._lib import SerHipError
    from .batchloop import make_batches, prefetch, run_or_each
    from .frontend import feature_path, load_wav_16k, save_feature
    args = build_parser().parse_args(argv)
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
        from .engine import ProsodyEncoder
        try:
            if args.synthetic_weights and not args.checkpoint:
                sd = synthetic_state_dict(ProsodySpec(), args.seed)
            else:
                sd = load_state_dict(args.checkpoint)
            encoder = ProsodyEncoder(sd, "cuda:0", args.mode)
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
