"""Times engine.XVectorHead behind its encoder (GPU; profiles/xvector_times.txt is this tool's output).

wavlm-base-plus geometry with the default TDNN lists (512, 512, 512, 512, 1500 / 5, 3, 3, 1, 1 / 1, 2, 3, 1, 1), synthetic weights, one
ragged-free batch of 16 x 10 s, modes bf16 and f16x.  Per mode, in one process: warm-up forwards, then REPEATS timed pairs of (encoder
forward, head forward) with HIP events on the launch stream -- per repeat the head's milliseconds, the encoder's, and the share
head / encoder; the spread over the repeats is printed, not hidden in a mean -- and one traced head forward (one event pair per step) that
says which launch the time goes to.

    python tools/xvector_bench.py [out.txt]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                     # noqa: E402

WARMUP, REPEATS, BATCH, SECONDS = 3, 10, 16, 10


def synthetic_head(geo, spec, seed: int) -> dict:
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape, std=1.0: torch.randn(*shape, generator=g) * std              # noqa: E731
    dims = spec.tdnn_dim
    head = {"projector.weight": f(dims[0], geo.hidden, std=geo.hidden ** -0.5), "projector.bias": f(dims[0], std=0.5)}
    for i, k in enumerate(spec.tdnn_kernel):
        d_in = dims[i - 1] if i else dims[0]
        head[f"tdnn.{i}.kernel.weight"] = f(dims[i], k * d_in, std=(2.0 / (k * d_in)) ** 0.5)
        head[f"tdnn.{i}.kernel.bias"] = f(dims[i], std=0.3)
    head["feature_extractor.weight"] = f(spec.xvector_output_dim, 2 * dims[-1], std=(2 * dims[-1]) ** -0.5)
    head["feature_extractor.bias"] = f(spec.xvector_output_dim, std=0.5)
    head["classifier.weight"] = f(spec.xvector_output_dim, spec.xvector_output_dim, std=spec.xvector_output_dim ** -0.5)
    head["classifier.bias"] = f(spec.xvector_output_dim, std=0.5)
    if spec.use_weighted_layer_sum:
        head["layer_weights"] = f(geo.num_layers + 1)
    return head


def main(out_path: str = "") -> None:
    from interspeech_ser_amd.engine import XVectorHead, build_encoder
    if not torch.cuda.is_available():
        raise SystemExit("xvector_bench needs the GPU: a CPU run measures nothing")
    geo = C.WAVLM_BASE_PLUS
    lines = [f"x-vector head behind {geo.name}: {BATCH} x {SECONDS} s, synthetic weights, default TDNN lists; HIP events, {WARMUP} warm-up + "
             f"{REPEATS} timed forwards per mode, one process"]
    sd = synthetic_state_dict(geo, 7, fast=True)
    rng = np.random.default_rng(0)
    waves = [(0.1 * rng.standard_normal(SECONDS * 16000)).astype(np.float32) for _ in range(BATCH)]
    lengths = [len(w) for w in waves]
    for weighted in (True, False):
        spec = C.XVectorSpec.from_config({"architectures": ["WavLMForXVector"], "use_weighted_layer_sum": weighted})
        hsd = synthetic_head(geo, spec, 3)
        for mode in ("bf16", "f16x"):
            enc = build_encoder(geo, sd, "cuda:0", mode)
            head = XVectorHead(enc, hsd, spec)
            dev = enc.upload(waves)
            ev = lambda: torch.cuda.Event(enable_timing=True)                       # noqa: E731
            t_enc, t_head = [], []
            for it in range(WARMUP + REPEATS):
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                hs = enc.forward(dev, lengths)
                e1.record()
                rows = head.forward_rows(hs)
                e2.record()
                torch.cuda.synchronize()
                hs.take_range_bits()
                if it >= WARMUP:
                    t_enc.append(e0.elapsed_time(e1))
                    t_head.append(e1.elapsed_time(e2))
            assert torch.isfinite(rows).all()
            frames = hs.frame_offs[-1]
            share = [h / e for h, e in zip(t_head, t_enc)]
            fmt = lambda v: f"median {np.median(v):.3f} min {min(v):.3f} max {max(v):.3f}"      # noqa: E731
            lines.append(f"mode {mode} weighted_layer_sum={int(weighted)} ({frames} frames): head ms/batch {fmt(t_head)}; encoder forward ms/batch "
                         f"{fmt(t_enc)}; head / encoder {fmt(share)}")
            head.trace = []
            hs = enc.forward(dev, lengths)
            head.forward_rows(hs)
            torch.cuda.synchronize()
            lines.append("    steps (ms, one traced forward): " + ", ".join(f"{n} {a.elapsed_time(b):.3f}" for n, a, b in head.trace))
            head.trace = None
            del enc, head
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
