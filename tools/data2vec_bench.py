"""data2vec-audio (layer-norm stem, post-LN encoder, 5 LayerNorm'd positional convs) on the GPU box: 16 x 10 s, synthetic weights.

    python tools/data2vec_bench.py [--models large,base] [--modes f16x,bf16] [--iters 20] [--oracle 1]

Prints one JSON line per (model, mode): forward utt/s (device events around replayed forwards, after warm-up), the positional stack's
time (its 5 grouped GEMMs + 5 ser_pos_ln_v row passes launched one by one over the batch's buffers, device events) and its share of a
forward, and the worst relative error against tests/data2vec_oracle.py (fp32 CPU) over --oracle utterances for hidden_states[0] and
[-1].  The split of the stack into GEMMs and row passes comes from a ``rocprofv3 --kernel-trace --stats`` run of this script
(pos_ln_kernel, and the GEMM dispatch in front of each of them)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from interspeech_ser_amd import config as C          # noqa: E402
from interspeech_ser_amd.engine import SpeechEncoder  # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict  # noqa: E402


def forward_rate(enc, dev, lengths, iters):
    enc.use_tape = True
    for _ in range(3):
        enc.forward(dev, lengths)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        enc.forward(dev, lengths)
    e1.record()
    torch.cuda.synchronize()
    return len(lengths) * iters / (e0.elapsed_time(e1) / 1e3)


def stack_ms(enc, lengths, iters):
    """mean time of the positional stack alone, over the buffers the last forward left (same shapes, same kernels)"""
    pl = enc._plan(lengths, 0)
    enc._st = torch.cuda.current_stream().cuda_stream
    enc._guard_word(pl)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    try:
        for _ in range(3):
            enc._pos_stack(pl, pl["states"])
        for e0, e1 in ev:
            e0.record()
            enc._pos_stack(pl, pl["states"])
            e1.record()
        torch.cuda.synchronize()
    finally:
        enc._st = None
    return float(np.mean([a.elapsed_time(b) for a, b in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="large,base")
    ap.add_argument("--modes", default="f16x,bf16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--oracle", type=int, default=1, help="utterances checked against the CPU oracle (0: none)")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    waves = [(0.1 * rng.standard_normal(160000)).astype(np.float32) for _ in range(16)]
    lengths = [len(w) for w in waves]
    for model in args.models.split(","):
        geo = {"large": C.DATA2VEC_AUDIO_LARGE, "base": C.DATA2VEC_AUDIO_BASE}[model]
        sd = synthetic_state_dict(geo, 7)
        refs = []
        if args.oracle:
            import data2vec_oracle as DO
            torch.set_num_threads(16)
            with torch.no_grad():
                refs = [DO.hidden_states(geo, sd, torch.from_numpy(DO.normalize_wave(waves[b]))) for b in range(args.oracle)]
        for mode in args.modes.split(","):
            enc = SpeechEncoder(geo, sd, "cuda:0", mode=mode)
            dev = enc.upload(waves)
            fwd = forward_rate(enc, dev, lengths, args.iters)
            hs = enc.forward(dev, lengths)
            torch.cuda.synchronize()
            err = {}
            for layer in (0, -1):
                err[f"hs{layer}"] = max([float((hs.utterance(b, layer).cpu() - r[layer]).abs().max() / max(1.0, float(r[layer].abs().max())))
                                         for b, r in enumerate(refs)], default=None)
            ms = stack_ms(enc, lengths, args.iters)
            step_ms = 1e3 * len(lengths) / fwd
            print(json.dumps({"model": geo.name, "mode": mode, "batch": "16 x 10 s", "forward_utt_per_s": round(fwd, 1),
                              "pos_stack_ms": round(ms, 3), "pos_stack_share_of_forward": round(ms / step_ms, 4),
                              "oracle_rel_err": {k: (None if v is None else float(f"{v:.3e}")) for k, v in err.items()}}), flush=True)
            del enc, hs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
