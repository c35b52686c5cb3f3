"""Times the forced-alignment step (GPU; profiles/ctc_align.txt quotes this tool's output).

engine.CTCHead.forward_align behind a speech encoder of hubert-xlarge geometry (D = 1280), V = 32, mode f16x, on the rows of 16 x 10 s
(T = 499 frames each, M = 7 984) of seeded hidden states, with seeded targets of L = 40, 150 and 500 tokens per utterance (cut to T, the longest target T frames can hold): WARMUP warm-up
calls, then REPEATS traced calls (one HIP event pair per step: the operand copy, the lm_head ser_gemm, ser_ctc_align_v's two kernels);
median, min and max over the repeats.  forward_tokens (ser_ctc_greedy_v) on the same rows and the encoder's forward of the same batch
(16 seeded ten-second waveforms, FWD_REPEATS calls) stand beside it.

    python tools/ctc_align_bench.py [out.txt]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from interspeech_ser_amd import config as C                                      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                     # noqa: E402
from ctc_bench import synthetic_lm_head                                    # noqa: E402

WARMUP, REPEATS, FWD_REPEATS, BATCH, SECONDS, V = 3, 20, 5, 16, 10, 32
TOKENS = (40, 150, 500)


def fmt(v) -> str:
    return f"median {np.median(v):.1f} min {min(v):.1f} max {max(v):.1f}"


def traced(head, call) -> dict:
    steps: dict = {}
    for it in range(WARMUP + REPEATS):
        head.trace = [] if it >= WARMUP else None
        call()
        torch.cuda.synchronize()
        if head.trace is not None:
            for n, a, b in head.trace:
                steps.setdefault(n, []).append(1e3 * a.elapsed_time(b))
    head.trace = None
    return steps


def main(out_path: str = "") -> None:
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import CTCHead, HiddenStates, build_encoder
    mode = "f16x"
    geo = C.geometry_for("facebook/hubert-xlarge-ls960-ft")
    enc = build_encoder(geo, synthetic_state_dict(geo, 7, fast=True), "cuda:0", mode)
    head = CTCHead(enc, synthetic_lm_head(geo.hidden, 3), C.CTCSpec(V, 0, "HubertForCTC"))
    T = geo.frames_for(SECONDS * 16000)
    offs = [b * T for b in range(BATCH + 1)]
    g = torch.Generator(device="cuda").manual_seed(5)
    hs = HiddenStates(torch.randn((1, offs[-1], geo.hidden), generator=g, device="cuda", dtype=torch.float32), offs)
    lines = [f"CTC forced alignment: {BATCH} x {SECONDS} s (T = {T}, M = {offs[-1]}), D = {geo.hidden} ({geo.name}), V = {V}, mode {mode}, seeded "
             f"weights and targets, HIP events, {WARMUP} warm-up + {REPEATS} traced calls, one process; us per call"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    steps = traced(head, lambda: head.forward_tokens(hs))
    emit("forward_tokens (greedy): " + "; ".join(f"{n} {fmt(v)}" for n, v in steps.items()))
    rng = np.random.default_rng(9)
    for L in TOKENS:
        L = min(L, T)                                                             # 500 tokens cannot be placed on 499 frames: the longest feasible target
        targets = []
        for _ in range(BATCH):
            y = [int(rng.integers(1, V))]
            while len(y) < L:                                                     # no equal neighbours: L <= T is enough frames
                v = int(rng.integers(1, V))
                if v != y[-1]:
                    y.append(v)
            targets.append(y)
        for frames in (False, True):
            steps = traced(head, lambda: head.forward_align(hs, targets, frames=frames))
            status = CTCHead.unpack_align(head.forward_align(hs, targets, frames=frames).cpu().numpy(), BATCH, L, offs[-1] if frames else 0)["status"]
            assert not status.any(), status
            emit(f"forward_align L = {L}, per-frame outputs {'on' if frames else 'off'}: " + "; ".join(f"{n} {fmt(v)}" for n, v in steps.items()))
    # the encoder's forward of the same batch
    waves = [np.random.default_rng(100 + b).standard_normal(SECONDS * 16000).astype(np.float32) * 0.1 for b in range(BATCH)]
    dev = enc.upload(waves, 0)
    lengths = [len(w) for w in waves]
    times = []
    for it in range(2 + FWD_REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        enc.forward(dev, lengths)
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times.append(1e3 * e0.elapsed_time(e1))
    emit(f"encoder forward of the same batch ({FWD_REPEATS} calls after 2 warm-up): {fmt(times)}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "")
