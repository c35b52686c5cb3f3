"""Times the audio-classification tail (ser_layer_pool_v + ser_cls_tail_v) on an MI355X against the literal order in torch, on the same device
tensors, at WavLM-large geometry: 16 utterances of 10 s (499 frames each), D = 1024, 25 hidden states; projector 256, 8 labels.

Two arms: the softmax-weighted sum over all 25 states, and the last state alone.  Per arm and round, alternated in one process after a
warm-up of every shape: the two launchers back to back; the torch form (stack-weighted sum -> [M, D] x [D, P] projection -> per-utterance
mean -> classifier); and a device-to-device copy of the bytes the kernel reads, for the copy rate of the same run.  Times are HIP events
around ITERS calls; bytes are those the algorithm needs (the states once).

    python tools/audio_cls_bench.py [--rounds 7] [--iters 20]
"""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, D, L1, PROJ, LABELS = 16, 499, 1024, 25, 256, 8


def timed(fn, iters: int) -> float:
    """milliseconds per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no MI355X visible: this tool measures on the GPU only")
    from interspeech_ser_amd import _lib
    dev = "cuda:0"
    M = B * T
    g = torch.Generator(device=dev).manual_seed(0)
    states = torch.randn((L1, M, D), generator=g, device=dev, dtype=torch.float32)
    P, bp = torch.randn((PROJ, D), generator=g, device=dev) / 32, torch.randn(PROJ, generator=g, device=dev)
    Cw, bc = torch.randn((LABELS, PROJ), generator=g, device=dev) / 16, torch.randn(LABELS, generator=g, device=dev)
    w64 = torch.softmax(torch.randn(L1, generator=g, device=dev).double(), 0)
    one64 = torch.ones(1, dtype=torch.float64, device=dev)
    offs_host = (ctypes.c_int32 * (B + 1))(*[b * T for b in range(B + 1)])
    offs = torch.tensor(list(offs_host), dtype=torch.int32, device=dev)
    chunks = -(-T // _lib.LAYER_POOL_FC)
    work = torch.empty(B * chunks * D, dtype=torch.float64, device=dev)
    pooled = torch.empty((B, D), dtype=torch.float32, device=dev)
    out = torch.empty((B, LABELS), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def new_tail(n_states: int):
        first = states if n_states > 1 else states[-1:]
        p = _lib.LayerPoolArgs()
        p.s, p.state_stride, p.lds, p.w = first.data_ptr(), states.stride(0), D, (w64 if n_states > 1 else one64).data_ptr()
        p.frame_offs, p.frame_offs_host = offs.data_ptr(), ctypes.cast(offs_host, ctypes.c_void_p)
        p.work, p.work_elems, p.out, p.ldo = work.data_ptr(), work.numel(), pooled.data_ptr(), D
        p.n_states, p.B, p.D, p.rows, p.max_frames = n_states, B, D, M, T
        t = _lib.ClsTailArgs()
        t.pooled, t.ldp, t.P, t.bp, t.C, t.bc = pooled.data_ptr(), D, P.data_ptr(), bp.data_ptr(), Cw.data_ptr(), bc.data_ptr()
        t.out, t.ldo, t.B, t.D, t.proj, t.n_labels = out.data_ptr(), LABELS, B, D, PROJ, LABELS

        def pool_only():
            _lib.check(_lib.lib.ser_layer_pool_v(ctypes.byref(p), st), "ser_layer_pool_v")

        def both():
            pool_only()
            _lib.check(_lib.lib.ser_cls_tail_v(ctypes.byref(t), st), "ser_cls_tail_v")
        return pool_only, both

    w32 = w64.float().view(L1, 1, 1)

    def torch_tail(n_states: int):
        def run():
            x = (w32 * states).sum(0) if n_states > 1 else states[-1]
            y = torch.addmm(bp, x, P.t())
            return torch.addmm(bc, y.view(B, T, PROJ).mean(1), Cw.t())
        return run

    print(f"audio_cls_bench: B={B} T={T} D={D} states={L1} proj={PROJ} labels={LABELS}; {args.rounds} rounds x {args.iters} calls, alternated")
    for n_states in (L1, 1):
        pool_only, both = new_tail(n_states)
        ref = torch_tail(n_states)
        src = states if n_states > 1 else states[-1]
        dst = torch.empty_like(src)
        nbytes = src.numel() * 4
        both()
        got, want = out.clone(), ref()
        torch.cuda.synchronize()
        print(f"arm n_states={n_states}: max |new - torch| = {float((got - want).abs().max()):.3e} (max |torch| {float(want.abs().max()):.3f})")
        for fn in (pool_only, both, ref, lambda: dst.copy_(src)):                 # warm-up of every shape
            timed(fn, 3)
        rows = {"pool": [], "pool+tail": [], "torch": [], "copy": []}
        for _ in range(args.rounds):
            rows["pool"].append(timed(pool_only, args.iters))
            rows["pool+tail"].append(timed(both, args.iters))
            rows["torch"].append(timed(ref, args.iters))
            rows["copy"].append(timed(lambda: dst.copy_(src), args.iters))
        for k, v in rows.items():
            print(f"  {k:10s} ms/call: median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}   rounds " + " ".join(f"{x:.4f}" for x in v))
        pool_ms, copy_ms = statistics.median(rows["pool"]), statistics.median(rows["copy"])
        print(f"  ser_layer_pool_v: {nbytes / 1e6:.1f} MB read once -> {nbytes / pool_ms / 1e9:.3f} TB/s; copy of the same bytes (read + write, "
              f"{2 * nbytes / 1e6:.1f} MB): {2 * nbytes / copy_ms / 1e9:.3f} TB/s")
        print(f"  torch / new tail: {statistics.median(rows['torch']) / statistics.median(rows['pool+tail']):.1f}x "
              f"(slowest new {max(rows['pool+tail']):.4f} ms vs fastest torch {min(rows['torch']):.4f} ms)")


if __name__ == "__main__":
    main()
