"""Times Whisper's segment-timestamp step (GPU; profiles/whisper_segments.txt quotes this tool's output).

engine.WhisperDecoder at large-v3 geometry (seeded weights, random encoder states, the checkpoint's token layout), B = 16, mode f16x, HIP
events.  The greedy step -- this tree's default plan, whose command list and kernels the change leaves as the parent commit has them; the
parent commit's own library is not loaded -- is measured twice in the same session: the difference of the
two runs is the spread a difference between two steps has to exceed.  Then the step that ends in ser_dec_select_ts_v, and the two select
kernels replayed alone.  eos is suppressed, so no row finishes and every row scans its logits at every step.

    python tools/whisper_segments_bench.py [out.txt] [--tiny]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from interspeech_ser_amd import _lib, config as Cfg                                    # noqa: E402
from interspeech_ser_amd.weights import synthetic_decoder_state_dict                   # noqa: E402

REPEATS, STEPS, BATCH = 5, 32, 16


def med(v):
    return f"median {np.median(v):.4f} min {min(v):.4f} max {max(v):.4f}"


def main(out_path: str = "", tiny: bool = False) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("whisper_segments_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import WhisperDecoder
    geo = Cfg.TINY_WHISPER_DEC if tiny else Cfg.WHISPER_LARGE_V3
    T, S, D, V, B = geo.max_target_positions, geo.max_source_positions, geo.hidden, geo.decoder_vocab_size, BATCH
    no_ts = V - 1502 if not tiny else V - 41                                  # large-v3: 50364, <|0.00|> = 50365, 1 501 timestamp tokens
    eos, start = no_ts - 107 if not tiny else no_ts - 11, (no_ts - 106 if not tiny else no_ts - 10)
    spec = Cfg.GenerationSpec(decoder_start_token_id=start, eos_token_id=eos, pad_token_id=eos, suppress_tokens=(eos, start, no_ts - 1),
                              begin_suppress_tokens=(220,), no_timestamps_token_id=no_ts, lang_ids=(start + 1, start + 2, start + 3),
                              task_id=no_ts - 4, max_length=T, max_initial_timestamp_index=50 if not tiny else 20)
    dec = WhisperDecoder(geo, synthetic_decoder_state_dict(geo, 0, fast=True), "cuda:0", "f16x", spec)
    gen = torch.Generator(device="cuda").manual_seed(3)
    warm = 8 if tiny else 64
    lines = [f"Whisper segment timestamps: {geo.name}, B = {B}, V = {V}, ts_begin = {spec.timestamp_begin}, {S} frames, mode f16x, seeded weights, "
             f"HIP events; {STEPS} steps from position {warm}, {REPEATS} windows"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    def window(pl, step):
        """ms per step over REPEATS windows of STEPS steps, the position put back before each"""
        out = []
        for _ in range(REPEATS):
            pl["pos"].fill_(warm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(STEPS):
                step()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / STEPS)
        return out

    stream = lambda: torch.cuda.current_stream().cuda_stream

    def replay(t):
        return lambda: _lib.check(_lib.lib.ser_run(t.cmds, t.n, None, stream()), "ser_run")

    def run(timestamps: bool):
        enc = torch.randn((B * S, D), device="cuda", generator=gen)
        pl = dec.begin(B, spec, timestamps=timestamps)
        dec.project_cross(pl, enc)
        for pos in range(warm):
            dec._run_step(pl, with_logits=pl["forced_host"][pos] < 0)
        torch.cuda.synchronize()
        assert int(pl["pos"].item()) == warm and int(pl["unfinished"].item()) == B
        step = window(pl, lambda: dec._run_step(pl, True))
        op = _lib.OP_DEC_SELECT_TS if timestamps else _lib.OP_DEC_SELECT
        select = window(pl, replay(pl["tape"].subset(lambda o: o == op)))
        assert int(pl["unfinished"].item()) == B, "a row finished: the select no longer scans every row"
        return step, select, int(pl["err"].item()), pl["ids"][:, : warm + 1].cpu().numpy()

    g1, s1, e1, _ = run(False)
    emit(f"greedy step (this tree's default plan), run 1: {med(g1)} ms; ser_dec_select_v alone: {med(s1)} ms")
    t1, st1, et, ids = run(True)
    g2, s2, e2, _ = run(False)
    emit(f"greedy step (this tree's default plan), run 2: {med(g2)} ms; ser_dec_select_v alone: {med(s2)} ms")
    spread = abs(np.median(g1) - np.median(g2))
    n_ts = int((ids[:, 3:] >= spec.timestamp_begin).sum())
    emit(f"timestamp step: {med(t1)} ms; ser_dec_select_ts_v alone: {med(st1)} ms = {100 * np.median(st1) / np.median(t1):.2f} % of the step "
         f"({n_ts} of {B * (warm - 2)} generated tokens are timestamps; error word {et:#x}, greedy {e1 | e2:#x})")
    g = min(np.median(g1), np.median(g2))
    emit(f"timestamp step - greedy step: {np.median(t1) - g:+.4f} ms (ratio {np.median(t1) / g:.4f}); spread of the two greedy runs {spread:.4f} ms; "
         f"select_ts - select alone: {np.median(st1) - min(np.median(s1), np.median(s2)):+.4f} ms")
    emit(f"the select reads B V 4 = {B * V * 4 / 1e6:.2f} MB of logits per step (+ {3 * V * 4 / 1e3:.0f} KB of mask rows, shared): "
         f"{B * V * 4 / 1e6 / np.median(st1):.1f} MB/ms alone; a row is one block of 512 threads ({V // 512 + 1} loads per thread), so "
         f"B = {B} blocks are in flight")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tiny"]
    main(args[0] if args else "", "--tiny" in sys.argv)
