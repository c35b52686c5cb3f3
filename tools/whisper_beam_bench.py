"""Times Whisper beam search (GPU; profiles/whisper_beams.txt quotes this tool's output).

engine.WhisperDecoder at large-v3 geometry (seeded weights, random encoder states), B = 16 utterances, mode f16x, HIP events.  Per K in
{2, 5}: the beam step (B K rows: body, logits, ser_beam_select_v) against the greedy step at B = 16 and at B = 16 K rows -- the greedy
plan and its kernels are the parent commit's, untouched, so the greedy B = 16 K step is the fair price of the extra rows --, then the
select's two launches and the table attention's launches replayed alone (against ser_dec_attn_v's of the greedy B = 16 K step), and the
cache bytes.  With seeded weights no row emits eos: every utterance stays live.

    python tools/whisper_beam_bench.py [out.txt] [--tiny]
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
    return f"median {np.median(v):.3f} min {min(v):.3f} max {max(v):.3f}"


def main(out_path: str = "", tiny: bool = False) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("whisper_beam_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import WhisperDecoder
    geo = Cfg.TINY_WHISPER_DEC if tiny else Cfg.WHISPER_LARGE_V3
    T, S, D, L, B = geo.max_target_positions, geo.max_source_positions, geo.hidden, geo.decoder_layers, BATCH
    spec = Cfg.GenerationSpec(decoder_start_token_id=1, eos_token_id=2, pad_token_id=0, suppress_tokens=(1, 2), begin_suppress_tokens=(3,),
                              no_timestamps_token_id=5, lang_ids=(6, 7, 8), task_id=4, max_length=T)
    dec = WhisperDecoder(geo, synthetic_decoder_state_dict(geo, 0, fast=True), "cuda:0", "f16x", spec)
    gen = torch.Generator(device="cuda").manual_seed(3)
    warm = 8 if tiny else 64
    lines = [f"Whisper beam search: {geo.name}, B = {B}, {S} frames, mode f16x, seeded weights, HIP events; "
             f"{STEPS} steps from position {warm}, {REPEATS} windows"]

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

    def greedy(rows):
        enc = torch.randn((rows * S, D), device="cuda", generator=gen)
        pl = dec.begin(rows, spec)
        dec.project_cross(pl, enc)
        for _ in range(warm):
            dec._run_step(pl, True)
        step = window(pl, lambda: dec._run_step(pl, True))
        attn = window(pl, replay(pl["tape"].subset(lambda op: op == _lib.OP_DEC_ATTN)))
        return step, attn

    g16, _ = greedy(B)
    emit(f"greedy step, {B} rows: {med(g16)} ms")
    for K in (2, 5):
        rows = B * K
        gk, gk_attn = greedy(rows)
        enc = torch.randn((B * S, D), device="cuda", generator=gen)
        pl = dec.begin(B, spec, num_beams=K)
        dec.project_cross(pl, enc)
        for pos in range(warm):
            dec._run_step(pl, with_logits=pl["forced_host"][pos] < 0, beam=pos >= spec.PROMPT_LEN - 1)
        torch.cuda.synchronize()
        assert int(pl["err"].item()) == 0 and int(pl["pos"].item()) == warm
        step = window(pl, lambda: dec._run_step(pl, True, beam=True))
        tape = pl["tape"]
        select = window(pl, replay(tape.subset(lambda op: op == _lib.OP_BEAM_SELECT)))
        attn = window(pl, replay(tape.subset(lambda op: op == _lib.OP_DEC_ATTN_BEAM)))
        assert int(pl["err"].item()) == 0
        emit(f"K = {K}: beam step, {rows} rows: {med(step)} ms; greedy step at {rows} rows: {med(gk)} ms "
             f"(ratio of medians {np.median(step) / np.median(gk):.3f}; against {B} rows {np.median(step) / np.median(g16):.3f})")
        emit(f"K = {K}: ser_beam_select_v alone (scan + merge): {med(select)} ms = {100 * np.median(select) / np.median(step):.1f} % of the step; "
             f"ser_dec_attn_beam_v x {2 * L} alone: {med(attn)} ms against ser_dec_attn_v x {2 * L} at {rows} rows: {med(gk_attn)} ms")
        self_bytes, cross_bytes = 2 * L * rows * T * D * 4, L * B * S * 2 * D * 4
        table_bytes, greedy_cross = 2 * rows * T * 4, L * rows * S * 2 * D * 4
        emit(f"K = {K}: self cache {self_bytes / 1e9:.2f} GB ({K} x the greedy {2 * L * B * T * D * 4 / 1e9:.2f} GB), cross cache {cross_bytes / 1e9:.2f} GB "
             f"(shared by the beams; {rows} greedy rows would hold {greedy_cross / 1e9:.2f} GB), ancestor table {table_bytes / 1e3:.0f} KB; "
             f"per step the select copies at most {rows * T * 4 / 1e3:.0f} KB of table, not the {2 * L * rows * warm * D * 4 / 1e9:.2f} GB of keys and "
             f"values a cache reorder gathers at position {warm}")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tiny"]
    main(args[0] if args else "", "--tiny" in sys.argv)
