"""Times Whisper's scored decode step against the unscored one (GPU; profiles/whisper_scores.txt quotes this tool's output).

tools/whisper_segments_bench.py's set-up: engine.WhisperDecoder at large-v3 geometry (seeded weights, random encoder states, the
checkpoint's token layout), B = 16, mode f16x, HIP events, eos suppressed so that every row scans its logits at every step.  Per plan
kind (greedy, timestamps) the unscored step, the scored step and the unscored step again, alternated in one process -- the two unscored
runs' difference is the spread a difference has to exceed -- and the select kernels replayed alone.

    python tools/whisper_scores_bench.py [out.txt] [--tiny]
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
        raise SystemExit("whisper_scores_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import WhisperDecoder
    geo = Cfg.TINY_WHISPER_DEC if tiny else Cfg.WHISPER_LARGE_V3
    T, S, D, V, B = geo.max_target_positions, geo.max_source_positions, geo.hidden, geo.decoder_vocab_size, BATCH
    no_ts = V - 1502 if not tiny else V - 41
    eos, start = no_ts - 107 if not tiny else no_ts - 11, (no_ts - 106 if not tiny else no_ts - 10)
    spec = Cfg.GenerationSpec(decoder_start_token_id=start, eos_token_id=eos, pad_token_id=eos, suppress_tokens=(eos, start, no_ts - 1),
                              begin_suppress_tokens=(220,), no_timestamps_token_id=no_ts, lang_ids=(start + 1, start + 2, start + 3),
                              task_id=no_ts - 4, max_length=T, max_initial_timestamp_index=50 if not tiny else 20)
    dec = WhisperDecoder(geo, synthetic_decoder_state_dict(geo, 0, fast=True), "cuda:0", "f16x", spec)
    warm = 8 if tiny else 64
    lines = [f"Whisper transcript scores: {geo.name}, B = {B}, V = {V}, ts_begin = {spec.timestamp_begin}, {S} frames, mode f16x, seeded weights, "
             f"HIP events; {STEPS} steps from position {warm}, {REPEATS} windows"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    def window(pl, step):
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

    def run(timestamps: bool, scores: bool):
        enc = torch.randn((B * S, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
        pl = dec.begin(B, spec, timestamps=timestamps, scores=scores)
        dec.project_cross(pl, enc)
        for pos in range(warm):
            dec._run_step(pl, with_logits=pl["forced_host"][pos] < 0 or (scores and pos == 0))
        torch.cuda.synchronize()
        assert int(pl["pos"].item()) == warm and int(pl["unfinished"].item()) == B
        step = window(pl, lambda: dec._run_step(pl, True))
        op = _lib.OP_DEC_SELECT_SCORE if scores else (_lib.OP_DEC_SELECT_TS if timestamps else _lib.OP_DEC_SELECT)
        select = window(pl, replay(pl["tape"].subset(lambda o: o == op)))
        assert int(pl["unfinished"].item()) == B, "a row finished: the select no longer scans every row"
        return step, select, int(pl["err"].item()), pl["ids"][:, : warm + 1].cpu().numpy()

    for ts in (False, True):
        kind = "timestamps" if ts else "greedy"
        name = "ser_dec_select_ts_v" if ts else "ser_dec_select_v"
        u1, su1, e1, ids1 = run(ts, False)
        emit(f"{kind} step, unscored, run 1: {med(u1)} ms; {name} alone: {med(su1)} ms")
        s1, ss1, es, ids_s = run(ts, True)
        u2, su2, e2, _ = run(ts, False)
        emit(f"{kind} step, unscored, run 2: {med(u2)} ms; {name} alone: {med(su2)} ms")
        emit(f"{kind} step, scored: {med(s1)} ms; ser_dec_select_score_v (rule {int(ts)}) alone: {med(ss1)} ms = "
             f"{100 * np.median(ss1) / np.median(s1):.2f} % of the step (error words {es:#x} / {e1 | e2:#x}; the same ids as the unscored run: "
             f"{bool(np.array_equal(ids1, ids_s))})")
        u, su = min(np.median(u1), np.median(u2)), min(np.median(su1), np.median(su2))
        emit(f"{kind}: scored - unscored step {np.median(s1) - u:+.4f} ms (ratio {np.median(s1) / u:.4f}); spread of the two unscored runs "
             f"{abs(np.median(u1) - np.median(u2)):.4f} ms; the select's own growth {np.median(ss1) - su:+.4f} ms "
             f"({B} blocks x {V} float64 exp = {B * V / 1e6:.2f} M exp per step)")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tiny"]
    main(args[0] if args else "", "--tiny" in sys.argv)
