"""Times Whisper's token timestamps (GPU; profiles/whisper_timestamps.txt quotes this tool's output).

engine.WhisperDecoder at large-v3 geometry (seeded weights, random encoder states, the checkpoint's ten alignment heads), B = 16, mode f16x,
1 500 frames per utterance.  With seeded weights no row emits eos, so ``max_length`` sets the token count: 64 (60 generated tokens) and
448 (444).  Per token count, HIP events around
  the decode loop of the batch without and with the capture (``generate``; REPEATS calls after one warm-up, median),
  the recorded step replayed alone, default tape against capture tape, and the capture's launches alone (STEPS steps from position 64),
  ser_ts_weights_v, ser_ts_matrix_v (both kernels) and ser_dtw_v inside ``generate(token_times=True)``,
and, on this host's CPU, the wall time of HF's own ``_dynamic_time_warping`` on ONE matrix of the same size (one utterance; HF runs it
once per utterance).

    python tools/whisper_timestamps_bench.py [out.txt] [--tiny]
"""
from __future__ import annotations

import dataclasses
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from interspeech_ser_amd import _lib, config as Cfg                                    # noqa: E402
from interspeech_ser_amd.weights import synthetic_decoder_state_dict                   # noqa: E402

LARGE_V3_HEADS = ((7, 0), (10, 17), (12, 18), (13, 12), (16, 1), (17, 14), (19, 11), (21, 4), (24, 1), (25, 6))   # its generation_config.json
REPEATS, STEPS, BATCH = 3, 32, 16


def med(v):
    return f"median {np.median(v):.3f} min {min(v):.3f} max {max(v):.3f}"


def main(out_path: str = "", tiny: bool = False) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("whisper_timestamps_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import WhisperDecoder
    geo = Cfg.TINY_WHISPER_DEC if tiny else Cfg.WHISPER_LARGE_V3
    heads = ((0, 0), (0, 1), (1, 0)) if tiny else LARGE_V3_HEADS
    T, S, D, B = geo.max_target_positions, geo.max_source_positions, geo.hidden, BATCH
    base = Cfg.GenerationSpec(decoder_start_token_id=1, eos_token_id=2, pad_token_id=0, suppress_tokens=(1, 2), begin_suppress_tokens=(3,),
                              no_timestamps_token_id=5, lang_ids=(6, 7, 8), task_id=4, max_length=T, alignment_heads=heads)
    dec = WhisperDecoder(geo, synthetic_decoder_state_dict(geo, 0, fast=True), "cuda:0", "f16x", base)
    enc = torch.randn((B * S, D), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    lengths = [320 * S] * B
    lines = [f"Whisper token timestamps: {geo.name}, B = {B}, {len(heads)} alignment heads, {S} frames, mode f16x, seeded weights, HIP events; ms"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    for max_length in ((12, 20) if tiny else (64, T)):
        spec = dataclasses.replace(base, max_length=max_length)
        n = max_length - spec.PROMPT_LEN
        plain, with_times, stages = [], [], {}
        for it in range(1 + REPEATS):
            dec.ts_trace = None
            ms, res = timed(lambda: dec.generate(enc, B, spec))
            assert not res.failed
            dec.ts_trace = []
            ms_t, res_t = timed(lambda: dec.generate(enc, B, spec, token_times=True, lengths=lengths))
            assert np.array_equal(res.sequences, res_t.sequences) and all(len(t) == n for t in res_t.token_times), res_t.ts_status
            if it:
                plain.append(ms)
                with_times.append(ms_t)
                for name, a, b in dec.ts_trace:
                    stages.setdefault(name, []).append(a.elapsed_time(b))
        dec.ts_trace = None
        emit(f"{n} tokens: generate() {med(plain)}; generate(token_times=True) {med(with_times)} (cross projection, {max_length - 1} steps, read-back)")
        emit(f"{n} tokens: " + "; ".join(f"{k} {med(v)}" for k, v in stages.items()) + f" (sum of medians {sum(np.median(v) for v in stages.values()):.3f})")
        # the dynamic time warping of ONE utterance's matrix on the host, HF's own function
        try:
            from transformers.models.whisper.generation_whisper import _dynamic_time_warping
            m = res_t.ts_matrix[0, : n - 1, :S].cpu().double().numpy()
            t0 = time.perf_counter()
            _dynamic_time_warping(-m)
            emit(f"{n} tokens: HF _dynamic_time_warping on one {n - 1} x {S} matrix, this host's CPU: {1e3 * (time.perf_counter() - t0):.1f} ms wall")
        except ImportError:
            emit("transformers is not installed: no host figure")
    # the step alone: default tape against capture tape, from position 64
    stream = lambda: torch.cuda.current_stream().cuda_stream
    warm = 8 if tiny else 64
    for name, token_times in (("default", False), ("capture", True)):
        pl = dec.begin(B, base, token_times=token_times)
        dec.project_cross(pl, enc)
        for _ in range(warm):
            dec._run_step(pl, True)
        tape = pl["tape"]
        tapes = [(f"{name} step ({tape.n} launches)", tape)]
        if token_times:
            sub = tape.subset(lambda op: op == _lib.OP_DEC_KEEP_Q)
            tapes.append((f"the capture's {sub.n} launches alone", sub))
        for label, t in tapes:
            out = []
            for _ in range(5):
                pl["pos"].fill_(warm)

                def run():
                    for _ in range(STEPS):
                        _lib.check(_lib.lib.ser_run(t.cmds, t.n, None, stream()), "ser_run")
                out.append(1e3 * timed(run)[0] / STEPS)
            emit(f"{label}: {med(out)} us per step (positions {warm}..{warm + STEPS - 1})")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tiny"]
    main(args[0] if args else "", "--tiny" in sys.argv)
