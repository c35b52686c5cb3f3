"""Whisper decoder at large-v3 geometry (seeded weights, random encoder states, B = 16): time per decode step and its anatomy by kernel
class, the bytes a step must read against the HBM rate measured in the same run, and the one-off cross-cache projection (GPU).

    python tools/transcribe_bench.py [--modes bf16 f16x] [--batch 16] [--warm 64] [--steps 32]

Method: the decoder's own recorded step list is replayed (ser_run) from position ``warm`` on; ``steps`` consecutive steps between two
events, median of 5 repeats, each repeat restarted at the same position so the self cache has the same length.  Anatomy: copies of the
recorded commands of ONE class (Tape.subset's mechanism) replayed alone over the same buffers, the same way.  Classes: the GEMMs, the self
attention, the cross attention, the LayerNorms, embed + select.  A class alone loses the overlap of its neighbours' tails, so the classes
need not add up to the step.  HBM rate: tools/hbm_probe.py, run as a child process before this process opens the GPU; the figure used is
its 1024 MB copy (read + write).  Files/s (--files N, default 256 ten-second clips of seeded noise + tone, in memory, so no wav decoding is
timed on either side): WhisperTranscriber.transcribe against the encoder-only forward over the same clips in batches of 16, alternated,
--rounds times each (default 2), every figure printed.  With seeded weights no row ever emits eos (it is suppressed), so every batch decodes
to max_length: the transcription rate is a lower bound for real speech.  Prints one line per figure."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import _lib, config as Cfg                                   # noqa: E402
from interspeech_ser_amd.engine import WhisperDecoder                           # noqa: E402
from interspeech_ser_amd.weights import synthetic_decoder_state_dict                  # noqa: E402


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        before = fn(None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(before)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def hbm_rate():
    """bytes/s of tools/hbm_probe.py's largest copy, from a child process of its own"""
    import re
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "hbm_probe.py")], capture_output=True,
                         text=True, check=True, timeout=300).stdout
    line = [ln for ln in out.splitlines() if ln.strip().startswith("1024 MB")][-1]
    us = float(re.search(r"copy\s+([0-9.]+) us", line).group(1))            # its own TB/s column is mis-scaled: take the time
    return 2 * 1024 * 1048576 / (us * 1e-6), line.strip()


def files_per_second(a, geo, spec, sd_dec):
    import time
    from interspeech_ser_amd.engine import WhisperEncoder
    from interspeech_ser_amd.transcribe import BATCH, WhisperTranscriber
    from interspeech_ser_amd.weights import synthetic_state_dict
    rng = np.random.default_rng(0)
    t = np.arange(160000) / 16000.0
    waves = [np.clip(0.1 * rng.standard_normal(160000) + 0.2 * np.sin(2 * np.pi * (200 + i) * t), -1, 1).astype(np.float32) for i in range(a.files)]
    for mode in a.modes:
        sd = synthetic_state_dict(geo, 0, fast=True)
        enc = WhisperEncoder(geo, sd, "cuda:0", mode)
        del sd
        tr = WhisperTranscriber(enc, WhisperDecoder(geo, sd_dec, "cuda:0", mode, spec), spec)

        def encode_only():
            for n, i in enumerate(range(0, len(waves), BATCH)):
                w = waves[i:i + BATCH]
                hs = enc.forward(enc.upload(w, n % 2), [len(x) for x in w], slot=n % 2)
                hs.take_range_bits()
        tr.transcribe(waves[:BATCH])                         # plans, command lists
        encode_only()
        for r in range(a.rounds):
            for name, fn in (("encoder only", encode_only), ("transcribe", lambda: tr.transcribe(waves))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                print(f"TRANSCRIBE {mode} files/s round {r} {name}: {len(waves) / dt:.1f} files/s ({len(waves)} x 10 s in {dt:.2f} s)", flush=True)
        del tr, enc
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="+", default=["bf16", "f16x"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["step", "files"], default=None)
    ap.add_argument("--tiny", action="store_true", help="the tiny fixture geometry (a functional check of this tool)")
    a = ap.parse_args()
    geo = Cfg.TINY_WHISPER_DEC if a.tiny else Cfg.WHISPER_LARGE_V3
    V, T = geo.decoder_vocab_size, geo.max_target_positions
    if a.warm + a.steps + 8 >= T:
        a.warm, a.steps = T // 2, T // 8
    spec = Cfg.GenerationSpec(decoder_start_token_id=1, eos_token_id=2, pad_token_id=0, suppress_tokens=(1, 2), begin_suppress_tokens=(3,),
                              no_timestamps_token_id=5, lang_ids=(6, 7, 8), task_id=4, max_length=T)
    sd = synthetic_decoder_state_dict(geo, 0, fast=True)
    if a.only == "files":
        return files_per_second(a, geo, spec, sd)
    rate, line = hbm_rate()
    print(f"TRANSCRIBE hbm copy rate {rate / 1e12:.2f} TB/s (tools/hbm_probe.py: {line})", flush=True)
    B, D, S, L = a.batch, geo.hidden, geo.max_source_positions, geo.decoder_layers
    enc = torch.randn((B * S, D), device="cuda")
    stream = lambda: torch.cuda.current_stream().cuda_stream
    for mode in a.modes:
        dec = WhisperDecoder(geo, sd, "cuda:0", mode, spec)
        pl = dec.begin(B, spec)
        ms, lo, hi = median_ms(lambda b: dec.project_cross(pl, enc) if b is not None else 0, 3)
        print(f"TRANSCRIBE {mode} cross-cache projection: {ms:.2f} ms per batch of {B} (min {lo:.2f}, max {hi:.2f}; {L} GEMMs of M = {B * S}, N = {2 * D})", flush=True)
        for _ in range(a.warm):
            dec._run_step(pl, True)
        torch.cuda.synchronize()
        assert int(pl["pos"].item()) == a.warm and int(pl["err"].item()) == 0, (int(pl["pos"].item()), int(pl["err"].item()))
        tape = dec.recorded_tape(B, 0)

        def run(t, n, resets_pos):
            def fn(before):
                if before is None:
                    pl["pos"].fill_(a.warm)
                    return 1
                for _ in range(n):
                    _lib.check(_lib.lib.ser_run(t.cmds, t.n, None, stream()), "ser_run")
            return median_ms(fn, 5)

        step, lo, hi = run(tape, a.steps, True)
        print(f"TRANSCRIBE {mode} step: {step / a.steps * 1e3:.1f} us (min {lo / a.steps * 1e3:.1f}, max {hi / a.steps * 1e3:.1f}; positions {a.warm}..{a.warm + a.steps - 1}, "
              f"{tape.n} launches, B = {B})", flush=True)
        classes = {                                       # Tape.subset with by_cmd: the two attentions are one op
            "GEMMs": lambda c: c.op == _lib.OP_GEMM,
            "self attention": lambda c: c.op == _lib.OP_DEC_ATTN and bool(c.u.dec_attn.k_new),
            "cross attention": lambda c: c.op == _lib.OP_DEC_ATTN and not c.u.dec_attn.k_new,
            "LayerNorms": lambda c: c.op == _lib.OP_LAYERNORM,
            "embed + select": lambda c: c.op in (_lib.OP_DEC_EMBED, _lib.OP_DEC_SELECT),
        }
        for name, keep in classes.items():
            t = tape.subset(keep, by_cmd=True)
            ms, lo, hi = run(t, a.steps, True)
            print(f"TRANSCRIBE {mode}   {name}: {ms / a.steps * 1e3:.1f} us per step ({t.n} launches; min {lo / a.steps * 1e3:.1f}, max {hi / a.steps * 1e3:.1f})", flush=True)
        lin = [dec.proj] + [lay[k] for lay in dec.layers for k in ("qkv", "out", "cq", "cout", "fc1", "fc2")]
        wbytes = sum(x.w.numel() * x.w.element_size() for x in lin)
        pos = a.warm + a.steps // 2
        self_b, cross_b = 2 * L * B * pos * D * 4, L * B * S * 2 * D * 4
        total = wbytes + self_b + cross_b
        print(f"TRANSCRIBE {mode} bytes per step: weight planes {wbytes / 1e9:.2f} GB, self cache at position {pos} {self_b / 1e9:.3f} GB, cross cache "
              f"{cross_b / 1e9:.2f} GB = {total / 1e9:.2f} GB -> {total / rate * 1e6:.0f} us at the copy rate; the step takes "
              f"{step / a.steps * 1e3 / (total / rate * 1e6):.2f} x that", flush=True)
        del dec, pl, tape
        torch.cuda.empty_cache()
    if a.only is None and a.files > 0:
        files_per_second(a, geo, spec, sd)


if __name__ == "__main__":
    main()
