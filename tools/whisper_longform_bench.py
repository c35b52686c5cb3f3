"""Times Whisper long-form transcription (GPU; profiles/whisper_longform.txt quotes this tool's output).

engine.WhisperEncoder / WhisperDecoder at large-v3 geometry (seeded weights, seeded noise, the checkpoint's token layout), mode f16x, HIP
events.  Every A/B is measured A/B/A in one process and the two A runs are printed: their difference is the spread a difference between
A and B has to exceed.

  1. ser_logmel_long_v on 16 files of 5 min, per frame, beside ser_logmel_whisper on 16 x 30 s, per frame
  2. ser_mel_window_v at B = 16
  3. one round of forward_windows + timestamps decode against forward + generate(timestamps=True), B = 16, max_length cut to 48 tokens
  4. a list of mixed lengths through the window queue against "finish 16 files before admitting more": rows busy and windows per second

    python tools/whisper_longform_bench.py [out.txt] [--tiny]
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from interspeech_ser_amd import config as Cfg                                          # noqa: E402
from interspeech_ser_amd import transcribe as TR                                       # noqa: E402
from interspeech_ser_amd.weights import synthetic_decoder_state_dict, synthetic_state_dict   # noqa: E402

REPEATS, BATCH = 7, 16


def med(v):
    return f"median {np.median(v):.4f} min {min(v):.4f} max {max(v):.4f}"


def timed(fn, repeats=REPEATS):
    """ms per call over ``repeats`` calls, HIP events, one warm-up"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main(out_path: str = "", tiny: bool = False) -> None:
    if not torch.cuda.is_available():
        raise SystemExit("whisper_longform_bench needs the GPU: a CPU run measures nothing")
    from interspeech_ser_amd.engine import WhisperDecoder, WhisperEncoder
    import dataclasses
    geo = Cfg.with_decoder(dataclasses.replace(Cfg.TINY_WHISPER, name="tiny-whisper-long"), 2, 2, 512, 1983, 64) if tiny else Cfg.WHISPER_LARGE_V3
    V = geo.decoder_vocab_size
    no_ts = V - 1502
    eos, start = no_ts - 107, no_ts - 106
    spec = Cfg.GenerationSpec(decoder_start_token_id=start, eos_token_id=eos, pad_token_id=eos, suppress_tokens=(start, no_ts - 1),
                              begin_suppress_tokens=(220, eos), no_timestamps_token_id=no_ts, lang_ids=(start + 1, start + 2, start + 3),
                              task_id=no_ts - 4, max_length=24 if tiny else 48, max_initial_timestamp_index=50, language=start + 1)
    sd = dict(synthetic_state_dict(geo, 0, fast=True))
    sd.update(synthetic_decoder_state_dict(geo, 0, fast=True))
    enc = WhisperEncoder(geo, sd, "cuda:0", "f16x")
    dec = WhisperDecoder(geo, sd, "cuda:0", "f16x", spec)
    tr = TR.WhisperTranscriber(enc, dec, spec)
    rng = np.random.default_rng(0)
    noise = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    lines = [f"Whisper long-form: {geo.name}, n_mels {geo.n_mels}, mode f16x, seeded weights and noise, HIP events, {REPEATS} repeats, "
             f"language forced, max_length {spec.max_length}"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    # 1. the front ends, per frame
    minutes = 1 if tiny else 5
    long_waves = [noise(16000 * 60 * minutes + 7 * k) for k in range(BATCH)]
    short_waves = [w[:480000] for w in long_waves]
    packed_long, packed_short = enc.upload(long_waves, 0).clone(), enc.upload(short_waves, 1).clone()
    lens_long, lens_short = [len(w) for w in long_waves], [480000] * BATCH
    frames_long, frames_short = sum(n // 160 for n in lens_long), 3000 * BATCH
    handles = []

    def run_long():
        handles.clear()                                     # one handle alive at a time: the buffer is reused by the allocator
        handles.append(enc.log_mel_long(packed_long, lens_long))
    a1 = timed(lambda: enc.log_mel(packed_short, lens_short, slot=1))
    b = timed(run_long)
    a2 = timed(lambda: enc.log_mel(packed_short, lens_short, slot=1))
    emit(f"1. ser_logmel_whisper 16 x 30 s ({frames_short} frames), run 1: {med(a1)} ms = {1e6 * np.median(a1) / frames_short:.2f} ns/frame; "
         f"run 2: {med(a2)} ms = {1e6 * np.median(a2) / frames_short:.2f} ns/frame")
    emit(f"   ser_logmel_long_v 16 x {minutes} min ({frames_long} frames; tables uploaded inside the timed call): {med(b)} ms = "
         f"{1e6 * np.median(b) / frames_long:.2f} ns/frame; spread of the two 30 s runs {abs(np.median(a1) - np.median(a2)) * 1e6 / frames_short:.2f} ns/frame")

    # 2. the gather
    h = handles[0]
    rows = [(k, 1001 + 13 * k, 3000) for k in range(BATCH)]
    pl = enc._plan_of(BATCH, 0)
    enc.forward_windows(h, rows, slot=0)
    tape = pl["win"]["tape"]
    from interspeech_ser_amd import _lib
    sub = tape.subset(lambda o: o == _lib.OP_MEL_WINDOW)
    stream = lambda: torch.cuda.current_stream().cuda_stream
    w1 = timed(lambda: _lib.check(_lib.lib.ser_run(sub.cmds, sub.n, None, stream()), "ser_run"))
    w2 = timed(lambda: _lib.check(_lib.lib.ser_run(sub.cmds, sub.n, None, stream()), "ser_run"))
    mb = BATCH * geo.n_mels * 3000 * 4 * 2 / 1e6
    emit(f"2. ser_mel_window_v B = 16 (odd seeks, nf = 3000; {mb:.1f} MB read + written), run 1: {med(w1)} ms; run 2: {med(w2)} ms")

    # 3. one round, A/B/A
    def round_forward():
        hs = enc.forward(packed_short, lens_short, slot=1)
        return dec.generate(hs.states[-1], BATCH, spec, slot=1, timestamps=True, lengths=lens_short)

    def round_windows():
        hs = enc.forward_windows(h, [(k, 0, 3000) for k in range(BATCH)], slot=0)
        return dec.generate(hs.states[-1], BATCH, spec, slot=0, timestamps=True, num_frames=[3000] * BATCH)
    r = 3 if not tiny else REPEATS
    f1 = timed(round_forward, r)
    wn = timed(round_windows, r)
    f2 = timed(round_forward, r)
    emit(f"3. one round at B = 16: forward + generate(timestamps=True), run 1: {med(f1)} ms; run 2: {med(f2)} ms")
    emit(f"   forward_windows + generate(timestamps=True, num_frames=): {med(wn)} ms; windows - forward: "
         f"{np.median(wn) - min(np.median(f1), np.median(f2)):+.3f} ms; spread of the two forward runs {abs(np.median(f1) - np.median(f2)):.3f} ms "
         f"(the forward round computes its log-mel, the windows round gathers it and uploads the row table)")
    handles.clear()
    del h

    # 4. the queue on mixed lengths
    n_files = 24 if tiny else 40
    secs = np.exp(rng.uniform(np.log(35.0), np.log(600.0 if not tiny else 120.0), size=n_files))
    secs[:4] = [10.0, 20.0, 29.0, 30.0]                      # the short files of a mixed list: the one-window path, outside the queue
    items = [(f"f{k}.wav", noise(int(16000 * s) + k)) for k, s in enumerate(secs)]
    longs = [it for it in items if TR.is_long(len(it[1]))]

    def run(chunks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rounds, failed = [], 0
        for chunk in chunks:
            tr.transcribe_long(iter(chunk), batch=BATCH)
            rounds += [len(r[1]) for r in tr.rounds]
            failed += len(tr.failed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return sum(rounds), len(rounds), dt, failed
    run([longs[:BATCH]])                                     # plans and command lists of both slots exist before anything is timed
    for name, chunks in (("window queue (a finished file's row is refilled)", [longs]),
                         ("finish 16 files before admitting more", [longs[i: i + BATCH] for i in range(0, len(longs), BATCH)]),
                         ("window queue, again", [longs])):
        windows, rounds, dt, failed = run(chunks)
        emit(f"4. {len(longs)} files of {min(len(w) for _, w in longs) / 16000:.0f} to {max(len(w) for _, w in longs) / 16000:.0f} s, {name}: "
             f"{windows} windows in {rounds} rounds, rows busy {100.0 * windows / (rounds * BATCH):.1f} %, {dt:.2f} s wall = {windows / dt:.2f} windows/s"
             f"{'' if not failed else f' ({failed} files failed)'}")
    windows, rounds, dt, failed = run([items])
    emit(f"   the whole list of {len(items)} files ({len(items) - len(longs)} of them <= 30 s, on the one-window path): {dt:.2f} s wall")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--tiny"]
    main(args[0] if args else "", "--tiny" in sys.argv)
