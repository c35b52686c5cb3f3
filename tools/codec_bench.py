"""HIP-event time of the 512-wide third stream (prosody rows | timbre rows) at 16 x 10 s on the reference's geometry (ngf 32, strides
2 / 4 / 5 / 5, 256 channels out, timbre encoder D = 256; seeded weights): one forward (replayed command list) in each numerics mode, its
split by level -- the recorded commands of each part replayed on their own --, the algorithmic FLOPs and HBM bytes of each level, the
plain prosody stream's forward beside it, and the reference-style CPU figure: tests/codec_ref.py's fp32 torch twin on one clip, as
preprocess_ns3_prosody_speaker.py runs (device = 'cpu' there).  Not a gate: nobody had timed this path.

    python tools/codec_bench.py [repetitions, default 20] [output file]
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from interspeech_ser_amd import _lib, prosody as P                            # noqa: E402
from interspeech_ser_amd.engine import ProsodyEncoder, SpeakerProsodyEncoder, Tape   # noqa: E402
import codec_ref as R                                                         # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else ""
DEV, B, N = "cuda:0", 16, 160000


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def part_tape(tape, lo, hi):
    t = Tape(max(1, hi - lo))
    C.memmove(C.byref(t.cmds[0]), C.byref(tape.cmds[lo]), (hi - lo) * C.sizeof(_lib.Cmd))
    t.n = hi - lo
    return t


def level_work(spec, lens):
    """(name, algorithmic FLOPs, algorithmic HBM bytes) per part: every tensor that must exist between two levels counted once per use --
    a unit reads x and writes y, a down-convolution reads its level and writes the next; an activation is 12 + 12 FMAs and a sine per element"""
    M = [sum(l[i] for l in lens) for i in range(len(spec.channels))]
    out = [("conv_in", 2.0 * M[0] * 7 * spec.ngf, 4.0 * (sum(N for _ in lens) + M[0] * spec.ngf))]
    for i, s in enumerate(spec.strides):
        Cc = spec.channels[i]
        act = 50.0 * M[i] * Cc
        fl = 3 * (2.0 * M[i] * 7 * Cc * Cc + 2.0 * M[i] * Cc * Cc + 2 * act) + act + 2.0 * M[i + 1] * (2 * s * Cc) * (2 * Cc)
        by = 3 * (2 * 4.0 * M[i] * Cc) + 4.0 * M[i] * Cc + 4.0 * M[i + 1] * 2 * Cc
        out.append((f"level_{i + 1}", fl, by))
    Cl, D, ts = spec.channels[-1], spec.out_channels, spec.timbre
    Mf = M[-1]
    per_layer = 2.0 * Mf * D * 3 * D + 2.0 * Mf * D * D + 2.0 * Mf * ts.kernel * D * ts.ffn + 2.0 * Mf * ts.ffn * D + sum(4.0 * l[-1] ** 2 * D for l in lens)
    out.append(("final + timbre", 50.0 * Mf * Cl + 2.0 * Mf * 3 * Cl * D + ts.num_layers * per_layer, 4.0 * Mf * (Cl + 2 * D)))
    return out


rng = np.random.default_rng(5)
waves = [(0.3 * np.sin(np.arange(N) * (0.03 + 0.01 * b)) + 0.05 * rng.standard_normal(N)).astype(np.float32) for b in range(B)]
dec = P.synthetic_state_dict(seed=11)
dec.update(P.synthetic_timbre_state_dict(seed=13))
enc_sd = P.synthetic_codec_state_dict()
spec = P.CodecSpec()
lengths = [N] * B
lens = [spec.level_lengths(n) for n in lengths]
work = level_work(spec, lens)
lines = [f"Prosody + speaker stream, {B} x {N / 16000:.0f} s = {sum(l[-1] for l in lens)} frames, ngf {spec.ngf}, strides {spec.strides}; {reps} repetitions "
         f"after 3 warm-up, HIP events on one stream; {sum(w[1] for w in work) / 1e12:.3f} algorithmic TFLOP per batch in the speaker half"]
for mode in ("f16x", "fp32x", "bf16"):
    enc = SpeakerProsodyEncoder(dec, enc_sd, DEV, mode)
    packed = enc.upload(waves)
    for _ in range(3):
        out = enc.forward(packed, lengths)
    assert out.take_range_bits() == 0
    t_fwd = timed(lambda: enc.forward(packed, lengths), reps)
    tape = enc.recorded_tape(lengths, 0)
    st = torch.cuda.current_stream().cuda_stream
    marks = [("start", 0)] + list(tape.parts) + [("final + timbre", tape.n)]
    lines.append(f"  mode {mode:5s}: forward (replayed command list, {tape.n} commands) {t_fwd:9.1f} us = {B * 1e6 / t_fwd:7.0f} utt/s")
    t_parts = {}
    for (_, lo), (name, hi) in zip(marks[:-1], marks[1:]):
        sub = part_tape(tape, lo, hi)
        t_parts[name] = timed(lambda: _lib.check(_lib.lib.ser_run(sub.cmds, sub.n, None, st), "ser_run"), reps)
    lines.append(f"      prosody half {t_parts['prosody']:9.1f} us ({100 * t_parts['prosody'] / t_fwd:4.1f} %)")
    for name, fl, by in work:
        t = t_parts[name]
        lines.append(f"      {name:15s} {t:9.1f} us ({100 * t / t_fwd:4.1f} %)  {fl / 1e9:7.2f} GFLOP {by / 1e6:8.1f} MB algorithmic = "
                     f"{fl / t / 1e6:6.2f} TFLOP/s, {by / t / 1e3:7.1f} GB/s")
    del enc
    plain = ProsodyEncoder(dec, DEV, mode)
    for _ in range(3):
        plain.forward(packed, lengths)
    lines.append(f"      the plain prosody stream alone (engine.ProsodyEncoder) {timed(lambda: plain.forward(packed, lengths), reps):9.1f} us")
    del plain
torch.set_num_threads(16)
R.torch_twin(enc_sd, waves[0][:16000])                                       # warm-up on one second
t0 = time.perf_counter()
R.torch_twin(enc_sd, waves[0])
dt = time.perf_counter() - t0
lines.append(f"  reference-style CPU path of the codec alone (fp32 torch, batch of one, {torch.get_num_threads()} threads): {dt * 1e3:.0f} ms per 10 s "
             f"utterance = {1.0 / dt:.2f} utt/s  ({B * dt:.1f} s per {B})")
text = "\n".join(lines)
print(text)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
