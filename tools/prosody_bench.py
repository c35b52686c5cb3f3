"""HIP-event time of the prosody stream at 16 x 10 s (16 x 160 000 samples, 12 816 frames) on the reference's geometry (D = 256, 4 layers,
1024 codes; seeded weights): the mel launch alone (ser_prosody_mel_v with melspec_linear), the whole forward (replayed command list) in
each numerics mode, and -- beside them -- the reference-style CPU rate: tests/prosody_ref.py's fp32 torch twin, one utterance at a time,
as preprocess_ns3_prosody.py runs (device = 'cpu' there).  Not a gate: nobody had timed this path.

    python tools/prosody_bench.py [repetitions, default 50] [output file]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from interspeech_ser_amd import prosody as P                                  # noqa: E402
from interspeech_ser_amd.engine import ProsodyEncoder                         # noqa: E402
import prosody_ref as R                                                       # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
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


def flops(spec, T_list):
    """algorithmic FLOPs of one batch: DFT of the kept bins, the GEMMs and attention of the layers, the code search"""
    M = sum(T_list)
    D, F, k = spec.hidden, spec.ffn, spec.kernel
    per_layer = 2.0 * M * D * (3 * D) + 2.0 * M * D * D + 2.0 * M * (k * D) * F + 2.0 * M * F * D + sum(4.0 * T * T * D for T in T_list)
    return 2.0 * M * 800 * 52 * 2 + 2.0 * M * 20 * D + spec.num_layers * per_layer + 2.0 * M * (8 * D + 8 * spec.n_codes)


rng = np.random.default_rng(5)
waves = [(0.3 * np.sin(np.arange(N) * (0.03 + 0.01 * b)) + 0.05 * rng.standard_normal(N)).astype(np.float32) for b in range(B)]
sd = P.synthetic_state_dict(seed=11)
spec = P.ProsodySpec()
T_list = [n // 200 + 1 for n in [N] * B]
lines = [f"Prosody stream, {B} x {N / 16000:.0f} s = {sum(T_list)} frames, D = {spec.hidden}, {spec.num_layers} layers, {spec.n_codes} codes; "
         f"{reps} repetitions after 5 warm-up, HIP events on one stream; {flops(spec, T_list) / 1e12:.3f} algorithmic TFLOP per batch"]
for mode in ("f16x", "fp32x", "bf16"):
    enc = ProsodyEncoder(sd, DEV, mode)
    packed = enc.upload(waves)
    lengths = [len(w) for w in waves]
    pl = enc._plan(lengths, 0)
    for _ in range(5):
        out = enc.forward(packed, lengths)
        enc._mel(pl, packed)
    assert out.take_range_bits() == 0
    t_fwd = timed(lambda: enc.forward(packed, lengths), reps)
    t_mel = timed(lambda: enc._mel(pl, packed), reps)
    enc.use_tape = False
    t_eager = timed(lambda: enc.forward(packed, lengths), max(5, reps // 5))
    lines.append(f"  mode {mode:5s}: forward (replayed command list) {t_fwd:8.1f} us = {B * 1e6 / t_fwd:8.0f} utt/s, "
                 f"{flops(spec, T_list) / t_fwd / 1e6:6.1f} TFLOP/s algorithmic;  launched one by one {t_eager:8.1f} us;  "
                 f"mel launch alone {t_mel:7.1f} us")
    del enc
torch.set_num_threads(16)
R.torch_twin(sd, waves[0], 4)                                                # warm-up
t0 = time.perf_counter()
n_cpu = 4
for w in waves[:n_cpu]:
    R.torch_twin(sd, w, 4)
dt = (time.perf_counter() - t0) / n_cpu
lines.append(f"  reference-style CPU path (fp32 torch, batch of one, {torch.get_num_threads()} threads): {dt * 1e3:.1f} ms per 10 s utterance = "
             f"{1.0 / dt:.1f} utt/s  ({B * dt * 1e3:.0f} ms per {B})")
text = "\n".join(lines)
print(text)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
