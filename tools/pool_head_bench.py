"""HIP-event time of each step of engine.PoolHead behind a WavLM-large forward, at 16 x 10 s and 1 x 10 s, next to the
algorithmic bytes of the step (every operand / result element once) and to the forward itself.

    python tools/pool_head_bench.py [mode, default bf16] [repetitions, default 200] [output file]

Steps: pack = ser_pack_rows_flagged (operand copy of the last state), gemm = ser_gemm with sap_linear, asp_pool = ser_asp_pool_v
(two kernels: scores, weighted moments), mlp_head = ser_mlp_head_v (two kernels: hidden units, LayerNorm / ReLU / outputs).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import config as C                                   # noqa: E402
from interspeech_ser_amd.baseline import synthetic_head_state_dicts          # noqa: E402
from interspeech_ser_amd.engine import _PLANES, PoolHead, SpeechEncoder      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                 # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
out_path = sys.argv[3] if len(sys.argv) > 3 else ""
FWD_WARM = 10
fwd_reps = max(10, reps // 4)             # the forward every percentage is relative to: warmed, and timed over a comparable span
geo = C.WAVLM_LARGE
D, H, n_out = geo.hidden, 1024, 8
enc = SpeechEncoder(geo, synthetic_state_dict(geo, 3, fast=True), "cuda:0", mode=mode, normalize=False)
head = PoolHead(enc, *synthetic_head_state_dicts(D, H, n_out, seed=3))
planes = _PLANES[head.op_mode]
rng = np.random.default_rng(0)
lines = [f"PoolHead behind WavLM-large, mode {mode} (head GEMM operands: {planes} plane(s)), head_dim {H}, n_out {n_out}; "
         f"{reps} repetitions after 20 warm-up, HIP events around each step on one stream"]
for B in (16, 1):
    waves = [rng.standard_normal(160000).astype(np.float32) for _ in range(B)]
    lengths = [len(w) for w in waves]
    dev = enc.upload(waves)
    hs = enc.forward(dev, lengths)
    M = hs.frame_offs[-1]
    for _ in range(20):
        head.forward(hs)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(FWD_WARM):
        hs = enc.forward(dev, lengths)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(fwd_reps):
        hs = enc.forward(dev, lengths)
    e1.record()
    torch.cuda.synchronize()
    fwd_ms = e0.elapsed_time(e1) / fwd_reps
    head.trace = []
    for _ in range(reps):
        head.forward(hs)
    torch.cuda.synchronize()
    per = {}
    for name, a, b in head.trace:
        per.setdefault(name, []).append(a.elapsed_time(b) * 1e3)
    head.trace = None
    e0.record()
    for _ in range(reps):
        head.forward(hs)
    e1.record()
    torch.cuda.synchronize()
    whole_us = e0.elapsed_time(e1) * 1e3 / reps
    nbytes = {"pack": 4 * M * D + 2 * planes * M * D,
              "gemm": 2 * planes * (M * D + D * D) + 4 * D + 4 * M * D,
              "asp_pool": (4 * M * D + 4 * D + 4 * M) + (4 * M * D + 4 * M * (D // 64) + 8 * B * D),
              "mlp_head": 4 * (2 * D * H + 2 * D * B + 3 * H + 2 * B * H + n_out * H + n_out + B * n_out)}
    lines.append(f"-- {B} x 10 s ({M} rows): forward alone {fwd_ms * 1e3:.0f} us (mean of {fwd_reps} after {FWD_WARM} warm-up; stream launches, one batch in flight)")
    total = 0.0
    for name in ("pack", "gemm", "asp_pool", "mlp_head"):
        t = np.array(per[name])
        med = float(np.median(t))
        total += med
        lines.append(f"   {name:9s} median {med:8.1f} us  (min {t.min():8.1f}, p90 {np.percentile(t, 90):8.1f})   {nbytes[name] / 1e6:8.2f} MB "
                     f"algorithmic -> {nbytes[name] / med / 1e3:7.1f} GB/s")
    lines.append(f"   sum of medians {total:.1f} us = {100 * total / (fwd_ms * 1e3):.2f} % of the forward; the five steps back to back without "
                 f"events: {whole_us:.1f} us per head = {100 * whole_us / (fwd_ms * 1e3):.2f} %")
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a") as f:
        f.write(text + "\n")
