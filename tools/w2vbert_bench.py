"""HIP-event time of one w2v-BERT 2.0 forward at full geometry (24 conformer layers, D = 1024, 16 heads of 64; seeded weights) over
16 x 10 s, in the bf16 and f16x modes: the replayed command list, and the same launches replayed by class -- GEMMs, relative-key table +
attention, the convolution-module kernel, the swish rows, the fbank front end, the LayerNorms -- each class alone on one stream (the
classes do not add up exactly to the forward: a class replayed alone re-reads what the others would have left in L2).  Not a gate:
nothing existed to compare with.  The swish rows' time is what the fp32 round trip of FC1's output costs (no fused epilogue).

    python tools/w2vbert_bench.py [repetitions, default 20] [output file]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interspeech_ser_amd import _lib                                          # noqa: E402
from interspeech_ser_amd import config as C                                   # noqa: E402
from interspeech_ser_amd.engine import W2vBertEncoder, _stream                # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
out_path = sys.argv[2] if len(sys.argv) > 2 else ""
DEV, B, N = "cuda:0", 16, 160000
CLASSES = (("GEMMs", (_lib.OP_GEMM,)), ("relative-key table + attention", (_lib.OP_RELKEY_TABLE, _lib.OP_ATTENTION_RK)),
           ("  of which the table", (_lib.OP_RELKEY_TABLE,)), ("conv-module kernel", (_lib.OP_CONFORMER_CONV,)),
           ("swish rows", (_lib.OP_SWISH_ROWS,)), ("fbank", (_lib.OP_FBANK,)), ("LayerNorms", (_lib.OP_LAYERNORM,)))


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                                           # ms


geo = C.W2V_BERT_2
rng = np.random.default_rng(5)
waves = [(0.3 * np.sin(np.arange(N) * (0.03 + 0.01 * b)) + 0.05 * rng.standard_normal(N)).astype(np.float32) for b in range(B)]
lengths = [N] * B
M = B * geo.frames_for(N)
sd = synthetic_state_dict(geo, 11, fast=True)
gemm_flop = geo.num_layers * 2.0 * M * (4 * geo.hidden * geo.ffn + 4 * geo.hidden ** 2 + 3 * geo.hidden ** 2)
lines = [f"w2v-BERT 2.0, {B} x {N / 16000:.0f} s = {M} rows, D = {geo.hidden}, {geo.num_layers} layers, K = {geo.conv_depthwise_kernel}, "
         f"clamp -{geo.left_max_positions} .. {geo.right_max_positions}; {reps} repetitions after 3 warm-up, HIP events on one stream; "
         f"{gemm_flop / 1e12:.2f} algorithmic TFLOP in the layers' GEMMs; FC1's fp32 output is {M * geo.ffn * 4 / 1e6:.0f} MB per feed-forward block"]
for mode in ("bf16", "f16x"):
    enc = W2vBertEncoder(geo, sd, DEV, mode)
    packed = enc.upload(waves)
    for _ in range(3):
        hs = enc.forward(packed, lengths)
    bits = hs.take_range_bits()
    t_fwd = timed(lambda: enc.forward(packed, lengths), reps)
    lines.append(f"  mode {mode:5s}: forward (replayed command list, {enc.recorded_tape(lengths, 0).n} launches) {t_fwd:8.2f} ms = "
                 f"{B / t_fwd * 1e3:7.0f} utt/s, {gemm_flop / t_fwd / 1e9:6.1f} TFLOP/s over the GEMMs' FLOPs; range bits {bits}")
    tape = enc.recorded_tape(lengths, 0)
    st = _stream()
    for name, ops in CLASSES:
        sub = tape.subset(lambda op, ops=ops: op in ops)
        t = timed(lambda: sub.run({}, st), reps)
        lines.append(f"      {name:32s} {sub.n:4d} launches {t:8.3f} ms  ({100.0 * t / t_fwd:5.1f} % of the forward)")
    del enc
    torch.cuda.empty_cache()
text = "\n".join(lines)
print(text)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
