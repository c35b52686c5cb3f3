"""HIP-event time of one wav2vec2-conformer forward at the large geometry (24 conformer layers, D = 1024, 16 heads of 64, ffn 4096; seeded
weights) over 16 x 10 s, for both position types in the f16x, fp32x and bf16 modes: the replayed command list, and the same launches
replayed by class on one stream (the classes do not add up exactly to the forward: a class replayed alone re-reads what the others would
have left in L2).  For the relative type the positional term is shown in its three parts -- the P GEMMs, ser_relpos_bias_v and the
attention that reads the bias -- with the bytes of the bias buffer.  Not a gate.

    python tools/w2v_conformer_bench.py [repetitions, default 20] [output file]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interspeech_ser_amd import _lib                                          # noqa: E402
from interspeech_ser_amd import config as C                                   # noqa: E402
from interspeech_ser_amd.engine import ConformerSpeechEncoder, _stream        # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                  # noqa: E402

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
    return e0.elapsed_time(e1) / n                                           # ms


rng = np.random.default_rng(5)
waves = [(0.3 * np.sin(np.arange(N) * (0.03 + 0.01 * b)) + 0.05 * rng.standard_normal(N)).astype(np.float32) for b in range(B)]
lengths = [N] * B
lines = []
for geo in (C.W2V_CONFORMER_ROPE_LARGE, C.W2V_CONFORMER_REL_LARGE):
    T = geo.frames_for(N)
    M = B * T
    sd = synthetic_state_dict(geo, 11, fast=True)
    rel = geo.position_type == "relative"
    gemm_flop = geo.num_layers * 2.0 * M * (4 * geo.hidden * geo.ffn + 4 * geo.hidden ** 2 + 3 * geo.hidden ** 2)
    lines.append(f"wav2vec2-conformer large, {geo.position_type} positions, {B} x {N / 16000:.0f} s = {M} rows ({T} per utterance), D = {geo.hidden}, "
                 f"{geo.num_layers} layers, K = {geo.conv_depthwise_kernel}; {reps} repetitions after 3 warm-up, HIP events on one stream; "
                 f"{gemm_flop / 1e12:.2f} algorithmic TFLOP in the layers' GEMMs (without the stem and the P GEMMs)")
    for mode in ("f16x", "fp32x", "bf16"):
        enc = ConformerSpeechEncoder(geo, sd, DEV, mode)
        packed = enc.upload(waves)
        for _ in range(3):
            hs = enc.forward(packed, lengths)
        bits = hs.take_range_bits()
        t_fwd = timed(lambda: enc.forward(packed, lengths), reps)
        tape = enc.recorded_tape(lengths, 0)
        lines.append(f"  mode {mode:5s}: forward (replayed command list, {tape.n} launches) {t_fwd:8.2f} ms per batch = "
                     f"{B / t_fwd * 1e3:7.0f} utt/s, {gemm_flop / t_fwd / 1e9:6.1f} TFLOP/s over the layers' GEMM FLOPs; range bits {bits}")
        st = _stream()
        pos_w = {lay["pos"].w.data_ptr() for lay in enc.layers} if rel else set()
        stem_w = {enc.conv0.w.data_ptr(), enc.proj.w.data_ptr()} | {c.w.data_ptr() for c in enc.convs}
        is_gemm = lambda c: c.op == _lib.OP_GEMM                                                   # noqa: E731
        classes = [("conv stem + projection GEMMs", lambda c: is_gemm(c) and c.u.gemm.W in stem_w),
                   ("layer GEMMs", lambda c: is_gemm(c) and c.u.gemm.W not in stem_w and c.u.gemm.W not in pos_w)]
        if rel:
            pl = enc._plan(lengths, 0)
            pb_bytes = M * geo.heads * pl["ld_pb"] * 4
            classes += [(f"P GEMMs ({2 * pl['P_T']} rows of P per layer)", lambda c: is_gemm(c) and c.u.gemm.W in pos_w),
                        (f"ser_relpos_bias_v (pb {pb_bytes / 1e6:.0f} MB, written once per layer)", lambda c: c.op == _lib.OP_RELPOS_BIAS),
                        ("ser_attention_rb_v (reads pb once per layer)", lambda c: c.op == _lib.OP_ATTENTION_RB)]
        else:
            classes += [("ser_rope_rows_v", lambda c: c.op == _lib.OP_ROPE_ROWS), ("ser_attention_v", lambda c: c.op == _lib.OP_ATTENTION)]
        classes += [("conv-module kernel (BatchNorm form)", lambda c: c.op == _lib.OP_CONFORMER_CONV_BN),
                    ("swish rows", lambda c: c.op == _lib.OP_SWISH_ROWS), ("LayerNorms", lambda c: c.op == _lib.OP_LAYERNORM),
                    ("wave frames", lambda c: c.op == _lib.OP_WAVE_FRAMES)]
        for name, keep in classes:
            sub = tape.subset(keep, by_cmd=True)
            t = timed(lambda: sub.run({}, st), reps)
            lines.append(f"      {name:64s} {sub.n:4d} launches {t:8.3f} ms  ({100.0 * t / t_fwd:5.1f} % of the forward)")
        del enc
        torch.cuda.empty_cache()
    del sd
text = "\n".join(lines)
print(text)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
