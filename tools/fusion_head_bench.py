"""HIP-event time of each step of engine.FusionHead at 16 x 10 s and 1 x 10 s (499 speech rows, 80 text rows per utterance), next to the
algorithmic FLOPs and bytes of the step; ser_gru_v's time per recurrence step for R = 1 and the chosen R; and the same batch through the
torch / MIOpen head (head.MultiModalEmotionClassifier) on the same GPU, alternated in the same call -- as the reference's evaluation runs
it (a batch of one per utterance) and as head.evaluate's torch path runs it (one padded batch).

    python tools/fusion_head_bench.py [mode, default f16x] [repetitions, default 50] [output file]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from interspeech_ser_amd.engine import _PLANES, FusionHead                  # noqa: E402
from interspeech_ser_amd.head import MultiModalEmotionClassifier             # noqa: E402
from oracle.fusion_head import seeded_head_weights                           # noqa: E402
import fusion_ref as R                                                        # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "f16x"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else ""
DEV, T1, T2, h = "cuda:0", 499, 80, 512
E = 2 * h
lines = [f"FusionHead, mode {mode}; {reps} repetitions after 5 warm-up, HIP events around each step on one stream; T1 = {T1}, T2 = {T2}"]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for d1, d2 in ((1280, 1024), (1024, 1024)):
    sd = seeded_head_weights(R.head_shapes(d1, d2), 31)
    heads = {"chosen R": FusionHead(sd, d1, d2, DEV, mode), "R = 1": FusionHead(sd, d1, d2, DEV, mode, cluster=1)}
    planes = _PLANES[heads["chosen R"].op_mode]
    tm = MultiModalEmotionClassifier(d1, d2).to(DEV).eval()
    tm.load_state_dict(sd)
    rng = np.random.default_rng(0)
    for B in (16, 1):
        x1 = torch.from_numpy(rng.standard_normal((B * T1, d1)).astype(np.float32)).to(DEV)
        x2 = torch.from_numpy(rng.standard_normal((B * T2, d2)).astype(np.float32)).to(DEV)
        o1, o2 = [b * T1 for b in range(B + 1)], [b * T2 for b in range(B + 1)]
        M1, M2 = B * T1, B * T2
        lines.append(f"-- D1 = {d1}, D2 = {d2}, {B} x 10 s ({M1} speech rows, {M2} text rows)")
        for tag, head in heads.items():
            for _ in range(5):
                head.forward(x1, o1, x2, o2)
            assert head.status() == (0, 0)
            head.trace = []
            for _ in range(reps):
                head.forward(x1, o1, x2, o2)
            torch.cuda.synchronize()
            per = {}
            for name, a, b in head.trace:
                per.setdefault(name, []).append(a.elapsed_time(b) * 1e3)
            head.trace = None
            whole = timed(lambda: head.forward(x1, o1, x2, o2), reps)
            assert head.status() == (0, 0)
            if tag == "chosen R":
                flops = {"projection": lambda M, D: 2 * M * D * h, "gx": lambda M, D: 2 * M * h * 6 * h,
                         "gru": lambda M, D: 2 * M * 2 * 3 * h * h, "q": lambda M, D: 2 * M * E * E, "kv": lambda M, D: 2 * M * E * 2 * E,
                         "xattn": lambda M, D: 4 * B * T1 * T2 * E, "out_proj": lambda M, D: 2 * M * E * E}
                nbytes = {"pack": lambda M, D: 4 * M * D + 2 * planes * M * D, "projection": lambda M, D: 2 * planes * (M * D + D * h) + 4 * M * h,
                          "layernorm": lambda M, D: 4 * M * h + 2 * planes * M * h, "gx": lambda M, D: 2 * planes * (M * h + 6 * h * h) + 4 * M * 6 * h,
                          "gru": lambda M, D: 4 * M * 6 * h + 4 * 6 * h * h + 4 * M * E + 2 * planes * M * E,
                          "q": lambda M, D: 2 * planes * (M * E + E * E) + 4 * M * E, "kv": lambda M, D: 2 * planes * (M * E + 2 * E * E) + 8 * M * E,
                          "xattn": lambda M, D: 4 * M * E + 8 * (M1 + M2 - M) * E + 2 * planes * M * E,
                          "out_proj": lambda M, D: 2 * planes * (M * E + E * E) + 4 * M * E, "attn_pool": lambda M, D: 2 * 8 * M * E + 4 * B * E}
                total = 0.0
                for name in per:
                    t = np.array(per[name])
                    med = float(np.median(t))
                    total += med
                    side, step = (name.split(" ", 1) + [""])[:2] if " " in name else ("", name)
                    M, D = (M1, d1) if side == "speech" else (M2, d2)
                    if step == "kv":                       # the k | v projection reads the OTHER side's rows
                        M = M2 if side == "speech" else M1
                    fl = flops.get(step, lambda M, D: 0)(M, D)
                    nb = nbytes.get(step, lambda M, D: 4 * B * (4 * E + 2 * h) + 4 * (4 * E * h + 8 * h))(M, D)
                    extra = f"  = {med / (T1 if side == 'speech' else T2):6.2f} us per recurrence step" if step == "gru" else ""
                    lines.append(f"   {name:18s} median {med:8.1f} us (min {t.min():8.1f})  {fl / 1e9:7.3f} GFLOP  {nb / 1e6:7.2f} MB algorithmic{extra}")
                lines.append(f"   sum of medians {total:.1f} us; the whole head back to back without events: {whole:.1f} us (R = {head.R})")
            else:
                for name in ("speech gru", "text gru"):
                    med = float(np.median(per[name]))
                    lines.append(f"   {name} with R = 1 (block-local, weights streamed from L2): median {med:8.1f} us = "
                                 f"{med / (T1 if name[0] == 's' else T2):6.2f} us per recurrence step; whole head {whole:.1f} us")
        p1, p2 = x1.view(B, T1, d1), x2.view(B, T2, d2)
        with torch.no_grad():
            for _ in range(3):
                tm(p1, p2)
                for b in range(B):
                    tm(p1[b:b + 1], p2[b:b + 1])
            rounds = []
            for _ in range(3):                             # alternated: padded batch, batch-of-one loop, the kernels
                rounds.append((timed(lambda: tm(p1, p2), max(3, reps // 5)),
                               timed(lambda: [tm(p1[b:b + 1], p2[b:b + 1]) for b in range(B)], max(3, reps // 5)),
                               timed(lambda: heads["chosen R"].forward(x1, o1, x2, o2), max(3, reps // 5))))
        for i, (a, b, c) in enumerate(rounds):
            lines.append(f"   round {i}: torch / MIOpen head, one padded batch of {B}: {a:9.1f} us; as {B} batches of one: {b:9.1f} us; FusionHead: {c:9.1f} us")
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a") as f:
        f.write(text + "\n")
