"""HIP-event time of each step of engine.FusionHead at 16 x 10 s and 1 x 10 s (499 speech rows, 80 text rows per utterance), next to the
algorithmic FLOPs and bytes of the step; ser_gru_v's time per recurrence step for R = 1 and the chosen R; and the same batch through the
torch / MIOpen head (head.MultiModalEmotionClassifier) on the same GPU, alternated in the same call -- as the reference's evaluation runs
it (a batch of one per utterance) and as head.evaluate's torch path runs it (one padded batch).

With ``trimodal`` as the fourth argument: engine.TrimodalHead at 16 x (499 speech, 80 text, 800 third-stream) rows, H = 512, per step,
alternated with the bimodal head on the same first two streams and with head.TrimodalEmotionClassifier looped at batch_size=1.

    python tools/fusion_head_bench.py [mode, default f16x] [repetitions, default 50] [output file] [bimodal (default) | trimodal | all]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from interspeech_ser_amd.engine import _PLANES, FusionHead, TrimodalHead    # noqa: E402
from interspeech_ser_amd.head import MultiModalEmotionClassifier, TrimodalEmotionClassifier      # noqa: E402
from oracle.fusion_head import seeded_head_weights                           # noqa: E402
import fusion_ref as R                                                        # noqa: E402
import fusion3_ref as R3                                                      # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "f16x"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else ""
which = sys.argv[4] if len(sys.argv) > 4 else "bimodal"
DEV, T1, T2, h = "cuda:0", 499, 80, 512
E = 2 * h
lines = [] if which == "trimodal" else [f"FusionHead, mode {mode}; {reps} repetitions after 5 warm-up, HIP events around each step on one stream; T1 = {T1}, T2 = {T2}"]


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for d1, d2 in ((1280, 1024), (1024, 1024)) if which != "trimodal" else ():
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
def trimodal():
    """16 x (499, 80, 800) rows at the reference's trimodal widths (1280, 1024, 512), H = 512"""
    dims, Ts, B = (1280, 1024, 512), (T1, T2, 800), 16
    names = R3.NAMES
    sd = seeded_head_weights(R3.head_shapes(*dims), 31)
    sd2 = {k: v for k, v in seeded_head_weights(R.head_shapes(dims[0], dims[1]), 31).items()}
    tri, bi = TrimodalHead(sd, *dims, DEV, mode), FusionHead(sd2, dims[0], dims[1], DEV, mode)
    planes = _PLANES[tri.op_mode]
    tm = TrimodalEmotionClassifier(*dims).to(DEV).eval()
    tm.load_state_dict(sd)
    rng = np.random.default_rng(0)
    xs = [torch.from_numpy(rng.standard_normal((B * T, d)).astype(np.float32)).to(DEV) for T, d in zip(Ts, dims)]
    offs = [[b * T for b in range(B + 1)] for T in Ts]
    Ms = [B * T for T in Ts]
    args3 = (xs[0], offs[0], xs[1], offs[1], xs[2], offs[2])
    args2 = args3[:4]
    lines.append(f"TrimodalHead, mode {mode}, heads {tri.heads}; {reps} repetitions after 5 warm-up, HIP events around each step on one stream")
    lines.append(f"-- dims {dims}, {B} x ({Ts[0]}, {Ts[1]}, {Ts[2]}) rows = {tuple(Ms)}, H = {h}, R = {tri.R}")
    for _ in range(5):
        tri.forward(*args3)
        bi.forward(*args2)
    assert tri.status() == (0, 0) and bi.status() == (0, 0)
    tri.trace = []
    for _ in range(reps):
        tri.forward(*args3)
    torch.cuda.synchronize()
    per = {}
    for name, a, b in tri.trace:
        per.setdefault(name, []).append(a.elapsed_time(b) * 1e3)
    tri.trace = None
    side_of = {n: i for i, n in enumerate(names)}
    total, by_kind = 0.0, {}
    for name, ts in per.items():
        t = np.array(ts)
        med = float(np.median(t))
        total += med
        parts = name.split(" ")
        i = side_of.get(parts[0], 0)
        step = parts[1] if len(parts) > 1 else name
        M, D, T = Ms[i], dims[i], Ts[i]
        fl, nb = 0.0, 0.0
        if step == "pack":
            nb = 4 * M * D + 2 * planes * M * D
        elif step == "projection":
            fl, nb = 2 * M * D * h, 2 * planes * (M * D + D * h) + 4 * M * h
        elif step == "layernorm":
            nb = 4 * M * h + 2 * planes * M * h
        elif step == "gx":
            fl, nb = 2 * M * h * 6 * h, 2 * planes * (M * h + 6 * h * h) + 4 * M * 6 * h
        elif step == "gru":
            fl, nb = 2 * M * 2 * 3 * h * h, 4 * M * 6 * h + 4 * 6 * h * h + 4 * M * E + 2 * planes * M * E
        elif step == "q":
            fl, nb = 2 * M * E * E, 2 * planes * (M * E + E * E) + 4 * M * E
        elif step == "kv":
            fl, nb = 2 * M * E * 4 * E, 2 * planes * (M * E + 4 * E * E) + 16 * M * E
        elif step == "xattn":
            j = side_of[parts[2]]
            fl, nb = 4 * B * T * Ts[j] * E, 4 * M * E + 8 * Ms[j] * E + 2 * planes * M * E
        elif step == "out_proj":
            fl, nb = 2 * M * E * E, 2 * planes * (M * E + E * E) + 4 * M * E * (2 if parts[2] == [n for n in names if n != parts[0]][1] else 1)
        elif step == "attn_pool":
            nb = 2 * 8 * M * E + 4 * B * E
        else:
            nb = 4 * B * (6 * E + 2 * h) + 4 * (6 * E * h + 8 * h)
        by_kind[step] = by_kind.get(step, 0.0) + med
        extra = f"  = {med / T:6.2f} us per recurrence step" if step == "gru" else ""
        lines.append(f"   {name:26s} median {med:9.1f} us (min {t.min():9.1f})  {fl / 1e9:8.3f} GFLOP  {nb / 1e6:8.2f} MB algorithmic{extra}")
    whole = timed(lambda: tri.forward(*args3), reps)
    lines.append(f"   sum of medians {total:.1f} us; the whole head back to back without events: {whole:.1f} us")
    lines.append("   share of the sum by kind of step: " + ", ".join(f"{k} {100.0 * v / total:.1f} %" for k, v in sorted(by_kind.items(), key=lambda kv: -kv[1])))
    p = [x.view(B, T, d) for x, T, d in zip(xs, Ts, dims)]
    n = max(3, reps // 5)
    with torch.no_grad():
        for _ in range(2):
            for b in range(B):
                tm(p[0][b:b + 1], p[1][b:b + 1], p[2][b:b + 1])
        for i in range(3):                                 # alternated: the torch module as 16 batches of one, the bimodal head, the trimodal head
            a = timed(lambda: [tm(p[0][b:b + 1], p[1][b:b + 1], p[2][b:b + 1]) for b in range(B)], n)
            c = timed(lambda: bi.forward(*args2), n)
            d = timed(lambda: tri.forward(*args3), n)
            lines.append(f"   round {i}: torch / MIOpen trimodal module as {B} batches of one: {a:9.1f} us; FusionHead on the first two streams: {c:9.1f} us; "
                         f"TrimodalHead: {d:9.1f} us")
    assert tri.status() == (0, 0) and bi.status() == (0, 0)


if which in ("trimodal", "all"):
    trimodal()
text = "\n".join(lines)
print(text)
if out_path:
    with open(out_path, "a") as f:
        f.write(text + "\n")
