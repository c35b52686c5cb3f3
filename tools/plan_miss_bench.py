"""Host time of a plan MISS: per waveform encoder, two length lists of 16 utterances (1 .. 3 s) alternate, so every ``_plan`` lays its O(B)
tables out anew (arena.TableBlob: begin, puts, one copy) and rebuilds the O(rows) tables with ser_ragged_index.  Tiny geometries and
seeded weights: what is timed is the host side, which does not depend on the model's width.  Per encoder: the wall time per ``_plan``
over a run of plans with one device synchronisation at the end, and the same for plan + forward.  The other tools replay one plan.

    python tools/plan_miss_bench.py [plans, default 300] [output file]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from interspeech_ser_amd import config as C, prosody as P                     # noqa: E402
from interspeech_ser_amd.engine import ProsodyEncoder, SpeakerProsodyEncoder, build_encoder      # noqa: E402
from interspeech_ser_amd.weights import synthetic_state_dict                  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
out_path = sys.argv[2] if len(sys.argv) > 2 else ""
DEV, B = "cuda:0", 16
rng = np.random.default_rng(3)
LISTS = [[int(n) for n in rng.integers(16000, 48001, B)] for _ in range(2)]


def tiny(name):
    geo = getattr(C, name)
    return lambda: build_encoder(geo, synthetic_state_dict(geo, 5), DEV, "f16x")


def codec():
    dec = P.synthetic_state_dict(seed=11)
    dec.update(P.synthetic_timbre_state_dict(seed=13))
    return SpeakerProsodyEncoder(dec, P.synthetic_codec_state_dict(), DEV, "f16x")


def per_call(fn, n):
    """(us per call with the final synchronisation, us per call until the last call returned)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n, (t1 - t0) * 1e6 / n


HOSTS = (("SpeechEncoder (tiny WavLM)", tiny("TINY_WAVLM"), True), ("WhisperEncoder (tiny)", tiny("TINY_WHISPER"), True),
         ("ProsodyEncoder", lambda: ProsodyEncoder(P.synthetic_state_dict(seed=11), DEV, "f16x"), False),
         ("SpeakerProsodyEncoder", codec, False), ("W2vBertEncoder (tiny)", tiny("TINY_W2V_BERT"), True))
lines = [f"plan miss: two lists of {B} utterances of 1 .. 3 s alternate; {reps} plans and {max(reps // 4, 20)} plan + forward pairs per encoder "
         f"after 4 warm-up pairs; wall time per call, one device synchronisation at the end of each run"]
for name, build, positional in HOSTS:
    enc = build()
    waves = [enc.upload([(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lens]) for lens in LISTS]
    forward = (lambda i: enc.forward(waves[i & 1], LISTS[i & 1])) if positional else (lambda i: enc.forward(waves[i & 1], lengths=LISTS[i & 1]))
    for i in range(4):
        forward(i)
    plan, plan_host = per_call(lambda i: enc._plan(LISTS[i & 1], 0), reps)
    both, both_host = per_call(forward, max(reps // 4, 20))
    lines.append(f"  {name:28s} _plan {plan:8.1f} us ({plan_host:8.1f} us until the last call returned);  _plan + forward {both:9.1f} us "
                 f"({both_host:9.1f} us until the last call returned)")
    del enc, waves
print("\n".join(lines))
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
