"""Time ser_resample_v alone (GPU box), next to the H2D copy of the same raw batch: 16 x 10 s at 44.1 and 48 kHz (and whatever rates are
given), HIP events, warmed up.  The two-slot pipeline hides the launch behind the copy only while it is not the longer of the two.

    python tools/resample_bench.py [rate ...]

Per rate: us per launch, the algorithmic bytes (raw samples in, 16 kHz samples out) per second, the fp64 FMA rate, the pinned H2D copy
of the raw batch, and the copy of the 16 kHz batch a 16 kHz corpus would have paid."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import _lib as L
from interspeech_ser_amd.frontend import polyphase_bank, resample_ratio, resampled_len

DEV = "cuda:0"
B, SECONDS = 16, 10


def timed(fn, reps=5, rounds=8):
    ts = []
    for r in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if r:                                                       # round 0 is the warm-up
            ts.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


for sr in [int(a) for a in sys.argv[1:]] or [44100, 48000]:
    up, down = resample_ratio(sr)
    h, half = polyphase_bank(up, down)
    n = SECONDS * sr
    n_out = resampled_len(n, sr)
    raw_host = (0.1 * torch.randn(B * n)).pin_memory()
    out_host = torch.empty(B * n_out).pin_memory()
    raw, out = torch.empty(B * n, device=DEV), torch.empty(B * n_out, device=DEV)
    raw.copy_(raw_host)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    in_offs, out_offs, boff = i64([b * n for b in range(B + 1)]), i64([b * n_out for b in range(B + 1)]), i64([0] * B)
    ups, downs, halves = i32([up] * B), i32([down] * B), i32([half] * B)
    bank = torch.from_numpy(h.copy()).to(DEV)
    a = L.ResampleArgs()
    a.wav, a.in_offs, a.out_offs, a.up, a.down, a.half = raw.data_ptr(), in_offs.data_ptr(), out_offs.data_ptr(), ups.data_ptr(), downs.data_ptr(), halves.data_ptr()
    a.bank_off, a.bank, a.out = boff.data_ptr(), bank.data_ptr(), out.data_ptr()
    a.total_in, a.total_out, a.max_out, a.B = B * n, B * n_out, n_out, B
    st = torch.cuda.current_stream().cuda_stream
    k_ms, k_lo, k_hi = timed(lambda: L.check(L.lib.ser_resample_v(ctypes.byref(a), st), "ser_resample_v"))
    c_ms, c_lo, c_hi = timed(lambda: raw.copy_(raw_host, non_blocking=True))
    o_ms, _, _ = timed(lambda: out.copy_(out_host, non_blocking=True))
    taps = 2 * half // up + 1
    algo = 4.0 * B * (n + n_out)
    print(f"{sr} Hz ({up}/{down}, {taps} taps, bank {len(h) * 8 / 1024:.0f} KB) 16 x 10 s: ser_resample_v {k_ms * 1e3:7.1f} us "
          f"[{k_lo * 1e3:.1f} .. {k_hi * 1e3:.1f}]  {algo / k_ms / 1e9:6.3f} TB/s algorithmic, {2.0 * B * n_out * taps / k_ms / 1e9:5.2f} TFLOP/s fp64 | "
          f"H2D of the raw batch ({4 * B * n / 1e6:.1f} MB) {c_ms * 1e3:7.1f} us [{c_lo * 1e3:.1f} .. {c_hi * 1e3:.1f}]  {4 * B * n / c_ms / 1e6:5.1f} GB/s | "
          f"H2D of the 16 kHz batch ({4 * B * n_out / 1e6:.1f} MB) {o_ms * 1e3:7.1f} us | launch / raw copy {k_ms / c_ms:.2f}", flush=True)
