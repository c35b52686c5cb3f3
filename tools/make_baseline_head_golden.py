"""Writes tests/golden/baseline_head.npz: what the reference's own modules (benchmark/net: AttentiveStatisticsPooling,
EmotionRegression) compute, in fp32 on the CPU, for seeded weights and one ragged input.  Arrays only.

    python tools/make_baseline_head_golden.py /path/to/interspeech_ser/benchmark

Run where the reference checkout exists; the fixture it leaves is what tests/test_baseline_head_host.py compares tests/asp_ref.py to.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, H, LENGTHS = 64, 96, (1, 2, 70, 333)


def main(benchmark_dir: str) -> None:
    sys.path.insert(0, benchmark_dir)
    from net.pooling import AttentiveStatisticsPooling
    from net.ser import EmotionRegression
    g = np.random.default_rng(20250)

    def n(*shape, std=1.0, mean=0.0):
        return torch.from_numpy((g.standard_normal(shape) * std + mean).astype(np.float32))
    out = {}
    pool = AttentiveStatisticsPooling(D)
    pool_sd = {"attention": n(D, 1), "sap_linear.weight": n(D, D, std=1.0 / np.sqrt(D)), "sap_linear.bias": n(D, std=0.1)}
    out["pool_keys"] = np.array(list(pool.state_dict().keys()))
    pool.load_state_dict(pool_sd)
    pool.eval()
    x = n(sum(LENGTHS), D)                                   # zero-mean columns (see the host test's note on m2 - mu^2)
    offs = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    with torch.no_grad():
        rows = []
        for b, T in enumerate(LENGTHS):                      # the evaluation scripts run a batch of one; all T frames take part
            xs = x[offs[b]: offs[b + 1]].unsqueeze(0)
            mask = torch.ones(1, (T - 1) * 320 + 400)        # a waveform of T frames: feat_len = (len - 1) // 320 + 1 >= T
            rows.append(pool(xs, mask)[0])
        pooled = torch.stack(rows)
        out.update(x=x.numpy(), frame_offs=offs, pooled=pooled.numpy())
        out.update({"pool." + k: v.numpy() for k, v in pool_sd.items()})
        for n_out in (8, 3):
            ser = EmotionRegression(2 * D, H, 1, n_out, dropout=0.5)
            ser_sd = {"fc.0.0.weight": n(H, 2 * D, std=1.0 / np.sqrt(2 * D)), "fc.0.0.bias": n(H, std=0.1),
                      "fc.0.1.weight": n(H, std=0.1, mean=1.0), "fc.0.1.bias": n(H, std=0.1),
                      "out.0.weight": n(n_out, H, std=1.0 / np.sqrt(H)), "out.0.bias": n(n_out, std=0.1)}
            out["ser_keys"] = np.array(list(ser.state_dict().keys()))
            ser.load_state_dict(ser_sd)
            ser.eval()
            out[f"logits{n_out}"] = ser(pooled).numpy()
            out.update({f"ser{n_out}." + k: v.numpy() for k, v in ser_sd.items()})
    path = os.path.join(ROOT, "tests", "golden", "baseline_head.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
