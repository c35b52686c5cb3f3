"""The resampler's arithmetic, stated once more in float64 numpy for the tests (tests/test_resample_host.py, tests/test_gpu_resample.py):
they do not lean on frontend.polyphase_bank or on the kernel.

    g = gcd(sr, 16000), up = 16000 / g, down = sr / g, R = max(up, down), half = 10 R
    h[k] = up w[k] / sum(w),  w[k] = sinc((k - half) / R) / R * kaiser_14(2 half + 1)[k],  k = 0 .. 2 half
    y[m] = sum_j x[j] h[m down - j up + half]  over 0 <= j < n, 0 <= m down - j up + half <= 2 half;  m < (n up + down - 1) // down
"""
from math import gcd

import numpy as np

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000)


def ratio(sr):
    g = gcd(int(sr), 16000)
    return 16000 // g, int(sr) // g


def out_len(n, sr):
    up, down = ratio(sr)
    return (int(n) * up + down - 1) // down


def bank(sr):
    up, down = ratio(sr)
    R = max(up, down)
    half = 10 * R
    k = np.arange(2 * half + 1, dtype=np.float64)
    w = np.sinc((k - half) / R) / R * np.kaiser(2 * half + 1, 14.0)
    return up * w / w.sum(), half


def resample(x, sr):
    """float64 result of the statement above for fp32 (or any) samples x; the sum runs in ascending j."""
    up, down = ratio(sr)
    h, half = bank(sr)
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    m = np.arange(out_len(n, sr), dtype=np.int64)
    q = m * down + half
    j_hi = q // up
    y = np.zeros(len(m), dtype=np.float64)
    for t in range(2 * half // up, -1, -1):                    # j = j_hi - t ascending
        j = j_hi - t
        k = q - j * up
        ok = (j >= 0) & (j < n) & (k <= 2 * half)
        y[ok] += x[j[ok]] * h[k[ok]]
    return y


def within_one_ulp(got, ref, xmax):
    """|got - ref| <= spacing_fp32(|ref|) + 1e-13 max|x| for EVERY sample: one fp32 ulp plus 4 x the float64 accumulation bound
    121 * 2^-53 * 1.911 * max|x| = 2.6e-14 max|x| (121 taps at most, max over phases of sum|h| <= 1.911).  Returns the worst excess."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-13 * float(xmax)
    return float((np.abs(got - ref) - tol).max()) if len(ref) else -1.0
