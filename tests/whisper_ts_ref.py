"""Whisper token timestamps stated in numpy (include/ser_hip.h, "a33"): the three stages behind HF's
``WhisperGenerationMixin._extract_token_timestamps`` for one utterance given alone -- the cross-attention weights of the alignment heads,
the matrix (z-score over the token rows, median along the frames, mean over the heads, one rounding to fp32) and the dynamic time warping.
Test infrastructure, never imported by the package."""
import numpy as np

TIME_PRECISION = 0.02


def weights(q: np.ndarray, k: np.ndarray, scale: float, n_frames: int) -> np.ndarray:
    """q [A, R, 64] and k [A, S, 64] (fp32) -> fp32 [A, R, n_frames]: the softmax over ALL S keys in float64, the first frames kept."""
    s = np.einsum("ard,asd->ars", q.astype(np.float64), k.astype(np.float64)) * float(scale)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)[..., :n_frames]


def median_filter(z: np.ndarray, width: int) -> np.ndarray:
    """HF's ``_median_filter`` along the last axis: reflect padding, the middle of each sorted window; an axis no longer than the pad
    comes back as it is."""
    pad = width // 2
    if z.shape[-1] <= pad:
        return z
    zp = np.pad(z, [(0, 0)] * (z.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(zp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def matrix64(w: np.ndarray, width: int = 7) -> np.ndarray:
    """fp32 weights [A, R, F] -> the float64 matrix [R, F] BEFORE its rounding: sums in ascending row / head order."""
    w = w.astype(np.float64)
    A, R, F = w.shape
    s = np.zeros((A, F))
    for r in range(R):
        s += w[:, r]
    mean = s / R
    v = np.zeros((A, F))
    for r in range(R):
        v += (w[:, r] - mean) ** 2
    std = np.sqrt(v / R)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (w - mean[:, None]) / std[:, None]
    z = median_filter(z, width)
    out = np.zeros((R, F))
    for a in range(A):
        out += z[a]
    return out / A


def matrix(w: np.ndarray, width: int = 7) -> np.ndarray:
    return matrix64(w, width).astype(np.float32)


def dtw(m: np.ndarray):
    """HF's ``_dynamic_time_warping`` on ``-m`` (m fp32 [N, M]): (text_indices, time_indices) in path order, and the fp32 cost table."""
    m = np.asarray(m, dtype=np.float32)
    N, M = m.shape
    neg = -m.astype(np.float64)
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for j in range(1, M + 1):
            for i in range(1, N + 1):
                c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
                if c0 < c1 and c0 < c2:
                    c, t = c0, 0
                elif c1 < c0 and c1 < c2:
                    c, t = c1, 1
                else:
                    c, t = c2, 2
                cost[i, j] = np.float32(neg[i - 1, j - 1] + np.float64(c))
                trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64), cost


def dtw_diag(m: np.ndarray):
    """``dtw`` with the cells of an anti-diagonal computed at once (they depend on the two diagonals before only): the same conversions,
    float64 additions, roundings and comparisons, cell for cell -- tests/test_whisper_timestamps_host.py holds it equal to ``dtw`` --, fast
    enough for a 444 x 1500 matrix."""
    m = np.asarray(m, dtype=np.float32)
    N, M = m.shape
    neg = -m.astype(np.float64)
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.full((N + 1, M + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for d in range(2, N + M + 1):
            i = np.arange(max(1, d - M), min(N, d - 1) + 1)
            j = d - i
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            t = np.where((c0 < c1) & (c0 < c2), 0, np.where((c1 < c0) & (c1 < c2), 1, 2)).astype(np.int8)
            c = np.where(t == 0, c0, np.where(t == 1, c1, c2))
            cost[i, j] = (neg[i - 1, j - 1] + c.astype(np.float64)).astype(np.float32)
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = N, M
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return np.array(text[::-1], dtype=np.int64), np.array(time[::-1], dtype=np.int64), cost


def first_frames(text: np.ndarray, time: np.ndarray) -> np.ndarray:
    """HF's jump times in frames: the frame at which the path first enters each token row."""
    if len(text) == 0:
        return np.zeros(0, dtype=np.int64)
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps]


def token_times(first: np.ndarray, n_tokens: int) -> np.ndarray:
    """fp32 seconds of the n generated tokens from the n - 1 first frames: the last token repeats the one before it; n = 1 gives 0."""
    out = np.zeros(n_tokens, dtype=np.float32)
    if n_tokens >= 2:
        out[: n_tokens - 1] = (np.asarray(first[: n_tokens - 1], dtype=np.float64) * TIME_PRECISION).astype(np.float32)
        out[n_tokens - 1] = out[n_tokens - 2]
    return out
