"""CTC forced alignment stated in numpy (include/ser_hip.h, "a32"): the float64 Viterbi trellis over raw logits, its tie rules, the
feasibility rule, the per-frame and per-token scores, the status bits; and a brute-force enumeration of every valid path for tiny cases.
TEST INFRASTRUCTURE ONLY.

One utterance: fp32 logits z[T, V], a blank id, a target y[0 .. L-1].  S = 2 L + 1 states; state s emits the blank when s is even and
y[s // 2] when s is odd; alpha is float64 over RAW logits: one max of exact values and one float64 addition per cell, so the device's
alpha equals this loop's bit for bit."""
from __future__ import annotations

import numpy as np

INFEASIBLE, NONFINITE, BAD_TARGET = 1, 2, 4


def labels(y, blank: int) -> np.ndarray:
    """the emitted label of each of the 2 L + 1 states"""
    lab = np.full(2 * len(y) + 1, blank, dtype=np.int64)
    lab[1::2] = np.asarray(y, dtype=np.int64)
    return lab


def feasible(T: int, y) -> bool:
    """a path exists iff T >= 1 and T >= L + #{j : y[j] == y[j-1]}"""
    rep = sum(1 for j in range(1, len(y)) if y[j] == y[j - 1])
    return T >= 1 and T >= len(y) + rep


def lse64(z, V: int) -> np.ndarray:
    """float64 log-sum-exp of each row's V columns, the max subtracted first (NaN for a row with a NaN)"""
    x = np.asarray(z, dtype=np.float32)[:, :V].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=1)
        return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def trellis(z, y, blank: int, dtype=np.float32):
    """(final alpha as float64, the state of every frame) of the best path under the rule's ties; needs a feasible, valid target.
    ``dtype=np.float64`` runs the same recurrence on float64 logits (HF's, for the bound on path_logit end to end)."""
    z = np.asarray(z, dtype=dtype)
    T, L = z.shape[0], len(y)
    S = 2 * L + 1
    lab = labels(y, blank)
    can_skip = np.zeros(S, dtype=bool)
    for s in range(3, S, 2):
        can_skip[s] = y[s // 2] != y[s // 2 - 1]
    em = z[:, lab].astype(np.float64)                                          # [T, S], exact
    ninf = -np.inf
    alpha = np.full(S, ninf, dtype=np.float64)
    alpha[0] = em[0, 0]
    if S > 1:
        alpha[1] = em[0, 1]
    back = np.zeros((T, S), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a1 = np.concatenate(([ninf], alpha))[:S]
            a2 = np.where(can_skip, np.concatenate(([ninf, ninf], alpha))[:S], ninf)
            best, mv = alpha.copy(), np.zeros(S, dtype=np.int8)
            step = a1 > best                                                   # strictly greater: stay wins a tie
            best[step], mv[step] = a1[step], 1
            skp = a2 > best
            best[skp], mv[skp] = a2[skp], 2
            alpha = best + em[t]
            back[t] = mv
        end = S - 1
        if L > 0 and not alpha[S - 1] > alpha[S - 2]:
            end = S - 2
    states = np.zeros(T, dtype=np.int64)
    s = end
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    return np.float64(alpha[end]), states


def align(z, y, V: int, blank: int, max_tokens: int = 1023) -> dict:
    """The whole rule for one utterance: dict(status, and for status 0: path_logit, states, pos, starts, ends, frame_score64,
    frame_score, tok_score)."""
    z = np.asarray(z, dtype=np.float32)
    y = [int(v) for v in y]
    T, L = z.shape[0], len(y)
    if L > max_tokens or any(v < 0 or v >= V or v == blank for v in y):
        return dict(status=BAD_TARGET)
    if not feasible(T, y):
        return dict(status=INFEASIBLE)
    cols = sorted(set(y) | {blank})
    read = z[:, cols]
    score, states = trellis(z, y, blank)
    if np.isnan(read).any() or (read == np.inf).any() or not np.isfinite(score):
        return dict(status=NONFINITE, path_logit=score)
    pos = np.where(states % 2 == 1, states // 2, -1).astype(np.int32)
    emitted = labels(y, blank)[states]
    with np.errstate(invalid="ignore"):
        fs64 = z[np.arange(T), emitted].astype(np.float64) - lse64(z, V)
    starts, ends = np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.int32)
    for j in range(L):
        t = np.nonzero(pos == j)[0]
        starts[j], ends[j] = t[0], t[-1] + 1
        assert len(t) == ends[j] - starts[j], "a token's frames are contiguous"
    fs = fs64.astype(np.float32)
    return dict(status=0, path_logit=score, states=states, pos=pos, starts=starts, ends=ends, frame_score64=fs64, frame_score=fs,
                tok_score=token_means(fs, starts, ends))


def token_means(frame_score, starts, ends) -> np.ndarray:
    """fp32 of the float64 mean of the fp32 frame scores of each token, summed in frame order"""
    out = np.zeros(len(starts), dtype=np.float32)
    for j, (s, e) in enumerate(zip(starts, ends)):
        acc = np.float64(0.0)
        for t in range(int(s), int(e)):
            acc = acc + np.float64(frame_score[t])
        with np.errstate(invalid="ignore"):
            out[j] = np.float32(acc / np.float64(int(e) - int(s)))
    return out


def brute_force(z, y, blank: int):
    """Every valid state sequence of T frames enumerated: (best score, the set of state sequences that reach it).  A valid sequence starts
    in state 0 or 1, ends in S - 1 or S - 2, and moves by 0, 1, or 2 (2 only onto an odd state whose label differs from the previous
    token's).  The score is summed in frame order in float64, as the trellis sums it."""
    z = np.asarray(z, dtype=np.float32)
    T, L = z.shape[0], len(y)
    S = 2 * L + 1
    lab = labels(y, blank)
    best, arg = -np.inf, []

    def walk(seq, acc):
        nonlocal best, arg
        if len(seq) == T:
            if seq[-1] >= S - 2:
                if acc > best:
                    best, arg = acc, [tuple(seq)]
                elif acc == best:
                    arg.append(tuple(seq))
            return
        a = seq[-1]
        for d in (0, 1, 2):
            c = a + d
            if c >= S or (d == 2 and not (c % 2 == 1 and y[c // 2] != y[c // 2 - 1])):
                continue
            walk(seq + [c], acc + np.float64(z[len(seq), lab[c]]))

    for s0 in range(min(2, S)):
        walk([s0], np.float64(z[0, lab[s0]]))
    return best, arg


def tie_broken(paths):
    """Of equally good state sequences, the one the rule's ties select.  The backtrack runs from the last frame: the end state is S - 2
    unless S - 1 is strictly better, i.e. the SMALLER end state among the tied ones; then, at each earlier frame, given the later states, the
    smaller jump into the later state wins, i.e. the LARGER earlier state.  (Among tied complete paths that share frames t + 1 .., the
    prefix scores alpha[t][.] of their states at t plus the common rest are equal, so the trellis' choice at frame t + 1 is between tied
    candidates exactly when complete paths tie.)"""
    cand = list(paths)
    T = len(cand[0])
    last = min(p[-1] for p in cand)
    cand = [p for p in cand if p[-1] == last]
    for t in range(T - 2, -1, -1):
        keep = max(p[t] for p in cand)
        cand = [p for p in cand if p[t] == keep]
    assert len(cand) == 1
    return cand[0]


def sticky_targets(rng, L: int, V: int, blank: int, repeat_every: int = 5):
    """a target of L ids from [0, V) without the blank; every ``repeat_every``-th id repeats its predecessor (a forced blank between them)"""
    ids = [v for v in range(V) if v != blank]
    y = []
    for j in range(L):
        if j and (len(ids) == 1 or j % repeat_every == 0):
            y.append(y[-1])
        else:
            y.append(int(ids[int(rng.integers(len(ids)))]))
    return y


def n_repeats(y) -> int:
    return sum(1 for j in range(1, len(y)) if y[j] == y[j - 1])
