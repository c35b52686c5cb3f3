"""Host side of the Whisper beam search (numpy only; the device side is csrc/beam.hip, include/ser_hip.h "a34"): the table the device
divides by, and the reading of the trace it leaves -- hypotheses are never stored, only (parent, token) per step, and any of them is
recovered by walking the parents back."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np


def lenpow_table(n: int, length_penalty: float) -> np.ndarray:
    """float64 [n]: i ** length_penalty, each a scalar float64 power, so that the device divides by the number a numpy scalar gives."""
    lp = np.float64(length_penalty)
    with np.errstate(all="ignore"):
        return np.array([float(np.float64(i) ** lp) for i in range(n)], dtype=np.float64)


def backtrack(trace_run: np.ndarray, trace_cand: np.ndarray, b: int, step: int, rank: int, first: int) -> List[int]:
    """The generated tokens of candidate ``rank`` of utterance ``b`` at position ``step``.  trace_run int [T, B, K, 2] and trace_cand int
    [T, B, 2K, 2] hold (parent, token) per position; ``first``: the position of the first beam step."""
    parent, tok = (int(v) for v in trace_cand[step, b, rank])
    if parent < 0:
        raise ValueError(f"utterance {b}: step {step} has no candidate of rank {rank}")
    out = [tok]
    for s in range(step - 1, first - 1, -1):
        parent, tok = (int(v) for v in trace_run[s, b, parent])
        if parent < 0:
            raise ValueError(f"utterance {b}: the trace breaks at step {s}")
        out.append(tok)
    return out[::-1]


def running_history(trace_run: np.ndarray, b: int, step: int, row: int, first: int) -> List[int]:
    """The generated tokens running row ``row`` of utterance ``b`` holds after position ``step``."""
    out = []
    for s in range(step, first - 1, -1):
        row, tok = (int(v) for v in trace_run[s, b, row])
        if row < 0:
            raise ValueError(f"utterance {b}: the trace breaks at step {s}")
        out.append(tok)
    return out[::-1]


def nbest(trace_run: np.ndarray, trace_cand: np.ndarray, fin_score: np.ndarray, fin_handle: np.ndarray, n_fin: Sequence[int], first: int
          ) -> List[List[Tuple[List[int], float]]]:
    """Per utterance its finished hypotheses, best first: [(generated tokens with the closing eos where there is one, score)].  The
    device keeps the finished set in descending order (an older entry first on a tie); fin_handle [B, K, 2] = (position, rank)."""
    out = []
    for b in range(fin_score.shape[0]):
        rows = []
        for k in range(int(n_fin[b])):
            step, rank = (int(v) for v in fin_handle[b, k])
            rows.append((backtrack(trace_run, trace_cand, b, step, rank, first), float(fin_score[b, k])))
        if any(rows[i][1] < rows[i + 1][1] for i in range(len(rows) - 1)):
            raise ValueError(f"utterance {b}: the finished set is not in descending order")
        out.append(rows)
    return out
