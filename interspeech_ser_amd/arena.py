"""Grow-only buffer sets, one per pipeline slot: the one protocol behind every encoder's arena and every head's buffers.

A slot's set is sized by the largest batch the slot has seen; a batch that fits re-uses it, so pointers stay where they are from batch to
batch and a command list recorded over the set can be replayed.  A batch that does not fit gets a FRESH set at the per-key maximum of the
old capacities and its need.  Nothing of the old dict survives that: the recorded list and the laid-out plan point into the old buffers
and go with them."""
from typing import Callable, Dict


class SlotArenas:
    """``build(cap)`` returns the buffers (a dict) for the capacities ``cap``; ``fit`` adds ``"cap"`` and ``"plan"`` (None) to it."""

    def __init__(self, build: Callable[[Dict[str, int]], dict]):
        self._build = build
        self._slots: Dict[int, dict] = {}

    def fit(self, slot: int, **need: int) -> dict:
        """The slot's set, large enough for ``need``.  The hit path only compares integers: it runs inside hipGraph capture."""
        ar = self._slots.get(slot)
        old = ar["cap"] if ar is not None else {}
        if ar is not None and all(old.get(k, 0) >= v for k, v in need.items()):
            return ar
        cap = {k: max(int(v), old.get(k, 0)) for k, v in need.items()}
        ar = self._build(cap)
        ar["cap"], ar["plan"] = cap, None
        self._slots[slot] = ar
        return ar

    def __getitem__(self, slot: int) -> dict:
        return self._slots[slot]

    def get(self, slot: int, default=None):
        return self._slots.get(slot, default)
