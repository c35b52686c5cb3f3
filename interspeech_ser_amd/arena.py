"""Grow-only buffer sets, one per pipeline slot: the one protocol behind every encoder's arena and every head's buffers.

A slot's set is sized by the largest batch the slot has seen; a batch that fits re-uses it, so pointers stay where they are from batch to
batch and a command list recorded over the set can be replayed.  A batch that does not fit gets a FRESH set at the per-key maximum of the
old capacities and its need.  Nothing of the old dict survives that: the recorded list and the laid-out plan point into the old buffers
and go with them.  ``TableBlob`` is the part of a set that carries a batch's O(B) integer tables from the host to the device."""
from typing import Callable, Dict

import numpy as np
import torch


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


class Pinned:
    """A page-locked host tensor and the event behind the last asynchronous copy out of it.  The protocol: ``wait`` before the buffer is
    rewritten (the one host wait; none before the first copy), ``sent`` right after a copy out of it was enqueued on the current stream."""

    def __init__(self, numel: int, dtype):
        self.host = torch.empty(numel, dtype=dtype).pin_memory()
        self._evt = torch.cuda.Event()

    def wait(self) -> None:
        self._evt.synchronize()

    def sent(self) -> None:
        self._evt.record()


class TableLayout:
    """Arithmetic of a table blob: ``regions`` fixed regions of ``cap_b + 2`` int64 words each.  An int64 table of up to cap_b + 2 entries
    or an int32 table of up to 2 cap_b + 4 (two per word) fits a region; offsets depend on the capacity and the region index alone."""

    def __init__(self, cap_b: int, regions: int):
        self.region, self.regions = int(cap_b) + 2, int(regions)
        self.words = self.region * self.regions

    def offset(self, r: int, n: int, per_word: int = 1) -> int:
        """element offset (in 8 / per_word-byte elements) of region ``r``'s table of ``n`` entries; refuses what does not fit"""
        if not 0 <= r < self.regions or n > per_word * self.region:
            raise ValueError(f"table {r} of {n} entries does not fit a blob of {self.regions} regions of {self.region} words")
        return per_word * r * self.region


class TableBlob(Pinned):
    """The O(B) integer tables of one plan (sample offsets, frame offsets per level, halo / tap base rows): one pinned int64 host tensor,
    its device twin and the event behind the last copy, laid out by ``TableLayout``.  A plan miss is ``begin``, one ``put64`` / ``put32``
    per table, ``send``, and only then the launches that read a table.  What holds:
      1. fixed addresses: a table's device address depends on the blob's capacity and on the order of the puts, never on the batch;
         recorded command lists hold these addresses (so a host puts its tables in one order);
      2. a plan hit does not touch the blob: no host write, no copy, no event (the hit path runs inside hipGraph capture);
      3. the host tensor is rewritten only after the event behind its previous copy has completed (``begin``), and nothing else waits;
      4. ``send`` is one copy on the current stream, enqueued ahead of the first launch that reads a table;
      5. every region starts on an 8-byte boundary; an int32 table is packed two per word from its region's first word."""

    def __init__(self, cap_b: int, regions: int, device):
        self.layout = TableLayout(cap_b, regions)
        super().__init__(self.layout.words, torch.int64)
        self.dev = torch.empty(self.layout.words, dtype=torch.int64, device=device)
        self._host = {1: self.host.numpy(), 2: self.host.numpy().view(np.int32)}
        self._dev = {1: self.dev, 2: self.dev.view(torch.int32)}

    def begin(self) -> "TableBlob":
        """wait for the copy of the previous plan's tables; the puts start over at region 0"""
        self.wait()
        self._next = 0
        return self

    def put64(self, values, per_word: int = 1) -> torch.Tensor:
        """``values`` into the next region as int64; returns the device view of exactly ``len(values)`` elements"""
        n = len(values)
        o = self.layout.offset(self._next, n, per_word)
        self._next += 1
        self._host[per_word][o:o + n] = values
        return self._dev[per_word][o:o + n]

    def put32(self, values) -> torch.Tensor:
        """the same as int32, two to a word"""
        return self.put64(values, 2)

    def send(self) -> None:
        self.dev.copy_(self.host, non_blocking=True)
        self.sent()
