"""The loops that feed batches to the GPU, once (host only: no torch, no device call of its own).

The failure contract every driver and head keeps: a file that cannot be loaded, or that still fails alone, is reported through the site's
``fail`` and costs only itself; a batch that fails is run again file by file, so one bad file cannot drop its neighbours.  What a site
keeps for itself is how an item is loaded, how a batch is run, what a result is and how a failure is worded.

``prefetch``      loads batch i + 1 on a thread pool while the caller works on batch i.
``run_or_each``   the synchronous shape: run the batch, else each file alone (head._run_hip, predictor.score_from_wav, transcribe).
``SlotPipeline``  the pipelined shape over an extractor's ``submit`` / ``collect`` / ``extract`` (driver._run, baseline._run_eval).
``write_result_csv`` / ``close_logger``: the tail of the heads' evaluation and scoring functions.
"""
from __future__ import annotations

import csv
import os
from collections import deque
from typing import Callable, Iterator, List, Optional, Sequence

import numpy as np


def make_batches(files: Sequence, batch_size: int) -> List[list]:
    return [list(files[i:i + batch_size]) for i in range(0, len(files), batch_size)]


def prefetch(batches: Sequence[Sequence], pool, load: Callable) -> Iterator[list]:
    """``[load(item) for item in batch]`` per batch, in order; the next batch is on ``pool.map`` while the caller holds this one (one
    batch ahead, never more).  ``load`` reports its own failures inside what it returns."""
    pending = pool.map(load, batches[0]) if batches else []
    for bi in range(len(batches)):
        loaded = list(pending)
        if bi + 1 < len(batches):
            pending = pool.map(load, batches[bi + 1])
        yield loaded


def run_or_each(items: Sequence, run: Callable, fail: Callable, catch=Exception) -> None:
    """``run(items)`` -> None, or an error (returned, or raised as a ``catch``).  A failed batch of more than one item runs each item
    alone and ``fail(item, error)`` names what still fails; a failed batch of one is reported as it is, with no second run."""
    def attempt(batch):
        try:
            return run(batch)
        except catch as e:
            return e

    err = attempt(items)
    if err is None:
        return
    if len(items) == 1:
        fail(items[0], err)
        return
    for item in items:
        e1 = attempt([item])
        if e1 is not None:
            fail(item, e1)


class SlotPipeline:
    """Batches over ``slots`` pipeline slots: batch ``bi`` is submitted to slot ``bi % slots`` and ``slots - 1`` tickets stay in flight while
    the caller prepares the next batch; tickets are collected oldest first.

    ``submit(good, slot) -> ticket``, ``collect(ticket) -> results`` and ``extract(good) -> results`` (synchronous) wrap the extractor's;
    ``done(good, results, ticket)`` receives a finished batch (``ticket`` None for what came through ``extract``) and
    ``fail(item, error)`` a file that failed alone.  A batch whose ``collect`` raises is extracted file by file; when ``submit`` raises,
    everything in flight is finished first and then the batch goes file by file, which keeps the per-slot order simple.
    ``before_retry`` runs ahead of each such retry: the synchronous path shares slot 0's arena with the pipeline, so the sites
    synchronize the device there.  ``pipelined=False``: every batch goes through ``extract`` as a whole."""

    def __init__(self, submit: Callable, collect: Callable, extract: Callable, slots: int, done: Callable, fail: Callable,
                 before_retry: Optional[Callable] = None, pipelined: bool = True):
        self.submit, self.collect, self.extract, self.slots = submit, collect, extract, slots
        self.done, self.fail, self.before_retry, self.pipelined = done, fail, before_retry, pipelined
        self.inflight: deque = deque()

    def each(self, good) -> None:
        if self.before_retry is not None:
            self.before_retry()
        for item in good:
            try:
                self.done([item], self.extract([item]), None)
            except Exception as e:                                      # noqa: BLE001
                self.fail(item, e)

    def push(self, bi: int, good) -> None:
        try:
            if self.pipelined:
                self.inflight.append((good, self.submit(good, bi % self.slots)))
            else:
                self.done(good, self.extract(good), None)
        except Exception:                                               # noqa: BLE001
            self.drain(0)
            self.each(good)

    def drain(self, keep: Optional[int] = None) -> None:
        """collect until ``keep`` tickets are in flight (default: all but one slot's); ``drain(0)`` ends the run"""
        keep = self.slots - 1 if keep is None else keep
        while len(self.inflight) > keep:
            good, ticket = self.inflight.popleft()
            try:
                results = self.collect(ticket)
            except Exception:                                           # noqa: BLE001
                self.each(good)
                continue
            self.done(good, results, ticket)


def write_result_csv(model_path: str, split: str, first_cell: str, names: Sequence[str], rows, letters: Sequence[str]) -> str:
    """``<model_path>/results/<split>.csv``: ``first_cell`` (the reference writes ``Filename`` in dev.csv and ``FileName`` in test.csv),
    Prediction (the letter of the argmax), the logits as class_i_prob with four decimals.  Returns the file's path."""
    os.makedirs(os.path.join(model_path, "results"), exist_ok=True)
    csv_file = os.path.join(model_path, "results", split + ".csv")
    with open(csv_file, mode="w", newline="") as f:
        w = csv.writer(f)
        w.writerow([first_cell, "Prediction"] + [f"class_{i}_prob" for i in range(len(letters))])
        for row, utt in zip(rows, names):
            w.writerow([utt, letters[int(np.argmax(row))]] + [f"{p:.4f}" for p in np.asarray(row).flatten()])
    return csv_file


def close_logger(log) -> None:
    for h in list(log.handlers):
        h.close()
        log.removeHandler(h)
