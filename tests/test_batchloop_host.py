"""Host tests of interspeech_ser_amd/batchloop.py (no GPU).

1. The recorded behaviour of the six batch loops as they were written out per site (tests/golden/batch_loop_traces.json, recorded by
   tools/record_batch_loops.py before the loops moved): every scenario is replayed on the shared code and must give the recording, call
   for call on the stub and line for line on stdout.
2. The module's own mechanisms, directly."""
import importlib.util
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import pytest

from interspeech_ser_amd import batchloop as BL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_batch_loops", os.path.join(ROOT, "tools", "record_batch_loops.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)
SCENARIOS = REC.scenarios()


@pytest.fixture(scope="module")
def recorded():
    with open(REC.GOLDEN) as f:
        return json.load(f)


def test_every_recorded_scenario_is_replayed(recorded):
    assert {(site, name) for site, name, _ in SCENARIOS} == {(site, name) for site, names in recorded.items() for name in names}


@pytest.mark.parametrize("site,name,fn", SCENARIOS, ids=[f"{s}-{n}" for s, n, _ in SCENARIOS])
def test_batch_loop_matches_the_recording(recorded, built_library, site, name, fn):
    got, want = REC.run_scenario(site, name, fn), recorded[site][name]
    assert got["calls"] == want["calls"]
    assert got["lines"] == want["lines"]
    assert got == want                                      # pool lines (sorted), results, counters, the files and tables written


# ----------------------------------------------------------------------------------------------------- prefetch
class _CountingPool:
    """``map`` as ThreadPoolExecutor's, counting the batches handed over and not yet read to their end"""

    def __init__(self):
        self.mapped, self.pool = [], ThreadPoolExecutor(2)

    def map(self, fn, batch):
        self.mapped.append(list(batch))
        return self.pool.map(fn, batch)


def test_prefetch_stays_one_batch_ahead_and_keeps_the_order():
    pool = _CountingPool()
    batches = BL.make_batches(list(range(11)), 3)
    assert batches == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10]]
    seen = []
    for bi, loaded in enumerate(BL.prefetch(batches, pool, lambda i: (i, threading.current_thread() is not threading.main_thread()))):
        assert [i for i, _ in loaded] == batches[bi] and all(off_main for _, off_main in loaded)
        assert len(pool.mapped) == min(bi + 2, len(batches))            # this batch and at most the next one were handed to the pool
        seen.append(loaded)
    assert len(seen) == 4 and pool.mapped == batches
    pool.pool.shutdown()


def test_prefetch_of_nothing_yields_nothing():
    pool = _CountingPool()
    assert list(BL.prefetch([], pool, lambda i: i)) == [] and pool.mapped == []
    pool.pool.shutdown()


# ----------------------------------------------------------------------------------------------------- run_or_each
@pytest.mark.parametrize("how", ["returns", "raises"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_run_or_each_runs_a_failing_batch_once_more_per_item_unless_it_is_one(n, how):
    runs, failures = [], []

    def run(items):
        runs.append(list(items))
        if "bad" in items:
            if how == "raises":
                raise RuntimeError("bad item")
            return "bad item"

    items = ["bad"] + [f"ok{i}" for i in range(n - 1)]
    BL.run_or_each(items, run, lambda item, err: failures.append((item, str(err))))
    assert len(runs) == (1 if n == 1 else 1 + n)
    assert runs[0] == items and runs[1:] == ([[it] for it in items] if n > 1 else [])
    assert failures == [("bad", "bad item")]
    runs.clear()
    BL.run_or_each(items[1:] or ["ok"], run, lambda item, err: failures.append((item, str(err))))
    assert len(runs) == 1 and len(failures) == 1                         # a clean batch runs once and reports nothing


def test_run_or_each_lets_through_what_the_site_does_not_catch():
    def run(items):
        raise KeyError("not mine")
    with pytest.raises(KeyError):
        BL.run_or_each([1, 2], run, lambda *a: None, catch=())
    with pytest.raises(KeyError):
        BL.run_or_each([1, 2], run, lambda *a: None, catch=ValueError)


# ----------------------------------------------------------------------------------------------------- SlotPipeline
@pytest.mark.parametrize("fails", ["nothing", "collect 2", "submit 3", "submit 1"])
@pytest.mark.parametrize("slots", [2, 3])
def test_slot_pipeline_never_refills_a_slot_before_its_ticket_was_collected(slots, fails):
    busy, events, finished, failed, synced = {}, [], [], [], []

    def submit(good, slot):
        n = good[0] // 2 + 1
        events.append(("submit", n, slot))
        if fails == f"submit {n}":
            raise RuntimeError("no launch")
        assert slot not in busy, "slot refilled before its batch was collected"
        assert len(busy) <= slots - 1
        busy[slot] = n
        return dict(slot=slot, batch=n)

    def collect(ticket):
        assert busy.pop(ticket["slot"]) == ticket["batch"]
        events.append(("collect", ticket["batch"], ticket["slot"]))
        if fails == f"collect {ticket['batch']}":
            raise RuntimeError("lost")
        return ["pipelined"] * 2

    def extract(good):
        assert not (fails.startswith("submit") and busy), "the synchronous path ran with tickets in flight after a failed submit"
        events.append(("extract", good[0]))
        if good[0] == 5:
            raise RuntimeError("still bad")
        return ["alone"]

    pipe = BL.SlotPipeline(submit, collect, extract, slots, lambda good, res, ticket: finished.append((list(good), list(res), ticket is None)),
                           lambda item, err: failed.append((item, str(err))), before_retry=lambda: synced.append(len(events)))
    for bi in range(5):
        pipe.push(bi, [2 * bi, 2 * bi + 1])
        pipe.drain()
        assert len(pipe.inflight) <= slots - 1
    pipe.drain(0)
    assert not busy and not pipe.inflight
    collects = [e[1] for e in events if e[0] == "collect"]
    assert collects == sorted(collects)                                 # oldest first
    assert all(e[2] == (e[1] - 1) % slots for e in events if e[0] == "submit")
    retried = {"nothing": None, "collect 2": 2, "submit 3": 3, "submit 1": 1}[fails]
    done_items = sorted(i for good, _, _ in finished for i in good)
    if retried is None:
        assert done_items == list(range(10)) and not failed and not synced
        assert [e[0] for e in events[:slots]] == ["submit"] * slots     # ``slots`` batches are submitted before the first wait
    else:
        pair = [2 * (retried - 1), 2 * (retried - 1) + 1]
        assert [e[1] for e in events if e[0] == "extract"] == pair and len(synced) == 1
        assert failed == ([(5, "still bad")] if 5 in pair else [])
        assert done_items == [i for i in range(10) if not (i == 5 and 5 in pair)]
        assert [(good, res) for good, res, alone in finished if alone] == [([i], ["alone"]) for i in pair if i != 5]


def test_slot_pipeline_without_slots_extracts_whole_batches():
    calls, finished, failed = [], [], []

    def extract(good):
        calls.append(list(good))
        if len(good) > 1 and 3 in good:
            raise RuntimeError("batch")
        return [f"r{i}" for i in good]

    pipe = BL.SlotPipeline(None, None, extract, 2, lambda good, res, ticket: finished.append((list(good), list(res))),
                           lambda item, err: failed.append(item), pipelined=False)
    for bi in range(3):
        pipe.push(bi, [2 * bi, 2 * bi + 1])
        pipe.drain()
    pipe.drain(0)
    assert calls == [[0, 1], [2, 3], [2], [3], [4, 5]] and not failed
    assert finished == [([0, 1], ["r0", "r1"]), ([2], ["r2"]), ([3], ["r3"]), ([4, 5], ["r4", "r5"])]


# ----------------------------------------------------------------------------------------------------- the heads' tail
def test_result_csv_keeps_the_two_headers_apart(tmp_path):
    import csv
    import logging
    rows = [[0.1, 2.0, -1.0], [3.14159, 0.0, 0.00004]]
    for split, cell in (("dev", "Filename"), ("test", "FileName")):
        path = BL.write_result_csv(str(tmp_path), split, cell, ["a.wav", "b.wav"], rows, ["X", "Y", "Z"])
        assert path == os.path.join(str(tmp_path), "results", split + ".csv")
        with open(path, newline="") as f:
            assert list(csv.reader(f)) == [[cell, "Prediction", "class_0_prob", "class_1_prob", "class_2_prob"],
                                           ["a.wav", "Y", "0.1000", "2.0000", "-1.0000"], ["b.wav", "X", "3.1416", "0.0000", "0.0000"]]
    log = logging.getLogger("test_batchloop_host")
    log.addHandler(logging.FileHandler(str(tmp_path / "x.log")))
    BL.close_logger(log)
    assert log.handlers == []
