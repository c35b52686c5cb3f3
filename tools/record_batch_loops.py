"""Record what the batch loops of the drivers do, around stubbed models (no GPU): for every scenario the sequence of calls the main thread
makes on the stub (``submit(n, slot)``, ``collect``, ``extract``, ``hold``, ``run(names)``) and the lines it prints, in order; lines
printed from pool threads (a failing ``write``) as a sorted set.  Nothing that depends on timing is kept.

    python tools/record_batch_loops.py            # writes tests/golden/batch_loop_traces.json

``tests/test_batchloop_host.py`` replays every scenario and requires equality with the recording, call for call and line for line.
The sites: ``driver._run``, ``baseline._run_eval``, ``head._run_hip``, ``predictor.score_from_wav`` (its encoders, weights and predictor
patched out, ``torch.cuda.is_available`` answered with yes) and ``transcribe.WhisperTranscriber.transcribe``."""
import contextlib
import json
import os
import re
import shutil
import sys
import tempfile
import threading
import wave
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_loop_traces.json")
BASE = 2000                     # file u<i> holds BASE + 100 i samples: a stub tells the files apart by their lengths


class _Capture:
    """stdout that keeps the main thread's lines in order and the other threads' apart"""

    def __init__(self):
        self.main, self.pool, self.part = [], [], {}

    def write(self, text):
        me = threading.current_thread()
        buf = self.part.get(me, "") + text
        *lines, self.part[me] = buf.split("\n")
        (self.main if me is threading.main_thread() else self.pool).extend(lines)
        return len(text)

    def flush(self):
        pass


def _clean(lines, root):
    """tmp paths and everything a clock decides taken out"""
    out = []
    for ln in lines:
        ln = re.sub(r"\.\d+\.tmp", ".PID.tmp", ln.replace(root, "<root>"))      # a partial output carries its writer's pid
        if ln.startswith("SER_RUN "):
            d = json.loads(ln[8:])
            ln = f"SER_RUN utterances {d['utterances']} audio_s {d['audio_s']}"
        ln = re.sub(r"(utterances on \d+ GPU\(s\)) in .*", r"\1", ln)
        if ln.startswith("launch thread:") or ln.startswith("  submit ="):
            ln = re.sub(r"[0-9.]+ s", "T s", ln)
        out.append(ln)
    return out


def _record(fn, root):
    cap = _Capture()
    raised = None
    with contextlib.redirect_stdout(cap), contextlib.redirect_stderr(open(os.devnull, "w")):
        try:
            result = fn()
        except Exception as e:                                          # noqa: BLE001
            result, raised = None, f"{type(e).__name__}: {e}"
    return result, raised, _clean(cap.main, root), sorted(_clean(cap.pool, root))


def write_wav(path, n, rate=16000, seed=0):
    pcm = (np.random.default_rng(seed + n).integers(-3000, 3000, size=n)).astype("<i2")
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())


def name_of(n_samples):
    return f"u{(int(n_samples) - BASE) // 100}"


def corpus(root, n, broken=(), rate_of=None, tag=""):
    d = os.path.join(root, "wav")
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    for i in range(n):
        p = os.path.join(d, f"u{i}{tag}.wav")
        if i in broken:
            with open(p, "wb") as f:
                f.write(b"not a wav file" * (200 - i))                  # its size keeps its place in the length order
        else:
            write_wav(p, BASE + 100 * i, (rate_of or {}).get(i, 16000))
    return d


# ----------------------------------------------------------------------------------------------------- driver._run / baseline._run_eval
def pipeline_stub(calls, slots=2, pipelined=True, submit_fail=(), collect_fail=(), extract_fail=(), hold=True, rates=False, has_slots=True,
                  logits=False):
    """A stub of ``driver._Extractor`` (``logits``: of ``baseline.BaselinePredictor``).  ``submit_fail`` / ``collect_fail``: numbers of the
    submit calls (from 1) that raise there; ``extract_fail``: names of the files whose ``extract`` raises."""
    from interspeech_ser_amd import config as C

    class Stub:
        def __init__(self, *a):
            self.geo, self.weight_source, self.n = C.TINY_WAVLM, "stub", 0

        def prepare(self, wav):
            return np.ascontiguousarray(wav, dtype=np.float32)

        def _out(self, waves, v):
            if logits:
                return np.stack([np.full(8, v, dtype=np.float32) + np.arange(8) * (len(w) % 7) for w in waves])
            return [torch.full((2, 4), float(v)) for _ in waves]

        def _submit(self, waves, layer_index, slot, r=None):
            self.n += 1
            calls.append(f"submit({self.n}: {' '.join(name_of(len(w)) for w in waves)}; slot {slot}; layer {layer_index}"
                         + (f"; rates {list(r)}" if r is not None else "") + ")")
            if self.n in submit_fail:
                raise RuntimeError(f"submit {self.n} failed")
            return dict(slot=slot, batch=self.n, waves=waves)

        def collect(self, ticket):
            calls.append(f"collect({ticket['batch']})")
            if ticket["batch"] in collect_fail:
                raise RuntimeError(f"collect {ticket['batch']} failed")
            return self._out(ticket["waves"], ticket["batch"])

        def _extract(self, waves, layer_index, r=None):
            calls.append(f"extract({' '.join(name_of(len(w)) for w in waves)}; layer {layer_index}" + (f"; rates {list(r)}" if r is not None else "") + ")")
            for w in waves:
                if name_of(len(w)) in extract_fail:
                    raise RuntimeError(f"extract of {name_of(len(w))} failed")
            return self._out(waves, -1)

    if logits:
        Stub.submit = lambda self, waves, layer_index=None, slot=0, rates=None: self._submit(waves, layer_index, slot)
        Stub.extract = lambda self, waves, layer_index=None, rates=None: self._extract(waves, layer_index)
    elif rates:
        Stub.upload_resampled = None                                    # its presence makes the driver hand the rates over
        Stub.submit = lambda self, waves, layer_index, slot, rates=None: self._submit(waves, layer_index, slot, rates)
        Stub.extract = lambda self, waves, layer_index, rates=None: self._extract(waves, layer_index, rates)
    else:
        Stub.submit = lambda self, waves, layer_index, slot: self._submit(waves, layer_index, slot)
        Stub.extract = lambda self, waves, layer_index: self._extract(waves, layer_index)
    if hold:
        def _hold(self, slot, futures):
            calls.append(f"hold(slot {slot}, {len(list(futures))} futures)")
        Stub.hold = _hold
    if has_slots:
        Stub.SLOTS = slots
    if not pipelined:                                                   # such an extractor has ``extract`` and nothing of the pipeline
        Stub.pipelined = False
        del Stub.submit, Stub.collect, Stub.hold
    return Stub


PIPE_SCENARIOS = {            # name -> (files, corpus keywords, stub keywords, extra flags of the driver)
    **{f"{b}_batches_slots{s}": (n, {}, dict(slots=s), []) for s in (2, 3) for b, n in ((0, 0), (1, 1), (2, 3), (5, 9))},
    "file_fails_to_decode": (5, dict(broken=(1,)), {}, []),
    "batch_fails_to_decode": (7, dict(broken=(3, 2)), {}, []),
    "submit_raises_batch1_nothing_in_flight": (5, {}, dict(submit_fail=(1,)), []),
    "submit_raises_batch3_in_flight_slots2": (9, {}, dict(submit_fail=(3,)), []),
    "submit_raises_batch3_in_flight_slots3": (9, {}, dict(slots=3, submit_fail=(3,)), []),
    "collect_raises_slots2": (9, {}, dict(collect_fail=(2,)), []),
    "collect_raises_slots3": (9, {}, dict(slots=3, collect_fail=(2, 5)), []),
    "file_still_fails_in_retry": (7, {}, dict(collect_fail=(2,), extract_fail=("u2",)), []),
    "submit_raises_and_file_still_fails": (7, {}, dict(submit_fail=(2,), extract_fail=("u3",)), []),
    "failing_batch_of_one": (5, {}, dict(submit_fail=(3,), extract_fail=("u0",)), []),
    "not_pipelined": (5, {}, dict(pipelined=False), []),
    "not_pipelined_batch_fails_once": (5, {}, dict(pipelined=False, extract_fail=("u2",)), []),
}
DRIVER_ONLY = {
    "layer_out_of_range": (5, dict(broken=(1,)), {}, ["--n_layer", "9"]),
    "rates_with_gpu_resample": (5, dict(rate_of={2: 8000}), dict(rates=True, collect_fail=(1,)), ["--resample"]),
    "average": (3, {}, {}, ["--use_average", "y"]),
    "timing": (3, {}, {}, ["--timing"]),
    "write_fails_in_the_pool": (5, {}, {}, []),
}


BASELINE_ONLY = {"slots_default_when_absent": (5, {}, dict(has_slots=False, collect_fail=(1,)), [])}


def driver_scenario(root, name):
    from interspeech_ser_amd import driver
    n, ckw, skw, flags = {**PIPE_SCENARIOS, **DRIVER_ONLY}[name]
    wav_dir, out = corpus(root, n, **ckw), os.path.join(root, "out")
    shutil.rmtree(out, ignore_errors=True)
    if name == "write_fails_in_the_pool":
        os.makedirs(os.path.join(out, "u2.pt", "in_the_way"))           # the rename onto a non-empty directory fails in the writer thread
    calls = []
    argv = ["--wav_dir", wav_dir, "--save_path", out, "--batch_size", "2", "--use_n_layer", "--n_layer", "1", "--num_workers", "2"] + flags
    rc, raised, lines, pool_lines = _record(lambda: driver._run(argv, whisper=False, extractor_factory=pipeline_stub(calls, **skw)), root)
    written = sorted(f for f in os.listdir(out) if os.path.isfile(os.path.join(out, f)))
    last = {k: driver.LAST_RUN[k] for k in ("done", "audio_s")} if raised is None else None
    return dict(calls=calls, lines=lines, pool_lines=pool_lines, raised=raised, rc=rc, written=written, last_run=last,
                last_run_keys=sorted(driver.LAST_RUN), launch_thread_keys=list(driver.LAST_RUN.get("launch_thread", {})))


def baseline_scenario(root, name):
    from interspeech_ser_amd import baseline
    n, ckw, skw, _ = {**PIPE_SCENARIOS, **BASELINE_ONLY}[name]
    skw = dict(skw, hold=False, logits=True)
    wav_dir, model = corpus(root, n, tag="_test3", **ckw), os.path.join(root, "model")
    shutil.rmtree(model, ignore_errors=True)
    os.makedirs(model)
    cfg = os.path.join(root, "config.json")
    with open(cfg, "w") as f:
        json.dump({"wav_dir": wav_dir}, f)
    calls = []
    stub = pipeline_stub(calls, **skw)()
    argv = ["--model_path", model, "--config_path", cfg, "--batch_size", "2", "--num_workers", "2"]
    rc, raised, lines, pool_lines = _record(lambda: baseline._run_eval(argv, "cat", lambda *a: stub), root)
    with open(os.path.join(model, "results", "test3.csv")) as f:
        table = f.read().splitlines()
    return dict(calls=calls, lines=lines, pool_lines=pool_lines, raised=raised, rc=rc, csv=table)


# ----------------------------------------------------------------------------------------------------- the synchronous sites
SYNC_SCENARIOS = {            # name -> (files, files that cannot be loaded, files whose batch reports an error, files whose batch raises)
    "0_batches": (0, (), (), ()),
    "1_batch_of_one": (1, (), (), ()),
    "2_batches": (3, (), (), ()),
    "5_batches": (9, (), (), ()),
    "file_fails_to_load": (5, (1,), (), ()),
    "batch_fails_to_load": (5, (2, 3), (), ()),
    "batch_reports_an_error": (5, (), (2,), ()),
    "batch_raises": (5, (), (), (3,)),
    "two_files_still_fail": (7, (), (0,), (1,)),
    "failing_batch_of_one_reports": (5, (), (4,), ()),
    "failing_batch_of_one_raises": (5, (), (), (4,)),
    "failing_batch_after_a_load_failure_left_one": (5, (2,), (3,), ()),
}


def _scaled(n, bad, per):
    """the scenario's file numbers stretched to batches of ``per`` files: file k of batch b -> per b / 2 + k"""
    move = lambda i: (i // 2) * per + (i % 2)                           # noqa: E731
    return (n // 2) * per + (n % 2), [tuple(move(i) for i in s) for s in bad]


def run_hip_scenario(root, name, modalities=2):
    from interspeech_ser_amd import head as HD
    n, (missing, reports, raises) = _scaled(SYNC_SCENARIOS[name][0], SYNC_SCENARIOS[name][1:], HD.HIP_BATCH)
    lazy = [os.path.join(root, f"lazy{m + 1}") for m in range(modalities)]
    for d in lazy:
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
    names = [f"u{i}.wav" for i in range(n)]
    for i in range(n):
        for m, d in enumerate(lazy):
            if i in missing and m == 1:
                continue
            torch.save(torch.full((1 + i % 3, 4), float(i)), os.path.join(d, f"u{i}.pt"))
    calls = []

    class Head:
        def forward(self, x1, offs1, *rest):
            ids = [int(x1[int(o), 0]) for o in offs1[:-1]]
            calls.append("run(" + " ".join(f"u{i}" for i in ids) + ")")
            if any(i in raises for i in ids):
                raise RuntimeError("forward of " + " ".join(f"u{i}" for i in ids if i in raises) + " failed")
            self.err = [i for i in ids if i in reports]
            return torch.tensor([[float(i)] * 8 for i in ids])

        def status(self):
            return (len(self.err), 0)

        def failure(self, bits, err):
            return f"error word set by {self.err}" if bits else None

    config = {f"lazy_dir{m + 1}": d for m, d in enumerate(lazy)}
    res, raised, lines, pool_lines = _record(lambda: HD._run_hip(Head(), config, names, "cpu", modalities), root)
    done, rows, failed = res
    return dict(calls=calls, lines=lines, pool_lines=pool_lines, raised=raised, done=list(done), rows=[float(r[0]) for r in rows], failed=failed)


def score_from_wav_scenario(root, name):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import predictor as P
    n, missing, _, raises = SYNC_SCENARIOS[name]
    raises = tuple(raises) + tuple(SYNC_SCENARIOS[name][2])               # this site's ``run`` reports nothing: every error is raised
    wav_dir, model = corpus(root, n), os.path.join(root, "model")
    for i in missing:
        os.remove(os.path.join(wav_dir, f"u{i}.wav"))
    shutil.rmtree(model, ignore_errors=True)
    os.makedirs(model)
    torch.save({}, os.path.join(model, "multimodal_ser.pt"))
    names = [f"u{i}.wav" for i in range(n)]
    test_csv, txt = os.path.join(root, "test.csv"), os.path.join(root, "txt.csv")
    with open(test_csv, "w") as f:
        f.write("FileName\n" + "".join(f"{x}\n" for x in names))
    with open(txt, "w") as f:
        f.write("FileName,transcription\n" + "".join(f"{x},text of {x}\n" for x in names if (x, name) != ("u3.wav", "file_fails_to_load")))
    calls = []

    class Predictor:
        def __init__(self, streams, head_sd, head_mode):
            pass

        def predict(self, waves, ids, mask, rows):
            who = [name_of(len(w)) for w in waves]
            calls.append(f"run({' '.join(who)}; tokens {ids})")
            bad = [w for w in who if int(w[1:]) in raises]
            if bad:
                raise RuntimeError(f"predict of {' '.join(bad)} failed")
            return np.stack([np.arange(8, dtype=np.float32) * 0.25 + int(w[1:]) for w in who])

    geo_a, geo_t = C.TINY_WAVLM, C.TINY_ROBERTA
    config = dict(model_path=model, wav_dir=wav_dir, txt_dir=txt, feat1_dim=geo_a.hidden, feat2_dim=geo_t.hidden)
    enc = SimpleNamespace(mode_name="stub")
    with mock.patch("torch.cuda.is_available", lambda: True), mock.patch.object(P, "FusionPredictor", Predictor), \
            mock.patch.object(P, "_stream_kinds", lambda *a: [geo_a, geo_t]), \
            mock.patch("interspeech_ser_amd.driver.find_weights", lambda *a, **k: ({}, "stub")), \
            mock.patch("interspeech_ser_amd.engine.build_encoder", lambda *a, **k: enc), \
            mock.patch("torch.cuda.manual_seed_all", lambda s: None):
        res, raised, lines, pool_lines = _record(lambda: P.score_from_wav(
            config, ["audio", "text"], test_csv=test_csv, batch_size=2, num_workers=2, device="cpu",
            tokenize=lambda texts: (list(texts), None)), root)
    with open(os.path.join(model, "results", "test.csv")) as f:
        table = f.read().splitlines()
    return dict(calls=calls, lines=lines, pool_lines=pool_lines, raised=raised, n=res["n"], failed=res["failed"], csv=table)


def transcribe_scenario(root, name):
    from interspeech_ser_amd import transcribe as T
    first_batch = 1 if name == "first_batch_1" else 0
    key = "2_batches" if name in ("first_batch_1", "crop") else name
    n, (_, reports, raises) = _scaled(SYNC_SCENARIOS[key][0], SYNC_SCENARIOS[key][1:], T.BATCH)
    calls = []
    waves = [np.zeros(BASE + 100 * i, dtype=np.float32) for i in range(n)]
    if name == "crop":
        waves[1] = np.zeros(T.N_SAMPLES + 5, dtype=np.float32)
    who = lambda k: "u999" if k == T.N_SAMPLES else name_of(k)           # noqa: E731  (u999: the file cut to 30 s)

    class Enc:
        def upload(self, ws, slot):
            calls.append(f"upload({' '.join(who(len(w)) for w in ws)}; slot {slot})")
            return [who(len(w)) for w in ws]

        def forward(self, dev, lengths, slot):
            return SimpleNamespace(states=[None, dev], take_range_bits=lambda: 0)

    class Dec:
        def generate(self, state, B, spec, slot):
            calls.append(f"run({' '.join(state)}; slot {slot})")
            bad = [w for w in state if int(w[1:]) in raises]
            if bad:
                raise RuntimeError(f"generate of {' '.join(bad)} failed")
            err = sum(1 << (int(w[1:]) % 8) for w in state if int(w[1:]) in reports)
            return SimpleNamespace(failed=bool(err), err=err, range_bits=2 * bool(err), lists=[[int(w[1:]), 7] for w in state],
                                   languages=[100 + int(w[1:]) for w in state])

    tr = T.WhisperTranscriber(Enc(), Dec(), None)
    names = [f"u{i}.wav" for i in range(n)] if name != "1_batch_of_one" else None      # without names the lines say "utterance i"
    out, raised, lines, pool_lines = _record(lambda: tr.transcribe(waves, names, first_batch=first_batch), root)
    return dict(calls=calls, lines=lines, pool_lines=pool_lines, raised=raised, out=out, last_languages=tr.last_languages)


def scenarios():
    """(site, scenario, function) of everything recorded"""
    out = [("driver", k, driver_scenario) for k in list(PIPE_SCENARIOS) + list(DRIVER_ONLY)]
    out += [("baseline", k, baseline_scenario) for k in list(PIPE_SCENARIOS) + list(BASELINE_ONLY) if not k.startswith("not_pipelined")]
    sync = [k for k in SYNC_SCENARIOS]
    out += [("run_hip", k, run_hip_scenario) for k in sync] + [("run_hip", "trimodal", lambda r, k: run_hip_scenario(r, "2_batches", 3))]
    out += [("score_from_wav", k, score_from_wav_scenario) for k in sync]
    out += [("transcribe", k, transcribe_scenario) for k in sync if "load" not in k] + [("transcribe", k, transcribe_scenario) for k in ("first_batch_1", "crop")]
    return out


def run_scenario(site, name, fn):
    root = tempfile.mkdtemp(prefix="batch_loops_")
    try:
        return json.loads(json.dumps(fn(root, name)))                   # as the file holds it: tuples are lists there
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    traces = {}
    for site, name, fn in scenarios():
        traces.setdefault(site, {})[name] = run_scenario(site, name, fn)
    with open(GOLDEN, "w") as f:
        json.dump(traces, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in traces.values())} scenarios written to {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
