"""Emotion predictions of the challenge organisers' baseline: the counterparts of the reference's
benchmark/train_eval_files/eval_cat_ser.py (8 classes) and eval_dim_ser.py (arousal / valence / dominance).

The reference runs, one file at a time: fine-tuned WavLM -> ``last_hidden_state`` -> AttentiveStatisticsPooling
(benchmark/net/pooling.py) -> EmotionRegression (benchmark/net/ser.py) -> ``<model_path>/results/test3.csv``.  Here the files
go through ragged batches on the two-slot pipeline of the extraction drivers, the pooling and the head run on the device behind
the encoder (engine.PoolHead), and what comes back per utterance is ``n_out`` floats instead of a ``[T, D]`` matrix.

What is kept from the reference (eval_cat_ser.py:95-111,164-200, eval_dim_ser.py:127-146, utils/dataset/dataset.py:143-206):
* the files are the names in ``config["wav_dir"]`` that contain ``test3`` (``--subset``), cut to their first 12 s (192 000 samples);
* the input is ``(wav - wav_mean) / (wav_std + 0.000001)`` with the two scalars of ``<model_path>/train_norm_stat.pkl`` -- NOT the
  per-utterance normalisation of the extraction drivers;
* cat: the letter of the argmax out of ``A,S,H,U,F,D,C,N``; dim: ``min(max(1, v * 6 + 1), 7)`` with EmoVal = pred[2] and
  EmoDom = pred[1] (eval_dim_ser.py:136); rows sorted by FileName;
* the label file named by the config is never read (the reference builds class weights from it and does not use them).

Trusted inputs: ``train_norm_stat.pkl`` is a pickle and is unpickled as the reference does; ``final_*.pt`` are read with
``torch.load(..., weights_only=True)``.  Parity of this path is established on synthetic weights only.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import pickle
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import SlotPipeline, make_batches, prefetch
from .driver import _Extractor
from .frontend import TARGET_SR, UnsupportedAudio, decode_wav

MAX_SAMPLES = 12 * TARGET_SR                        # utils/dataset/dataset.py: min(longest file, 12 s)
CAT_LETTERS = ("A", "S", "H", "U", "F", "D", "C", "N")
POOLING_TYPES = ("AttentiveStatisticsPooling",)
SSL_BOOK = {"wavlm-large": "microsoft/wavlm-large", "wavlm-base": "microsoft/wavlm-base"}     # utils/etc.py get_ssl_type
POOL_KEYS = ("attention", "sap_linear.weight", "sap_linear.bias")
SER_KEYS = ("fc.0.0.weight", "fc.0.0.bias", "fc.0.1.weight", "fc.0.1.bias", "out.0.weight", "out.0.bias")
N_OUT = {"cat": 8, "dim": 3}


class HeadError(ValueError):
    """a model directory this driver refuses, with the reason"""


def scale_wave(wav: np.ndarray, wav_mean, wav_std) -> np.ndarray:
    """The reference's input scaling (WavSet.__getitem__), then the ``.float()`` of its evaluation loop."""
    return ((wav - wav_mean) / (wav_std + 0.000001)).astype(np.float32)


def cut_wave(wav: np.ndarray) -> np.ndarray:
    return wav[:MAX_SAMPLES]


def check_head_state_dicts(pool_sd, ser_sd, D: int, head_dim: int, n_out: int) -> None:
    """Names and shapes of ``final_pool.pt`` / ``final_ser.pt`` against the encoder width, ``--head_dim`` and the task."""
    if any(k.startswith("fc.1.") for k in ser_sd):
        raise HeadError("final_ser.pt has more than one hidden layer (fc.1.*); the reference's evaluation scripts build one")
    for name, sd, keys in (("final_pool.pt", pool_sd, POOL_KEYS), ("final_ser.pt", ser_sd, SER_KEYS)):
        if sorted(sd) != sorted(keys):
            raise HeadError(f"{name}: keys {sorted(sd)} (expected {sorted(keys)})")
    want = {"attention": (D, 1), "sap_linear.weight": (D, D), "sap_linear.bias": (D,),
            "fc.0.0.weight": (head_dim, 2 * D), "fc.0.0.bias": (head_dim,), "fc.0.1.weight": (head_dim,), "fc.0.1.bias": (head_dim,),
            "out.0.weight": (n_out, head_dim), "out.0.bias": (n_out,)}
    for sd in (pool_sd, ser_sd):
        for k, v in sd.items():
            if tuple(v.shape) != want[k]:
                raise HeadError(f"{k}: shape {tuple(v.shape)}, expected {want[k]} (hidden width {D}, --head_dim {head_dim}, {n_out} outputs)")


def check_pooling_type(pooling_type: str) -> None:
    if pooling_type not in POOLING_TYPES:
        raise HeadError(f"--pooling_type {pooling_type}: only {', '.join(POOLING_TYPES)} is implemented")


def load_baseline_head(model_path: str, D: int, head_dim: int, n_out: int, pooling_type: str = POOLING_TYPES[0]):
    """(pool state dict, head state dict, wav_mean, wav_std) of a model directory of the reference's baseline trainers."""
    check_pooling_type(pooling_type)
    pool_sd = torch.load(os.path.join(model_path, "final_pool.pt"), map_location="cpu", weights_only=True)
    ser_sd = torch.load(os.path.join(model_path, "final_ser.pt"), map_location="cpu", weights_only=True)
    check_head_state_dicts(pool_sd, ser_sd, D, head_dim, n_out)
    with open(os.path.join(model_path, "train_norm_stat.pkl"), "rb") as f:          # a pickle: a trusted input, as in the reference
        stat = pickle.load(f)
    if not isinstance(stat, (tuple, list)) or len(stat) != 2:
        raise HeadError(f"train_norm_stat.pkl holds {type(stat).__name__}, expected the pair (wav_mean, wav_std)")
    return pool_sd, ser_sd, stat[0], stat[1]


def synthetic_head_state_dicts(D: int, head_dim: int, n_out: int, seed: int = 0):
    """Seeded pooling / head weights of the reference's names and shapes (``--synthetic_weights``, tests, benchmarks)."""
    g = np.random.default_rng(int(seed) + 7919)

    def n(*shape, std=1.0, mean=0.0):
        return torch.from_numpy((g.standard_normal(shape) * std + mean).astype(np.float32))
    pool = {"attention": n(D, 1), "sap_linear.weight": n(D, D, std=1.0 / np.sqrt(D)), "sap_linear.bias": n(D, std=0.1)}
    ser = {"fc.0.0.weight": n(head_dim, 2 * D, std=1.0 / np.sqrt(2 * D)), "fc.0.0.bias": n(head_dim, std=0.1),
           "fc.0.1.weight": n(head_dim, std=0.1, mean=1.0), "fc.0.1.bias": n(head_dim, std=0.1),
           "out.0.weight": n(n_out, head_dim, std=1.0 / np.sqrt(head_dim)), "out.0.bias": n(n_out, std=0.1)}
    return pool, ser


def resolve_ssl_type(ssl_type: str) -> C.EncoderGeometry:
    """The reference knows ``wavlm-large`` and ``wavlm-base`` (utils/etc.py); any other name must resolve to a speech encoder here."""
    try:
        geo = C.geometry_for(SSL_BOOK.get(ssl_type, ssl_type))
    except OSError:
        raise HeadError("Invalid SSL type!")
    if geo.family not in C.SPEECH_FAMILIES:
        raise HeadError("Invalid SSL type!")
    return geo


# ------------------------------------------------------------------------------- the model
class BaselinePredictor(_Extractor):
    """Encoder + pooling + head on one GPU.  ``submit`` / ``collect`` are the extraction pipeline's with the head behind the forward:
    the slot's D2H copy is the ``[B, n_out]`` logits.  Waveforms handed to ``submit`` / ``extract`` are already cut and scaled;
    ``predict`` takes raw 16 kHz waveforms."""

    def __init__(self, geo, ssl_sd, pool_sd, ser_sd, wav_mean, wav_std, device: str = "cuda:0", mode: str = "f16mf", batch_size: int = 16):
        from .engine import PoolHead, build_encoder
        self.geo, self.whisper = geo, False
        self.average, self.layer_index = False, geo.num_layers        # the extraction pipeline's selection: the last hidden state
        self.mode = self.supported_mode(geo, mode, False, geo.name)
        self.enc = build_encoder(geo, ssl_sd, device, self.mode, normalize=False)      # the model gets the scaled samples directly
        self.head = PoolHead(self.enc, pool_sd, ser_sd)
        self.n_out = self.head.n_out
        self.wav_mean, self.wav_std, self.batch_size = wav_mean, wav_std, max(1, int(batch_size))

    def prepare(self, wav: np.ndarray) -> np.ndarray:
        return np.ascontiguousarray(scale_wave(cut_wave(wav), self.wav_mean, self.wav_std))

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        """what ``submit`` copies to the host: the ``[B, n_out]`` logits of the head, enqueued behind the forward on the slot's stream"""
        return self.head.forward(hs, slot=slot)

    def extract(self, waves: List[np.ndarray], layer_index=None, rates=None) -> np.ndarray:
        """One ragged batch of prepared waveforms -> ``[B, n_out]`` logits, synchronously (slot 0)."""
        dev, lengths = self.upload_resampled(waves, None)
        hs = self.enc.forward(dev, lengths)
        out = self.select(hs, None)
        bits = hs.take_range_bits()
        host = out.cpu().numpy().copy()
        self._check_range(bits)
        return host

    def submit(self, waves: List[np.ndarray], layer_index=None, slot: int = 0, rates=None):
        return super().submit(waves, self.layer_index, slot, None)

    def collect(self, ticket) -> np.ndarray:
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))
        return ticket["host"].numpy().copy()

    def predict(self, waves: Sequence[np.ndarray]) -> np.ndarray:
        """Raw 16 kHz mono waveforms -> ``[n, n_out]`` float32 logits, in order.  Each is cut to 12 s and scaled with the model's
        statistics; a result does not depend on which other waveforms share its batch."""
        waves = [self.prepare(np.asarray(w, dtype=np.float32)) for w in waves]
        out = np.empty((len(waves), self.n_out), dtype=np.float32)
        if torch.cuda.is_available():
            torch.cuda.synchronize()                          # slot 0's arena is shared with the pipeline
        for i in range(0, len(waves), self.batch_size):
            out[i:i + self.batch_size] = self.extract(waves[i:i + self.batch_size])
        return out


def predict(predictor: BaselinePredictor, waves: Sequence[np.ndarray]) -> np.ndarray:
    """``predictor.predict(waves)``: logits ``[n, n_out]`` for waveforms held in memory."""
    return predictor.predict(waves)


# ------------------------------------------------------------------------------- CLI
def build_parser(kind: str) -> argparse.ArgumentParser:
    p = argparse.ArgumentParser()
    # the reference's flags, names and defaults unchanged (eval_cat_ser.py / eval_dim_ser.py)
    p.add_argument("--ssl_type", type=str, default="wavlm-large")
    p.add_argument("--model_path", type=str, default=f"./model/{kind}_ser/7/")
    p.add_argument("--pooling_type", type=str, default="AttentiveStatisticsPooling")
    p.add_argument("--head_dim", type=int, default=1024)
    p.add_argument("--store_path")                                      # parsed and unused, as in the reference
    # additive
    p.add_argument("--config_path", type=str, default=f"configs/config_{kind}.json", help="JSON with wav_dir (label_path is not read)")
    p.add_argument("--subset", type=str, default="test3", help="files whose name contains this tag; also the CSV's name")
    p.add_argument("--mode", type=str, default="f16mf", choices=["f16mf", "f16x", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16"])
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--synthetic_weights", action="store_true", help="seeded random encoder / pooling / head weights (benchmarking)")
    p.add_argument("--seed", type=int, default=7)
    return p


def _build_predictor(args, kind: str, device: str) -> BaselinePredictor:
    from .weights import load_checkpoint, synthetic_state_dict
    geo = resolve_ssl_type(args.ssl_type)
    n_out = N_OUT[kind]
    check_pooling_type(args.pooling_type)
    if args.synthetic_weights:
        ssl_sd = synthetic_state_dict(geo, args.seed)
        pool_sd, ser_sd = synthetic_head_state_dicts(geo.hidden, args.head_dim, n_out, args.seed)
        stat = os.path.join(args.model_path, "train_norm_stat.pkl")
        if os.path.isfile(stat):
            with open(stat, "rb") as f:
                wav_mean, wav_std = pickle.load(f)
        else:
            print(f"{stat} not found: synthetic weights run with wav_mean 0, wav_std 1")
            wav_mean, wav_std = 0.0, 1.0
    else:
        pool_sd, ser_sd, wav_mean, wav_std = load_baseline_head(args.model_path, geo.hidden, args.head_dim, n_out, args.pooling_type)
        ssl_sd = load_checkpoint(os.path.join(args.model_path, "final_ssl.pt"))
    return BaselinePredictor(geo, ssl_sd, pool_sd, ser_sd, wav_mean, wav_std, device, args.mode, args.batch_size)


def format_rows(kind: str, names: Sequence[str], logits: np.ndarray):
    """(header, rows sorted by FileName) of the reference's CSV."""
    rows = []
    for name, pred in zip(names, logits):
        if kind == "cat":
            rows.append([name, CAT_LETTERS[int(np.argmax(pred))]])
        else:
            v = [float(x) for x in pred]
            c = [min(max(1, x * 6 + 1), 7) for x in v]
            rows.append([name, c[0], c[2], c[1]])                       # EmoVal = pred[2], EmoDom = pred[1] (eval_dim_ser.py:136)
    rows.sort(key=lambda r: r[0])
    return (["FileName", "EmoClass"] if kind == "cat" else ["FileName", "EmoAct", "EmoVal", "EmoDom"]), rows


def _run_eval(argv: Optional[Sequence[str]], kind: str, predictor_factory=None) -> int:
    """``predictor_factory(args, kind, device)`` replaces the model (the host tests hand in a stub with ``prepare`` / ``submit`` /
    ``collect`` / ``extract`` / ``SLOTS``): everything around the model call then runs without a GPU."""
    args = build_parser(kind).parse_args(argv)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print("This driver is single-GPU, like the reference's evaluation scripts: run it as one process (WORLD_SIZE is "
              f"{os.environ['WORLD_SIZE']})")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    device = "cuda:0" if torch.cuda.is_available() else "cpu"
    try:
        with open(args.config_path, "r") as f:
            wav_dir = json.load(f)["wav_dir"]
        names = sorted(fn for fn in os.listdir(wav_dir) if args.subset in fn)
    except (OSError, ValueError, KeyError) as e:
        print(f"Error reading {args.config_path}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"{len(names)} {args.subset} files in {wav_dir}")
    if device == "cpu" and predictor_factory is None:
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"Loading pre-trained {args.ssl_type} model...")
    try:
        ex = (predictor_factory or _build_predictor)(args, kind, device)
    except (OSError, NotImplementedError, ValueError, KeyError, RuntimeError, TypeError, EOFError, pickle.UnpicklingError) as e:
        print(f"Error: cannot build the model from {args.model_path}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0

    def decode(name):
        path = os.path.join(wav_dir, name)
        try:
            x, sr = decode_wav(path)
            if sr != TARGET_SR:
                raise UnsupportedAudio(f"sample rate {sr} Hz: only {TARGET_SR} Hz input is supported")
            return name, ex.prepare(x), None
        except Exception as e:                              # noqa: BLE001  (per-file failure, as in the extraction drivers)
            return name, None, e

    done: List[str] = []
    logits: List[np.ndarray] = []
    failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(wav_dir, name)}: {err}")

    def finished(good, out, ticket):
        for (name, _), row in zip(good, out):
            done.append(name)
            logits.append(np.asarray(row))

    # the extraction drivers' slot pipeline (batchloop: a failed batch is retried per utterance, a file that still fails costs itself)
    pipe = SlotPipeline(submit=lambda good, slot: ex.submit([w for _, w in good], None, slot=slot), collect=ex.collect,
                        extract=lambda good: ex.extract([w for _, w in good]), slots=getattr(ex, "SLOTS", 2), done=finished,
                        fail=lambda item, err: fail(item[0], err),
                        before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        # the next batch is decoded while the GPU works
        for bi, decoded in enumerate(prefetch(make_batches(names, max(1, args.batch_size)), pool, decode)):
            good = []
            for name, wave, err in decoded:
                if err is not None:
                    fail(name, err)
                else:
                    good.append((name, wave))
            if good:
                pipe.push(bi, good)
            pipe.drain()
        pipe.drain(0)

    dt = time.perf_counter() - t0
    print(f"{len(done)} utterances on 1 GPU(s) in {dt:.2f} s ({len(done) / max(dt, 1e-9):.1f} utt/s)")
    header, rows = format_rows(kind, done, np.stack(logits) if logits else np.zeros((0, N_OUT[kind]), dtype=np.float32))
    out_dir = os.path.join(args.model_path, "results")
    os.makedirs(out_dir, exist_ok=True)
    csv_path = os.path.join(out_dir, args.subset + ".csv")
    with open(csv_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)
    print(f"{len(rows)} rows written to {csv_path}; {failed} files failed")
    return 0


def run_eval_cat(argv: Optional[Sequence[str]] = None, predictor_factory=None) -> int:
    return _run_eval(argv, "cat", predictor_factory)


def run_eval_dim(argv: Optional[Sequence[str]] = None, predictor_factory=None) -> int:
    return _run_eval(argv, "dim", predictor_factory)
