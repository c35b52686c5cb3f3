"""Hub x-vector checkpoints, from waveform to speaker embedding: what ``AutoModelForAudioXVector`` runs for a snapshot whose
``config.json`` names ``Wav2Vec2ForXVector``, ``WavLMForXVector``, ``Data2VecAudioForXVector`` or ``Wav2Vec2BertForXVector``
(microsoft/wavlm-base-sv, microsoft/wavlm-base-plus-sv, anton-l/wav2vec2-base-superb-sv).

The encoder is the extraction drivers'; the head (optional softmax-weighted layer sum, projector, ReLU TDNN layers, statistics pooling,
feature_extractor, classifier) runs on the device behind it (engine.XVectorHead), so what comes back per utterance is
``xvector_output_dim`` floats -- HF's ``embeddings``, un-normalised -- and the classifier's logits.

Semantics: every utterance alone.  The embedding of a file is that of the HF class given that file at batch size 1 with no padding,
whatever else shares its ragged batch.  (HF's masked branch takes its lengths from ``_get_tdnn_output_lengths``, which ignores the
dilation; at batch size 1 that slice is longer than the tensor and clamps to all T' rows, so masked and unmasked agree there.)  An
utterance whose TDNN output has fewer than two rows has no unbiased std: it fails alone.
"""
from __future__ import annotations

import argparse
import csv
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import SlotPipeline, make_batches, prefetch
from .driver import _Extractor, find_weights
from .frontend import RESAMPLE_MAX_R, TARGET_SR, UnsupportedAudio, decode_wav, host_resample, resample_ratio, tmp_name

MODES = ("f16mf", "f16x", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16")
HEAD_MODES = ("f16x", "fp32x", "bf16")


def head_mode(mode: str, name: str) -> str:
    """``mode``, or "f16x" where the x-vector head has no such mode (said in one printed line)"""
    if mode not in HEAD_MODES:
        print(f"--mode {mode} is not implemented for the x-vector head ({name}): using f16x")
        return "f16x"
    return mode


class SpeakerEmbedder(_Extractor):
    """Encoder + x-vector head on one GPU.  ``submit`` / ``collect`` are the extraction pipeline's with the head behind the forward: the
    slot's D2H copy is ``[B, xvector_output_dim + num_labels]``, embeddings then logits.  ``state_dict``: the checkpoint under normalised
    names (``weights.load_checkpoint``), encoder and head tensors together."""

    def __init__(self, geo, spec, state_dict, device: str = "cuda:0", mode: str = "f16x", batch_size: int = 16, normalize: bool = True):
        from .engine import XVectorHead, build_encoder
        from .weights import split_xvector_head
        if spec is None:
            raise ValueError("not an x-vector checkpoint (config.json names none of " + ", ".join(C.XVECTOR_ARCHITECTURES) + ")")
        if geo.family not in C.SPEECH_FAMILIES + (C.FAMILY_W2V_BERT,):
            raise ValueError(f"{geo.name}: the {geo.family} encoder has no x-vector head")
        self.geo, self.spec, self.whisper = geo, spec, False
        self.average, self.layer_index = False, geo.num_layers           # the extraction pipeline's selection: the full forward
        self.mode = self.supported_mode(geo, head_mode(mode, geo.name), False, geo.name)
        enc_sd, head_sd = split_xvector_head(state_dict)
        self.enc = build_encoder(geo, enc_sd, device, self.mode, normalize=normalize)
        self.head = XVectorHead(self.enc, head_sd, spec)
        self.dim, self.num_labels = self.head.dim, self.head.n_out
        self.batch_size = max(1, int(batch_size))
        self.failed: List[tuple] = []                                    # (index, error) of the last ``embed``
        self.logits: Optional[np.ndarray] = None                         # [n, num_labels] of the last ``embed(..., with_logits=True)``

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        """what ``submit`` copies to the host: the head's ``[B, dim + num_labels]`` rows, enqueued behind the forward on the slot's stream"""
        return self.head.forward_rows(hs, slot=slot)

    def extract(self, waves: List[np.ndarray], layer_index=None, rates=None) -> np.ndarray:
        """One ragged batch -> ``[B, dim + num_labels]`` (embeddings | logits), synchronously (slot 0)."""
        dev, lengths = self.upload_resampled(waves, rates)
        hs = self.enc.forward(dev, lengths)
        out = self.select(hs, None)
        bits = hs.take_range_bits()
        host = out.cpu().numpy().copy()
        self._check_range(bits)
        return host

    def submit(self, waves: List[np.ndarray], layer_index=None, slot: int = 0, rates=None):
        return super().submit(waves, None, slot, rates)                 # last_state None: the head may read every state

    def collect(self, ticket) -> np.ndarray:
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))
        return ticket["host"].numpy().copy()

    def embed(self, waves: Sequence[np.ndarray], with_logits: bool = False) -> np.ndarray:
        """16 kHz mono waveforms -> ``[n, xvector_output_dim]`` float32 embeddings, in order, through the two-slot pipeline; with
        ``with_logits`` the classifier's ``[n, num_labels]`` are left in ``self.logits``.  A batch that fails (an utterance too short for
        the TDNN stack, the fp16 range guard) is retried item by item; an item that still fails is printed, listed in ``self.failed`` as
        (index, error), and its row is NaN."""
        waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in waves]
        rows = np.full((len(waves), self.dim + self.num_labels), np.nan, dtype=np.float32)
        self.failed = []

        def fail(item, err):
            self.failed.append((item[0], err))
            print(f"Failed to process item {item[0]}: {err}")

        def done(good, got, ticket):
            for (i, _), row in zip(good, got):
                rows[i] = row

        if torch.cuda.is_available():
            torch.cuda.synchronize()                          # slot 0's arena is shared with the synchronous path
        pipe = SlotPipeline(submit=lambda good, slot: self.submit([w for _, w in good], None, slot=slot), collect=self.collect,
                            extract=lambda good: self.extract([w for _, w in good]), slots=self.SLOTS, done=done, fail=fail,
                            before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
        for bi, batch in enumerate(make_batches(list(enumerate(waves)), self.batch_size)):
            pipe.push(bi, batch)
            pipe.drain()
        pipe.drain(0)
        self.logits = np.ascontiguousarray(rows[:, self.dim:]) if with_logits else None
        return np.ascontiguousarray(rows[:, : self.dim])


# ------------------------------------------------------------------------------- CLI
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="x-vector speaker embeddings of a hub AutoModelForAudioXVector checkpoint for every wav file of a directory")
    p.add_argument("--model", type=str, required=True, help="hub id (offline HF cache) or local snapshot directory")
    p.add_argument("--wav_dir", type=str, required=True)
    p.add_argument("--save_path", type=str, required=True, help="directory of the <utt>.pt files ([xvector_output_dim] float32 each)")
    p.add_argument("--mode", type=str, default="f16x", choices=list(MODES))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resample", action="store_true", help="accept non-16 kHz wav files (resampled on the GPU ahead of the forward)")
    p.add_argument("--checkpoint", type=str, default="", help="local *.safetensors / pytorch_model.bin (or directory) instead of --model's weights")
    p.add_argument("--trials", type=str, default="", help="text file of 'fileA fileB' lines to score by cosine similarity")
    p.add_argument("--scores_csv", type=str, default="", help="where --trials writes fileA,fileB,cosine")
    p.add_argument("--num_workers", type=int, default=4)
    return p


def _build_embedder(args, device: str) -> SpeakerEmbedder:
    """The shared load path of the drivers: config.json -> geometry and head spec, weights by ``find_weights``."""
    spec = C.resolve_xvector(args.model, args.checkpoint)             # first: an x-vector class over an unbuilt encoder is named as such
    if spec is None:
        raise OSError(f"{args.model} is not an x-vector checkpoint (its config.json names none of " + ", ".join(C.XVECTOR_ARCHITECTURES) + ")")
    geo = C.resolve_geometry(args.model, args.checkpoint)
    geo = C.resolve_fbank(geo, args.model, args.checkpoint)
    sd, source = find_weights(args.model, args.checkpoint, False, 0, geo)
    ex = SpeakerEmbedder(geo, spec, sd, device, args.mode, args.batch_size, normalize=C.resolve_do_normalize(args.model, args.checkpoint))
    ex.weight_source = source
    return ex


def save_embedding(row: np.ndarray, path: str) -> None:
    """``torch.save`` of a bare [dim] float32 CPU tensor, through libserhip's writer; under a temporary name, renamed when complete"""
    from ._lib import check, lib
    t = np.ascontiguousarray(np.asarray(row, dtype=np.float32).reshape(-1))
    tmp = tmp_name(path)
    try:
        check(lib.ser_pt_write_f32_vec(os.fsencode(tmp), t.ctypes.data, t.size), "ser_pt_write_f32_vec")
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


def utt_name(file_name: str) -> str:
    return os.path.splitext(file_name)[0]


def score_trials(trials_path: str, save_path: str, scores_csv: str) -> int:
    """Each line ``fileA fileB`` of ``trials_path`` -> ``fileA,fileB,cosine`` in ``scores_csv``; the cosine in float64 on the host from
    the saved embeddings.  A pair with a missing embedding is printed and left out.  Returns the number of rows written."""
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = torch.load(os.path.join(save_path, utt_name(name) + ".pt")).numpy().astype(np.float64)
        return cache[name]

    rows = []
    with open(trials_path, "r") as f:
        for line in f:
            pair = line.split()
            if not pair:
                continue
            if len(pair) != 2:
                print(f"Failed to score '{line.strip()}': a trial is 'fileA fileB'")
                continue
            try:
                a, b = load(pair[0]), load(pair[1])
            except (OSError, RuntimeError) as e:
                print(f"Failed to score {pair[0]} {pair[1]}: {e}")
                continue
            rows.append([pair[0], pair[1], repr(float(np.dot(a, b) / (np.sqrt(np.dot(a, a)) * np.sqrt(np.dot(b, b)))))])
    os.makedirs(os.path.dirname(os.path.abspath(scores_csv)), exist_ok=True)
    with open(scores_csv, "w", newline="") as f:
        csv.writer(f).writerows(rows)
    return len(rows)


def run_embed(argv: Optional[Sequence[str]] = None, embedder_factory=None) -> int:
    """``embedder_factory(args, device)`` replaces the model (the host tests hand in a stub with ``submit`` / ``collect`` / ``extract`` /
    ``dim``): everything around the model call then runs without a GPU."""
    args = build_parser().parse_args(argv)
    if bool(args.trials) != bool(args.scores_csv):
        print("Error: --trials and --scores_csv go together")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    device = "cuda:0" if torch.cuda.is_available() else "cpu"
    try:
        names = sorted(fn for fn in os.listdir(args.wav_dir) if os.path.isfile(os.path.join(args.wav_dir, fn)))
    except OSError as e:
        print(f"Error reading {args.wav_dir}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"{len(names)} file are going to be processed...")
    if device == "cpu" and embedder_factory is None:
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    try:
        ex = (embedder_factory or _build_embedder)(args, device)
    except (OSError, NotImplementedError) as e:
        print(f"Error: No pretrained model found with the name {args.model}")
        print(f"  ({e})")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"Weights: {getattr(ex, 'weight_source', 'caller')}; numerics mode {getattr(ex, 'mode', args.mode)}; {ex.dim}-dimensional embeddings")
    os.makedirs(args.save_path, exist_ok=True)
    gpu_resample = args.resample and hasattr(ex, "upload_resampled")

    def decode(name):
        """(name, (samples, their rate), None) or (name, None, error)."""
        path = os.path.join(args.wav_dir, name)
        try:
            x, sr = decode_wav(path)
            if sr != TARGET_SR:
                if not args.resample:
                    raise UnsupportedAudio(f"sample rate {sr} Hz: only {TARGET_SR} Hz input is supported (--resample converts)")
                if not gpu_resample or max(resample_ratio(sr)) > RESAMPLE_MAX_R:
                    x, sr = host_resample(x, sr), TARGET_SR
            return name, (x, sr), None
        except Exception as e:                              # noqa: BLE001  (per-file failure, as in the extraction drivers)
            return name, None, e

    written = failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(args.wav_dir, name)}: {err}")

    def finished(good, out, ticket):
        nonlocal written
        for (name, _), row in zip(good, out):
            try:
                save_embedding(np.asarray(row)[: ex.dim], os.path.join(args.save_path, utt_name(name) + ".pt"))
                written += 1
            except Exception as e:                          # noqa: BLE001
                fail(name, e)

    def run(fn, good, **k):
        waves = [w for _, (w, _) in good]
        return fn(waves, None, rates=[sr for _, (_, sr) in good], **k) if gpu_resample else fn(waves, None, **k)

    pipe = SlotPipeline(submit=lambda good, slot: run(ex.submit, good, slot=slot), collect=ex.collect, extract=lambda good: run(ex.extract, good),
                        slots=getattr(ex, "SLOTS", 2), done=finished, fail=lambda item, err: fail(item[0], err),
                        before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        for bi, decoded in enumerate(prefetch(make_batches(names, max(1, args.batch_size)), pool, decode)):
            good = []
            for name, item, err in decoded:
                if err is not None:
                    fail(name, err)
                else:
                    good.append((name, item))
            if good:
                pipe.push(bi, good)
            pipe.drain()
        pipe.drain(0)
    dt = time.perf_counter() - t0
    print(f"{written} utterances on 1 GPU(s) in {dt:.2f} s ({written / max(dt, 1e-9):.1f} utt/s)")
    print(f"{written} embeddings written to {args.save_path}; {failed} files failed")
    if args.trials:
        try:
            n = score_trials(args.trials, args.save_path, args.scores_csv)
        except OSError as e:
            print(f"Error reading {args.trials}: {e}")
            return 0
        print(f"{n} trials scored to {args.scores_csv}")
    return 0
