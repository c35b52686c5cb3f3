"""Hub audio-classification checkpoints, from waveform to logits: what ``AutoModelForAudioClassification`` runs for a snapshot whose
``config.json`` names ``Wav2Vec2ForSequenceClassification``, ``WavLMForSequenceClassification``, ``HubertForSequenceClassification``,
``Data2VecAudioForSequenceClassification``, ``Wav2Vec2BertForSequenceClassification`` or ``WhisperForAudioClassification``.

The encoder is the extraction drivers'; the head (optional softmax-weighted layer sum, projector, mean over the frames, classifier) runs on
the device behind it (engine.ClassifierHead), so what comes back per utterance is ``num_labels`` floats.

Semantics: every utterance alone.  The logits of a file are those of the HF class given that file at batch size 1 with no padding,
whatever else shares its ragged batch -- for the GroupNorm-stem base models, whose feature extractor returns no attention mask, the only
well-defined meaning.  Input normalisation follows the snapshot's ``preprocessor_config.json`` (``do_normalize``), as in the speech driver.
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
from .frontend import RESAMPLE_MAX_R, TARGET_SR, UnsupportedAudio, decode_wav, host_resample, resample_ratio

MODES = ("f16mf", "f16x", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16")


class AudioClassifier(_Extractor):
    """Encoder + classification head on one GPU.  ``submit`` / ``collect`` are the extraction pipeline's with the head behind the
    forward: the slot's D2H copy is the ``[B, num_labels]`` logits.  ``state_dict``: the checkpoint under normalised names
    (``weights.load_checkpoint``), encoder and head tensors together."""

    def __init__(self, geo, spec, state_dict, device: str = "cuda:0", mode: str = "f16x", batch_size: int = 16, normalize: bool = True):
        from .engine import ClassifierHead, build_encoder
        from .weights import split_classifier_head
        if spec is None:
            raise ValueError("not an audio-classification checkpoint (config.json names none of " + ", ".join(C.AUDIO_CLASSIFICATION_ARCHITECTURES) + ")")
        if geo.family not in C.SPEECH_FAMILIES + (C.FAMILY_W2V_BERT, C.FAMILY_W2V_CONFORMER, C.FAMILY_WHISPER):
            raise ValueError(f"{geo.name}: the {geo.family} encoder has no audio-classification head")
        self.geo, self.spec, self.whisper = geo, spec, geo.family == C.FAMILY_WHISPER
        self.average, self.layer_index = False, geo.num_layers           # the extraction pipeline's selection: the full forward
        self.mode = self.supported_mode(geo, mode, self.whisper, geo.name)
        enc_sd, head_sd = split_classifier_head(state_dict)
        self.enc = build_encoder(geo, enc_sd, device, self.mode, normalize=normalize)
        self.head = ClassifierHead(self.enc, head_sd, spec)
        self.num_labels, self.labels = spec.num_labels, tuple(spec.labels)
        self.batch_size = max(1, int(batch_size))
        self.failed: List[tuple] = []                                    # (index, error) of the last ``predict``

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        """what ``submit`` copies to the host: the ``[B, num_labels]`` logits of the head, enqueued behind the forward on the slot's stream"""
        return self.head.forward(hs, slot=slot)

    def extract(self, waves: List[np.ndarray], layer_index=None, rates=None) -> np.ndarray:
        """One ragged batch -> ``[B, num_labels]`` logits, synchronously (slot 0)."""
        dev, lengths = self.upload_resampled(waves, rates)
        hs = self.enc.forward(dev, lengths)
        out = self.select(hs, None)
        bits = hs.take_range_bits()
        host = out.cpu().numpy().copy()
        self._check_range(bits)
        return host

    def submit(self, waves: List[np.ndarray], layer_index=None, slot: int = 0, rates=None):
        return super().submit(waves, None, slot, rates)                 # last_state None: the head reads every state

    def collect(self, ticket) -> np.ndarray:
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))
        return ticket["host"].numpy().copy()

    def predict(self, waves: Sequence[np.ndarray]) -> np.ndarray:
        """16 kHz mono waveforms -> ``[n, num_labels]`` float32 logits, in order, through the two-slot pipeline.  A batch that fails
        (the fp16 range guard, a waveform below the encoder's shortest input) is retried item by item; an item that still fails is
        printed, listed in ``self.failed`` as (index, error), and its row is NaN."""
        waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in waves]
        out = np.full((len(waves), self.num_labels), np.nan, dtype=np.float32)
        self.failed = []

        def fail(item, err):
            self.failed.append((item[0], err))
            print(f"Failed to process item {item[0]}: {err}")

        def done(good, rows, ticket):
            for (i, _), row in zip(good, rows):
                out[i] = row

        if torch.cuda.is_available():
            torch.cuda.synchronize()                          # slot 0's arena is shared with the synchronous path
        pipe = SlotPipeline(submit=lambda good, slot: self.submit([w for _, w in good], None, slot=slot), collect=self.collect,
                            extract=lambda good: self.extract([w for _, w in good]), slots=self.SLOTS, done=done, fail=fail,
                            before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
        for bi, batch in enumerate(make_batches(list(enumerate(waves)), self.batch_size)):
            pipe.push(bi, batch)
            pipe.drain()
        pipe.drain(0)
        return out


# ------------------------------------------------------------------------------- CLI
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Logits and labels of a hub audio-classification checkpoint for every wav file of a directory")
    p.add_argument("--model", type=str, required=True, help="hub id (offline HF cache) or local snapshot directory")
    p.add_argument("--wav_dir", type=str, required=True)
    p.add_argument("--out_csv", type=str, required=True)
    p.add_argument("--mode", type=str, default="f16x", choices=list(MODES))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resample", action="store_true", help="accept non-16 kHz wav files (resampled on the GPU ahead of the forward)")
    p.add_argument("--checkpoint", type=str, default="", help="local *.safetensors / pytorch_model.bin (or directory) instead of --model's weights")
    p.add_argument("--num_workers", type=int, default=4)
    return p


def _build_classifier(args, device: str) -> AudioClassifier:
    """The shared load path of the drivers: config.json -> geometry and head spec, weights by ``find_weights``."""
    geo = C.resolve_geometry(args.model, args.checkpoint)
    geo = C.resolve_fbank(geo, args.model, args.checkpoint)
    spec = C.resolve_classifier(args.model, args.checkpoint)
    if spec is None:
        raise OSError(f"{args.model} is not an audio-classification checkpoint (its config.json names none of "
                      + ", ".join(C.AUDIO_CLASSIFICATION_ARCHITECTURES) + ")")
    sd, source = find_weights(args.model, args.checkpoint, False, 0, geo)
    whisper = geo.family == C.FAMILY_WHISPER
    normalize = True if whisper else C.resolve_do_normalize(args.model, args.checkpoint)
    ex = AudioClassifier(geo, spec, sd, device, args.mode, args.batch_size, normalize=normalize)
    ex.weight_source = source
    return ex


def format_rows(labels: Sequence[str], names: Sequence[str], logits):
    """(header, rows in the sorted order of the names): FileName, the label of the argmax, the logits in index order."""
    rows = [[name, labels[int(np.argmax(row))]] + [repr(float(np.float32(x))) for x in np.asarray(row).reshape(-1)]
            for name, row in zip(names, logits)]
    rows.sort(key=lambda r: r[0])
    return ["FileName", "label"] + [str(l) for l in labels], rows


def run_classify(argv: Optional[Sequence[str]] = None, classifier_factory=None) -> int:
    """``classifier_factory(args, device)`` replaces the model (the host tests hand in a stub with ``submit`` / ``collect`` / ``extract`` /
    ``labels``): everything around the model call then runs without a GPU."""
    args = build_parser().parse_args(argv)
    device = "cuda:0" if torch.cuda.is_available() else "cpu"
    try:
        names = sorted(fn for fn in os.listdir(args.wav_dir) if os.path.isfile(os.path.join(args.wav_dir, fn)))
    except OSError as e:
        print(f"Error reading {args.wav_dir}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"{len(names)} file are going to be processed...")
    if device == "cpu" and classifier_factory is None:
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    try:
        ex = (classifier_factory or _build_classifier)(args, device)
    except (OSError, NotImplementedError) as e:
        print(f"Error: No pretrained model found with the name {args.model}")
        print(f"  ({e})")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    print(f"Weights: {getattr(ex, 'weight_source', 'caller')}; numerics mode {getattr(ex, 'mode', args.mode)}; {len(ex.labels)} labels")
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

    done: List[str] = []
    logits: List[np.ndarray] = []
    failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(args.wav_dir, name)}: {err}")

    def finished(good, out, ticket):
        for (name, _), row in zip(good, out):
            done.append(name)
            logits.append(np.asarray(row))

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
    print(f"{len(done)} utterances on 1 GPU(s) in {dt:.2f} s ({len(done) / max(dt, 1e-9):.1f} utt/s)")
    header, rows = format_rows(ex.labels, done, logits)
    out_dir = os.path.dirname(os.path.abspath(args.out_csv))
    os.makedirs(out_dir, exist_ok=True)
    with open(args.out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)
    print(f"{len(rows)} rows written to {args.out_csv}; {failed} files failed")
    return 0
