"""Waveforms -> Whisper's own transcript on one device: ``WhisperEncoder`` and ``WhisperDecoder`` behind each other.

The reference makes its transcript table with ``AutoModelForSpeechSeq2Seq.generate(input_features)`` (test/Whisper transcriptions.ipynb ->
``whisper_transcripts.csv``, columns FileName, transcription); ``preprocess_roberta.py --df_path`` and the heads' ``txt_dir`` read it.
``WhisperTranscriber.transcribe`` returns the generated token ids, ``.texts`` what ``batch_decode(skip_special_tokens=True)`` makes of them,
``run`` (preprocessing/transcribe_whisper.py) writes the table.
"""
from __future__ import annotations

import argparse
import csv
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import make_batches, run_or_each

N_SAMPLES = 480000            # 30 s: WhisperFeatureExtractor cuts longer input, and so does this path
BATCH = 16


class WhisperTranscriber:
    """``transcribe(waves)``: per utterance the generated ids without the prompt, up to and excluding eos (None for a file that failed).
    Batches of ``BATCH`` alternate between the encoder's and decoder's two slots.  A batch whose fp16 range-guard word or decoder error
    word is set goes through ``batchloop.run_or_each``: retried file by file, a file that still fails is printed and left out.  What
    the encoder or the decoder raises is not caught."""

    def __init__(self, encoder, decoder, spec: C.GenerationSpec):
        self.enc, self.dec, self.spec = encoder, decoder, spec
        self.last_languages: List[Optional[int]] = []

    def _batch(self, waves: Sequence[np.ndarray], slot: int):
        """(DecodeResult, failed) of one batch; one encoder forward serves the decoder (its LAST state: the forward does not stop early)."""
        lengths = [len(w) for w in waves]
        hs = self.enc.forward(self.enc.upload(waves, slot), lengths, slot=slot)
        res = self.dec.generate(hs.states[-1], len(waves), self.spec, slot=slot)
        bits = hs.take_range_bits()
        return res, res.failed or bool(bits & 1), hs

    def transcribe(self, waves: Sequence[np.ndarray], names: Optional[Sequence[str]] = None, first_batch: int = 0) -> List[Optional[List[int]]]:
        """``first_batch``: the index of the first batch in the caller's own sequence of calls (a driver that hands over 16 files at a time
        keeps the slots alternating with it)."""
        waves = [np.ascontiguousarray(w[:N_SAMPLES], dtype=np.float32) for w in waves]
        names = list(names) if names is not None else [f"utterance {i}" for i in range(len(waves))]
        out: List[Optional[List[int]]] = [None] * len(waves)
        self.last_languages = [None] * len(waves)
        for n, idx in enumerate(make_batches(range(len(waves)), BATCH), start=int(first_batch)):
            def run(js):
                res, failed, _ = self._batch([waves[j] for j in js], n % 2)
                if failed:
                    return res
                for k, j in enumerate(js):
                    out[j], self.last_languages[j] = res.lists[k], int(res.languages[k])

            run_or_each(idx, run, lambda j, res: print(f"Failed to process {names[j]}: decoder error word {res.err:#x}, "
                                                       f"range-guard bits {res.range_bits:#x}"), catch=())
        return out

    def texts(self, waves: Sequence[np.ndarray], tokenizer, names: Optional[Sequence[str]] = None) -> List[Optional[str]]:
        """``tokenizer``: anything with HF's ``decode(ids, skip_special_tokens=True)``."""
        return [None if ids is None else tokenizer.decode(ids, skip_special_tokens=True) for ids in self.transcribe(waves, names)]


def load_tokenizer(name_or_path: str):
    """The checkpoint's tokenizer from local files (as the text drivers load theirs); None without vocabulary files."""
    try:
        from transformers import WhisperTokenizer
        return WhisperTokenizer.from_pretrained(name_or_path, local_files_only=True)
    except Exception as e:                                  # noqa: BLE001
        print(f"No tokenizer files for {name_or_path} ({type(e).__name__}): writing token ids instead of text")
        return None


def write_table(path: str, names: Sequence[str], texts: Sequence[str]) -> None:
    """The reference's transcript table: header FileName,transcription, one row per file."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["FileName", "transcription"])
        for n, t in zip(names, texts):
            w.writerow([n, t])


def read_table(path: str) -> dict:
    """FileName -> transcription: the loader of ``predictor.score_from_wav``, reading as ``preprocess_roberta.py`` does (pandas; as there,
    an empty transcription comes back as the string "nan")."""
    import pandas as pd
    df = pd.read_csv(path)
    return {str(f): str(t) for f, t in zip(df.FileName.values, df.transcription.values)}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Whisper transcripts of a wav directory -> the reference's transcript table")
    p.add_argument("--ssl_type", type=str, default="openai/whisper-large-v3")
    p.add_argument("--wav_dir", type=str, required=True)
    p.add_argument("--out_csv", type=str, required=True)
    p.add_argument("--language", type=str, default=None, help="e.g. en; default: detected per utterance, as generate() does")
    p.add_argument("--mode", type=str, default="f16x")
    p.add_argument("--checkpoint", type=str, default="")
    p.add_argument("--tokenizer_path", type=str, default="")
    p.add_argument("--resample", action="store_true", help="accept wav files that are not 16 kHz")
    p.add_argument("--synthetic_weights", action="store_true", help="seeded weights (benchmarks and tests; the generation spec then comes from run(spec=...) or a generation_config.json beside --checkpoint)")
    p.add_argument("--seed", type=int, default=0)
    return p


def build(args, device: str = "cuda:0", spec: Optional[C.GenerationSpec] = None, geo=None):
    """(WhisperTranscriber, tokenizer or None) for the command line's checkpoint."""
    from .driver import find_weights
    from .engine import WhisperDecoder, WhisperEncoder
    from .weights import synthetic_decoder_state_dict
    geo = geo or C.resolve_geometry(args.ssl_type, args.checkpoint)
    if geo.family != C.FAMILY_WHISPER or geo.decoder_layers < 1:
        raise OSError(f"{args.ssl_type} is not a whisper checkpoint with a decoder")
    sd, _ = find_weights(args.ssl_type, args.checkpoint, args.synthetic_weights, args.seed, geo)
    if args.synthetic_weights:
        sd = dict(sd)
        sd.update(synthetic_decoder_state_dict(geo, args.seed))
    if spec is None:
        cfg = C.find_config_json(args.ssl_type, args.checkpoint)
        if not cfg:
            raise OSError(f"no generation_config.json for {args.ssl_type} (it lies beside config.json in a local snapshot)")
        spec = C.GenerationSpec.from_snapshot(os.path.dirname(cfg), args.language)
    enc_mode = args.mode if args.mode in ("f16x", "fp32x", "bf16") else "f16x"
    enc = WhisperEncoder(geo, sd, device, enc_mode)
    dec = WhisperDecoder(geo, sd, device, args.mode, spec)
    tok = None if args.synthetic_weights else load_tokenizer(args.tokenizer_path or args.ssl_type)
    return WhisperTranscriber(enc, dec, spec), tok


def run(argv: Optional[Sequence[str]] = None, spec: Optional[C.GenerationSpec] = None, geo=None, tokenizer=None) -> int:
    from .frontend import load_wav_16k
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        print("Error: no MI355X visible -- this build has no CPU path")
        return 0
    try:
        tr, tok = build(args, spec=spec, geo=geo)
    except OSError as e:
        print(f"Error: No pretrained model found with the name {args.ssl_type}")
        print(f"  ({e})")
        return 0
    tok = tokenizer or tok
    names = sorted(f for f in os.listdir(args.wav_dir) if f.lower().endswith(".wav"))
    rows = []
    for i in range(0, len(names), BATCH):
        chunk, waves = [], []
        for n in names[i:i + BATCH]:
            try:
                waves.append(load_wav_16k(os.path.join(args.wav_dir, n), resample=args.resample))
                chunk.append(n)
            except Exception as e:                          # noqa: BLE001
                print(f"Failed to process {n}: {e}")
        for n, ids in zip(chunk, tr.transcribe(waves, chunk, first_batch=i // BATCH)):
            if ids is not None:
                rows.append((n, tok.decode(ids, skip_special_tokens=True) if tok is not None else " ".join(str(t) for t in ids)))
    write_table(args.out_csv, [r[0] for r in rows], [r[1] for r in rows])
    print(f"Wrote {len(rows)} of {len(names)} transcripts to {args.out_csv}")
    return 0
