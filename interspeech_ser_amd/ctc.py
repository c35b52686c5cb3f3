"""Hub CTC checkpoints, from waveform to transcript: what ``AutoModelForCTC`` runs for a snapshot whose ``config.json`` names
``Wav2Vec2ForCTC``, ``HubertForCTC``, ``WavLMForCTC``, ``Data2VecAudioForCTC`` or ``Wav2Vec2BertForCTC`` (facebook/wav2vec2-base-960h,
facebook/hubert-large-ls960-ft, facebook/hubert-xlarge-ls960-ft, facebook/data2vec-audio-base-960h, ...), decoded greedily.

The encoder is the extraction drivers'; the head (lm_head, argmax per frame, equal neighbours merged, blanks dropped) runs on the device
behind it (engine.CTCHead), so what comes back per batch is one buffer of token ids, their frame offsets and the smallest margins.

Semantics: every utterance alone.  The ids of a file are those of the HF class given that file at batch size 1 with no padding and no
attention mask, then ``argmax(-1)``, whatever else shares its ragged batch.  Greedy only: no beams, no language model.  A CTC transcript
is not Whisper's: the 960h models write upper-case letters without punctuation.

Forced alignment (``CTCAligner``, ``run_align``) rides on the same forward: given an utterance and its KNOWN text (Whisper's transcript),
the best CTC path that spells it, found on the device (engine.CTCHead.forward_align, ser_ctc_align_v): where each character and word
starts and ends, and the mean log-probability the acoustic model gives it.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import config as C
from .batchloop import SlotPipeline, make_batches, prefetch
from .driver import _Extractor, find_weights
from .frontend import RESAMPLE_MAX_R, TARGET_SR, UnsupportedAudio, decode_wav, host_resample, resample_ratio
from .transcribe import write_table

MODES = ("f16mf", "f16x", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16")
HEAD_MODES = ("f16x", "fp32x", "bf16")


def head_mode(mode: str, name: str) -> str:
    """``mode``, or "f16x" where the CTC head has no such mode (said in one printed line)"""
    if mode not in HEAD_MODES:
        print(f"--mode {mode} is not implemented for the CTC head ({name}): using f16x")
        return "f16x"
    return mode


def frame_hop(geo) -> int:
    """samples between two encoder frames: the product of the conv strides (320), or the fbank hop times the frame stacking"""
    if geo.family == C.FAMILY_W2V_BERT:
        return 160 * int(geo.fbank_stride)
    hop = 1
    for s in geo.conv_stride:
        hop *= int(s)
    return hop


class Transcript:
    """One utterance's result: ``ids`` (collapsed, blanks dropped), ``offsets`` [(start frame, one past the run's last frame)] per id,
    ``min_margin`` (the smallest top1 - top2 over its frames)."""
    __slots__ = ("ids", "offsets", "min_margin")

    def __init__(self, ids: List[int], offsets: List[Tuple[int, int]], min_margin: float):
        self.ids, self.offsets, self.min_margin = ids, offsets, min_margin


def split_blob(words: np.ndarray, B: int, max_frames: int) -> List[Transcript]:
    """the per-utterance results of one batch's host copy (engine.CTCHead.unpack's layout); ``RuntimeError`` when the error word is set"""
    from .engine import CTCHead
    p = CTCHead.unpack(words, B, max_frames)
    if p["err"]:
        raise RuntimeError(f"CTC error word {p['err']:#x}: a frame's winning logit was not finite (NaN or Inf in the logits)")
    out = []
    for b in range(B):
        n = int(p["counts"][b])
        out.append(Transcript([int(t) for t in p["ids"][b, :n]], [(int(s), int(e)) for s, e in zip(p["starts"][b, :n], p["ends"][b, :n])],
                              float(p["min_margin"][b])))
    return out


class CTCTranscriber(_Extractor):
    """Encoder + CTC head on one GPU.  ``submit`` / ``collect`` are the extraction pipeline's with the head behind the forward: the
    slot's D2H copy is the head's one buffer (counts | ids | starts | ends | min_margin | error word).  ``state_dict``: the checkpoint
    under normalised names with ``lm_head`` kept (``weights.load_checkpoint(..., keep=CTC_HEAD_PREFIXES)``)."""

    def __init__(self, geo, spec, state_dict, device: str = "cuda:0", mode: str = "f16x", batch_size: int = 16, normalize: bool = True):
        from .engine import CTCHead, build_encoder
        from .weights import split_ctc_head
        if spec is None:
            raise ValueError("not a CTC checkpoint (config.json names none of " + ", ".join(C.CTC_ARCHITECTURES) + ")")
        if geo.family not in C.SPEECH_FAMILIES + (C.FAMILY_W2V_BERT,):
            raise ValueError(f"{geo.name}: the {geo.family} encoder has no CTC head")
        self.geo, self.spec, self.whisper = geo, spec, False
        self.average, self.layer_index = False, geo.num_layers           # the extraction pipeline's selection: the full forward
        self.mode = self.supported_mode(geo, head_mode(mode, geo.name), False, geo.name)
        enc_sd, head_sd = split_ctc_head(state_dict)
        self.enc = build_encoder(geo, enc_sd, device, self.mode, normalize=normalize)
        self.head = CTCHead(self.enc, head_sd, spec)
        self.batch_size = max(1, int(batch_size))
        self.hop = frame_hop(geo)
        self.failed: List[tuple] = []                                    # (index, error) of the last ``transcribe``
        self.offsets: List[Optional[List[Tuple[int, int]]]] = []         # per item of the last ``transcribe``: (start, end) frames per id
        self.min_margins: List[Optional[float]] = []

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        """what ``submit`` copies to the host: the head's int32 words as an fp32 [n, 1] view (a copy keeps the bits), enqueued behind
        the forward on the slot's stream"""
        return self.head.forward_tokens(hs, slot=slot).view(torch.float32).view(-1, 1)

    @staticmethod
    def _results(host: np.ndarray, frame_offs: Sequence[int]) -> List[Transcript]:
        B = len(frame_offs) - 1
        return split_blob(host.reshape(-1).view(np.int32), B, max(frame_offs[b + 1] - frame_offs[b] for b in range(B)))

    def extract(self, waves: List[np.ndarray], layer_index=None, rates=None) -> List[Transcript]:
        """One ragged batch -> one ``Transcript`` per utterance, synchronously (slot 0)."""
        dev, lengths = self.upload_resampled(waves, rates)
        hs = self.enc.forward(dev, lengths)
        out = self.select(hs, None)
        bits = hs.take_range_bits()
        host = out.cpu().numpy().copy()
        self._check_range(bits)
        return self._results(host, hs.frame_offs)

    def submit(self, waves: List[np.ndarray], layer_index=None, slot: int = 0, rates=None):
        return super().submit(waves, None, slot, rates)                 # last_state None: the head reads the last state

    def collect(self, ticket) -> List[Transcript]:
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))
        return self._results(ticket["host"].numpy().copy(), ticket["frame_offs"])

    def transcribe(self, waves: Sequence[np.ndarray]) -> List[Optional[List[int]]]:
        """16 kHz mono waveforms -> per item the list of token ids, in order, through the two-slot pipeline; ``self.offsets`` and
        ``self.min_margins`` hold the frame pairs and the smallest margins.  A batch that fails (the error word, the fp16 range guard,
        an utterance too short for the stem) is retried item by item; an item that still fails is printed, listed in ``self.failed`` as
        (index, error), and its entries are None."""
        waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in waves]
        ids: List[Optional[List[int]]] = [None] * len(waves)
        self.offsets, self.min_margins, self.failed = [None] * len(waves), [None] * len(waves), []

        def fail(item, err):
            self.failed.append((item[0], err))
            print(f"Failed to process item {item[0]}: {err}")

        def done(good, got, ticket):
            for (i, _), r in zip(good, got):
                ids[i], self.offsets[i], self.min_margins[i] = r.ids, r.offsets, r.min_margin

        if torch.cuda.is_available():
            torch.cuda.synchronize()                          # slot 0's arena is shared with the synchronous path
        pipe = SlotPipeline(submit=lambda good, slot: self.submit([w for _, w in good], None, slot=slot), collect=self.collect,
                            extract=lambda good: self.extract([w for _, w in good]), slots=self.SLOTS, done=done, fail=fail,
                            before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
        for bi, batch in enumerate(make_batches(list(enumerate(waves)), self.batch_size)):
            pipe.push(bi, batch)
            pipe.drain()
        pipe.drain(0)
        return ids


class Alignment:
    """One utterance's forced alignment: the target ``ids``, per id its ``spans`` (first frame, one past the last) and ``tok_scores`` (the
    mean log-probability of its frames), ``score`` (the float64 mean of ALL frames' log-probabilities on the path, blanks included),
    ``path_logit`` (the best path's sum of raw logits), and per frame ``pos`` (the index into ``ids``, -1 for a blank frame) and
    ``frame_scores``."""
    __slots__ = ("ids", "spans", "tok_scores", "score", "path_logit", "pos", "frame_scores")

    def __init__(self, ids, spans, tok_scores, score, path_logit, pos, frame_scores):
        self.ids, self.spans, self.tok_scores, self.score, self.path_logit = ids, spans, tok_scores, score, path_logit
        self.pos, self.frame_scores = pos, frame_scores


class AlignmentError(ValueError):
    """an utterance's non-zero status word (``_lib.CTC_ALIGN_*``)"""

    def __init__(self, status: int, frames: int, tokens: int):
        from . import _lib
        why = {_lib.CTC_ALIGN_INFEASIBLE: f"{frames} frames are too few for a target of {tokens} tokens",
               _lib.CTC_ALIGN_NONFINITE: "a logit on the target's columns is NaN or +Inf, or no path has a finite score",
               _lib.CTC_ALIGN_BAD_TARGET: f"the target ({tokens} tokens, at most {_lib.CTC_ALIGN_MAX_TOKENS}) holds the blank or an id outside the vocabulary"}
        super().__init__(why.get(status, f"alignment status {status:#x}"))
        self.status = status


def split_align_blob(words: np.ndarray, frame_offs: Sequence[int], targets: Sequence[Sequence[int]]) -> list:
    """per utterance the ``Alignment`` of one batch's host copy (engine.CTCHead.unpack_align's layout, frames included), or the
    ``AlignmentError`` of its status word: an utterance fails alone"""
    from . import _lib
    from .engine import CTCHead
    B, rows = len(targets), int(frame_offs[-1])
    Lm = min(max(len(y) for y in targets), _lib.CTC_ALIGN_MAX_TOKENS)
    p = CTCHead.unpack_align(words, B, Lm, rows)
    out = []
    for b, y in enumerate(targets):
        r0, r1, L = int(frame_offs[b]), int(frame_offs[b + 1]), len(y)
        if int(p["status"][b]):
            out.append(AlignmentError(int(p["status"][b]), r1 - r0, L))
            continue
        fs = p["frame_score"][r0:r1].copy()
        out.append(Alignment([int(t) for t in y], [(int(s), int(e)) for s, e in zip(p["starts"][b, :L], p["ends"][b, :L])],
                             [float(v) for v in p["tok_score"][b, :L]], float(fs.astype(np.float64).mean()), float(p["path_logit"][b]),
                             p["pos"][r0:r1].copy(), fs))
    return out


class CTCAligner(CTCTranscriber):
    """Encoder + CTC head + forced alignment on one GPU: ``CTCTranscriber`` whose ``submit`` / ``collect`` / ``extract`` carry one target
    (a sequence of token ids) per utterance.  The slot's D2H copy is ``engine.CTCHead.forward_align``'s buffer.  ``collect`` and ``extract``
    return per utterance an ``Alignment`` or the ``AlignmentError`` of its status word."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.vocab: Optional["CTCVocab"] = None                          # ``align``'s default for text targets
        self._targets: Dict[int, list] = {}                              # slot -> the targets ``select`` aligns (set ahead of the forward)

    def select(self, hs, layer_index, slot: int = 0) -> torch.Tensor:
        return self.head.forward_align(hs, self._targets[slot], slot=slot, frames=True).view(torch.float32).view(-1, 1)

    def extract(self, waves: List[np.ndarray], targets=None, rates=None) -> list:
        """One ragged batch and its targets -> one result per utterance, synchronously (slot 0)."""
        self._targets[0] = targets = [list(y) for y in targets]
        dev, lengths = self.upload_resampled(waves, rates)
        hs = self.enc.forward(dev, lengths)
        out = self.select(hs, None)
        bits = hs.take_range_bits()
        host = out.cpu().numpy().copy()
        self._check_range(bits)
        return split_align_blob(host.reshape(-1).view(np.int32), hs.frame_offs, targets)

    def submit(self, waves: List[np.ndarray], targets=None, slot: int = 0, rates=None):
        self._targets[slot] = targets = [list(y) for y in targets]
        ticket = _Extractor.submit(self, waves, None, slot, rates)
        ticket["targets"] = targets
        return ticket

    def collect(self, ticket) -> list:
        ticket["event"].synchronize()
        if ticket.get("watch") is not None:
            self._check_range(int(ticket["watch"][0]))
        return split_align_blob(ticket["host"].numpy().copy().reshape(-1).view(np.int32), ticket["frame_offs"], ticket["targets"])

    def align(self, waves: Sequence[np.ndarray], targets: Sequence, vocab: Optional["CTCVocab"] = None) -> List[Optional[Alignment]]:
        """16 kHz mono waveforms and per item a target (token ids, or a text that ``vocab.encode`` turns into ids) -> per item an
        ``Alignment`` or None, through the two-slot pipeline.  A batch that fails as a whole (the fp16 range guard, an utterance too
        short for the stem) is retried item by item; an item whose status word is set fails ALONE: it is printed, listed in
        ``self.failed`` as (index, error) and gets None, and its batch mates are not run again."""
        waves = [np.ascontiguousarray(np.asarray(w, dtype=np.float32)) for w in waves]
        if len(targets) != len(waves):
            raise ValueError(f"{len(targets)} targets for {len(waves)} waveforms")
        vocab = vocab or self.vocab
        if any(isinstance(y, str) for y in targets) and vocab is None:
            raise ValueError("a text target needs the vocabulary (vocab=, or the aligner's .vocab)")
        tg = [vocab.encode(y) if isinstance(y, str) else [int(t) for t in y] for y in targets]
        out: List[Optional[Alignment]] = [None] * len(waves)
        self.failed = []

        def fail(item, err):
            self.failed.append((item[0], err))
            print(f"Failed to process item {item[0]}: {err}")

        def done(good, got, ticket):
            for item, r in zip(good, got):
                if isinstance(r, Exception):
                    fail(item, r)
                else:
                    out[item[0]] = r

        if torch.cuda.is_available():
            torch.cuda.synchronize()                          # slot 0's arena is shared with the synchronous path
        pipe = SlotPipeline(submit=lambda good, slot: self.submit([w for _, w, _ in good], [y for _, _, y in good], slot=slot),
                            collect=self.collect, extract=lambda good: self.extract([w for _, w, _ in good], [y for _, _, y in good]),
                            slots=self.SLOTS, done=done, fail=fail,
                            before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
        for bi, batch in enumerate(make_batches([(i, w, y) for i, (w, y) in enumerate(zip(waves, tg))], self.batch_size)):
            pipe.push(bi, batch)
            pipe.drain()
        pipe.drain(0)
        return out


def words(alignment: Alignment, encoded_words) -> List[tuple]:
    """[(word, start frame, end frame, score)] of an alignment whose target was ``CTCVocab.join(encoded_words)``: a word's span runs from
    its first id's first frame to one past its last id's last frame, its score is the float64 mean of its frames' log-probabilities
    (the token means weighted by their span lengths, on the host).  An unalignable word (no ids) gets None times and score."""
    n_ids = sum(len(ids) for _, ids in encoded_words)
    n_words = sum(1 for _, ids in encoded_words if ids)
    gap = 1 if n_words > 1 and len(alignment.ids) == n_ids + n_words - 1 else 0          # a word delimiter between two alignable words
    if len(alignment.ids) != n_ids + gap * (n_words - 1):
        raise ValueError(f"the alignment has {len(alignment.ids)} ids, the words {n_ids}")
    out, j = [], 0
    for word, ids in encoded_words:
        if not ids:
            out.append((word, None, None, None))
            continue
        n = len(ids)
        if alignment.ids[j:j + n] != [int(t) for t in ids]:
            raise ValueError(f"the alignment's ids do not spell the words (at {word!r})")
        spans, sc = alignment.spans[j:j + n], alignment.tok_scores[j:j + n]
        total = sum(e - s for s, e in spans)
        score = sum(np.float64(v) * (e - s) for v, (s, e) in zip(sc, spans)) / np.float64(total)
        out.append((word, spans[0][0], spans[-1][1], float(score)))
        j += n + gap
    return out


# ------------------------------------------------------------------------------- vocabulary
def _token(v, default):
    """a special token of tokenizer_config.json / special_tokens_map.json: a string, or an AddedToken dict with ``content``"""
    if isinstance(v, dict):
        v = v.get("content")
    return default if v is None else str(v)


class CTCVocab:
    """What ``Wav2Vec2CTCTokenizer.decode`` does to the per-frame ids, with its defaults, applied to ALREADY COLLAPSED ids and without the
    ``transformers`` tokenizer: an id becomes its token (``unk_token`` for an id outside the vocabulary), the pad token is dropped, the
    word delimiter becomes ``replace_word_delimiter_char``, the tokens are joined without separator and the string is stripped; special
    tokens are not skipped.  HF groups equal neighbours and then drops the pad token; the device has done both (the blank is the pad id)."""

    def __init__(self, vocab: Dict[str, int], pad_token: str = "<pad>", unk_token: str = "<unk>", word_delimiter_token: str = "|",
                 replace_word_delimiter_char: str = " ", do_lower_case: bool = False):
        self.encoder = {str(k): int(v) for k, v in vocab.items()}
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.pad_token, self.unk_token, self.word_delimiter_token = pad_token, unk_token, word_delimiter_token
        self.replace_word_delimiter_char, self.do_lower_case = replace_word_delimiter_char, bool(do_lower_case)

    @staticmethod
    def from_dir(path: str) -> Optional["CTCVocab"]:
        """From the local files of a snapshot directory (``vocab.json``; ``tokenizer_config.json`` and ``special_tokens_map.json`` where
        present); None without ``vocab.json``."""
        vf = os.path.join(path, "vocab.json")
        if not os.path.isfile(vf):
            return None
        with open(vf, "r", encoding="utf-8") as f:
            vocab = json.load(f)
        cfg: dict = {}
        for fn in ("special_tokens_map.json", "tokenizer_config.json"):              # the tokenizer's own config wins
            p = os.path.join(path, fn)
            if os.path.isfile(p):
                with open(p, "r", encoding="utf-8") as f:
                    cfg.update(json.load(f))
        lang = cfg.get("target_lang")
        if lang is not None:                                                         # a nested, per-language vocabulary
            vocab = vocab[lang]
        return CTCVocab(vocab, pad_token=_token(cfg.get("pad_token"), "<pad>"), unk_token=_token(cfg.get("unk_token"), "<unk>"),
                        word_delimiter_token=_token(cfg.get("word_delimiter_token"), "|"),
                        replace_word_delimiter_char=_token(cfg.get("replace_word_delimiter_char"), " "),
                        do_lower_case=bool(cfg.get("do_lower_case", False)))

    def chars(self, ids: Sequence[int], offsets: Optional[Sequence[Tuple[int, int]]] = None):
        """(processed characters, their offsets) of collapsed ids: pad dropped, the delimiter replaced"""
        out, offs = [], []
        for j, i in enumerate(ids):
            tok = self.decoder.get(int(i), self.unk_token)
            if tok == self.pad_token:
                continue
            out.append(self.replace_word_delimiter_char if tok == self.word_delimiter_token else tok)
            if offsets is not None:
                offs.append((int(offsets[j][0]), int(offsets[j][1])))
        return out, offs

    def _specials(self) -> set:
        """tokens that never spell a character: pad, unk, the word delimiter, and every multi-character token (<s>, </s>, ...)"""
        return {self.pad_token, self.unk_token, self.word_delimiter_token} | {t for t in self.encoder if len(t) != 1}

    def encode_words(self, text: str) -> List[Tuple[str, List[int]]]:
        """[(word, [ids])] of a text that did not come from this vocabulary (Whisper's transcript): the inverse of ``chars``.  The text is
        split on whitespace; per character the first of c, c.upper(), c.lower() whose every character is a vocabulary token is taken
        (so "ß" against an upper-case vocabulary is "SS"); everything else is dropped (digits, punctuation).  A word left with no
        ids is UNALIGNABLE."""
        special = self._specials()
        ok = lambda t: t in self.encoder and t not in special                     # noqa: E731
        out = []
        for word in str(text).split():
            ids: List[int] = []
            for c in word:
                for form in (c, c.upper(), c.lower()):
                    if form and all(ok(t) for t in form):
                        ids.extend(self.encoder[t] for t in form)
                        break
            out.append((word, ids))
        return out

    def join(self, encoded_words) -> List[int]:
        """the alignment target of ``encode_words``'s result: the alignable words' ids joined by the word-delimiter id (where the
        vocabulary has one), no delimiter at either end and none doubled around an unalignable word"""
        delim = self.encoder.get(self.word_delimiter_token)
        out: List[int] = []
        for _, ids in encoded_words:
            if not ids:
                continue
            if out and delim is not None:
                out.append(delim)
            out.extend(ids)
        return out

    def encode(self, text: str) -> List[int]:
        return self.join(self.encode_words(text))

    def text(self, ids: Sequence[int]) -> str:
        s = "".join(self.chars(ids)[0]).strip()
        return s.lower() if self.do_lower_case else s

    def char_offsets(self, ids: Sequence[int], offsets: Sequence[Tuple[int, int]]) -> List[dict]:
        """HF's ``char_offsets`` (``decode(..., output_char_offsets=True)``): one {"char", "start_offset", "end_offset"} per kept token, in frames"""
        ch, offs = self.chars(ids, offsets)
        return [{"char": c, "start_offset": s, "end_offset": e} for c, (s, e) in zip(ch, offs)]


def load_vocab(name_or_path: str) -> Optional[CTCVocab]:
    """The checkpoint's vocabulary from local files: a directory, else the offline HF cache's snapshot of a hub id; None (said in one
    line) without ``vocab.json``."""
    dirs = [name_or_path] if os.path.isdir(name_or_path) else []
    if not dirs and name_or_path:
        home = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
        snap = os.path.join(home, "hub", "models--" + name_or_path.replace("/", "--"), "snapshots")
        if os.path.isdir(snap):
            dirs = [os.path.join(snap, rev) for rev in sorted(os.listdir(snap))]
    for d in dirs:
        try:
            v = CTCVocab.from_dir(d)
        except (OSError, ValueError, KeyError) as e:
            print(f"Cannot read the vocabulary files under {d} ({type(e).__name__}: {e})")
            v = None
        if v is not None:
            return v
    print(f"No vocabulary files for {name_or_path}: writing token ids instead of text")
    return None


# ------------------------------------------------------------------------------- CLI
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="greedy CTC transcripts of a hub AutoModelForCTC checkpoint for a wav directory -> the reference's transcript table")
    p.add_argument("--model", type=str, required=True, help="hub id (offline HF cache) or local snapshot directory")
    p.add_argument("--wav_dir", type=str, required=True)
    p.add_argument("--out_csv", type=str, required=True, help="FileName,transcription: the table --df_path / txt_dir read")
    p.add_argument("--mode", type=str, default="f16x", choices=list(MODES))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resample", action="store_true", help="accept non-16 kHz wav files (resampled on the GPU ahead of the forward)")
    p.add_argument("--checkpoint", type=str, default="", help="local *.safetensors / pytorch_model.bin (or directory) instead of --model's weights")
    p.add_argument("--tokenizer_path", type=str, default="", help="directory of vocab.json (default: --model's)")
    p.add_argument("--offsets_json", type=str, default="", help="per file the (char, start_s, end_s) triples")
    p.add_argument("--num_workers", type=int, default=4)
    return p


def _build_transcriber(args, device: str, cls=None) -> "CTCTranscriber":
    """The shared load path of the drivers: config.json -> geometry and head spec, weights by ``find_weights`` with ``lm_head`` kept."""
    from .weights import CTC_HEAD_PREFIXES
    spec = C.resolve_ctc(args.model, args.checkpoint)                 # first: a CTC class over an unbuilt encoder is named as such
    if spec is None:
        raise OSError(f"{args.model} is not a CTC checkpoint (its config.json names none of " + ", ".join(C.CTC_ARCHITECTURES) + ")")
    geo = C.resolve_geometry(args.model, args.checkpoint)
    geo = C.resolve_fbank(geo, args.model, args.checkpoint)
    sd, source = find_weights(args.model, args.checkpoint, False, 0, geo, keep=CTC_HEAD_PREFIXES)
    tr = (cls or CTCTranscriber)(geo, spec, sd, device, args.mode, args.batch_size, normalize=C.resolve_do_normalize(args.model, args.checkpoint))
    tr.weight_source = source
    return tr


def _build_aligner(args, device: str) -> "CTCAligner":
    return _build_transcriber(args, device, CTCAligner)


def _open(args, factory):
    """The set-up both command lines share: (sorted file names, the model object), or None after the printed error (exit code 0, as the
    extraction drivers do)."""
    device = "cuda:0" if torch.cuda.is_available() else "cpu"
    try:
        names = sorted(fn for fn in os.listdir(args.wav_dir) if os.path.isfile(os.path.join(args.wav_dir, fn)))
    except OSError as e:
        print(f"Error reading {args.wav_dir}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return None
    print(f"{len(names)} file are going to be processed...")
    if device == "cpu" and factory in (_build_transcriber, _build_aligner):
        print("Error: no MI355X visible -- this build has no CPU path (the CPU oracle under oracle/ is test-only)")
        print("Something went wrong, make sure everything is correct before running again!")
        return None
    try:
        tr = factory(args, device)
    except (OSError, NotImplementedError) as e:
        print(f"Error: No pretrained model found with the name {args.model}")
        print(f"  ({e})")
        print("Something went wrong, make sure everything is correct before running again!")
        return None
    print(f"Weights: {getattr(tr, 'weight_source', 'caller')}; numerics mode {getattr(tr, 'mode', args.mode)}")
    return names, tr


def _decoder(args, gpu_resample: bool):
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
    return decode


def run(argv: Optional[Sequence[str]] = None, transcriber_factory=None, vocab: Optional[CTCVocab] = None) -> int:
    """``transcriber_factory(args, device)`` replaces the model (the host tests hand in a stub with ``submit`` / ``collect`` / ``extract``
    / ``hop``): everything around the model call then runs without a GPU.  ``vocab`` replaces the vocabulary files."""
    args = build_parser().parse_args(argv)
    opened = _open(args, transcriber_factory or _build_transcriber)
    if opened is None:
        return 0
    names, tr = opened
    if vocab is None:
        vocab = load_vocab(args.tokenizer_path or args.model)
    gpu_resample = args.resample and hasattr(tr, "upload_resampled")
    seconds = float(getattr(tr, "hop", 320)) / TARGET_SR
    decode = _decoder(args, gpu_resample)

    rows: Dict[str, str] = {}
    offsets: Dict[str, list] = {}
    failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(args.wav_dir, name)}: {err}")

    def finished(good, out, ticket):
        for (name, _), r in zip(good, out):
            if vocab is not None:
                rows[name] = vocab.text(r.ids)
                ch, offs = vocab.chars(r.ids, r.offsets)
            else:
                rows[name] = " ".join(str(t) for t in r.ids)
                ch, offs = [str(t) for t in r.ids], list(r.offsets)
            offsets[name] = [[c, s * seconds, e * seconds] for c, (s, e) in zip(ch, offs)]

    def go(fn, good, **k):
        waves = [w for _, (w, _) in good]
        return fn(waves, None, rates=[sr for _, (_, sr) in good], **k) if gpu_resample else fn(waves, None, **k)

    pipe = SlotPipeline(submit=lambda good, slot: go(tr.submit, good, slot=slot), collect=tr.collect, extract=lambda good: go(tr.extract, good),
                        slots=getattr(tr, "SLOTS", 2), done=finished, fail=lambda item, err: fail(item[0], err),
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
    done = [n for n in names if n in rows]
    os.makedirs(os.path.dirname(os.path.abspath(args.out_csv)), exist_ok=True)
    write_table(args.out_csv, done, [rows[n] for n in done])
    if args.offsets_json:
        with open(args.offsets_json, "w", encoding="utf-8") as f:
            json.dump({n: offsets[n] for n in done}, f)
    print(f"{len(done)} utterances on 1 GPU(s) in {dt:.2f} s ({len(done) / max(dt, 1e-9):.1f} utt/s)")
    print(f"Wrote {len(done)} of {len(names)} transcripts to {args.out_csv}; {failed} files failed")
    return 0


# ------------------------------------------------------------------------------- CLI: forced alignment
def build_align_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="word times and acoustic scores of a transcript table, by CTC forced alignment with a hub AutoModelForCTC checkpoint")
    p.add_argument("--model", type=str, required=True, help="hub id (offline HF cache) or local snapshot directory")
    p.add_argument("--wav_dir", type=str, required=True)
    p.add_argument("--df_path", type=str, required=True, help="FileName,transcription: the table transcribe_whisper.py / transcribe_ctc.py write")
    p.add_argument("--out_json", type=str, required=True, help='{file: {"score": mean frame log-prob, "words": [[word, start_s, end_s, score], ...]}}')
    p.add_argument("--mode", type=str, default="f16x", choices=list(MODES))
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--resample", action="store_true", help="accept non-16 kHz wav files (resampled on the GPU ahead of the forward)")
    p.add_argument("--checkpoint", type=str, default="", help="local *.safetensors / pytorch_model.bin (or directory) instead of --model's weights")
    p.add_argument("--tokenizer_path", type=str, default="", help="directory of vocab.json (default: --model's)")
    p.add_argument("--chars", action="store_true", help='add "chars": [[char, start_s, end_s, score], ...] per file')
    p.add_argument("--num_workers", type=int, default=4)
    return p


def _read_texts(path: str) -> Dict[str, str]:
    """FileName -> transcription of the transcript table, an empty transcription as the empty string"""
    import csv
    with open(path, newline="", encoding="utf-8") as f:
        return {str(r["FileName"]): str(r.get("transcription") or "") for r in csv.DictReader(f)}


def run_align(argv: Optional[Sequence[str]] = None, aligner_factory=None, vocab: Optional[CTCVocab] = None) -> int:
    """``aligner_factory(args, device)`` replaces the model (the host tests hand in a stub with ``submit`` / ``collect`` / ``extract`` /
    ``hop``, whose results are ``Alignment`` or exception objects); ``vocab`` replaces the vocabulary files."""
    args = build_align_parser().parse_args(argv)
    if vocab is None:
        vocab = load_vocab(args.tokenizer_path or args.model)
    if vocab is None:                                               # (load_vocab has said which files are missing)
        print("Error: forced alignment needs the checkpoint's vocabulary (vocab.json) to turn the transcripts into token ids")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    try:
        texts = _read_texts(args.df_path)
    except (OSError, KeyError, ValueError) as e:
        print(f"Error reading {args.df_path}: {e}")
        print("Something went wrong, make sure everything is correct before running again!")
        return 0
    opened = _open(args, aligner_factory or _build_aligner)
    if opened is None:
        return 0
    names, tr = opened
    gpu_resample = args.resample and hasattr(tr, "upload_resampled")
    seconds = float(getattr(tr, "hop", 320)) / TARGET_SR
    decode = _decoder(args, gpu_resample)
    result: Dict[str, dict] = {}
    failed = 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {os.path.join(args.wav_dir, name)}: {err}")

    def finished(good, out, ticket):
        for (name, _, enc), r in zip(good, out):
            if isinstance(r, Exception):
                fail(name, r)
                continue
            entry = {"score": r.score,
                     "words": [[w, None if s is None else s * seconds, None if e is None else e * seconds, sc] for w, s, e, sc in words(r, enc)]}
            if args.chars:
                ch, offs = vocab.chars(r.ids, r.spans)
                entry["chars"] = [[c, s * seconds, e * seconds, sc] for c, (s, e), sc in zip(ch, offs, r.tok_scores)]
            result[name] = entry

    def go(fn, good, **k):
        waves, tg = [w for _, (w, _), _ in good], [vocab.join(enc) for _, _, enc in good]
        return fn(waves, tg, rates=[sr for _, (_, sr), _ in good], **k) if gpu_resample else fn(waves, tg, **k)

    pipe = SlotPipeline(submit=lambda good, slot: go(tr.submit, good, slot=slot), collect=tr.collect, extract=lambda good: go(tr.extract, good),
                        slots=getattr(tr, "SLOTS", 2), done=finished, fail=lambda item, err: fail(item[0], err),
                        before_retry=torch.cuda.synchronize if torch.cuda.is_available() else None)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=max(1, args.num_workers)) as pool:
        for bi, decoded in enumerate(prefetch(make_batches(names, max(1, args.batch_size)), pool, decode)):
            good = []
            for name, item, err in decoded:
                if err is None and name not in texts:
                    err = KeyError(f"no row for it in {args.df_path}")
                enc = vocab.encode_words(texts[name]) if err is None else None
                if err is None and not any(ids for _, ids in enc):
                    err = ValueError(f"its transcription {texts[name]!r} has no word the vocabulary can spell")
                if err is not None:
                    fail(name, err)
                else:
                    good.append((name, item, enc))
            if good:
                pipe.push(bi, good)
            pipe.drain()
        pipe.drain(0)
    dt = time.perf_counter() - t0
    done = [n for n in names if n in result]
    os.makedirs(os.path.dirname(os.path.abspath(args.out_json)), exist_ok=True)
    with open(args.out_json, "w", encoding="utf-8") as f:
        json.dump({n: result[n] for n in done}, f)
    print(f"{len(done)} utterances on 1 GPU(s) in {dt:.2f} s ({len(done) / max(dt, 1e-9):.1f} utt/s)")
    print(f"Wrote {len(done)} of {len(names)} alignments to {args.out_json}; {failed} files failed")
    return 0
