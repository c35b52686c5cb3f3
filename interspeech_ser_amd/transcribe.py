"""Waveforms -> Whisper's own transcript on one device: ``WhisperEncoder`` and ``WhisperDecoder`` behind each other.

The reference makes its transcript table with ``AutoModelForSpeechSeq2Seq.generate(input_features)`` (test/Whisper transcriptions.ipynb ->
``whisper_transcripts.csv``, columns FileName, transcription); ``preprocess_roberta.py --df_path`` and the heads' ``txt_dir`` read it.
``WhisperTranscriber.transcribe`` returns the generated token ids, ``.texts`` what ``batch_decode(skip_special_tokens=True)`` makes of them,
``run`` (preprocessing/transcribe_whisper.py) writes the table.

``transcribe(..., token_times=True)`` also keeps HF's ``token_timestamps`` of every file given alone (``.token_times``), read from the
alignment heads' cross-attention by the decoder itself (engine.WhisperDecoder.generate); ``token_words`` groups tokens into words as HF's
``_combine_tokens_into_words`` does, and ``--times_json`` writes both.

``transcribe(..., timestamps=True)`` runs the model's own segment times instead (HF's ``return_timestamps=True``, one 30 s window):
``.segments`` and ``.next_seek`` per file, ``segments_of`` being HF's ``_retrieve_segment``; ``--segments_json`` writes them.

``transcribe_long(items)`` is the seek loop over files longer than 30 s (HF's long-form ``generate``): whole-file features, one window
per file and round through a window queue, the segments with absolute times; ``--long_form`` runs it.

``transcribe(..., scores=True)`` keeps what HF's ``generate`` thresholds read: ``.scores[i]`` = the file's ``avg_logprob``,
``no_speech_prob``, ``compression_ratio``, ``needs_fallback`` and ``token_logprobs`` (``--scores_json`` writes them).  ``need_fallback`` is
HF's ``_need_fallback``; with thresholds in the spec ``transcribe_long`` skips a window whose ``should_skip`` holds, as HF's seek loop does.
Temperature fallback is not built: ``needs_fallback`` is reported and changes nothing.
"""
from __future__ import annotations

import argparse
import csv
import json
import math
import os
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import make_batches, run_or_each

N_SAMPLES = 480000            # 30 s: WhisperFeatureExtractor cuts longer input, and so does ``transcribe`` (``transcribe_long`` does not)
BATCH = 16
N_FRAMES = 3000               # mel frames of a window
HOP = 160                     # samples per mel frame
TIME_PRECISION = C.GenerationSpec.TIME_PRECISION  # seconds per timestamp token step (HF: time_precision)
TIME_PRECISION_FEATURES = 0.01  # seconds per mel frame
INPUT_STRIDE = 2              # mel frames per timestamp step


def window_frames(n_samples: Optional[int]) -> int:
    """HF's ``seek_num_frames`` of a first window when the feature extractor's attention mask is passed: min(3000, len // 160); None:
    the whole window."""
    return N_FRAMES if n_samples is None else min(N_FRAMES, int(n_samples) // HOP)


def is_long(n_samples: int) -> bool:
    """more mel frames than one window holds: the file goes through the long-form loop (``WhisperTranscriber.transcribe_long``)"""
    return int(n_samples) // HOP > N_FRAMES


def segments_of(tokens: Sequence[int], ts_begin: int, num_frames: int, time_offset: float = 0.0):
    """HF's ``WhisperGenerationMixin._retrieve_segment`` for one window's generated tokens (prompt and eos removed): ``(segments,
    segment_offset)`` with segments ``[(start_s, end_s, ids)]`` and the offset in mel frames.  The tokens are sliced behind every pair of
    consecutive timestamp tokens; a sequence that ends [text, timestamp] closes its last segment there and the whole window is consumed;
    otherwise what follows the last pair is dropped and the seek advances to that pair's time.  Without a pair the whole sequence is one
    segment from the offset to its last timestamp (if it has one other than <|0.00|>), else to the window's end."""
    tok = [int(t) for t in tokens]
    n = len(tok)
    is_ts = [t >= ts_begin for t in tok]
    single_ending = is_ts[-2:] == [False, True]
    slices = [i + 1 for i in range(n - 1) if is_ts[i] and is_ts[i + 1]]
    off = float(time_offset)
    if slices:
        if single_ending:
            slices.append(n)
        else:
            slices[-1] += 1                                 # the closing pair stays in the last segment: it was no single ending
        segments, last = [], 0
        for i, cur in enumerate(slices):
            part = tok[last:cur]
            end_at = -1 if i < len(slices) - 1 or single_ending else -2
            segments.append((off + float(part[0] - ts_begin) * TIME_PRECISION, off + float(part[end_at] - ts_begin) * TIME_PRECISION, part))
            last = cur
        return segments, int(num_frames) if single_ending else (tok[last - 2] - ts_begin) * INPUT_STRIDE
    stamps = [t for t in tok if t >= ts_begin]
    last_pos = float(int(num_frames * TIME_PRECISION_FEATURES / TIME_PRECISION))
    if stamps and stamps[-1] != ts_begin:
        last_pos = float(stamps[-1] - ts_begin)
    return [(off, off + last_pos * TIME_PRECISION, tok)], int(num_frames)


def compression_ratio(tokens: Sequence[int], vocab_size: int) -> float:
    """HF's ``_retrieve_compression_ratio``: every token as ``int(log2(V) / 8) + 1`` little-endian bytes; the raw length over zlib's."""
    length = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(length, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def check_thresholds(thresholds: dict) -> None:
    """HF's ``_need_fallback`` reads the average log-probability in its no-speech branch and computes it only under
    ``logprob_threshold``: with ``no_speech_threshold`` alone it raises on the unbound name.  Refused by name instead."""
    if thresholds.get("no_speech_threshold") is not None and thresholds.get("logprob_threshold") is None:
        raise ValueError("no_speech_threshold without logprob_threshold: HF's rule compares the average log-probability in its no-speech "
                         "branch, so --no_speech_threshold needs --logprob_threshold")


def need_fallback(tokens_with_eos: Sequence[int], avg_logprob: float, no_speech_prob: float, thresholds: dict, vocab_size: int):
    """HF's ``WhisperGenerationMixin._need_fallback`` branch by branch -> ``(needs_fallback, should_skip)``.  ``tokens_with_eos``: the
    window's generated tokens, the closing eos included (HF keeps it for this call); ``thresholds``: ``logprob_threshold``,
    ``no_speech_threshold`` and ``compression_ratio_threshold``, None or absent where not set."""
    check_thresholds(thresholds)
    needs_fallback, should_skip = False, False
    ratio, logprob, silence = (thresholds.get(k) for k in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold"))
    if ratio is not None:
        if compression_ratio(tokens_with_eos, vocab_size) > ratio:
            needs_fallback = True
    if logprob is not None:
        if avg_logprob < logprob:
            needs_fallback = True
    if silence is not None:
        if avg_logprob < logprob and no_speech_prob > silence:
            needs_fallback = False
            should_skip = True
    return needs_fallback, should_skip


def score_entry(tokens_with_eos: Sequence[int], avg_logprob: float, no_speech_prob: float, thresholds: dict, vocab_size: int) -> dict:
    """The scores of one decoded window as the JSON files carry them, and ``skipped`` = HF's should_skip."""
    needs, skip = need_fallback(tokens_with_eos, avg_logprob, no_speech_prob, thresholds, vocab_size)
    return dict(avg_logprob=float(avg_logprob), no_speech_prob=float(no_speech_prob),
                compression_ratio=float(compression_ratio(tokens_with_eos, vocab_size)), needs_fallback=bool(needs), skipped=bool(skip))


def _with_eos(res, k: int, spec) -> List[int]:
    """the generated tokens of row k of a DecodeResult, the first eos included: one per entry of its token_logprobs"""
    return [int(t) for t in res.sequences[k, spec.prompt_len(res.segments is not None):][: len(res.token_logprobs[k])]]


class WhisperTranscriber:
    """``transcribe(waves)``: per utterance the generated ids without the prompt, up to and excluding eos (None for a file that failed).
    Batches of ``BATCH`` alternate between the encoder's and decoder's two slots.  A batch whose fp16 range-guard word or decoder error
    word is set goes through ``batchloop.run_or_each``: retried file by file, a file that still fails is printed and left out.  What
    the encoder or the decoder raises is not caught."""

    def __init__(self, encoder, decoder, spec: C.GenerationSpec):
        self.enc, self.dec, self.spec = encoder, decoder, spec
        self.last_languages: List[Optional[int]] = []
        self.token_times: List[Optional[List[float]]] = []      # per item of the last transcribe(token_times=True)
        self.segments: List[Optional[list]] = []                # per item of the last transcribe(timestamps=True): [(start_s, end_s, ids)]
        self.next_seek: List[Optional[int]] = []                # ... and the mel frames the next window would begin at
        self.failed: List[str] = []                             # names of the files the last transcribe() left out
        self.sequences: List[Optional[List[int]]] = []          # per item of the last transcribe_long(): the segments' ids, timestamps included
        self.windows: List[Optional[list]] = []                 # ... its windows [(seek, nf, advance)] in mel frames
        self.rounds: List[tuple] = []                           # ... and the rounds that ran: (language key, item indices, [(seek, nf)])
        self.scores: List[Optional[dict]] = []                  # per item of the last transcribe(scores=True): score_entry + token_logprobs

    def _batch(self, waves: Sequence[np.ndarray], slot: int, token_times: bool = False, num_beams: Optional[int] = None,
               length_penalty: Optional[float] = None, timestamps: bool = False, scores: bool = False):
        """(DecodeResult, failed) of one batch; one encoder forward serves the decoder (its LAST state: the forward does not stop early)."""
        lengths = [len(w) for w in waves]
        hs = self.enc.forward(self.enc.upload(waves, slot), lengths, slot=slot)
        extra = dict(token_times=True, lengths=lengths) if token_times else {}       # the default call is the one it always was
        if num_beams is not None:
            extra["num_beams"] = int(num_beams)
        if length_penalty is not None:
            extra["length_penalty"] = float(length_penalty)
        if timestamps:
            extra.update(timestamps=True, lengths=lengths)
        if scores:
            extra["scores"] = True
        res = self.dec.generate(hs.states[-1], len(waves), self.spec, slot=slot, **extra)
        bits = hs.take_range_bits()
        return res, res.failed or bool(bits & 1), hs

    def transcribe(self, waves: Sequence[np.ndarray], names: Optional[Sequence[str]] = None, first_batch: int = 0,
                   token_times: bool = False, num_beams: Optional[int] = None, length_penalty: Optional[float] = None,
                   timestamps: bool = False, scores: bool = False) -> List[Optional[List[int]]]:
        """``first_batch``: the index of the first batch in the caller's own sequence of calls (a driver that hands over 16 files at a time
        keeps the slots alternating with it).  ``token_times``: ``self.token_times[i]`` becomes the seconds of item i's generated non-eos
        tokens.  A file whose times have a status word set (no frame, a matrix entry that is not finite) fails ALONE: it is printed,
        named in ``self.failed`` and has no times (its ids stay: the transcript table does not depend on the flag), and its batch mates are
        neither touched nor run again.  ``num_beams`` / ``length_penalty``: None takes the spec's; K >= 2 returns the best beam's ids
        (``self.last_scores[i]``: its score) and does not go with ``token_times``.  ``timestamps``: the model's own segment times of
        each file's first 30 s window: ``self.segments[i]`` = ``[(start_s, end_s, ids)]``, ``self.next_seek[i]`` = the mel frames the
        seek would advance by, and the returned ids are the generated ones with the timestamp tokens removed.  Does not go with
        ``token_times`` or beams.  ``scores``: the greedy or the timestamps run on the decoder's scored plan; ``self.scores[i]`` =
        ``score_entry`` of the file's tokens under the spec's thresholds plus ``token_logprobs``.  Nothing is skipped here (HF's skip
        belongs to its seek loop: ``transcribe_long``).  Does not go with ``token_times`` or beams."""
        if scores and (token_times or int(self.spec.num_beams if num_beams is None else num_beams) > 1):
            raise ValueError("scores=True with " + ("token_times" if token_times else "num_beams > 1") + ": transcript scores with "
                             + ("token times" if token_times else "beam search") + " are not built")
        if scores:
            check_thresholds(self.spec.thresholds)
        if timestamps and token_times:
            raise ValueError("timestamps=True with token_times: segment timestamps with token times are not built")
        if timestamps and int(self.spec.num_beams if num_beams is None else num_beams) > 1:
            raise ValueError("timestamps=True with num_beams > 1: segment timestamps with beam search are not built")
        if token_times:
            self.spec.require_alignment_heads()
        self.last_scores: List[Optional[float]] = [None] * len(waves)
        waves = [np.ascontiguousarray(w[:N_SAMPLES], dtype=np.float32) for w in waves]
        names = list(names) if names is not None else [f"utterance {i}" for i in range(len(waves))]
        out: List[Optional[List[int]]] = [None] * len(waves)
        self.last_languages = [None] * len(waves)
        self.token_times = [None] * len(waves)
        self.segments, self.next_seek = [None] * len(waves), [None] * len(waves)
        self.scores = [None] * len(waves)
        self.failed = []
        V = self.dec.geo.decoder_vocab_size if scores else 0

        def fail(j, res):
            self.failed.append(names[j])
            print(f"Failed to process {names[j]}: decoder error word {res.err:#x}, range-guard bits {res.range_bits:#x}")

        for n, idx in enumerate(make_batches(range(len(waves)), BATCH), start=int(first_batch)):
            def run(js):
                res, failed, _ = self._batch([waves[j] for j in js], n % 2, token_times, num_beams, length_penalty, timestamps, scores)
                if failed:
                    return res
                for k, j in enumerate(js):
                    out[j], self.last_languages[j] = res.lists[k], int(res.languages[k])
                    if timestamps:
                        out[j] = [t for t in res.lists[k] if t < self.spec.timestamp_begin]
                        self.segments[j], self.next_seek[j] = res.segments[k], int(res.next_seek[k])
                    if scores:
                        self.scores[j] = score_entry(_with_eos(res, k, self.spec), res.avg_logprob[k], res.no_speech_prob[k],
                                                     self.spec.thresholds, V)
                        self.scores[j]["token_logprobs"] = [float(x) for x in res.token_logprobs[k]]
                    if getattr(res, "beam_scores", None) is not None:
                        self.last_scores[j] = float(res.beam_scores[k])
                    if token_times and int(res.ts_status[k]) != 0:
                        self.failed.append(names[j])
                        print(f"Failed to process {names[j]}: token times status {int(res.ts_status[k]):#x} "
                              f"({len(waves[j])} samples, {len(res.lists[k])} tokens)")
                    elif token_times:
                        self.token_times[j] = [float(t) for t in res.token_times[k][: len(res.lists[k])]]

            run_or_each(idx, run, fail, catch=())
        return out

    def transcribe_long(self, items, batch: int = BATCH, scores: bool = False) -> List[Optional[List[int]]]:
        """Long-form transcription (HF's ``generate`` on input over 30 s with ``return_timestamps=True``, greedy, every file given alone)
        through a WINDOW QUEUE.  ``items``: an iterable of ``(name, wave)``, consumed as room frees up (a driver loads lazily).

        Up to ``batch`` long files (``is_long``) are resident, each with one pending window ``[seek, seek + nf)`` of its whole-file
        features (``WhisperEncoder.log_mel_long``: one launch for all files admitted in a round).  A round takes up to ``batch`` pending
        windows -- all of them still to have their language detected, or all of one language: the decoder's forced prompt is one row
        per batch --, gathers and encodes them (``forward_windows``), decodes on the timestamps plan and advances each file's seek by
        ``segments_of``.  A file's language is detected on its first window and forced on its later ones; with ``spec.language`` set it
        is forced from the start.  A finished file leaves and the next item is admitted.

        A round whose error word or range guard is set is run again window by window (``batchloop.run_or_each``); a window that still
        fails, or whose advance is 0 (HF's loop would not end), fails its FILE: printed, named in ``self.failed``, dropped with its
        later windows, no partial transcript.  The other files are neither touched nor run again.

        With thresholds in the spec (``logprob_threshold``, ``no_speech_threshold``, ``compression_ratio_threshold``) every window is
        decoded on the SCORED timestamps plan, and a window whose ``need_fallback`` says ``should_skip`` contributes no segments and
        advances the seek by its whole ``nf`` -- HF's seek loop, for every file, one-window files included.  A skipped window is
        progress.  A file whose windows were all skipped has the empty transcript and is no failure.  ``self.windows`` entries then are
        ``(seek, nf, advance, score_entry)``; ``scores=True`` asks for the scored plan and these entries without any threshold.

        Returns per item the ids without timestamp tokens (None: failed) and fills ``self.sequences`` (HF's: the segments' ids,
        timestamp tokens included), ``self.segments`` (absolute times), ``self.windows`` (per file ``[(seek, nf, advance)]``),
        ``self.next_seek`` (the final seek) and ``self.last_languages``.  Short files go through ``transcribe(..., timestamps=True)``."""
        if int(self.spec.num_beams) > 1:
            raise ValueError("long-form with num_beams > 1: long-form transcription with beam search is not built")
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch >= 1")
        tsb = self.spec.timestamp_begin
        limits = self.spec.thresholds
        scored = bool(scores) or any(v is not None for v in limits.values())
        check_thresholds(limits)
        V = self.dec.geo.decoder_vocab_size if scored else 0
        out: List[Optional[List[int]]] = []
        seqs: List[Optional[List[int]]] = []
        segments: List[Optional[list]] = []
        windows: List[Optional[list]] = []
        seeks: List[Optional[int]] = []
        langs: List[Optional[int]] = []
        failed: List[str] = []
        names: List[str] = []
        rounds: List[tuple] = []                            # (language key or None, [item index], [(seek, nf)]) per round that ran
        self.rounds = rounds

        def slot_for(name):
            for lst in (out, seqs, segments, windows, seeks, langs):
                lst.append(None)
            names.append(name)
            return len(out) - 1

        shorts: List[tuple] = []                            # (item index, wave)

        def flush_shorts():
            if not shorts:
                return
            idx = [i for i, _ in shorts]
            got = self.transcribe([w for _, w in shorts], [names[i] for i in idx], timestamps=True, **(dict(scores=True) if scored else {}))
            for k, i in enumerate(idx):
                out[i], segments[i], seeks[i], langs[i] = got[k], self.segments[k], self.next_seek[k], self.last_languages[k]
                if got[k] is not None and scored and self.scores[k]["skipped"]:
                    nf = window_frames(len(shorts[k][1]))                  # the one window is skipped whole: no segments, the seek at its end
                    out[i], segments[i], seqs[i], seeks[i] = [], [], [], nf
                    windows[i] = [(0, nf, nf, {n: v for n, v in self.scores[k].items() if n != "token_logprobs"})]
                elif got[k] is not None:
                    seqs[i] = [t for _, _, ids in self.segments[k] for t in ids]
                    windows[i] = [(0, window_frames(len(shorts[k][1])), int(self.next_seek[k]))]
                    if scored:
                        windows[i][0] += ({n: v for n, v in self.scores[k].items() if n != "token_logprobs"},)
            failed.extend(self.failed)
            shorts.clear()

        it = iter(items)
        exhausted = False
        resident: List[dict] = []
        handle = None
        forced = self.spec.language
        n_round = 0

        def drop(f, why=None):
            resident.remove(f)
            handle.release(f["file"])
            if why is not None:
                failed.append(names[f["i"]])
                print(f"Failed to process {names[f['i']]}: {why}")

        while True:
            new = []
            while not exhausted and len(resident) + len(new) < batch:
                try:
                    name, wave = next(it)
                except StopIteration:
                    exhausted = True
                    break
                wave = np.ascontiguousarray(wave, dtype=np.float32)
                i = slot_for(str(name))
                if is_long(len(wave)):
                    new.append((i, wave))
                else:
                    shorts.append((i, wave))
                    if len(shorts) == BATCH:
                        flush_shorts()
            if new:
                waves = [w for _, w in new]
                first = 0 if handle is None else len(handle)
                handle = self.enc.log_mel_long(self.enc.upload(waves, n_round % 2), [len(w) for w in waves], into=handle)
                for k, (i, w) in enumerate(new):
                    resident.append(dict(i=i, file=first + k, F=len(w) // HOP, seek=0, lang=forced, last=-1, seq=[], segs=[], wins=[]))
            if not resident:
                break
            key = min(resident, key=lambda f: f["last"])["lang"]      # the window that has waited longest names the round's language
            chosen = [f for f in resident if f["lang"] == key][:batch]
            slot = n_round % 2
            for f in chosen:
                f["last"] = n_round
            n_round += 1

            def run(fs):
                rows = [(f["file"], f["seek"], min(N_FRAMES, f["F"] - f["seek"])) for f in fs]
                rounds.append((key, [f["i"] for f in fs], [(s, nf) for _, s, nf in rows]))
                hs = self.enc.forward_windows(handle, rows, slot)
                res = self.dec.generate(hs.states[-1], len(fs), self.spec, language=key, slot=slot, timestamps=True,
                                        num_frames=[nf for _, _, nf in rows], **(dict(scores=True) if scored else {}))
                bits = hs.take_range_bits()
                if res.failed or bool(bits & 1):
                    return res
                for k, f in enumerate(fs):
                    seek, nf = rows[k][1], rows[k][2]
                    segs, adv = segments_of(res.lists[k], tsb, nf, float(seek) * TIME_PRECISION / INPUT_STRIDE)
                    f["lang"] = int(res.languages[k])
                    entry = None
                    if scored:
                        entry = score_entry(_with_eos(res, k, self.spec), res.avg_logprob[k], res.no_speech_prob[k], limits, V)
                    if entry is not None and entry["skipped"]:
                        segs, adv = [], nf                                  # HF: seek += seek_num_frames, and nothing is retrieved
                    elif adv <= 0:
                        drop(f, f"window at {seek * TIME_PRECISION_FEATURES:g} s made no progress")
                        continue
                    f["wins"].append((seek, nf, int(adv)) if entry is None else (seek, nf, int(adv), entry))
                    f["segs"].extend(segs)
                    f["seq"].extend(t for _, _, ids in segs for t in ids)
                    f["seek"] = seek + int(adv)
                    if f["seek"] >= f["F"]:
                        i = f["i"]
                        seqs[i], segments[i], windows[i], seeks[i], langs[i] = f["seq"], f["segs"], f["wins"], f["seek"], f["lang"]
                        out[i] = [t for t in f["seq"] if t < tsb]
                        drop(f)

            def fail(f, res):
                drop(f, f"window at {f['seek'] * TIME_PRECISION_FEATURES:g} s: decoder error word {res.err:#x}, "
                        f"range-guard bits {res.range_bits:#x}")

            run_or_each(chosen, run, fail, catch=())
        flush_shorts()
        self.sequences, self.segments, self.windows, self.next_seek, self.last_languages = seqs, segments, windows, seeks, langs
        self.failed = failed
        self.token_times = [None] * len(out)
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


_NO_SPACE_LANGUAGES = ("chinese", "japanese", "thai", "lao", "myanmar", "cantonese")
_PREPEND = "\"'\u201c\u00a1\u00bf([{-"
_APPEND = "\"'.\u3002,\uff0c!\uff01?\uff1f:\uff1a\u201d)]}\u3001"
_PUNCTUATION = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def _decode(tokenizer, ids):
    try:
        return tokenizer.decode(ids, decode_with_timestamps=True)
    except TypeError:                                       # a tokenizer without Whisper's keyword
        return tokenizer.decode(ids)


def combine_tokens_into_words(tokenizer, tokens: Sequence[int], language: Optional[str] = None):
    """HF's ``_combine_tokens_into_words`` (tokenization_whisper.py) restated over a tokenizer's ``decode``: (words, the token ids of each
    word, the token indices of each word).  Tokens join until their text decodes without a dangling replacement character; the pieces
    join into words at a leading space, a punctuation piece or a special token -- or stay as they are for the languages HF lists as
    written without spaces --; then punctuation merges into its neighbour."""
    tokens = [int(t) for t in tokens]
    if language is None:
        language = getattr(tokenizer, "language", None) or "english"
    full = _decode(tokenizer, tokens)
    pieces = []                                             # (text, ids, indices)
    cur, cur_idx, offset = [], [], 0
    for i, t in enumerate(tokens):
        cur.append(t)
        cur_idx.append(i)
        text = _decode(tokenizer, cur)
        at = text.find("\ufffd")
        if at < 0 or offset + at >= len(full) or full[offset + at] == "\ufffd":
            pieces.append((text, cur, cur_idx))
            cur, cur_idx = [], []
            offset += len(text)
    if language in _NO_SPACE_LANGUAGES:
        words = [[t, list(i), list(x)] for t, i, x in pieces]
    else:
        eos = getattr(tokenizer, "eos_token_id", None)
        words = []
        for text, ids, idx in pieces:
            special = eos is not None and ids[0] >= eos
            if special or text.startswith(" ") or text.strip() in _PUNCTUATION or not words:
                words.append([text, list(ids), list(idx)])
            else:
                words[-1][0] += text
                words[-1][1].extend(ids)
                words[-1][2].extend(idx)
    j = len(words) - 1                                      # punctuation that opens a word: right to left
    for i in range(len(words) - 2, -1, -1):
        if words[i][0].startswith(" ") and words[i][0].strip() in _PREPEND:
            words[j] = [words[i][0] + words[j][0], words[i][1] + words[j][1], words[i][2] + words[j][2]]
            words[i] = ["", [], []]
        else:
            j = i
    i = 0                                                   # punctuation that closes a word: left to right
    for j in range(1, len(words)):
        if not words[i][0].endswith(" ") and words[j][0] in _APPEND:
            words[i] = [words[i][0] + words[j][0], words[i][1] + words[j][1], words[i][2] + words[j][2]]
            words[j] = ["", [], []]
        else:
            i = j
    words = [w for w in words if w[0]]
    return [w[0] for w in words], [w[1] for w in words if w[1]], [w[2] for w in words if w[2]]


def token_spans(times: Sequence[float]):
    """(start, end) per token: its own time, and the time of the token behind it -- the last token ends where it starts (its time is the
    one HF repeats for the closing token)."""
    t = [float(x) for x in times]
    return [(t[k], t[k + 1] if k + 1 < len(t) else t[k]) for k in range(len(t))]


def token_words(tokenizer, ids: Sequence[int], times: Sequence[float], language: Optional[str] = None):
    """[(word, start_s, end_s)]: a word starts with its first token and ends where the token behind its last one starts."""
    spans = token_spans(times)
    words, _, indices = combine_tokens_into_words(tokenizer, ids, language)
    return [(w, spans[idx[0]][0], spans[idx[-1]][1]) for w, idx in zip(words, indices)]


def write_times_json(path: str, entries: dict) -> None:
    """``{file: {"text": s, "tokens": [[id, start_s, end_s], ...], "words": [[word, start_s, end_s], ...]}}``; ``words`` only where an
    entry has them (vocabulary files were found)."""
    with open(path, "w") as f:
        json.dump(entries, f, ensure_ascii=False, indent=1)
        f.write("\n")


def segments_entry(segments, next_seek: int, text: str, ts_begin: int, tokenizer=None) -> dict:
    """``{"text": s, "segments": [[start_s, end_s, text], ...], "next_seek_s": x}``; a segment's text is its ids without the timestamp
    tokens, decoded -- or, without vocabulary files, as numbers."""
    r = lambda x: round(float(x), 2)
    show = lambda t: tokenizer.decode(t, skip_special_tokens=True) if tokenizer is not None else " ".join(str(i) for i in t)
    return {"text": text, "segments": [[r(a), r(b), show([t for t in s if t < ts_begin])] for a, b, s in segments],
            "next_seek_s": r(next_seek * TIME_PRECISION_FEATURES)}


def times_entry(ids: Sequence[int], times: Sequence[float], text: str, tokenizer=None) -> dict:
    r = lambda x: round(float(x), 2)
    e = {"text": text, "tokens": [[int(t), r(a), r(b)] for t, (a, b) in zip(ids, token_spans(times))]}
    if tokenizer is not None:
        e["words"] = [[w, r(a), r(b)] for w, a, b in token_words(tokenizer, ids, times)]
    return e


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
    p.add_argument("--times_json", type=str, default="", help="also write token (and, with vocabulary files, word) times to this JSON file")
    p.add_argument("--num_beams", type=int, default=None, choices=range(1, C.GenerationSpec.MAX_BEAMS + 1), metavar="K",
                   help="beam search with K beams (HF's early_stopping=false); default: generation_config.json's num_beams, else greedy")
    p.add_argument("--length_penalty", type=float, default=None, help="with beams: the exponent of the length a finished score is divided by")
    p.add_argument("--segments_json", type=str, default="", help="decode with the model's own segment timestamps (first 30 s window of "
                   "each file) and also write them, with where the next window would begin, to this JSON file")
    p.add_argument("--long_form", action="store_true", help="decode every file with segment timestamps and files over 30 s window by "
                   "window to their end (HF's long-form generate); with --segments_json the segments carry absolute times")
    p.add_argument("--scores_json", type=str, default="", help="also write avg_logprob, no_speech_prob, compression_ratio, needs_fallback "
                   "and the token log-probabilities of every file to this JSON file (with --long_form: of every window)")
    p.add_argument("--logprob_threshold", type=float, default=None, help="with --long_form: HF generate()'s logprob_threshold; default: "
                   "generation_config.json's, else none")
    p.add_argument("--no_speech_threshold", type=float, default=None, help="with --long_form: a window whose no-speech probability is "
                   "above this and whose average log-probability is below --logprob_threshold is skipped whole")
    p.add_argument("--compression_ratio_threshold", type=float, default=None, help="with --long_form: reported as needs_fallback "
                   "(temperature fallback itself is not built)")
    return p


def parse_args(argv: Optional[Sequence[str]] = None):
    """The command line, with the combinations that are not built refused as argparse errors."""
    p = build_parser()
    args = p.parse_args(argv)
    if args.num_beams is not None and args.num_beams > 1 and args.times_json:
        p.error("--num_beams with --times_json: token times with beam search are not built")
    if args.segments_json and args.times_json:
        p.error("--segments_json with --times_json: segment timestamps with token times are not built")
    if args.segments_json and args.num_beams is not None and args.num_beams > 1:
        p.error("--segments_json with --num_beams: segment timestamps with beam search are not built")
    if args.long_form and args.times_json:
        p.error("--long_form with --times_json: long-form transcription with token times is not built")
    if args.long_form and args.num_beams is not None and args.num_beams > 1:
        p.error("--long_form with --num_beams: long-form transcription with beam search is not built")
    for flag in ("logprob_threshold", "no_speech_threshold", "compression_ratio_threshold"):
        if getattr(args, flag) is not None and not args.long_form:
            p.error(f"--{flag} without --long_form: the thresholds act in the long-form loop only (HF's skip of a silent window)")
    if args.no_speech_threshold is not None and args.logprob_threshold is None:
        p.error("--no_speech_threshold without --logprob_threshold: HF's rule compares the average log-probability in its no-speech branch")
    if args.scores_json and args.times_json:
        p.error("--scores_json with --times_json: transcript scores with token times are not built")
    if args.scores_json and args.num_beams is not None and args.num_beams > 1:
        p.error("--scores_json with --num_beams: transcript scores with beam search are not built")
    if args.length_penalty is not None and (args.num_beams is None or args.num_beams < 2):
        p.error("--length_penalty needs --num_beams K with K >= 2")
    return args


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
        try:
            with open(cfg, "r") as f:
                width = json.load(f).get("median_filter_width")
        except (OSError, ValueError):
            width = None
        if width is not None:                               # config.json's, where HF reads it
            import dataclasses
            spec = dataclasses.replace(spec, median_filter_width=int(width))
    enc_mode = args.mode if args.mode in ("f16x", "fp32x", "bf16") else "f16x"
    enc = WhisperEncoder(geo, sd, device, enc_mode)
    dec = WhisperDecoder(geo, sd, device, args.mode, spec)
    tok = None if args.synthetic_weights else load_tokenizer(args.tokenizer_path or args.ssl_type)
    return WhisperTranscriber(enc, dec, spec), tok


def run(argv: Optional[Sequence[str]] = None, spec: Optional[C.GenerationSpec] = None, geo=None, tokenizer=None) -> int:
    from .frontend import load_wav_16k
    args = parse_args(argv)
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
    want_times = bool(args.times_json)
    if want_times:
        try:
            tr.spec.require_alignment_heads()
        except ValueError as e:
            print(f"Error: {e}")
            return 0
    want_segments = bool(args.segments_json)
    if want_segments and args.num_beams is None and tr.spec.num_beams > 1:
        print("Error: --segments_json with num_beams > 1 in generation_config.json: segment timestamps with beam search are not built")
        return 0
    if args.long_form and tr.spec.num_beams > 1:
        print("Error: --long_form with num_beams > 1 in generation_config.json: long-form transcription with beam search is not built")
        return 0
    want_scores = bool(args.scores_json)
    if want_scores and args.num_beams is None and tr.spec.num_beams > 1:
        print("Error: --scores_json with num_beams > 1 in generation_config.json: transcript scores with beam search are not built")
        return 0
    given = {k: getattr(args, k) for k in ("logprob_threshold", "no_speech_threshold", "compression_ratio_threshold") if getattr(args, k) is not None}
    if given:                                               # the command line overrides generation_config.json's
        import dataclasses
        tr.spec = tr.dec.spec = dataclasses.replace(tr.spec, **given)
    if want_scores or args.long_form:                       # nothing else reads the thresholds: every other run is what it was
        try:
            check_thresholds(tr.spec.thresholds)
        except ValueError as e:
            print(f"Error: {e}")
            return 0
    entries, seg_entries, score_entries = {}, {}, {}
    if args.long_form:
        loaded = []

        def load_items():
            for n in names:
                try:
                    wave = load_wav_16k(os.path.join(args.wav_dir, n), resample=args.resample)
                except Exception as e:                      # noqa: BLE001
                    print(f"Failed to process {n}: {e}")
                    continue
                loaded.append(n)
                yield n, wave

        for k, ids in enumerate(tr.transcribe_long(load_items(), **(dict(scores=True) if want_scores else {}))):
            if ids is None:
                continue
            n = loaded[k]
            rows.append((n, tok.decode(ids, skip_special_tokens=True) if tok is not None else " ".join(str(t) for t in ids)))
            if want_segments and tr.segments[k] is not None:
                seg_entries[n] = segments_entry(tr.segments[k], tr.next_seek[k], rows[-1][1], tr.spec.timestamp_begin, tok)
                seg_entries[n]["windows"] = len(tr.windows[k])
            if want_scores:
                score_entries[n] = {"windows": [dict(seek_s=round(w[0] * TIME_PRECISION_FEATURES, 2), nf=int(w[1]), **w[3]) for w in tr.windows[k]]}
    for i in ([] if args.long_form else range(0, len(names), BATCH)):
        chunk, waves = [], []
        for n in names[i:i + BATCH]:
            try:
                waves.append(load_wav_16k(os.path.join(args.wav_dir, n), resample=args.resample))
                chunk.append(n)
            except Exception as e:                          # noqa: BLE001
                print(f"Failed to process {n}: {e}")
        beams = {} if args.num_beams is None else dict(num_beams=args.num_beams, length_penalty=args.length_penalty)
        if want_segments:
            beams["timestamps"] = True                      # the default call stays the one it always was
        if want_scores:
            beams["scores"] = True
        for k, (n, ids) in enumerate(zip(chunk, tr.transcribe(waves, chunk, first_batch=i // BATCH, token_times=want_times, **beams))):
            if ids is not None:
                rows.append((n, tok.decode(ids, skip_special_tokens=True) if tok is not None else " ".join(str(t) for t in ids)))
                if want_times and tr.token_times[k] is not None:
                    entries[n] = times_entry(ids, tr.token_times[k], rows[-1][1], tok)
                if want_segments and tr.segments[k] is not None:
                    seg_entries[n] = segments_entry(tr.segments[k], tr.next_seek[k], rows[-1][1], tr.spec.timestamp_begin, tok)
                if want_scores and tr.scores[k] is not None:
                    score_entries[n] = {f: v for f, v in tr.scores[k].items() if f != "skipped"}
    if want_scores:
        write_times_json(args.scores_json, score_entries)
        print(f"Wrote the scores of {len(score_entries)} files to {args.scores_json}")
    if want_segments:
        write_times_json(args.segments_json, seg_entries)
        print(f"Wrote the segments of {len(seg_entries)} files to {args.segments_json}")
    if want_times:
        write_times_json(args.times_json, entries)
        print(f"Wrote the token times of {len(entries)} files to {args.times_json}")
    write_table(args.out_csv, [r[0] for r in rows], [r[1] for r in rows])
    print(f"Wrote {len(rows)} of {len(names)} transcripts to {args.out_csv}")
    return 0
