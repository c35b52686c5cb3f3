"""Waveforms (+ transcripts, + a third stream's rows) -> the fusion heads' logits on one device, behind any of the encoders.

``bimodal.BimodalPredictor`` runs one speech encoder and one text encoder in front of ``engine.FusionHead``.  The reference's strongest
systems sit behind Whisper (``whisperlarge_roberta_1head``, ``whisperlarge_deberta_lasthidden_head1``), behind two audio encoders and no
text at all (``whisperlarge_hubertxlarge_head1``), or behind three streams.  ``FusionPredictor`` takes two or three streams of any kind:
every encoder's forward runs on the current stream, and the head reads each stream's rows WHERE THEY LIE (``engine.RowSource``, one
ser_select_rows_v launch per stream): of a Whisper window only the ``min(ceil(len / 320), D)`` rows the reference keeps
(preprocess_whisper.py:49-50,75-76), the mean of the last four states without a buffer of its own.  Only ``[B, n_out]`` floats come back.
``score_from_wav`` is the test-set scoring of ``head.score`` from wav files and a transcript table, with no feature file in between
(bin/predict_cat_from_wav.py).  One GPU, 16 kHz input."""
from __future__ import annotations

import ctypes as C_
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import config as C
from .batchloop import close_logger, make_batches, prefetch, run_or_each, write_result_csv
from ._lib import SelectRowsArgs, SerHipError, check, lib
from .engine import (FusionHead, ProsodyEncoder, RowSource, SpeakerProsodyEncoder, SpeechEncoder, TrimodalHead, W2vBertEncoder, WhisperEncoder,
                     _TextEncoderBase, _stream)
from .frontend import whisper_saved_rows
from .prosody import NS3_PROSODY, NS3_PROSODY_SPEAKER


class AudioStream:
    """A speech encoder (WavLM / wav2vec2 / HuBERT / data2vec-audio) or Whisper over the batch's waveforms: ``hidden_states[state]``
    (negative ``state`` as Python indexes), or with ``average`` the mean of the last four states."""

    def __init__(self, enc, state: int = -1, average: bool = False):
        self.enc, self.state, self.average = enc, int(state), bool(average)
        # (Whisper) set by ``FusionPredictor.transcribe_with``: the forward's HiddenStates, B -> (input_ids, attention_mask) of the
        # batch's own transcripts; the forward then runs to its end and feeds the head's state and the decoder alike
        self.tokens_from_states = None


class TextStream:
    """A text encoder (RoBERTa / DeBERTa) over the batch's tokens: the last state -- all ``max_len`` rows, as the text driver writes them --
    or with ``average`` the mean of the last four."""

    def __init__(self, enc, average: bool = False):
        self.enc, self.average = enc, bool(average)


class RowsStream:
    """``[T, dim]`` rows per utterance handed in by the caller: a third stream read from feature files (``--encoder3 files``), whatever
    wrote them -- preprocessing/preprocess_ns3_prosody.py for the prosody stream, which ``ProsodyStream`` computes from the waveforms."""

    def __init__(self, dim: int):
        self.dim = int(dim)


class ProsodyStream:
    """The prosody encoder (``engine.ProsodyEncoder``) over the batch's waveforms: the ``[len // 200 + 1, D]`` rows the reference's
    preprocess_ns3_prosody.py saves per file, read by the head where the quantizer's lookup left them."""

    def __init__(self, enc):
        self.enc = enc


def gather_rows(src: RowSource, offs: Sequence[int]) -> torch.Tensor:
    """The rows a head reads through ``src`` with packed offsets ``offs``, as one fp32 ``[offs[-1], D]`` device tensor (ser_select_rows_v's
    fp32 output): what the extraction drivers would have written to the utterances' files."""
    offs = [int(v) for v in offs]
    B, D = len(offs) - 1, int(src.states[0].shape[1])
    dev = src.states[0].device
    src.check("gathered", offs, D, dev)
    out = torch.empty((offs[-1], D), dtype=torch.float32, device=dev)
    so, do = torch.tensor(src.src_offs, dtype=torch.int32, device=dev), torch.tensor(offs, dtype=torch.int32, device=dev)
    g = SelectRowsArgs()
    for k, s in enumerate(src.states):
        g.src[k] = s.data_ptr()
    g.ld_src, g.src_offs, g.dst_offs, g.out_f32, g.ldo_f32 = src.states[0].stride(0), so.data_ptr(), do.data_ptr(), out.data_ptr(), D
    g.n_src, g.B, g.D, g.max_rows, g.mode = len(src.states), B, D, max(b - a for a, b in zip(offs[:-1], offs[1:])), 1
    check(lib.ser_select_rows_v(C_.byref(g), _stream()), "ser_select_rows_v")
    return out


class FusionPredictor:
    """``streams``: two (``engine.FusionHead``) or three (``engine.TrimodalHead``, ``heads`` = (1, 1, 2) unless given) of ``AudioStream`` /
    ``TextStream`` / ``ProsodyStream`` / ``RowsStream``, in the order of the head's modalities; ``head_sd``: the head's state dict; ``head_mode``: its numerics
    (default: the first encoder's ``mode_name``).  All encoders and the head live on one device.  Constructor errors are
    ``BimodalPredictor``'s: ``IndexError("tuple index out of range")`` for a state outside the tuple, ``ValueError`` for a mean over fewer
    than four states or a stream width the state dict contradicts."""

    def __init__(self, streams, head_sd, head_mode: Optional[str] = None, heads: Optional[Sequence[int]] = None):
        streams = list(streams)
        if len(streams) not in (2, 3):
            raise ValueError(f"FusionPredictor runs two streams (engine.FusionHead) or three (engine.TrimodalHead), got {len(streams)}")
        encs = [s.enc for s in streams if not isinstance(s, RowsStream)]
        if not encs:
            raise ValueError("FusionPredictor needs at least one encoder stream (rows alone go to the head directly)")
        if len(set(map(id, encs))) != len(encs):
            raise ValueError("one encoder object cannot serve two streams (its second forward would overwrite the first one's states)")
        dims = []
        for i, s in enumerate(streams):
            if isinstance(s, RowsStream):
                dims.append(s.dim)
                continue
            if isinstance(s, ProsodyStream):
                if not isinstance(s.enc, (ProsodyEncoder, SpeakerProsodyEncoder)):
                    raise ValueError(f"stream {i + 1}: a ProsodyStream needs the prosody encoder")
            elif isinstance(s, AudioStream):
                if not isinstance(s.enc, (SpeechEncoder, WhisperEncoder, W2vBertEncoder)):
                    raise ValueError(f"stream {i + 1}: an AudioStream needs a speech encoder or Whisper")
            elif isinstance(s, TextStream):
                if not isinstance(s.enc, _TextEncoderBase):
                    raise ValueError(f"stream {i + 1}: a TextStream needs a text encoder (RoBERTa / DeBERTa)")
            else:
                raise ValueError(f"stream {i + 1}: expected an AudioStream, a TextStream, a ProsodyStream or a RowsStream")
            if s.enc.device != encs[0].device:
                raise ValueError(f"all encoders must live on one device, got {encs[0].device} and {s.enc.device}")
            if isinstance(s, ProsodyStream):
                dims.append(s.enc.spec.hidden)                            # (the speaker encoder's spec: both halves, 2 D)
                continue
            L = s.enc.geo.num_layers
            if s.average:
                if L + 1 < 4:
                    raise ValueError(f"average takes the mean of the last four hidden states; stream {i + 1}'s encoder has only {L + 1}")
            elif isinstance(s, AudioStream):
                idx = s.state if s.state >= 0 else L + 1 + s.state
                if not 0 <= idx <= L:
                    raise IndexError("tuple index out of range")           # what hidden_states[N] raises in the reference
                s.index = idx
            dims.append(s.enc.geo.hidden)
        self.streams, self.device = streams, encs[0].device
        mode = head_mode or encs[0].mode_name                              # the first stream's (the first encoder's, behind a RowsStream)
        if len(streams) == 3:
            self.head = TrimodalHead(head_sd, *dims, self.device, mode, heads=tuple(heads) if heads is not None else (1, 1, 2))
        else:
            if heads is not None and tuple(heads) != (1, 1):
                raise ValueError("the bimodal head's two attention modules have one head each")
            self.head = FusionHead(head_sd, *dims, self.device, mode)
        self.n_out = self.head.n_out

    def transcribe_with(self, decoder, spec, tokenize, detokenize=None) -> None:
        """Texts from the Whisper stream's own transcript instead of the caller's tokens: ``decoder`` (``engine.WhisperDecoder`` over the
        Whisper stream's checkpoint) decodes greedily from the last state of that stream's forward, ``detokenize(ids) -> str`` (default:
        the ids as decimal numbers, what preprocessing/transcribe_whisper.py writes without vocabulary files) and ``tokenize(texts) ->
        (input_ids, attention_mask)`` turn the ids into the text stream's input.  A batch whose decoder error word or range guard is set
        raises ``SerHipError``, like a failed forward."""
        audio = [s for s in self.streams if isinstance(s, AudioStream) and isinstance(s.enc, WhisperEncoder)]
        if not audio or not any(isinstance(s, TextStream) for s in self.streams):
            raise ValueError("transcription needs a Whisper audio stream and a text stream")
        detok = detokenize or (lambda ids: " ".join(str(t) for t in ids))

        def tokens(hs, B):
            res = decoder.generate(hs.states[-1], B, spec)
            if res.failed:
                hs.take_range_bits()                    # predict() will not get to it: a bit left set would fail the next batch's first forward
                raise SerHipError(f"transcription failed: decoder error word {res.err:#x}, range-guard bits {res.range_bits:#x}")
            self.last_texts = [detok(ids) for ids in res.lists]
            return tokenize(self.last_texts)
        audio[0].tokens_from_states = tokens

    def transcribe_with_ctc(self, head, detokenize=None, tokenize=None) -> None:
        """Texts from a CTC checkpoint's greedy transcript: ``head`` (``engine.CTCHead``) sits behind the encoder of one of the speech
        ``AudioStream``s, whose snapshot is the CTC checkpoint's.  One forward of that stream then feeds both the fusion head (its selected
        state) and the text stream (the last state, through the head): ``detokenize(ids) -> str`` (default: the ids as decimal numbers,
        what preprocessing/transcribe_ctc.py writes without vocabulary files) and ``tokenize(texts) -> (input_ids, attention_mask)`` turn
        the ids into the text stream's input.  A batch whose error word is set raises ``SerHipError``, like a failed forward."""
        audio = [s for s in self.streams if isinstance(s, AudioStream) and s.enc is head.enc]
        if not audio or not any(isinstance(s, TextStream) for s in self.streams):
            raise ValueError("CTC transcription needs the audio stream whose encoder the CTC head sits behind, and a text stream")
        if tokenize is None:
            raise ValueError("CTC transcription needs tokenize(texts) -> (input_ids, attention_mask)")
        detok = detokenize or (lambda ids: " ".join(str(t) for t in ids))

        def tokens(hs, B):
            from .engine import CTCHead
            words = head.forward_tokens(hs).cpu().numpy()
            part = CTCHead.unpack(words, B, max(hs.frames(b) for b in range(B)))
            if part["err"]:
                hs.take_range_bits()                    # predict() will not get to it: a bit left set would fail the next batch's first forward
                raise SerHipError(f"transcription failed: CTC error word {part['err']:#x} (a frame's winning logit was not finite)")
            self.last_ids = [[int(t) for t in part["ids"][b, : int(part["counts"][b])]] for b in range(B)]
            self.last_texts = [detok(ids) for ids in self.last_ids]
            return tokenize(self.last_texts)
        audio[0].tokens_from_states = tokens

    @staticmethod
    def _source(s, hs, counts):
        """the stream's rows inside its forward's states, ``counts[b]`` of them from each utterance's first row"""
        if s.average:
            if hs.computed < hs.states.shape[0]:
                raise IndexError("mean of the last four states needs the full forward")
            states = [hs.states[k] for k in (-4, -3, -2, -1)]
        else:
            states = [hs.states[s.index if isinstance(s, AudioStream) else -1]]
        return RowSource(states, hs.frame_offs[:-1]), [0] + [int(v) for v in np.cumsum(counts)], hs

    def features(self, waves: Optional[Sequence[np.ndarray]] = None, input_ids: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, rows=None) -> List[tuple]:
        """Per stream ``(rows, packed offsets, the forward's HiddenStates)``: the rows are an ``engine.RowSource`` over the encoder's
        states (nothing copied; valid until that encoder's next forward), or for a ``RowsStream`` the caller's rows packed on the device
        (and None for the HiddenStates).  The forwards run on the current stream in the order of the streams."""
        B = None
        if any(isinstance(s, (AudioStream, ProsodyStream)) for s in self.streams):
            if waves is None:
                raise ValueError("an AudioStream or a ProsodyStream needs waves")
            waves = [np.ascontiguousarray(w, dtype=np.float32) for w in waves]
            B = len(waves)
        transcriber = next((s for s in self.streams if isinstance(s, AudioStream) and s.tokens_from_states is not None), None)
        if any(isinstance(s, TextStream) for s in self.streams) and transcriber is None:
            if input_ids is None or attention_mask is None:
                raise ValueError("a TextStream needs input_ids and attention_mask")
            if B is not None and input_ids.shape[0] != B:
                raise ValueError(f"{B} waveforms but {input_ids.shape[0]} token rows")
            B = int(input_ids.shape[0])
        if any(isinstance(s, RowsStream) for s in self.streams):
            if rows is None:
                raise ValueError("a RowsStream needs rows: one [T, D] matrix per utterance")
            if len(rows) != B:
                raise ValueError(f"{len(rows)} row matrices for {B} utterances")
        out = []
        # with a transcriber its stream goes first: the text stream's tokens come out of it
        order = self.streams if transcriber is None else [transcriber] + [s for s in self.streams if s is not transcriber]
        for s in order:
            if isinstance(s, AudioStream):
                lengths = [len(w) for w in waves]
                full = s.average or s is transcriber            # the decoder reads the LAST state: that forward does not stop early
                hs = s.enc.forward(s.enc.upload(waves), lengths, last_state=None if full else s.index)
                if s is transcriber:
                    input_ids, attention_mask = s.tokens_from_states(hs, B)
                if isinstance(s.enc, WhisperEncoder):                      # the rows the reference keeps of each 1 500-row window
                    counts = [min(whisper_saved_rows(n, s.enc.geo.hidden), hs.frames(b)) for b, n in enumerate(lengths)]
                else:
                    counts = [hs.frames(b) for b in range(B)]
                out.append(self._source(s, hs, counts))
            elif isinstance(s, TextStream):
                hs = s.enc.forward(input_ids, attention_mask)
                out.append(self._source(s, hs, [hs.frames(b) for b in range(B)]))
            elif isinstance(s, ProsodyStream):
                hs = s.enc.forward(waves)                                  # (a wave under 400 samples raises: the batch is retried file by file)
                out.append((RowSource(hs.rows, hs.frame_offs[:-1]), list(hs.frame_offs), hs))
            else:
                mats = []
                for r in rows:
                    r = torch.as_tensor(r)
                    if r.dim() == 3 and r.shape[-1] == 1:
                        r = r.squeeze(-1)                                  # the reference squeezes the third stream's last axis
                    if r.dim() != 2 or r.shape[0] < 1 or r.shape[1] != s.dim:
                        raise ValueError(f"rows must be [T >= 1, {s.dim}] matrices, got {tuple(r.shape)}")
                    mats.append(r.float().contiguous())
                out.append((torch.cat(mats).to(self.device), [0] + [int(v) for v in np.cumsum([m.shape[0] for m in mats])], None))
        if transcriber is not None:
            out = [out[order.index(s)] for s in self.streams]
        return out

    def predict(self, waves: Optional[Sequence[np.ndarray]] = None, input_ids: Optional[torch.Tensor] = None,
                attention_mask: Optional[torch.Tensor] = None, rows=None) -> np.ndarray:
        """Raw 16 kHz mono waveforms (every audio stream reads the same ones), right-padded tokens ``[B, T2]`` and / or per-utterance rows
        -> ``[B, n_out]`` float32 logits, every utterance alone.  Raises ``SerHipError`` when the fp16 range guard of a forward or of the
        head is set, or when ser_gru_v gave a cluster wait up."""
        feats = self.features(waves, input_ids, attention_mask, rows)
        args = []
        for x, offs, _ in feats:
            args += [x, offs]
        out = self.head.forward(*args).cpu().numpy().copy()
        bits = 0
        for _, _, hs in feats:
            if hs is not None:
                bits |= hs.take_range_bits()
        hbits, err = self.head.status()
        msg = FusionHead.failure(bits | hbits, err)
        if msg is not None:
            raise SerHipError(msg)
        return out


# ----------------------------------------------------------------------------------------------------- test-set scoring from wav files
FILES = "files"           # --encoder3 files: the third stream is read from config["lazy_dir3"]


def _stream_kinds(config: Dict, encoders: Sequence[str], checkpoints: Sequence[str], synthetic: bool = False):
    """(geometry, ``prosody.ProsodySpec`` for "ns3-prosody", or None for "files") per stream, checked against the config's feat{i}_dim
    -- before any weight is loaded (the prosody checkpoint's shapes are read, mapped where the file allows)"""
    if len(encoders) not in (2, 3):
        raise ValueError(f"two or three encoders, got {len(encoders)}")
    geos = []
    for i, name in enumerate(encoders):
        want = int(config[f"feat{i + 1}_dim"])
        if name == FILES:
            if i != 2:
                raise ValueError("only the third stream can be read from files (--encoder3 files)")
            geos.append(None)
            continue
        if name == NS3_PROSODY:
            from .prosody import resolve_spec
            geo = resolve_spec(checkpoints[i], synthetic)
        elif name == NS3_PROSODY_SPEAKER:
            from .prosody import resolve_codec_spec
            geo = resolve_codec_spec(checkpoints[i], synthetic)
        else:
            geo = C.resolve_fbank(C.resolve_geometry(name, checkpoints[i]), name, checkpoints[i])
        if geo.hidden != want:
            raise ValueError(f"feat{i + 1}_dim = {want} in the config, but {name} has hidden size {geo.hidden}")
        geos.append(geo)
    if all(g is None or g.family in (C.FAMILY_ROBERTA, C.FAMILY_DEBERTA) for g in geos):
        raise ValueError("no audio encoder among the streams: this command scores wav files (head.score reads feature files)")
    return geos


def score_from_wav(config: Dict, encoders: Sequence[str], layers: Optional[Sequence[int]] = None, averages: Optional[Sequence[bool]] = None,
                   checkpoints: Optional[Sequence[str]] = None, test_csv: Optional[str] = None, mode: str = "f16mf", text_mode: str = "f16x",
                   head_mode: Optional[str] = None, batch_size: int = 16, num_workers: int = 4, tokenizer_path: str = "", max_len: int = 80,
                   synthetic_weights: bool = False, seed: int = 7, device: Optional[str] = None, tokenize=None, transcribe: bool = False,
                   spec: Optional[C.GenerationSpec] = None, detokenize=None, language=None, transcribe_ctc: bool = False) -> Dict:
    """``head.score(engine="hip")`` from the corpus itself: the ``FileName`` column of ``test_csv``, wavs from ``config["wav_dir"]``
    (16 kHz), transcripts from the table ``config["txt_dir"]`` (columns FileName, transcription), the head's weights from
    ``<model_path>/multimodal_ser.pt`` -> ``<model_path>/results/test.csv`` in ``head.score``'s format.  ``encoders``: two or three
    encoder ids (``config.resolve_geometry``; the family decides the stream kind); "ns3-prosody" is the prosody stream
    (``engine.ProsodyEncoder``, checkpoint: a directory holding ns3_facodec_decoder_v2.bin, or the file), and the third may be "files"
    (rows from ``config["lazy_dir3"]``).  ``layers[i]`` / ``averages[i]``: the state an audio stream hands on; a text stream hands on its last state
    or the mean.  ``mode`` / ``text_mode`` / ``head_mode``: numerics of the audio encoders, the text encoders and the head (default: the
    first encoder's).  ``tokenize``: texts -> (input_ids, attention_mask), default ``driver.hf_tokenize_fn``.  A file that cannot be
    decoded, has no transcript or is empty is printed and gets no row; a batch whose range-guard or GRU error word is set is retried file
    by file (``batchloop.run_or_each``).  ``transcribe``: the texts are the Whisper stream's own transcripts (``FusionPredictor.transcribe_with``) and ``txt_dir`` is not
    read; ``spec`` (default: the checkpoint's generation_config.json, with ``language``) and ``detokenize`` (default: the checkpoint's
    tokenizer from local files, else the ids as numbers) belong to it.  ``transcribe_ctc``: the texts are the greedy CTC transcripts of the
    first speech stream whose snapshot is a CTC checkpoint (``FusionPredictor.transcribe_with_ctc``; ``detokenize`` default: the
    snapshot's vocab.json, else the ids as numbers) and ``txt_dir`` is not read.  Returns {"csv", "n", "failed"}."""
    from . import head as HD
    from .driver import _Extractor, find_weights, hf_tokenize_fn
    from .engine import build_encoder
    from .frontend import load_wav_16k
    n = len(encoders)
    layers = list(layers) if layers is not None else [-1] * n
    averages = list(averages) if averages is not None else [False] * n
    checkpoints = list(checkpoints) if checkpoints is not None else [""] * n
    geos = _stream_kinds(config, encoders, checkpoints, synthetic_weights)
    if max_len > 512:
        raise ValueError(f"max_len {max_len}: the text encoders have 512 positions (the reference uses 80)")
    if not torch.cuda.is_available():
        print(HD.NO_CPU_PATH)
        return {"csv": None, "n": 0, "failed": 0}
    import pandas as pd
    HD.set_deterministic(seed)
    dev = str(torch.device(device or "cuda:0"))
    model_path = config["model_path"]
    os.makedirs(model_path, exist_ok=True)
    log = HD._logger(model_path)
    names = pd.read_csv(test_csv or HD.TEST_CSV)["FileName"].tolist()
    texts: Dict[str, str] = {}
    streams = []
    decoder = None
    if transcribe and not (any(g is not None and g.family == C.FAMILY_WHISPER and g.decoder_layers > 0 for g in geos)
                           and any(g is not None and g.family in (C.FAMILY_ROBERTA, C.FAMILY_DEBERTA) for g in geos)):
        raise ValueError("transcribe needs a Whisper encoder whose checkpoint has a decoder, and a text encoder")
    ctc_head, ctc_at = None, -1
    if transcribe_ctc:
        if transcribe:
            raise ValueError("transcribe and transcribe_ctc are two sources of the same texts: choose one")
        speech = C.SPEECH_FAMILIES + (C.FAMILY_W2V_BERT,)
        ctc_at = next((i for i, g in enumerate(geos) if g is not None and g.family in speech and C.resolve_ctc(encoders[i], checkpoints[i]) is not None), -1)
        if ctc_at < 0 or not any(g is not None and g.family in (C.FAMILY_ROBERTA, C.FAMILY_DEBERTA) for g in geos):
            raise ValueError("transcribe_ctc needs an audio encoder whose snapshot is a CTC checkpoint (config.json names one of "
                             + ", ".join(C.CTC_ARCHITECTURES) + "), and a text encoder")
    own_text = transcribe or transcribe_ctc               # the texts come out of an audio stream: txt_dir is not read
    for i, (name, geo) in enumerate(zip(encoders, geos)):
        if geo is None:
            streams.append(RowsStream(int(config[f"feat{i + 1}_dim"])))
            continue
        if geo.family == NS3_PROSODY:
            from . import prosody as P
            if synthetic_weights and not checkpoints[i]:
                sd, src = P.synthetic_state_dict(geo, seed), f"synthetic weights (seed {seed})"
            else:
                sd, src = P.load_state_dict(checkpoints[i]), f"checkpoint {P.checkpoint_path(checkpoints[i])}"
            enc = ProsodyEncoder(sd, dev, mode if mode in ("f16x", "fp32x", "bf16") else "f16x")      # the encoders' mode where it has it
            streams.append(ProsodyStream(enc))
            print(f"Stream {i + 1}: {name} ({src}; numerics mode {enc.mode_name})")
            del sd
            continue
        if geo.family == NS3_PROSODY_SPEAKER:
            from . import prosody as P
            if synthetic_weights and not checkpoints[i]:
                sd, enc_sd = P.synthetic_state_dict(geo.timbre, seed), P.synthetic_codec_state_dict(geo, seed)
                sd.update(P.synthetic_timbre_state_dict(geo.timbre, seed))
                src = f"synthetic weights (seed {seed})"
            else:
                sd, enc_sd = P.load_state_dict(checkpoints[i]), P.load_encoder_state_dict(checkpoints[i])
                src = f"checkpoints {P.checkpoint_path(checkpoints[i])}, {P.encoder_checkpoint_path(checkpoints[i])}"
            enc = SpeakerProsodyEncoder(sd, enc_sd, dev, mode if mode in ("f16x", "fp32x", "bf16") else "f16x")
            streams.append(ProsodyStream(enc))
            print(f"Stream {i + 1}: {name} ({src}; numerics mode {enc.mode_name})")
            del sd, enc_sd
            continue
        text = geo.family in (C.FAMILY_ROBERTA, C.FAMILY_DEBERTA)
        whisper = geo.family == C.FAMILY_WHISPER
        if i == ctc_at:
            from .weights import CTC_HEAD_PREFIXES, split_ctc_head
            sd, src = find_weights(name, checkpoints[i], False, seed, geo, keep=CTC_HEAD_PREFIXES)      # never synthetic: they have no lm_head
            sd, ctc_sd = split_ctc_head(sd)
        else:
            sd, src = find_weights(name, checkpoints[i], synthetic_weights, seed, geo)
        if text:
            if tokenize is None:
                tokenize = hf_tokenize_fn(tokenizer_path or name, max_len, geo.family)
            if not texts and not own_text:
                from .transcribe import read_table
                texts = read_table(config["txt_dir"])
            enc = build_encoder(geo, sd, dev, text_mode)
            streams.append(TextStream(enc, averages[i]))
        else:
            m = _Extractor.supported_mode(geo, mode, whisper, name)
            enc = build_encoder(geo, sd, dev, m, normalize=True if whisper else C.resolve_do_normalize(name, checkpoints[i]))
            streams.append(AudioStream(enc, layers[i], averages[i]))
            if i == ctc_at:
                from .ctc import load_vocab
                from .engine import CTCHead
                ctc_head = CTCHead(enc, ctc_sd, C.resolve_ctc(name, checkpoints[i]))
                if detokenize is None:
                    cfg_json = C.find_config_json(name, checkpoints[i])
                    vocab = load_vocab(os.path.dirname(cfg_json) if cfg_json else name)
                    detokenize = None if vocab is None else vocab.text
            if transcribe and whisper and decoder is None and geo.decoder_layers > 0:
                from .engine import WhisperDecoder
                from .transcribe import load_tokenizer
                if synthetic_weights:
                    from .weights import synthetic_decoder_state_dict
                    sd = dict(sd)
                    sd.update(synthetic_decoder_state_dict(geo, seed))
                if spec is None:
                    cfg_json = C.find_config_json(name, checkpoints[i])
                    if not cfg_json:
                        raise OSError(f"no generation_config.json for {name} (it lies beside config.json in a local snapshot)")
                    spec = C.GenerationSpec.from_snapshot(os.path.dirname(cfg_json), language)
                decoder = WhisperDecoder(geo, sd, dev, m, spec)
                if detokenize is None and not synthetic_weights:
                    tok = load_tokenizer(tokenizer_path or name)
                    detokenize = None if tok is None else (lambda ids, tok=tok: tok.decode(ids, skip_special_tokens=True))
        print(f"Stream {i + 1}: {name} ({src}; numerics mode {enc.mode_name})")
        del sd
    head_sd = torch.load(os.path.join(model_path, "multimodal_ser.pt"), map_location="cpu", weights_only=True)
    pred = FusionPredictor(streams, head_sd, head_mode)
    if transcribe:
        pred.transcribe_with(decoder, spec, tokenize, detokenize)
    if transcribe_ctc:
        pred.transcribe_with_ctc(ctc_head, detokenize, tokenize)
    has_text, has_rows = any(isinstance(s, TextStream) for s in streams), any(isinstance(s, RowsStream) for s in streams)
    log.info("Starting scoring test samples...")
    done, rows_out, failed = [], [], 0

    def fail(name, err):
        nonlocal failed
        failed += 1
        print(f"Failed to process {name}: {err}")

    def load(name):
        """(name, waveform, transcript, third stream's rows, error)"""
        try:
            wave = load_wav_16k(os.path.join(config["wav_dir"], name))
            if len(wave) < 1:
                raise ValueError("empty waveform")
            text = None
            if has_text and not own_text:
                if name not in texts:
                    raise KeyError(f"no transcript in {config['txt_dir']}")
                text = texts[name]
            third = None
            if has_rows:
                third = torch.load(os.path.join(config["lazy_dir3"], name.replace(".wav", ".pt")), weights_only=True)
                if third.dim() == 3 and third.shape[-1] == 1:
                    third = third.squeeze(-1)                          # the reference squeezes the third stream's last axis
                if third.dim() != 2 or third.shape[0] < 1:
                    raise ValueError(f"feature files must hold [T >= 1, D] matrices, got {tuple(third.shape)}")
            return name, wave, text, third, None
        except Exception as e:                                          # noqa: BLE001  (per-file failure, as in the extraction drivers)
            return name, None, None, None, e

    def run(items):
        """items: (name, waveform, transcript, rows); appends the rows of a clean batch, raises what a failed one raises"""
        ids = mask = None
        if has_text and not own_text:
            ids, mask = tokenize([it[2] for it in items])
        out = pred.predict([it[1] for it in items], ids, mask, [it[3] for it in items] if has_rows else None)
        for it, row in zip(items, out):
            done.append(it[0])
            rows_out.append(row)

    with ThreadPoolExecutor(max_workers=max(1, int(num_workers))) as pool:
        # the next batch is decoded while the GPU works
        for loaded in prefetch(make_batches(names, max(1, int(batch_size))), pool, load):
            items = []
            for name, wave, text, third, err in loaded:
                if err is not None:
                    fail(name, err)
                else:
                    items.append((name, wave, text, third))
            if items:
                run_or_each(items, run, lambda it, e: fail(it[0], e))                         # one bad file must not drop its neighbours
    csv_file = write_result_csv(model_path, "test", "FileName", done, rows_out, HD.CLASS_LETTERS)
    print(f"{len(done)} rows written, {failed} files failed")
    close_logger(log)
    return {"csv": csv_file, "n": len(done), "failed": failed}


def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    import json
    from . import head as HD
    p = argparse.ArgumentParser(description="score a test set from wav files and transcripts: encoders and fusion head on one GPU")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--config_path", type=str, default="./configs/config_cat.json")
    for i in (1, 2, 3):
        p.add_argument(f"--encoder{i}", type=str, default="" if i == 3 else None, required=i < 3,
                       help="encoder id" + (' or "ns3-prosody" (the prosody stream, --checkpoint3 <dir or .bin>), "ns3-prosody-speaker" (prosody | timbre rows, '
                                           '--checkpoint3 <dir with both FACodec files>) or "files" (rows from lazy_dir3); '
                                           'empty: two streams' if i == 3 else ""))
        p.add_argument(f"--layer{i}", type=int, default=-1, help="audio stream: hidden_states[N]")
        p.add_argument(f"--average{i}", action="store_true", help="the mean of the last four hidden states")
        p.add_argument(f"--checkpoint{i}", type=str, default="")
    p.add_argument("--test_csv", type=str, default=HD.TEST_CSV)
    p.add_argument("--mode", type=str, default="f16mf", help="numerics of the audio encoders (the extraction drivers' --mode)")
    p.add_argument("--text_mode", type=str, default="f16x", help="numerics of the text encoders")
    p.add_argument("--head_mode", type=str, default=None, help="numerics of the head (default: the first encoder's)")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--tokenizer_path", type=str, default="")
    p.add_argument("--max_len", type=int, default=80)
    p.add_argument("--synthetic_weights", action="store_true")
    p.add_argument("--transcribe", action="store_true", help="texts from the Whisper stream's own transcripts (no txt_dir)")
    p.add_argument("--language", type=str, default=None, help="with --transcribe: e.g. en; default: detected per utterance")
    p.add_argument("--transcribe_ctc", action="store_true",
                   help="texts from the greedy CTC transcripts of the audio encoder whose snapshot is a CTC checkpoint (no txt_dir)")
    a = p.parse_args(argv)
    with open(a.config_path, "r") as f:
        config = json.load(f)
    k = 3 if a.encoder3 else 2
    pick = lambda what: [getattr(a, f"{what}{i}") for i in range(1, k + 1)]
    score_from_wav(config, pick("encoder"), pick("layer"), pick("average"), pick("checkpoint"), test_csv=a.test_csv, mode=a.mode,
                   text_mode=a.text_mode, head_mode=a.head_mode, batch_size=a.batch_size, num_workers=a.num_workers,
                   tokenizer_path=a.tokenizer_path, max_len=a.max_len, synthetic_weights=a.synthetic_weights, seed=a.seed,
                   transcribe=a.transcribe, language=a.language, transcribe_ctc=a.transcribe_ctc)
    return 0
