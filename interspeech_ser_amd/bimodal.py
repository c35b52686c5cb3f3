"""Waveform + tokens -> the bimodal head's logits on one device, with no feature file in between.

The reference's product path is three programs and a disk: the speech driver writes ``[T, D1]`` .pt files (preprocess_speech.py), the text
driver ``[80, D2]`` ones (preprocess_roberta.py), and bin/eval_cat_bimodal_lazy_1head.py reads both back for 8 logits.  ``BimodalPredictor``
runs the two encoders and ``engine.FusionHead`` back to back: the head reads the speech encoder's selected hidden state (or the mean of
the last four) and the text encoder's last state in place -- exactly the rows the two drivers would have written -- and only
``[B, n_out]`` floats come back.  Speech families only (not Whisper), one GPU, 16 kHz input."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ._lib import SerHipError
from .engine import FusionHead, SpeechEncoder, _TextEncoderBase, mean_last4


class BimodalPredictor:
    def __init__(self, speech_enc, text_enc, head_sd, speech_state: int, use_average: bool = False):
        if not isinstance(speech_enc, SpeechEncoder):
            raise ValueError("BimodalPredictor runs behind the speech encoders (WavLM / wav2vec2 / HuBERT / data2vec-audio), not Whisper")
        if not isinstance(text_enc, _TextEncoderBase):
            raise ValueError("BimodalPredictor needs a text encoder (RoBERTa / DeBERTa) for the second modality")
        if speech_enc.device != text_enc.device:
            raise ValueError(f"both encoders must live on one device, got {speech_enc.device} and {text_enc.device}")
        L = speech_enc.geo.num_layers
        if not use_average and not 0 <= int(speech_state) <= L:
            raise IndexError("tuple index out of range")               # what hidden_states[N] raises in the reference
        if use_average and L + 1 < 4:
            raise ValueError(f"use_average takes the mean of the last four hidden states; this speech encoder has only {L + 1}")
        self.speech, self.text = speech_enc, text_enc
        self.speech_state, self.use_average = int(speech_state), bool(use_average)
        self.head = FusionHead(head_sd, speech_enc.geo.hidden, text_enc.geo.hidden, speech_enc.device, speech_enc.mode_name)
        self.n_out = self.head.n_out

    def features(self, waves: Sequence[np.ndarray], input_ids: torch.Tensor, attention_mask: torch.Tensor):
        """(speech rows, their offsets, text rows, their offsets, the two forwards' HiddenStates): device tensors, nothing copied"""
        waves = [np.ascontiguousarray(w, dtype=np.float32) for w in waves]
        if len(waves) != input_ids.shape[0]:
            raise ValueError(f"{len(waves)} waveforms but {input_ids.shape[0]} token rows")
        lengths = [len(w) for w in waves]
        hs1 = self.speech.forward(self.speech.upload(waves), lengths, last_state=None if self.use_average else self.speech_state)
        x1 = mean_last4(hs1) if self.use_average else hs1.states[self.speech_state]
        hs2 = self.text.forward(input_ids, attention_mask)
        return x1, hs1.frame_offs, hs2.states[-1], hs2.frame_offs, hs1, hs2

    def predict(self, waves: Sequence[np.ndarray], input_ids: torch.Tensor, attention_mask: torch.Tensor) -> np.ndarray:
        """Raw 16 kHz mono waveforms and their tokenised transcripts (right-padded ``[B, T2]``) -> ``[B, n_out]`` float32 logits.  Every
        utterance alone: a result does not depend on which others share its batch.  Raises ``SerHipError`` when the fp16 range guard of
        either forward or of the head is set, or when ser_gru_v gave a cluster wait up."""
        x1, o1, x2, o2, hs1, hs2 = self.features(waves, input_ids, attention_mask)
        out = self.head.forward(x1, o1, x2, o2).cpu().numpy().copy()
        bits = hs1.take_range_bits() | hs2.take_range_bits()
        hbits, err = self.head.status()
        msg = FusionHead.failure(bits | hbits, err)
        if msg is not None:
            raise SerHipError(msg)
        return out
