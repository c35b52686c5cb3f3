#!/usr/bin/env python
"""Test-set scoring from the corpus itself: the ``FileName`` column of ``./test/Categorical_test.csv`` (``--test_csv``), the wav files of the
config's ``wav_dir`` and the transcripts of its ``txt_dir`` through two or three encoders (``--encoder1 .. --encoder3``; Whisper, the speech
families, w2v-BERT 2.0 (``--encoder1 facebook/w2v-bert-2.0``), the Wav2Vec2-Conformer encoders (``--encoder1 facebook/wav2vec2-conformer-rope-large``), RoBERTa / DeBERTa, ``--encoder3 ns3-prosody --checkpoint3 <dir or .bin>`` for the prosody stream, ``--encoder3 ns3-prosody-speaker --checkpoint3 <dir>`` for
the 512-wide prosody | timbre stream of the reference's trimodal ``*_ns3`` configurations, or ``--encoder3 files`` for rows
from ``lazy_dir3``) and ``multimodal_ser.pt`` into ``results/test.csv`` -- the
file bin/test_cat_{bi,tri}modal_lazy_stacking_1head.py write, with no feature file in between (interspeech_ser_amd/predictor.py,
``score_from_wav``).  ``--transcribe`` takes the texts from the Whisper stream's own transcripts, ``--transcribe_ctc`` from the greedy CTC
transcripts of the audio encoder whose snapshot is a CTC checkpoint (``--encoder1 facebook/hubert-xlarge-ls960-ft --encoder2 roberta-large
--transcribe_ctc``); ``txt_dir`` is then not read.  One GPU, 16 kHz input."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.predictor import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
