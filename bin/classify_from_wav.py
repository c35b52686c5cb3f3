#!/usr/bin/env python
"""Logits and labels of a hub audio-classification checkpoint (``AutoModelForAudioClassification``: the *ForSequenceClassification classes
of WavLM / wav2vec2 / HuBERT / data2vec-audio / w2v-BERT and WhisperForAudioClassification) for every wav file of a directory, on one GPU:

    bin/classify_from_wav.py --model NAME_OR_DIR --wav_dir W --out_csv preds.csv [--mode M] [--batch_size 16] [--resample] [--checkpoint FILE]

The CSV has the header ``FileName,label,<one column per label>`` and one row per file in sorted order; the values are the logits
(interspeech_ser_amd/classify.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.classify import run_classify  # noqa: E402

if __name__ == "__main__":
    sys.exit(run_classify())
