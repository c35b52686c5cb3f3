#!/usr/bin/env python
"""Greedy CTC transcripts of a wav directory from a hub AutoModelForCTC checkpoint, as the table the text drivers and the heads read
(FileName,transcription; the 960h models write upper-case letters without punctuation):

    python preprocessing/transcribe_ctc.py --model facebook/hubert-xlarge-ls960-ft --wav_dir W --out_csv ctc_transcripts.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.ctc import run  # noqa: E402

if __name__ == "__main__":
    sys.exit(run())
