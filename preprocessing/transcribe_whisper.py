#!/usr/bin/env python
"""Whisper's own transcripts of a wav directory, as the table the text drivers and the heads read (the reference:
test/Whisper transcriptions.ipynb -> whisper_transcripts.csv):

    python preprocessing/transcribe_whisper.py --ssl_type openai/whisper-large-v3 --wav_dir W --out_csv whisper_transcripts.csv
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.transcribe import run  # noqa: E402

if __name__ == "__main__":
    sys.exit(run())
