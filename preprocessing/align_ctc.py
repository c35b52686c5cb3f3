#!/usr/bin/env python
"""Word times and acoustic scores of a transcript table (FileName,transcription: what transcribe_whisper.py and transcribe_ctc.py write)
by CTC forced alignment with a hub AutoModelForCTC checkpoint:

    python preprocessing/align_ctc.py --model facebook/hubert-xlarge-ls960-ft --wav_dir W --df_path transcripts.csv --out_json words.json
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.ctc import run_align  # noqa: E402

if __name__ == "__main__":
    sys.exit(run_align())
