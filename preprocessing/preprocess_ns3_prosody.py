#!/usr/bin/env python
"""Same command line as the reference's preprocessing/preprocess_ns3_prosody.py:

    python preprocessing/preprocess_ns3_prosody.py --wav_dir W --save_path S --num_workers 4 [--checkpoint DIR_OR_BIN] [--mode f16x]

Only ns3_facodec_decoder_v2.bin is read (default ./pretrained_models/ns3/, the reference's path).  One GPU, 16 kHz input.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.prosody import run  # noqa: E402

if __name__ == "__main__":
    sys.exit(run())
