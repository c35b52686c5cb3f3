#!/usr/bin/env python
"""Same command line as the reference's preprocessing/preprocess_ns3_prosody_speaker.py:

    python preprocessing/preprocess_ns3_prosody_speaker.py --wav_dir W --save_path S --num_workers 4 [--checkpoint DIR_OR_BIN]
        [--encoder_checkpoint DIR_OR_BIN] [--mode f16x] [--batch_size 16] [--synthetic_weights]

Reads ns3_facodec_decoder_v2.bin and, beside it, ns3_facodec_encoder_v2.bin (default ./pretrained_models/ns3/, the reference's paths).
Every file gets a [len // 200 + 1, 512] float32 tensor: prosody rows | timbre rows.  One GPU, 16 kHz input.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.prosody import run_speaker  # noqa: E402

if __name__ == "__main__":
    sys.exit(run_speaker())
