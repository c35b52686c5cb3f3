#!/usr/bin/env python
"""x-vector speaker embeddings of a hub ``AutoModelForAudioXVector`` checkpoint (the *ForXVector classes of WavLM / wav2vec2 /
data2vec-audio / w2v-BERT, e.g. microsoft/wavlm-base-plus-sv) for every wav file of a directory, on one GPU:

    bin/embed_speakers_from_wav.py --model NAME_OR_DIR --wav_dir W --save_path S [--mode M] [--batch_size 16] [--resample]
                                   [--checkpoint FILE] [--trials T.txt --scores_csv out.csv]

Writes ``<S>/<utt>.pt``, a ``[xvector_output_dim]`` float32 tensor: HF's ``embeddings``, un-normalised.  With ``--trials`` every line
``fileA fileB`` of T.txt becomes a row ``fileA,fileB,cosine`` of out.csv (interspeech_ser_amd/xvector.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.xvector import run_embed  # noqa: E402

if __name__ == "__main__":
    sys.exit(run_embed())
