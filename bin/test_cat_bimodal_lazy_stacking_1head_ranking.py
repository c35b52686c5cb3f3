#!/usr/bin/env python
"""Counterpart of the reference's bin/test_cat_bimodal_lazy_stacking_1head_ranking.py: the ``FileName`` column of
``./test/Categorical_test.csv`` (``--test_csv``) through ``multimodal_ser.pt`` into ``results/test.csv`` (interspeech_ser_amd/head.py, ``score``).
The ranking checkpoint's second classifier is ignored, as the reference's script throws its output away.
``--engine hip [--mode f16x|fp32x|bf16]`` runs the head as kernels of this library; the default ``--engine torch`` is the PyTorch module."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.head import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main(score_only=True))
