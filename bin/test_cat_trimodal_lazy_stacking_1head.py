#!/usr/bin/env python
"""Counterpart of the reference's bin/test_cat_trimodal_lazy_stacking_1head.py: the ``FileName`` column of
``./test/Categorical_test.csv`` (``--test_csv``) through ``multimodal_ser.pt`` into ``results/test.csv`` (interspeech_ser_amd/head.py, ``score``).
``--engine hip [--mode f16x|fp32x|bf16]`` runs the head as kernels of this library; the default ``--engine torch`` is the PyTorch module."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.head import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main(score_only=True, modalities=3))
