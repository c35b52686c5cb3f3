#!/usr/bin/env python
"""The trimodal head's Development-split evaluation, as bin/eval_cat_bimodal_lazy_1head.py does it for the bimodal one: macro-F1 and
``results/dev.csv`` (interspeech_ser_amd/head.py).  ``--engine hip [--mode f16x|fp32x|bf16]`` runs engine.TrimodalHead; the default
``--engine torch`` is the PyTorch module."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd.head import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main(evaluate_only=True, modalities=3))
