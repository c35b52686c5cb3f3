#!/usr/bin/env python
"""Same command line as the reference's benchmark/train_eval_files/eval_dim_ser.py (run from benchmark/, where configs/ lives, or
pass --config_path):

    python train_eval_files/eval_dim_ser.py --ssl_type wavlm-large --model_path model/dim_ser/7 --head_dim 1024
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from interspeech_ser_amd.baseline import run_eval_dim  # noqa: E402

if __name__ == "__main__":
    sys.exit(run_eval_dim())
