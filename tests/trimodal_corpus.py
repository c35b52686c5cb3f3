"""The tiny synthetic scoring corpus shared by tests/test_trimodal_host.py and tests/test_gpu_trimodal.py: 5 files, feature widths
(64, 128, 64), a seeded head of hidden width 64 (bimodal or trimodal, plain or with a ranking checkpoint's extra keys), a test CSV."""
import json
import os

import numpy as np
import torch

import fusion3_ref as R3
import fusion_ref as R

DIMS, H, SEED = (64, 128, 64), 64, 5
LENGTHS = ((1, 17, 40, 9, 12), (5, 1, 16, 7, 3), (33, 2, 64, 5, 20))
NAMES = [f"MSP-PODCAST_test_{i:04d}.wav" for i in range(5)]
RANKING_PREFIX = {2: "neutral_classifier", 3: "classifier_neutral"}        # the second classifier of the reference's two ranking classes


def head_weights(modalities):
    from oracle.fusion_head import seeded_head_weights
    shapes = R3.head_shapes(*DIMS, h=H) if modalities == 3 else R.head_shapes(DIMS[0], DIMS[1], h=H)
    return seeded_head_weights(shapes, SEED)


def rows():
    return R3.seeded_rows(DIMS, LENGTHS, SEED + 1000)


def float64_logits(modalities, q=None):
    sd, xs = head_weights(modalities), rows()
    return R3.batch_logits(sd, *xs, q) if modalities == 3 else R.batch_logits(sd, xs[0], xs[1], q)


def torch_logits(modalities):
    sd, xs = head_weights(modalities), rows()
    return R3.torch_logits(sd, *xs) if modalities == 3 else R.oracle_logits(sd, xs[0], xs[1])


def make(root, modalities, ranking=False, third_axis=True):
    """write the corpus under ``root`` (a pathlib.Path) -> dict(cfg, cfg_path, test_csv, names, sd, xs).  ``third_axis``: file 1 of the
    third stream is stored [T, D, 1], the shape the reference's ``squeeze(-1)`` is there for."""
    import pandas as pd
    from interspeech_ser_amd.frontend import feature_path, save_feature
    xs = rows()
    lazy = [root / f"stream{i + 1}" for i in range(3)]
    for m, d in enumerate(lazy):
        d.mkdir(parents=True, exist_ok=True)
        for k, (name, x) in enumerate(zip(NAMES, xs[m])):
            if m == 2 and k == 1 and third_axis:
                torch.save(torch.from_numpy(x)[..., None].clone(), feature_path(str(d), name))
            else:
                save_feature(torch.from_numpy(x), feature_path(str(d), name))
    sd = dict(head_weights(modalities))
    if ranking:
        g = torch.Generator().manual_seed(9)
        pre = RANKING_PREFIX[modalities]
        sd.update({f"{pre}.0.weight": torch.randn(H, 2 * H * modalities, generator=g), f"{pre}.0.bias": torch.randn(H, generator=g),
                   f"{pre}.3.weight": torch.randn(1, H, generator=g), f"{pre}.3.bias": torch.randn(1, generator=g)})
    pd.DataFrame({"FileName": NAMES}).to_csv(root / "Categorical_test.csv", index=False)
    cfg = {"wav_dir": "/corpus/Audios", "lazy_dir1": str(lazy[0]), "lazy_dir2": str(lazy[1]), "lazy_dir3": str(lazy[2]),
           "feat1_dim": DIMS[0], "feat2_dim": DIMS[1], "feat3_dim": DIMS[2],
           "model_path": str(root / f"exp{modalities}{'r' if ranking else ''}"), "batch_size": 4}
    os.makedirs(cfg["model_path"], exist_ok=True)
    torch.save(sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
    cfg_path = root / f"cfg{modalities}{'r' if ranking else ''}.json"
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    return dict(cfg=cfg, cfg_path=str(cfg_path), test_csv=str(root / "Categorical_test.csv"), names=list(NAMES), sd=sd, xs=xs)


def read_csv(path):
    import csv
    with open(path, newline="") as f:
        rows_ = list(csv.reader(f))
    return rows_[0], [r[0] for r in rows_[1:]], [r[1] for r in rows_[1:]], np.array([[float(v) for v in r[2:]] for r in rows_[1:]])
