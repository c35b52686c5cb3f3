"""Generate tests/golden/trimodal_head_pins.npz -- run once where the reference is checked out, output committed.

The method of oracle/make_head_golden.py for the trimodal head: the reference script (bin/train_cat_trimodal_lazy_1head.py) trains at
import time, so its ``MultiModalEmotionClassifier`` is cut out of the source with ``ast`` -- nothing else of the file runs -- and executed
on seeded weights (oracle.fusion_head.seeded_head_weights over the class's own state-dict shapes) and seeded rows (tests/fusion3_ref.py),
one utterance at a time, as the reference's scoring scripts run it.  What is stored is DATA: the state-dict keys and shapes, the seeds and
the logits at the dims of the reference's trimodal config (1280, 1024, 512; H = 512) and at a small geometry (64, 128, 64; H = 64).

    python tools/make_trimodal_golden.py <reference checkout>

The tests never run this file: they read the stored data only (tests/test_trimodal_host.py).
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.fusion_head import seeded_head_weights       # noqa: E402
import fusion3_ref as R3                                  # noqa: E402

SEED_W, SEED_X = 41, 42
# (tag, dims, hidden width, (speech, text, third-stream) lengths per utterance)
PINS = (("big", (1280, 1024, 512), 512, ((149, 37), (80, 12), (64, 33))),
        ("small", (64, 128, 64), 64, ((1, 17, 40), (5, 1, 16), (33, 2, 64))))


def reference_class(ref):
    tree = ast.parse(open(ref).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MultiModalEmotionClassifier"]
    assert len(body) == 1
    ns = {}
    exec("import torch\nimport torch.nn as nn\nimport torch.nn.functional as F\n", ns)
    exec(compile(ast.Module(body=body, type_ignores=[]), ref, "exec"), ns)
    return ns["MultiModalEmotionClassifier"]


def main(argv):
    if len(argv) != 1:
        raise SystemExit("usage: python tools/make_trimodal_golden.py <reference checkout>")
    from interspeech_ser_amd.head import TrimodalEmotionClassifier
    RefHead = reference_class(os.path.join(argv[0], "bin", "train_cat_trimodal_lazy_1head.py"))
    out = {"seed_weights": np.array(SEED_W), "seed_rows": np.array(SEED_X), "tags": np.array([p[0] for p in PINS])}
    for tag, dims, h, lengths in PINS:
        ref = RefHead(features1_dim=dims[0], features2_dim=dims[1], features3_dim=dims[2], fusion_hidden_dim=h, num_emotions=8, dropout=0.5).eval()
        shapes = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
        weights = seeded_head_weights(shapes, SEED_W)
        ref.load_state_dict(weights, strict=True)
        rows = R3.seeded_rows(dims, lengths, SEED_X)
        ours = TrimodalEmotionClassifier(*dims, fusion_hidden_dim=h).eval()
        assert list(ours.state_dict().keys()) == list(shapes.keys()), "state-dict keys differ from the reference class"
        assert list(R3.head_shapes(*dims, h=h).items()) == list(shapes.items()), "tests/fusion3_ref.py head_shapes differs from the reference class"
        ours.load_state_dict(weights, strict=True)
        t = lambda a: torch.from_numpy(a)[None]
        with torch.no_grad():
            logits = torch.cat([ref(t(a), t(b), t(c)) for a, b, c in zip(*rows)])
            mine = torch.cat([ours(t(a), t(b), t(c)) for a, b, c in zip(*rows)])
        err = float((mine - logits).abs().max())
        print(f"{tag}: restated trimodal head vs reference class: {len(shapes)} state-dict keys identical, logits max abs diff {err:.2e}")
        assert err < 1e-5
        keys = list(shapes.keys())
        out.update({f"{tag}_keys": np.array(keys), f"{tag}_shapes": np.array([",".join(map(str, shapes[k])) for k in keys]),
                    f"{tag}_dims": np.array(dims), f"{tag}_h": np.array(h), f"{tag}_lengths": np.array(lengths),
                    f"{tag}_logits": logits.numpy().astype(np.float32)})
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "trimodal_head_pins.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1:])
