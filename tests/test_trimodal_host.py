"""CPU: ser_xattn_mh_v's export, struct layout and validation (before any launch); head.TrimodalEmotionClassifier against the reference's
pins; the float64 statement tests/fusion3_ref.py against it; head.score's torch engine on a tiny corpus (bimodal, trimodal, ranking
checkpoints); the scoring commands' engine switch without a device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fusion3_ref as R3
import fusion_ref as R
import trimodal_corpus as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ser_hip.h")
HEADER_ROW = ["FileName", "Prediction"] + [f"class_{i}_prob" for i in range(8)]


# ------------------------------------------------------------------------------- ABI
def test_xattn_mh_is_exported_declared_and_bound(built_library):
    from interspeech_ser_amd import _lib
    assert hasattr(ctypes.CDLL(built_library), "ser_xattn_mh_v") and "ser_xattn_mh_v" in _lib.EXPORTED_SYMBOLS
    text = open(HEADER).read()
    assert "int ser_xattn_mh_v(const ser_xattn_mh_args* args, void* stream);" in text and "} ser_xattn_mh_args;" in text
    assert _lib.lib.ser_version() == 18                                # additive: the ABI number stays


def test_xattn_mh_struct_layout_matches_c(built_library, tmp_path):
    from interspeech_ser_amd._lib import STRUCT_MIRRORS, XattnMhArgs
    assert STRUCT_MIRRORS["ser_xattn_mh_args"] is XattnMhArgs
    lines = ['printf("sizeof %zu\\n", sizeof(ser_xattn_mh_args));']
    for f, *_ in XattnMhArgs._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(ser_xattn_mh_args, {f}));')
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{' + "".join(lines) + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(XattnMhArgs)
    for f, *_ in XattnMhArgs._fields_:
        assert int(out[f]) == getattr(XattnMhArgs, f).offset, f


def _mh_args(_lib, **kw):
    x = _lib.XattnMhArgs()
    x.q, x.k, x.v, x.q_offs, x.k_offs, x.out_f32 = 256, 512, 768, 1024, 1280, 1536            # never dereferenced
    x.ldq = x.ldk = x.ldv = x.ldo_f32 = 256
    x.B, x.E, x.heads, x.q_rows, x.k_rows, x.max_q = 1, 256, 2, 4, 4, 4
    for k, v in kw.items():
        setattr(x, k, v)
    return x


def test_xattn_mh_validates_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    f, err = _lib.lib.ser_xattn_mh_v, _lib.lib.ser_last_error
    assert f(None, None) == -1 and b"ser_xattn_mh: null pointer" in err()
    for field in ("q", "k", "v", "q_offs", "k_offs", "out_f32"):       # out_f32 alone: neither output is given
        assert f(ctypes.byref(_mh_args(_lib, **{field: None})), None) == -1 and b"ser_xattn_mh: null pointer" in err(), field
    for kw, msg in (({"heads": 0}, b"ser_xattn_mh: bad heads=0"), ({"heads": -2}, b"ser_xattn_mh: bad heads=-2"),
                    ({"heads": 3}, b"ser_xattn_mh: bad heads=3"),                       # E % heads != 0
                    ({"heads": 8}, b"ser_xattn_mh: bad heads=8"),                       # dh = 32: not a multiple of 64
                    ({"E": 192, "heads": 2}, b"ser_xattn_mh: bad heads=2 for E=192"),   # dh = 96
                    ({"ldk": 128}, b"ser_xattn_mh: bad pitches"), ({"ldq": 258}, b"ser_xattn_mh: bad pitches"),
                    ({"ldo_f32": 64}, b"ser_xattn_mh: bad ldo_f32"),
                    ({"B": 0}, b"ser_xattn_mh: bad B=0"), ({"B": 65536}, b"ser_xattn_mh: bad B"), ({"E": 2048, "heads": 2}, b"ser_xattn_mh: bad B"),
                    ({"E": 96, "heads": 1}, b"ser_xattn_mh: bad B"), ({"max_q": 5}, b"ser_xattn_mh: bad B"), ({"k_rows": 0}, b"ser_xattn_mh: bad B"),
                    ({"q": 260}, b"ser_xattn_mh: q, k, v and out_f32 must be 16-byte aligned"),
                    ({"out_act": 2048, "ldo_act": 256, "mode": _lib.MODE_FP16}, b"ser_xattn_mh: mode")):
        assert f(ctypes.byref(_mh_args(_lib, **kw)), None) == -2, kw
        assert msg in err(), (kw, err())
    # the single-head entry point keeps its own messages
    assert _lib.lib.ser_xattn_v(ctypes.byref(_lib.XattnArgs()), None) == -1 and b"ser_xattn: null pointer" in err()


# ------------------------------------------------------------------------------- the torch class and the float64 statement
def _pins(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "trimodal_head_pins.npz"))
    shapes = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g[f"{tag}_keys"], g[f"{tag}_shapes"])}
    return g, shapes, tuple(int(v) for v in g[f"{tag}_dims"]), int(g[f"{tag}_h"]), [tuple(int(v) for v in ln) for ln in g[f"{tag}_lengths"]]


@pytest.mark.parametrize("tag", ["big", "small"])
def test_trimodal_class_has_the_pinned_keys_and_reproduces_the_pinned_logits(golden_dir, tag):
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.engine import TRIMODAL_KEYS
    from oracle.fusion_head import seeded_head_weights
    g, shapes, dims, h, lengths = _pins(golden_dir, tag)
    assert dims == ((1280, 1024, 512) if tag == "big" else (64, 128, 64))
    m = HD.TrimodalEmotionClassifier(*dims, fusion_hidden_dim=h).eval()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(shapes.items())          # keys, order and shapes of the reference class
    assert list(R3.head_shapes(*dims, h=h).items()) == list(shapes.items()) and set(TRIMODAL_KEYS) == set(shapes)
    m.load_state_dict(seeded_head_weights(shapes, int(g["seed_weights"])), strict=True)
    xs = R3.seeded_rows(dims, lengths, int(g["seed_rows"]))
    with torch.no_grad():
        got = torch.cat([m(*(torch.from_numpy(x)[None] for x in item)) for item in zip(*xs)]).numpy()
    want = g[f"{tag}_logits"]
    assert got.shape == want.shape == (len(lengths[0]), 8)
    assert np.abs(got - want).max() < 1e-5
    if tag == "small":                                                 # the third stream as [B, T, D, 1]: the reference's squeeze(-1)
        with torch.no_grad():
            again = m(torch.from_numpy(xs[0][2])[None], torch.from_numpy(xs[1][2])[None], torch.from_numpy(xs[2][2])[None, ..., None]).numpy()
        assert np.array_equal(again[0], got[2])


@pytest.mark.parametrize("seed", [31, 5])
def test_float64_statement_equals_the_torch_class_in_float64(seed):
    sd, xs1, xs2, xs3 = R3.seeded_case((64, 128, 64), ((1, 2, 37), (9, 1, 4), (3, 20, 1)), seed, h=64)
    mine = R3.batch_logits(sd, xs1, xs2, xs3)
    want = R3.torch_logits(sd, xs1, xs2, xs3, torch.float64)
    assert mine.shape == (3, 8) and np.abs(mine - want).max() < 1e-12
    one_head = R3.batch_logits(sd, xs1, xs2, xs3, heads=(1, 1, 1))     # the head count is part of the statement: it moves the logits
    assert np.abs(one_head - mine).max() > 1e-4
    e = {q: R.rel_err(R3.batch_logits(sd, xs1, xs2, xs3, q), mine) for q in ("f16x", "fp32x", "bf16")}
    assert 0 < e["f16x"] < 1e-5 and e["f16x"] < e["fp32x"] < 1e-3 and e["fp32x"] < e["bf16"] < 1e-1, e


# ------------------------------------------------------------------------------- head.score, torch engine
@pytest.mark.parametrize("modalities", [2, 3])
def test_score_torch_writes_test_csv_and_ignores_a_ranking_checkpoints_extra_keys(tmp_path, built_library, monkeypatch, modalities):
    from interspeech_ser_amd import head as HD
    monkeypatch.setattr(HD, "_device", lambda name: torch.device("cpu"))
    c = TC.make(tmp_path, modalities)
    res = HD.score(c["cfg"], seed=7, engine="torch", modalities=modalities, test_csv=c["test_csv"])
    assert res["n"] == 5 and res["failed"] == 0 and res["csv"] == os.path.join(c["cfg"]["model_path"], "results", "test.csv")
    header, names, letters, logits = TC.read_csv(res["csv"])
    assert header == HEADER_ROW and names == c["names"]                # "FileName", not dev.csv's "Filename"
    want = TC.torch_logits(modalities)                                 # the class on each utterance alone: batch_size=1
    assert np.abs(logits - want).max() <= 5.1e-5                       # the %.4f the rows are printed with
    assert letters == [HD.CLASS_LETTERS[int(np.argmax(r))] for r in want]
    assert all(len(v.split(".")[1]) == 4 for v in open(res["csv"]).read().splitlines()[1].split(",")[2:])
    plain = open(res["csv"], "rb").read()
    r = TC.make(tmp_path, modalities, ranking=True)                    # same weights + neutral_classifier.* / classifier_neutral.*
    assert any(k.startswith(TC.RANKING_PREFIX[modalities]) for k in r["sd"])
    res = HD.score(r["cfg"], seed=7, engine="torch", modalities=modalities, test_csv=r["test_csv"])
    assert open(res["csv"], "rb").read() == plain
    short = {k: v for k, v in c["sd"].items() if k != "text_norm.bias"}
    torch.save(short, os.path.join(c["cfg"]["model_path"], "multimodal_ser.pt"))
    with pytest.raises(ValueError, match="lacks"):
        HD.score(c["cfg"], seed=7, engine="torch", modalities=modalities, test_csv=c["test_csv"])
    with pytest.raises(ValueError, match="engine"):
        HD.score(c["cfg"], engine="triton", modalities=modalities, test_csv=c["test_csv"])
    with pytest.raises(ValueError, match="modalities"):
        HD.score(c["cfg"], modalities=4, test_csv=c["test_csv"])


def test_fusion_heads_check_missing_keys_only():
    """engine.FusionHead / TrimodalHead look for the keys they need and nothing else: a ranking checkpoint loads as the plain head.
    (The constructors need a device; what they check is the two key tables.)"""
    from interspeech_ser_amd.engine import FUSION_KEYS, TRIMODAL_KEYS, FusionHead, TrimodalHead
    assert set(FUSION_KEYS) == set(R.head_shapes(64, 128, h=64)) and set(TRIMODAL_KEYS) == set(R3.head_shapes(64, 128, 64, h=64))
    assert not any(k.startswith(("neutral_classifier", "classifier_neutral")) for k in list(FUSION_KEYS) + list(TRIMODAL_KEYS))
    assert FusionHead.KEYS is FUSION_KEYS and TrimodalHead.KEYS is TRIMODAL_KEYS and TrimodalHead.NAMES == ("speech", "text", "prosody")


@pytest.mark.parametrize("script,modalities", [("test_cat_bimodal_lazy_stacking_1head.py", 2), ("test_cat_bimodal_lazy_stacking_1head_ranking.py", 2),
                                               ("test_cat_trimodal_lazy_stacking_1head.py", 3), ("test_cat_trimodal_lazy_stacking_1head_ranking.py", 3)])
def test_scoring_commands_parse_their_options(tmp_path, built_library, monkeypatch, capsys, script, modalities):
    """each command is main(score_only=True[, modalities=3]); run in-process with the same arguments"""
    from interspeech_ser_amd import head as HD
    text = open(os.path.join(ROOT, "bin", script)).read()
    assert ("main(score_only=True, modalities=3)" if modalities == 3 else "main(score_only=True)") in text
    monkeypatch.setattr(HD, "_device", lambda name: torch.device("cpu"))
    c = TC.make(tmp_path, modalities, ranking="ranking" in script)
    assert HD.main(["--seed", "3", "--config_path", c["cfg_path"], "--engine", "torch", "--test_csv", c["test_csv"]], score_only=True,
                   modalities=modalities) == 0
    assert TC.read_csv(os.path.join(c["cfg"]["model_path"], "results", "test.csv"))[1] == c["names"]
    if not torch.cuda.is_available():
        before = sorted(os.listdir(os.path.join(c["cfg"]["model_path"], "results")))
        capsys.readouterr()
        assert HD.main(["--config_path", c["cfg_path"], "--engine", "hip", "--mode", "fp32x", "--test_csv", c["test_csv"]], score_only=True,
                       modalities=modalities) == 0
        assert "no CPU path" in capsys.readouterr().out and sorted(os.listdir(os.path.join(c["cfg"]["model_path"], "results"))) == before


def test_hip_engine_command_without_a_device_prints_the_no_cpu_path_line_and_exits_0(tmp_path, built_library):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    c = TC.make(tmp_path, 3)
    for script in ("test_cat_trimodal_lazy_stacking_1head.py", "eval_cat_trimodal_lazy_1head.py"):
        args = ["--config_path", c["cfg_path"], "--engine", "hip"] + (["--test_csv", c["test_csv"]] if script.startswith("test") else [])
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bin", script)] + args, capture_output=True, text=True)
        assert p.returncode == 0 and "no CPU path" in p.stdout, (script, p.stdout, p.stderr)
    assert not os.path.exists(os.path.join(c["cfg"]["model_path"], "results"))


# ------------------------------------------------------------------------------- head.evaluate / head.train with modalities=3
def test_trimodal_train_and_evaluate_on_a_tiny_corpus(tmp_path, built_library, monkeypatch):
    import pandas as pd
    from interspeech_ser_amd import head as HD
    monkeypatch.setattr(HD, "_device", lambda name: torch.device("cpu"))
    monkeypatch.setattr(HD, "_model", lambda config, device, modalities=2, hidden=512, _m=HD._model: _m(config, device, modalities, hidden=64))
    c = TC.make(tmp_path, 3, third_axis=False)                         # pad_sequence needs one shape per stream, here as in the reference
    cfg = dict(c["cfg"])
    rng = np.random.default_rng(2)
    lab = pd.DataFrame(np.eye(8, dtype=np.float32)[rng.integers(0, 8, 5)], columns=HD.CLASSES)
    lab.insert(0, "FileName", c["names"])
    lab["Split_Set"] = ["Train", "Train", "Train", "Development", "Development"]
    lab.to_csv(tmp_path / "labels.csv", index=False)
    pd.DataFrame({"FileName": c["names"], "transcription": ["x"] * 5}).to_csv(tmp_path / "text.csv", index=False)
    cfg.update(label_path=str(tmp_path / "labels.csv"), txt_dir=str(tmp_path / "text.csv"), batch_size=2, accum_step=1, epochs=1, lr=1e-3,
               model_path=str(tmp_path / "trained"))
    best = HD.train(cfg, seed=7, modalities=3)
    assert len(best["history"]) == 1 and np.isfinite(best["history"][0]["eval_loss"])
    if not os.path.isfile(best["model_file"]):                         # F1 = 0 on two files saves nothing: evaluate the initial weights
        torch.manual_seed(0)
        torch.save(HD.TrimodalEmotionClassifier(*TC.DIMS, fusion_hidden_dim=64).state_dict(), best["model_file"])
    assert set(torch.load(best["model_file"], weights_only=True)) == set(R3.head_shapes(*TC.DIMS, h=64))
    res = HD.evaluate(cfg, seed=7, modalities=3)
    assert res["n"] == 2 and np.isfinite(res["eval_loss"]) and 0.0 <= res["eval_f1"] <= 1.0
    header, names, _, logits = TC.read_csv(res["csv"])
    assert header[0] == "Filename" and names == c["names"][3:] and logits.shape == (2, 8)
