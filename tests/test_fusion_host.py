"""CPU: the fusion head's float64 statement (tests/fusion_ref.py) against the oracle and the reference's pins; the four entry points'
exports, struct layouts and validation (before any launch); head.evaluate's engine switch without a device."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import fusion_ref as R
from oracle import fusion_head as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ser_hip.h")
NEW_SYMBOLS = ("ser_gru_v", "ser_gru_work_bytes", "ser_xattn_v", "ser_attn_pool_v", "ser_fusion_cls_v")
NEW_STRUCTS = ("ser_gru_args", "ser_xattn_args", "ser_attn_pool_args", "ser_fusion_cls_args")


# ------------------------------------------------------------------------------- the reference statement
@pytest.mark.parametrize("seed", [31, 5])
def test_float64_statement_equals_the_oracle_on_each_utterance_alone(seed):
    sd, xs1, xs2 = R.seeded_case(64, 64, (1, 2, 37), seed, t2=9, h=64)
    mine = R.batch_logits(sd, xs1, xs2)
    want = R.oracle_logits(sd, xs1, xs2, torch.float64)
    assert mine.shape == (3, 8)
    assert np.abs(mine - want).max() < 1e-12


def test_float64_statement_reproduces_the_pinned_logits(golden_dir):
    """fusion_head_pins_d40x24.npz holds the reference class's logits on a batch padded to its longest utterance (499 frames; the text side
    is 80 rows for all).  Utterance 1 is that longest one: no pad frame enters its row, so the per-utterance statement must reproduce it."""
    g = np.load(os.path.join(golden_dir, "fusion_head_pins_d40x24.npz"))
    shapes = {str(k): tuple(int(x) for x in str(s).split(",")) for k, s in zip(g["keys"], g["shapes"])}
    sd = H.seeded_head_weights(shapes, int(g["seed_weights"]))
    batch = H.synthetic_batch(int(g["feat1_dim"]), int(g["feat2_dim"]), int(g["seed_batch"]))
    assert batch["feat1"].shape[1] == 499
    got = R.head_logits(sd, batch["feat1"][1].numpy(), batch["feat2"][1].numpy())
    assert np.abs(got - g["logits"][1].astype(np.float64)).max() < 1e-4
    assert set(R.head_shapes(40, 24)) == set(shapes) and all(R.head_shapes(40, 24)[k] == shapes[k] for k in shapes)


def test_operand_rounding_hook_costs_what_its_width_says():
    sd, xs1, xs2 = R.seeded_case(64, 64, (5, 19), 31, t2=7, h=64)
    ref = R.batch_logits(sd, xs1, xs2)
    e = {q: R.rel_err(R.batch_logits(sd, xs1, xs2, q), ref) for q in ("f16x", "fp32x", "bf16")}
    assert 0 < e["f16x"] < 1e-5 and e["f16x"] < e["fp32x"] < 1e-3 and e["fp32x"] < e["bf16"] < 1e-1, e
    x = np.array([1.0 + 2.0 ** -12, 3.0e-5, -1234.5678], dtype=np.float32)
    assert np.array_equal(R.round_planes(x, None), x.astype(np.float64))
    assert np.abs(R.round_planes(x, "f16x") - x).max() <= 2.0 ** -21 * 1234.6


# ------------------------------------------------------------------------------- ABI
def test_new_entry_points_are_exported_and_bound(built_library):
    from interspeech_ser_amd import _lib
    lib = ctypes.CDLL(built_library)
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.EXPORTED_SYMBOLS, n
    assert _lib.lib.ser_version() == 18                                # additive exports: the ABI number stays
    assert int(open(HEADER).read().split("#define SER_GRU_ERR_TIMEOUT ")[1].split()[0]) == _lib.GRU_ERR_TIMEOUT


def test_new_struct_layouts_match_c(built_library, tmp_path):
    from interspeech_ser_amd._lib import STRUCT_MIRRORS
    lines = []
    for cname in NEW_STRUCTS:
        cls = STRUCT_MIRRORS[cname]
        lines.append(f'printf("{cname}.sizeof %zu\\n", sizeof({cname}));')
        for f, *_ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{' + "".join(lines) + 'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname in NEW_STRUCTS:
        cls = STRUCT_MIRRORS[cname]
        assert int(out[f"{cname}.sizeof"]) == ctypes.sizeof(cls), cname
        for f, *_ in cls._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def _gru_args(_lib, **kw):
    g = _lib.GruArgs()
    g.gx, g.whh, g.bhh, g.frame_offs, g.out, g.work, g.err = 256, 512, 768, 1024, 1280, 1536, 1792          # never dereferenced
    g.B, g.H, g.rows, g.max_frames, g.cluster = 2, 64, 10, 5, 0
    g.ldgx, g.ldo, g.whh_plane_stride, g.work_bytes = 6 * 64, 2 * 64, 6 * 64 * 64, 1 << 30
    for k, v in kw.items():
        setattr(g, k, v)
    if "H" in kw and "ldgx" not in kw:
        g.ldgx, g.ldo, g.whh_plane_stride = 6 * g.H, 2 * g.H, 6 * g.H * g.H
    return g


def test_gru_validates_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    f, err = _lib.lib.ser_gru_v, _lib.lib.ser_last_error
    assert f(None, None) == -1 and b"ser_gru: null pointer" in err()
    for field in ("gx", "whh", "bhh", "frame_offs", "out"):
        assert f(ctypes.byref(_gru_args(_lib, **{field: None})), None) == -1 and b"ser_gru: null pointer" in err(), field
    for B in (0, -3):
        assert f(ctypes.byref(_gru_args(_lib, B=B)), None) == -2 and b"ser_gru: bad B" in err()
    for Hh in (0, 32, 96, 100, 576):
        assert f(ctypes.byref(_gru_args(_lib, H=Hh)), None) == -2 and b"multiple of 64" in err(), Hh
    for Hh, cl in ((64, 3), (64, 8), (512, 5), (512, 64), (512, -1), (192, 8)):        # H / 16 = 4, 32, 12 column tiles of 16 units
        assert f(ctypes.byref(_gru_args(_lib, H=Hh, cluster=cl)), None) == -2 and b"cluster" in err(), (Hh, cl)
    assert f(ctypes.byref(_gru_args(_lib, max_frames=11)), None) == -2
    assert f(ctypes.byref(_gru_args(_lib, ldo=64)), None) == -2 and b"pitches" in err()
    assert f(ctypes.byref(_gru_args(_lib, cluster=2, work=None)), None) == -1 and b"workspace" in err()
    assert f(ctypes.byref(_gru_args(_lib, cluster=2, work_bytes=1024)), None) == -2 and b"workspace" in err()
    assert f(ctypes.byref(_gru_args(_lib, out_act=2048, ldo_act=128, mode=_lib.MODE_FP16)), None) == -2 and b"mode" in err()


def test_gru_plan_picks_the_smallest_cluster_that_keeps_the_weights_resident(built_library):
    from interspeech_ser_amd import _lib
    r = ctypes.c_int32(-1)
    assert _lib.lib.ser_gru_work_bytes(64, 0, ctypes.byref(r)) == 0 and r.value == 1
    nbytes = _lib.lib.ser_gru_work_bytes(512, 0, ctypes.byref(r))
    assert r.value == 32 and nbytes == (256 // 64) * 2 * 2 * 512 * 16 * 8       # [clusters of a launch][parity][unit][utterance] granules
    assert _lib.lib.ser_gru_work_bytes(512, 1, ctypes.byref(r)) == 0 and r.value == 1
    assert _lib.lib.ser_gru_work_bytes(512, 8, ctypes.byref(r)) > 0 and r.value == 8
    assert _lib.lib.ser_gru_work_bytes(512, 7, None) == -1 and _lib.lib.ser_gru_work_bytes(100, 0, None) == -1
    for Hh in range(64, 513, 64):                                              # the chosen R divides the 16-unit tiles, and a launch fits 256 blocks
        assert _lib.lib.ser_gru_work_bytes(Hh, 0, ctypes.byref(r)) >= 0 and (Hh // 16) % r.value == 0 and 2 * r.value <= 256


def test_xattn_pool_and_classifier_validate_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    err = _lib.lib.ser_last_error
    x = _lib.XattnArgs()
    assert _lib.lib.ser_xattn_v(None, None) == -1 and _lib.lib.ser_xattn_v(ctypes.byref(x), None) == -1 and b"ser_xattn: null pointer" in err()
    x.q, x.k, x.v, x.q_offs, x.k_offs, x.out_f32 = 256, 512, 768, 1024, 1280, 1536
    x.ldq = x.ldk = x.ldv = x.ldo_f32 = 128
    x.B, x.E, x.q_rows, x.k_rows, x.max_q = 1, 128, 4, 4, 4
    for field, bad in (("B", 0), ("E", 96), ("E", 2048), ("max_q", 5), ("ldk", 64), ("k_rows", 0)):
        keep = getattr(x, field)
        setattr(x, field, bad)
        assert _lib.lib.ser_xattn_v(ctypes.byref(x), None) == -2 and b"ser_xattn: bad" in err(), field
        setattr(x, field, keep)
    p = _lib.AttnPoolArgs()
    assert _lib.lib.ser_attn_pool_v(None, None) == -1 and _lib.lib.ser_attn_pool_v(ctypes.byref(p), None) == -1 and b"ser_attn_pool: null pointer" in err()
    p.a, p.b, p.w, p.frame_offs, p.scores, p.out = 256, 512, 768, 1024, 1280, 1536
    p.lda = p.ldb = 64
    p.ldo, p.B, p.E, p.rows, p.max_frames = 128, 1, 64, 4, 4
    for field, bad in (("B", 0), ("E", 66), ("max_frames", 9), ("col0", 128), ("lda", 32)):
        keep = getattr(p, field)
        setattr(p, field, bad)
        assert _lib.lib.ser_attn_pool_v(ctypes.byref(p), None) == -2 and b"ser_attn_pool: bad" in err(), field
        setattr(p, field, keep)
    c = _lib.FusionClsArgs()
    assert _lib.lib.ser_fusion_cls_v(None, None) == -1 and _lib.lib.ser_fusion_cls_v(ctypes.byref(c), None) == -1 and b"ser_fusion_cls: null pointer" in err()
    c.p, c.gamma, c.beta, c.W1, c.b1, c.W2, c.b2, c.xn, c.hidden, c.out = (256 * i for i in range(1, 11))
    c.ldp, c.B, c.K, c.H1, c.n_out = 256, 2, 256, 64, 8
    for field, bad in (("n_out", 0), ("n_out", 9), ("B", 0), ("K", 8192), ("K", 254), ("ldp", 128)):
        keep = getattr(c, field)
        setattr(c, field, bad)
        assert _lib.lib.ser_fusion_cls_v(ctypes.byref(c), None) == -2 and b"ser_fusion_cls: " in err(), field
        setattr(c, field, keep)


# ------------------------------------------------------------------------------- head.evaluate's engine switch
def _tiny_corpus(tmp_path, n=6, d1=40, d2=24):
    import pandas as pd
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.frontend import feature_path, save_feature
    rng = np.random.default_rng(5)
    lazy1, lazy2 = tmp_path / "hubert", tmp_path / "roberta"
    lazy1.mkdir()
    lazy2.mkdir()
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(n)]
    cls = rng.integers(0, 8, n)
    for name in names:
        save_feature(torch.from_numpy(rng.standard_normal((int(rng.integers(3, 9)), d1)).astype(np.float32)), feature_path(str(lazy1), name))
        save_feature(torch.from_numpy(rng.standard_normal((5, d2)).astype(np.float32)), feature_path(str(lazy2), name))
    lab = pd.DataFrame(np.eye(8, dtype=np.float32)[cls], columns=HD.CLASSES)
    lab.insert(0, "FileName", names)
    lab["Split_Set"] = "Development"
    lab.to_csv(tmp_path / "labels.csv", index=False)
    pd.DataFrame({"FileName": names, "transcription": ["x"] * n}).to_csv(tmp_path / "text.csv", index=False)
    cfg = {"wav_dir": "/corpus/Audios", "txt_dir": str(tmp_path / "text.csv"), "lazy_dir1": str(lazy1), "lazy_dir2": str(lazy2),
           "label_path": str(tmp_path / "labels.csv"), "feat1_dim": d1, "feat2_dim": d2, "model_path": str(tmp_path / "exp"), "batch_size": 4}
    os.makedirs(cfg["model_path"])
    torch.manual_seed(3)
    torch.save(HD.MultiModalEmotionClassifier(d1, d2).state_dict(), os.path.join(cfg["model_path"], "multimodal_ser.pt"))
    with open(tmp_path / "cfg.json", "w") as f:
        json.dump(cfg, f)
    return cfg


def test_hip_engine_without_a_device_says_so_and_writes_nothing(tmp_path, capsys, built_library):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from interspeech_ser_amd import head as HD
    cfg = _tiny_corpus(tmp_path)
    before = sorted(os.listdir(cfg["model_path"]))
    res = HD.evaluate(cfg, seed=7, engine="hip")
    assert "no CPU path" in capsys.readouterr().out and res["n"] == 0 and res["csv"] is None
    assert sorted(os.listdir(cfg["model_path"])) == before
    assert HD.main(["--config_path", str(tmp_path / "cfg.json"), "--engine", "hip", "--mode", "fp32x"], evaluate_only=True) == 0
    assert "no CPU path" in capsys.readouterr().out and sorted(os.listdir(cfg["model_path"])) == before
    with pytest.raises(ValueError, match="engine"):
        HD.evaluate(cfg, seed=7, engine="triton")


def test_engine_torch_is_the_run_without_the_flag(tmp_path, built_library, monkeypatch):
    from interspeech_ser_amd import head as HD
    monkeypatch.setattr(HD, "_device", lambda name: torch.device("cpu"))      # the comparison is about the flag, not about a device
    cfg = _tiny_corpus(tmp_path)
    csv_file = os.path.join(cfg["model_path"], "results", "dev.csv")
    assert HD.main(["--config_path", str(tmp_path / "cfg.json")], evaluate_only=True) == 0
    plain = open(csv_file, "rb").read()
    os.remove(csv_file)
    assert HD.main(["--config_path", str(tmp_path / "cfg.json"), "--engine", "torch"], evaluate_only=True) == 0
    assert open(csv_file, "rb").read() == plain and plain.count(b"\n") == 7
    with pytest.raises(SystemExit):                                    # the train entry point keeps its flags
        HD.main(["--config_path", str(tmp_path / "cfg.json"), "--engine", "torch"])
