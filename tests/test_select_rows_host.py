"""CPU: ser_select_rows_v's argument checks and struct layout, and what predictor.score_from_wav decides before it touches a GPU."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ser_hip.h")


def _good_args():
    """a complete argument struct; the pointers are never dereferenced: validation comes before any launch"""
    from interspeech_ser_amd import _lib
    a = _lib.SelectRowsArgs()
    for k in range(4):
        a.src[k] = 4096 + 1024 * k
    a.ld_src, a.src_offs, a.dst_offs = 64, 256, 512
    a.out_act, a.ldo_act, a.out_plane_stride, a.out_f32, a.ldo_f32 = 8192, 64, 64 * 40, 16384, 64
    a.n_src, a.B, a.D, a.max_rows, a.mode = 1, 4, 64, 33, _lib.MODE_FP16X
    return a


def _null_src0(a): a.src[0] = None
def _null_src3(a): a.n_src, a.src[3] = 4, None
def _null_src_offs(a): a.src_offs = None
def _null_dst_offs(a): a.dst_offs = None
def _n_src_2(a): a.n_src = 2
def _n_src_0(a): a.n_src = 0
def _no_output(a): a.out_act, a.out_f32 = None, None
def _b_zero(a): a.B = 0
def _b_large(a): a.B = 65536
def _d_zero(a): a.D = 0
def _d_odd(a): a.D = 66
def _ld_src_odd(a): a.ld_src = 66
def _ldo_act_odd(a): a.ldo_act = 66
def _ldo_f32_odd(a): a.ldo_f32 = 66
def _max_rows_zero(a): a.max_rows = 0
def _mode_fp16(a): a.mode = 3
def _mode_zero(a): a.mode = 0
def _mode_99(a): a.mode = 99


BAD = [_null_src0, _null_src3, _null_src_offs, _null_dst_offs, _n_src_2, _n_src_0, _no_output, _b_zero, _b_large, _d_zero, _d_odd, _ld_src_odd,
       _ldo_act_odd, _ldo_f32_odd, _max_rows_zero, _mode_fp16, _mode_zero, _mode_99]


@pytest.mark.parametrize("spoil", BAD, ids=[f.__name__.lstrip("_") for f in BAD])
def test_select_rows_refuses_bad_arguments_before_any_launch(built_library, spoil):
    from interspeech_ser_amd import _lib
    a = _good_args()
    spoil(a)
    assert _lib.lib.ser_select_rows_v(ctypes.byref(a), None) < 0
    assert b"ser_select_rows" in _lib.lib.ser_last_error()


def test_select_rows_refuses_null_arguments(built_library):
    from interspeech_ser_amd import _lib
    assert _lib.lib.ser_select_rows_v(None, None) < 0


def test_select_rows_struct_layout_matches_c(built_library, tmp_path):
    from interspeech_ser_amd import _lib
    cls, cname = _lib.SelectRowsArgs, "ser_select_rows_args"
    assert _lib.STRUCT_MIRRORS[cname] is cls
    lines = [f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, *_ in cls._fields_]
    lines.append('printf("tile %d\\n", SER_SELECT_ROWS_TILE);')
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{' + "".join(lines) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(cls)
    for f, *_ in cls._fields_:
        assert int(out[f]) == getattr(cls, f).offset, f
    assert int(out["tile"]) == _lib.SELECT_ROWS_TILE


def _config(tmp_path, **kw):
    cfg = {"wav_dir": str(tmp_path / "wav"), "txt_dir": str(tmp_path / "text.csv"), "model_path": str(tmp_path / "exp"),
           "feat1_dim": 1280, "feat2_dim": 1024}
    cfg.update(kw)
    return cfg


def test_score_from_wav_without_a_gpu_returns_the_empty_record(built_library, tmp_path, capsys, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.predictor import score_from_wav
    res = score_from_wav(_config(tmp_path), ["openai/whisper-large-v3", "roberta-large"], synthetic_weights=True,
                         test_csv=str(tmp_path / "none.csv"))
    assert res == {"csv": None, "n": 0, "failed": 0}
    assert HD.NO_CPU_PATH in capsys.readouterr().out
    assert not os.path.exists(tmp_path / "exp")


def test_score_from_wav_checks_the_feature_widths_before_loading_weights(built_library, tmp_path, monkeypatch):
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.predictor import score_from_wav

    def no_weights(*a, **k):
        raise AssertionError("weights were looked for before the widths were checked")
    monkeypatch.setattr(driver, "find_weights", no_weights)
    with pytest.raises(ValueError, match="feat1_dim = 1024 .* hidden size 1280"):
        score_from_wav(_config(tmp_path, feat1_dim=1024), ["openai/whisper-large-v3", "roberta-large"], synthetic_weights=True)
    with pytest.raises(ValueError, match="feat2_dim"):
        score_from_wav(_config(tmp_path, feat2_dim=768), ["openai/whisper-large-v3", "roberta-large"], synthetic_weights=True)
    with pytest.raises(ValueError, match="two or three"):
        score_from_wav(_config(tmp_path), ["openai/whisper-large-v3"], synthetic_weights=True)
    with pytest.raises(ValueError, match="third stream"):
        score_from_wav(_config(tmp_path), ["openai/whisper-large-v3", "files"], synthetic_weights=True)
