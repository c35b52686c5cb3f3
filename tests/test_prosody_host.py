"""CPU: the prosody stream's host side.  The float64 statement tests/prosody_ref.py against the reference's own fp32 run
(tests/golden/tiny_prosody_d128h2.npz, tools/make_prosody_golden.py); the mel basis against transformers'; the frame count; the position-0
quirk; prosody.prepare's folds against the statement; key-name loading; the three kernels' export, layout and validation; the command
lines and the feat3_dim check of the scoring command."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import prosody_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ser_hip.h")
HEADS = 2
FACTOR = 4.0        # statement vs fixture <= FACTOR x (fp32 torch twin vs statement): two fp32 evaluations of one formula differ from
#                     each other by at most twice their common distance from the exact value; 2x more for the op orders that differ


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "tiny_prosody_d128h2.npz"))
    sd = {str(k): torch.from_numpy(g["w." + str(k)].astype(np.float32)) for k in g["keys"]}
    waves = [g[f"wave_{j}"].astype(np.float32) / 32768.0 for j in range(len(g["lengths"]))]
    offs = np.concatenate([[0], np.cumsum([R.frames(len(w)) for w in waves])])
    return dict(g=g, sd=sd, waves=waves, offs=offs, short=g["short_wave"].astype(np.float32) / 32768.0)


@pytest.fixture(scope="module")
def stated(gold):
    return [R.forward(gold["sd"], w, HEADS) for w in gold["waves"]]


def test_fixture_covers_the_edge_lengths(gold):
    g = gold["g"]
    assert [int(n) for n in g["lengths"]] == [400, 799, 12800, 16000, 25999] and len(gold["short"]) == 399
    assert [R.frames(int(n)) for n in g["lengths"]] == [3, 4, 65, 81, 130]
    assert len(np.unique(g["codes"])) >= 8 and float((g["gaps"] <= 1e-3).mean()) <= 0.05
    assert g["rows"].shape == (283, 128) and g["z"].shape == (283, 128) and g["mel"].shape == (283, 20)


def test_statement_matches_the_reference_run(gold, stated):
    g, offs = gold["g"], gold["offs"]
    for j, (w, st) in enumerate(zip(gold["waves"], stated)):
        sl = slice(offs[j], offs[j + 1])
        twin = R.torch_twin(gold["sd"], w, HEADS)
        e_mel, e_z = R.rel_err(twin["mel"], st["mel"]), R.rel_err(twin["z"], st["z"])
        d_mel, d_z = R.rel_err(st["mel"], g["mel"][sl]), R.rel_err(st["z"], g["z"][sl])
        print(f"wave {j}: mel {d_mel:.2e} (twin {e_mel:.2e})  z {d_z:.2e} (twin {e_z:.2e})")
        assert d_mel <= FACTOR * e_mel and d_z <= FACTOR * e_z
        sure = g["gaps"][sl] > 1e-5
        assert np.array_equal(st["codes"][sure], g["codes"][sl][sure])
        assert np.allclose(st["gaps"], g["gaps"][sl], atol=1e-5)
        assert R.rel_err(st["rows"][sure], g["rows"][sl][sure]) < 1e-6       # one fp32 rounding of an 8-term sum per element


def test_short_wave_cannot_be_padded(gold):
    with pytest.raises(ValueError):
        R.log_mel(gold["short"])
    with pytest.raises(RuntimeError):
        R.torch_log_mel(gold["short"])
    R.log_mel(np.zeros(400))


def test_mel_basis_against_transformers():
    from transformers.audio_utils import mel_filter_bank
    from interspeech_ser_amd.frontend import prosody_mel_filters
    ref = mel_filter_bank(513, 80, 0, 8000, 16000, norm="slaney", mel_scale="slaney").T.astype(np.float64)     # [80, 513]
    mine = prosody_mel_filters(20)
    n_bins = mine.shape[1]
    assert mine.dtype == np.float32 and mine.shape[0] == 20 and 40 <= n_bins <= 64
    assert np.abs(mine - ref[:20, :n_bins]).max() < 1e-8                    # fp32 rounding of values below 0.1
    assert not ref[:20, n_bins:].any() and ref[:20, n_bins - 1].any()       # cut exactly after the last non-zero bin
    assert np.abs(R.mel_basis() - ref[:20]).max() < 1e-8


def test_dft_table_is_the_windowed_transform(gold):
    """the kernel's table applied to frame t's 800 samples is the statement's rfft of the centrally padded, windowed 1024 samples"""
    from interspeech_ser_amd.frontend import prosody_dft_table, prosody_mel_filters
    n_bins = prosody_mel_filters().shape[1]
    tab = prosody_dft_table(n_bins)
    assert tab.shape == (800, n_bins, 2) and tab.dtype == np.float64
    y = R.padded(gold["waves"][2])
    for t in (0, 1, 30, 64):
        fr = y[t * 200 + 112: t * 200 + 912]                                 # = samples 200 t - 300 .. 200 t + 499 of the unreflected wave
        re, im = fr @ tab[:, :, 0], fr @ tab[:, :, 1]
        win = np.zeros(1024)
        win[112:912] = torch.hann_window(800).double().numpy()
        spec = np.fft.rfft(y[t * 200: t * 200 + 1024] * win)[:n_bins]
        assert np.abs(re - spec.real).max() < 1e-9 and np.abs(im - spec.imag).max() < 1e-9


def test_frame_count_including_multiples_of_200():
    from interspeech_ser_amd.frontend import PROSODY_MIN_SAMPLES, prosody_frames
    assert PROSODY_MIN_SAMPLES == 400
    for n in (400, 599, 600, 601, 799, 800, 12800, 16000, 25999, 160000):
        assert prosody_frames(n) == n // 200 + 1 == R.frames(n)
    for n in (400, 600, 601, 800, 12800):                                     # ... which is what the padded STFT yields
        assert R.log_mel(np.zeros(n)).shape == (n // 200 + 1, 20) and tuple(R.torch_log_mel(np.zeros(n)).shape) == (n // 200 + 1, 20)
    assert prosody_frames(12800) == 65 and prosody_frames(12799) == 64


def test_every_frame_gets_position_zero(gold, stated):
    """The reference adds pe[0] to every frame.  The fixture agrees with that and not with real positions; so does the folded bias."""
    from interspeech_ser_amd import prosody as P
    g, offs, sd64 = gold["g"], gold["offs"], R._f64(gold["sd"])
    j = 2
    sl = slice(offs[j], offs[j + 1])
    wrong = R.encoder(sd64, stated[j]["mel"], HEADS, real_positions=True)
    assert R.rel_err(stated[j]["z"], g["z"][sl]) < 1e-4 < 1e-2 < R.rel_err(wrong, g["z"][sl])
    w = P.prepare(gold["sd"], HEADS)
    pe0 = np.zeros(128)
    pe0[1::2] = 1.0
    assert np.array_equal(P.position0(128).numpy(), pe0)
    assert np.allclose(w["lin_b"].double().numpy(), sd64["melspec_linear.bias"] + pe0, atol=1e-7)


def test_weight_norm_fold_and_code_table(gold, stated):
    from interspeech_ser_amd import prosody as P
    sd64 = R._f64(gold["sd"])
    w = P.prepare(gold["sd"], HEADS)
    assert w["spec"] == P.TINY
    assert np.allclose(w["w_in"].double().numpy(), R.weight_norm(sd64, R.VQ + ".in_proj"), atol=1e-7)
    cb = sd64[R.VQ + "._codebook.weight"]
    table = cb @ R.weight_norm(sd64, R.VQ + ".out_proj").T + sd64[R.VQ + ".out_proj.bias"]       # of the RAW codes
    assert tuple(w["table"].shape) == (64, 128) and np.allclose(w["table"].double().numpy(), table, atol=1e-6)
    assert np.allclose(w["codes"].double().numpy(), cb / np.linalg.norm(cb, axis=1, keepdims=True), atol=1e-7)
    assert np.allclose(np.linalg.norm(w["codes"].double().numpy(), axis=1), 1.0, atol=1e-6)
    st = stated[3]
    assert np.allclose(w["table"].double().numpy()[st["codes"]], st["rows"], atol=1e-6)          # the output takes table rows only
    # FC1's weight as the implicit GEMM reads it: W[n][j * D + c] = w[n][c][j]
    w1 = gold["sd"][R.ENC + ".layers.1.ffn.ffn_1.weight"]
    fc1 = w["layers"][1]["fc1"][0]
    assert tuple(fc1.shape) == (128, 5 * 128) and fc1[7, 3 * 128 + 11] == w1[7, 11, 3]
    # the parametrization-style key names of newer PyTorch fold the same way
    sd2 = {k.replace("weight_g", "parametrizations.weight.original0").replace("weight_v", "parametrizations.weight.original1"): v
           for k, v in gold["sd"].items()}
    assert torch.equal(P.prepare(sd2, HEADS)["table"], w["table"])


def test_loading_by_key_names(gold, tmp_path):
    from interspeech_ser_amd import prosody as P
    assert P.spec_from_state_dict(gold["sd"], HEADS) == P.TINY
    full = P.synthetic_state_dict()
    assert P.spec_from_state_dict(full) == P.ProsodySpec() and P.ProsodySpec().hidden == 256 and P.ProsodySpec().n_codes == 1024
    extra = dict(full)
    extra["quantizer.1.layers.0._codebook.weight"] = torch.zeros(1024, 8)     # the checkpoint's other modules are ignored
    extra["timbre_encoder.layers.0.ln_1.weight"] = torch.zeros(256)
    assert P.spec_from_state_dict(extra) == P.ProsodySpec()
    with pytest.raises(KeyError, match="melspec_linear.weight"):
        P.spec_from_state_dict({})
    with pytest.raises(ValueError, match="heads"):
        P.prepare(full, heads=8)
    with pytest.raises(ValueError, match="heads"):
        P.spec_from_state_dict(full, heads=3)
    d = tmp_path / "ns3"
    d.mkdir()
    torch.save(gold["sd"], d / P.CHECKPOINT_FILE)
    assert P.checkpoint_path(str(d)) == str(d / P.CHECKPOINT_FILE) == P.checkpoint_path(str(d / P.CHECKPOINT_FILE))
    assert P.checkpoint_path("") == P.DEFAULT_CHECKPOINT == "./pretrained_models/ns3/ns3_facodec_decoder_v2.bin"
    assert P.resolve_spec(str(d), heads=HEADS) == P.TINY and P.resolve_spec("", synthetic=True) == P.ProsodySpec()
    assert set(P.load_state_dict(str(d))) == set(gold["sd"])
    with pytest.raises(OSError):
        P.load_state_dict(str(tmp_path / "nothing"))


# ------------------------------------------------------------------------------------------------------------------------- ABI
NEW = {"ser_prosody_mel": "PROSODY_MEL", "ser_fvq": "FVQ", "ser_act_rows": "ACT_ROWS"}


def test_kernels_are_exported_declared_and_bound(built_library):
    from interspeech_ser_amd import _lib
    text = open(HEADER).read()
    so = ctypes.CDLL(built_library)
    for val, (name, op) in enumerate(NEW.items(), start=13):
        assert hasattr(so, name + "_v") and name + "_v" in _lib.EXPORTED_SYMBOLS
        assert f"int {name}_v(const {name}_args* args, void* stream);" in text
        assert f"#define SER_OP_{op} {val}" in text and getattr(_lib, "OP_" + op) == val
    assert _lib.lib.ser_version() == 18                                       # additive: the ABI number stays
    assert "prosody.hip" in open(os.path.join(ROOT, "interspeech_ser_amd", "csrc", "Makefile")).read()


def test_struct_layouts_match_c(built_library, tmp_path):
    from interspeech_ser_amd._lib import STRUCT_MIRRORS
    lines = []
    for name in NEW:
        cname, cls = name + "_args", STRUCT_MIRRORS[name + "_args"]
        lines.append(f'printf("{cname}.sizeof %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, *_ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{' + "".join(lines) + 'return 0;}\n')
    subprocess.check_call(["gcc", str(src), "-o", str(tmp_path / "layout")])
    out = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for name in NEW:
        cname, cls = name + "_args", STRUCT_MIRRORS[name + "_args"]
        assert int(out[cname + ".sizeof"]) == ctypes.sizeof(cls)
        for f, *_ in cls._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_launchers_validate_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    L, err = _lib.lib, _lib.lib.ser_last_error
    assert L.ser_prosody_mel_v(None, None) == -1 and b"ser_prosody_mel: null pointer" in err()
    m = _lib.ProsodyMelArgs()
    m.wav, m.sample_offs, m.frame_offs, m.dft, m.mel, m.mel_out = 256, 512, 768, 1024, 1280, 1536      # never dereferenced
    m.B, m.max_frames, m.n_bins, m.n_mels = 1, 3, 65, 20
    assert L.ser_prosody_mel_v(ctypes.byref(m), None) == -2 and b"n_bins=65" in err()
    m.n_bins, m.out = 52, 2048
    assert L.ser_prosody_mel_v(ctypes.byref(m), None) == -1 and b"lin_w" in err()
    assert L.ser_fvq_v(None, None) == -1 and b"ser_fvq: null pointer" in err()
    q = _lib.FvqArgs()
    q.z, q.w_in, q.b_in, q.codes, q.table, q.idx, q.out_f32 = 256, 512, 768, 1024, 1280, 1536, 1792
    q.ldz = q.ld_table = q.ldo_f32 = 128
    q.rows, q.D, q.n_codes, q.code_dim, q.mode = 4, 128, 64, 4, _lib.MODE_BF16
    assert L.ser_fvq_v(ctypes.byref(q), None) == -2 and b"code_dim=4" in err()
    q.code_dim, q.D = 8, 130
    assert L.ser_fvq_v(ctypes.byref(q), None) == -2 and b"D=130" in err()
    q.D, q.ldz = 128, 130
    assert L.ser_fvq_v(ctypes.byref(q), None) == -3
    assert L.ser_act_rows_v(None, None) == -1 and b"ser_act_rows: null pointer" in err()
    r = _lib.ActRowsArgs()
    r.x, r.out_act, r.ldx, r.ldo_act, r.rows, r.D, r.mode, r.relu = 256, 512, 128, 128, 4, 128, _lib.MODE_FP16M, 1
    assert L.ser_act_rows_v(ctypes.byref(r), None) == -4 and b"bad mode" in err()
    r.mode, r.relu = _lib.MODE_FP16X, 2
    assert L.ser_act_rows_v(ctypes.byref(r), None) == -2 and b"relu=2" in err()
    cmds = (_lib.Cmd * 1)()
    cmds[0].op = _lib.OP_FVQ                                                  # the command list reaches the new launchers
    assert L.ser_run(cmds, 1, None, None) == -1 and b"ser_fvq" in err()


# ------------------------------------------------------------------------------------------------------------- command lines
def test_driver_command_line():
    from interspeech_ser_amd import prosody as P
    a = P.build_parser().parse_args(["--wav_dir", "W", "--save_path", "S", "--num_workers", "3"])
    assert (a.wav_dir, a.save_path, a.num_workers, a.seed, a.checkpoint, a.mode) == ("W", "S", 3, 7, "", "f16x")
    a = P.build_parser().parse_args(["--checkpoint", "ckpt", "--mode", "fp32x"])
    assert (a.checkpoint, a.mode, a.wav_dir, a.save_path, a.num_workers) == ("ckpt", "fp32x", "./", "./", 4)
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(["--mode", "f16m"])
    script = open(os.path.join(ROOT, "preprocessing", "preprocess_ns3_prosody.py")).read()
    assert "interspeech_ser_amd.prosody import run" in script


def test_scoring_command_line_takes_the_prosody_stream(tmp_path, monkeypatch):
    import json
    from interspeech_ser_amd import predictor as PR
    seen = {}
    monkeypatch.setattr(PR, "score_from_wav", lambda config, encoders, layers, averages, checkpoints, **kw: seen.update(
        config=config, encoders=encoders, checkpoints=checkpoints, kw=kw))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"feat3_dim": 256}))
    assert PR.main(["--config_path", str(cfg), "--encoder1", "openai/whisper-large-v3", "--encoder2", "roberta-large",
                    "--encoder3", "ns3-prosody", "--checkpoint3", "pretrained_models/ns3"]) == 0
    assert seen["encoders"] == ["openai/whisper-large-v3", "roberta-large", "ns3-prosody"] and PR.NS3_PROSODY == "ns3-prosody"
    assert seen["checkpoints"] == ["", "", "pretrained_models/ns3"] and seen["config"] == {"feat3_dim": 256}
    assert PR.main(["--config_path", str(cfg), "--encoder1", "a", "--encoder2", "b", "--encoder3", "files"]) == 0
    assert seen["encoders"] == ["a", "b", PR.FILES]


def test_stream_kinds_check_the_third_width(gold, tmp_path):
    from interspeech_ser_amd import predictor as PR
    from interspeech_ser_amd import prosody as P
    torch.save(gold["sd"], tmp_path / P.CHECKPOINT_FILE)
    cfg = {"feat1_dim": 1024, "feat2_dim": 1024, "feat3_dim": 256}
    enc, ck = ["microsoft/wavlm-large", "roberta-large", P.NS3_PROSODY], ["", "", ""]
    geos = PR._stream_kinds(cfg, enc, ck, synthetic=True)
    assert geos[2] == P.ProsodySpec() and geos[2].family == P.NS3_PROSODY
    with pytest.raises(ValueError, match="feat3_dim = 256 in the config, but ns3-prosody has hidden size 128"):
        PR._stream_kinds(cfg, enc, ["", "", str(tmp_path)])                   # the tiny checkpoint: D = 128
    with pytest.raises(OSError, match="no prosody checkpoint"):
        PR._stream_kinds(cfg, enc, ["", "", str(tmp_path / "missing.bin")])
    assert PR._stream_kinds(cfg, enc[:2] + [PR.FILES], ck)[2] is None         # --encoder3 files stays as it is
