"""CPU: the host side of the 512-wide third stream (prosody rows | timbre rows).  The float64 statement tests/codec_ref.py against the
reference's own fp32 run (tests/golden/tiny_codec_ngf8.npz, tools/make_codec_golden.py); prosody.prepare_codec's folds against the
statement; the activation filter's restatement; the level-length and halo arithmetic; the three kernels' export, layout and validation;
the extraction driver around a stub encoder; the command lines."""
import ctypes
import inspect
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

import codec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ser_hip.h")
HEADS = 2
LENGTHS = (400, 799, 12800, 16000, 25999)
NEW = {"ser_codec_unit": "CODEC_UNIT", "ser_codec_conv": "CODEC_CONV", "ser_snake": "SNAKE"}        # SER_OP codes 16, 17, 18
# The reference's fp32 run sits <= 1.6e-6 from its own float64 run at this geometry and scale; 1e-5 leaves 6x for the fp16-rounded inputs
# and the summation order.
STATEMENT_TOL = 1e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return R.load_golden(golden_dir)


@pytest.fixture(scope="module")
def stated(gold):
    return [R.forward(gold["enc"], gold["dec"], w, HEADS) for w in gold["waves"]]


def test_fixture_is_what_the_tool_promises(gold):
    g = gold["g"]
    assert [len(w) for w in gold["waves"]] == list(LENGTHS)
    assert g["encoded"].shape == (283, 128) and g["timbre"].shape == (283, 128)
    assert all(v.dtype != object for v in g.values())                               # arrays only
    for b, n in ((0, 400), (1, 799)):
        P = R.padded_len(n)
        assert g[f"lv{b}.conv_in"].shape == (P, 8)
        assert [g[f"lv{b}.level_{i}"].shape for i in (1, 2, 3, 4)] == [(P // 2, 16), (P // 8, 32), (P // 40, 64), (P // 200, 128)]
    offs = gold["offs"]
    for b in range(5):                                                             # a max(1, .) error form tests something
        assert np.abs(g["encoded"][offs[b]: offs[b + 1]]).max() >= 1.0
    sizes = [os.path.getsize(os.path.join(ROOT, "tests", "golden", name)) for name in R.GOLDEN_FILES]
    assert len(sizes) == 2 and max(sizes) < (1 << 20) and sum(sizes) < 1_500_000     # each under the limit for a committed file


def test_statement_matches_the_reference_run(gold, stated):
    g, offs = gold["g"], gold["offs"]
    for b, st in enumerate(stated):
        sl = slice(offs[b], offs[b + 1])
        errs = {"encoded": R.rel_err(st["encoded"], g["encoded"][sl]), "timbre": R.rel_err(st["timbre"], g["timbre"][sl])}
        for k in g:
            if k.startswith(f"lv{b}."):
                errs[k] = R.rel_err(st[k.split(".", 1)[1]], g[k])
        print(f"wave {b}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= STATEMENT_TOL, errs
        assert st["encoded"].shape == (R.frames(LENGTHS[b]), 128)


def test_twin_is_an_fp32_evaluation_of_the_statement(gold, stated):
    for b in (0, 1):
        twin = R.torch_twin(gold["enc"], gold["waves"][b])
        for k, v in twin.items():
            assert v.shape == stated[b][k].shape and R.rel_err(v, stated[b][k]) <= STATEMENT_TOL, k


def test_statement_does_not_use_the_product(gold):
    src = inspect.getsource(R)
    assert "interspeech_ser_amd" not in src and "P.prepare" not in src


def _folded_codec(w, wave):
    """the codec from prosody.prepare_codec_f64's tensors alone (tap-major weights, e^alpha, 1 / (e^beta + 1e-9), one filter)"""
    npy = lambda t: t.numpy().astype(np.float64)
    taps = npy(w["taps"])
    act = lambda a, x: R.activation1d_folded(x, npy(a[0]), npy(a[1]), taps, taps)

    def conv(x, wt, b, k, **kw):
        wt = npy(wt)
        return R.conv1d(x, wt.reshape(wt.shape[0], k, -1).transpose(0, 2, 1), npy(b), **kw)

    y = np.asarray(wave, dtype=np.float64)
    x = np.concatenate([y, np.zeros(R.padded_len(len(y)) - len(y))])[:, None]
    out = {}
    x = out["conv_in"] = conv(x, *w["conv_in"], 7, pad=3)
    for i, lv in enumerate(w["levels"], start=1):
        for j, u in enumerate(lv["units"]):
            h = conv(act(u["act1"], x), u["w7"], u["b7"], 7, pad=3 * u["d"], dilation=u["d"])
            x = out[f"u{i}_{j}"] = x + conv(act(u["act2"], h), u["w1"], u["b1"], 1)
        x = out[f"level_{i}"] = conv(act(lv["act"], x), *lv["down"], 2 * lv["stride"], stride=lv["stride"], pad=lv["pad"])
    out["encoded+pos0"] = conv(act(w["final"]["act"], x), w["final"]["w"], w["final"]["b"], 3, pad=1)
    return out


def test_prepare_folds_reproduce_the_statement(gold, stated):
    from interspeech_ser_amd import prosody as P
    w = P.prepare_codec_f64(gold["enc"], gold["dec"], HEADS)
    assert w["spec"] == P.TINY_CODEC and w["spec"].hidden == 256
    for b in (0, 1):
        mine = _folded_codec(w, gold["waves"][b])
        for k, v in mine.items():
            ref = stated[b]["encoded"] + P.position0(128).numpy() if k == "encoded+pos0" else stated[b][k]
            assert R.rel_err(v, ref) <= 1e-12, (b, k)
    w32 = P.prepare_codec(gold["enc"], gold["dec"], HEADS)
    assert w32["levels"][0]["units"][0]["w7"].dtype == torch.float32 and tuple(w32["levels"][3]["down"][0].shape) == (128, 10 * 64)
    assert tuple(w32["conv_in"][0].shape) == (8, 7) and tuple(w32["final"]["w"].shape) == (128, 3 * 128)
    assert len(w32["layers"]) == 2 and tuple(w32["layers"][0]["fc1"][0].shape) == (64, 5 * 128)
    # both spellings of weight norm
    alt = {k.replace(".weight_g", ".parametrizations.weight.original0").replace(".weight_v", ".parametrizations.weight.original1"): v
           for k, v in gold["enc"].items()}
    w2 = P.prepare_codec(alt, gold["dec"], HEADS)
    assert torch.equal(w2["levels"][2]["units"][1]["w7"], w32["levels"][2]["units"][1]["w7"])


def test_filter_restatement_and_its_refusals(gold):
    from interspeech_ser_amd import prosody as P
    mine = P.kaiser_sinc_taps()
    bufs = [v for k, v in gold["enc"].items() if k.endswith(".filter")]
    assert len(bufs) == 2 * (4 * 7 + 1)                                               # up + down of every activation
    for f in bufs:
        assert tuple(f.shape) == (1, 1, 12) and np.abs(f.reshape(-1).double().numpy() - mine).max() <= 1e-6
    assert np.abs(R.kaiser_sinc_taps() - mine).max() <= 1e-15 and abs(mine.sum() - 1.0) < 1e-12 and np.allclose(mine, mine[::-1])
    key = next(k for k in gold["enc"] if k.endswith("downsample.lowpass.filter"))
    bad = dict(gold["enc"])
    bad[key] = bad[key] + 3e-7                                                        # within 1e-6 of the restatement, but not the others' copy
    with pytest.raises(ValueError, match="differ from each other"):
        P.prepare_codec(bad, gold["dec"], HEADS)
    bad = {k: (v * 1.001 if k.endswith(".filter") else v) for k, v in gold["enc"].items()}
    with pytest.raises(ValueError, match="Kaiser-sinc"):
        P.prepare_codec(bad, gold["dec"], HEADS)


def test_unsupported_shapes_are_refused_with_a_message(gold):
    from interspeech_ser_amd import prosody as P
    sd = P.synthetic_codec_state_dict(P.CodecSpec(ngf=24, out_channels=128, timbre=P.TINY_CODEC.timbre), 1)
    with pytest.raises(ValueError, match="unsupported codec widths"):
        P.codec_spec_from_state_dict(sd, gold["dec"], HEADS)
    sd = P.synthetic_codec_state_dict(P.CodecSpec(ngf=64, out_channels=128, timbre=P.TINY_CODEC.timbre), 1)
    with pytest.raises(ValueError, match="ngf = 64"):
        P.codec_spec_from_state_dict(sd, gold["dec"], HEADS)
    with pytest.raises(ValueError, match="heads of 64"):
        P.codec_spec_from_state_dict(gold["enc"], gold["dec"], 4)
    with pytest.raises(KeyError, match="is missing"):
        P.codec_spec_from_state_dict({k: v for k, v in gold["enc"].items() if not k.startswith("block.6.")}, gold["dec"], HEADS)
    full = P.synthetic_codec_state_dict()
    dec = P.synthetic_timbre_state_dict()
    assert P.codec_spec_from_state_dict(full, dec) == P.CodecSpec()
    assert (P.CodecSpec().ngf, P.CodecSpec().strides, P.CodecSpec().out_channels, P.CodecSpec().channels) == (32, (2, 4, 5, 5), 256, (32, 64, 128, 256, 512))


def test_level_lengths_and_halos_are_exact(gold, stated):
    from interspeech_ser_amd import prosody as P
    want = {400: 600, 799: 800, 12800: 13000, 16000: 16200, 25999: 26000}
    for n in LENGTHS:
        for spec in (P.CodecSpec(), P.TINY_CODEC):
            lens = spec.level_lengths(n)
            assert lens == (want[n], want[n] // 2, want[n] // 8, want[n] // 40, want[n] // 200)
            assert lens[-1] == n // 200 + 1 == R.frames(n) and 1 <= lens[0] - n <= 200
            assert all(a == b * s for a, b, s in zip(lens[:-1], lens[1:], spec.strides))
    for b in (0, 1):                                                                  # the statement's convolutions give those lengths
        lens = P.TINY_CODEC.level_lengths(LENGTHS[b])
        assert [len(stated[b][k]) for k in ("conv_in", "level_1", "level_2", "level_3", "level_4")] == list(lens)
    assert [P.CodecSpec.unit_halo(d) for d in (1, 3, 9)] == [15, 21, 39] and P.WIDE_HALO >= 27 and P.ACT_HALO == 6
    # an activation's output reaches 5 input rows a side, inside the 6 the kernels load: a spike 6 rows away changes nothing
    taps = P.kaiser_sinc_taps()
    x = np.zeros((40, 1))
    base = R.activation1d_folded(x, np.ones(1), np.ones(1), taps, taps)
    for off, touched in ((5, True), (-5, True), (6, False), (-6, False)):
        y = x.copy()
        y[20 + off] = 1.0
        assert (R.activation1d_folded(y, np.ones(1), np.ones(1), taps, taps)[20] != base[20]) == touched


def test_synthetic_weights_follow_the_recipe():
    from interspeech_ser_amd import prosody as P
    sd = P.synthetic_codec_state_dict(P.TINY_CODEC, 3)
    assert sd is not P.synthetic_codec_state_dict(P.TINY_CODEC, 3) and torch.equal(sd["block.0.weight_v"], P.synthetic_codec_state_dict(P.TINY_CODEC, 3)["block.0.weight_v"])
    v, g = sd["block.2.block.1.block.1.weight_v"], sd["block.2.block.1.block.1.weight_g"]
    assert tuple(v.shape) == (16, 16, 7) and tuple(g.shape) == (16, 1, 1)
    assert torch.allclose(g.reshape(-1), v.pow(2).sum(dim=(1, 2)).sqrt() * (0.5 / (16 * 7)) ** 0.5)
    for k, t in sd.items():
        if k.endswith(".bias"):
            assert float(t.abs().max()) <= 0.1
        if k.endswith(".alpha") or k.endswith(".beta"):
            assert float(t.abs().max()) <= 0.5
    before = P.synthetic_state_dict(P.TINY, 7)                                        # the plain stream's draw is what it was
    assert float(before["melspec_linear.weight"][0, 0]) == float(P.synthetic_state_dict(P.TINY, 7)["melspec_linear.weight"][0, 0])
    assert set(P.synthetic_timbre_state_dict(P.TINY)) == {k.replace(P.ENC, P.TIMBRE) for k in before if k.startswith(P.ENC)}


# ------------------------------------------------------------------------------------------------------------- ABI
def test_new_exports_are_additive(built_library):
    from interspeech_ser_amd import _lib
    text = open(HEADER).read()
    so = ctypes.CDLL(built_library)
    for val, (name, op) in enumerate(NEW.items(), start=16):
        assert hasattr(so, name + "_v") and name + "_v" in _lib.EXPORTED_SYMBOLS
        assert f"int {name}_v(const {name}_args* args, void* stream);" in text
        assert f"#define SER_OP_{op} {val}" in text and getattr(_lib, "OP_" + op) == val
    assert _lib.lib.ser_version() == 18 == _lib.ABI_VERSION                            # additive: the ABI number stays
    assert f"#define SER_CODEC_TILE {_lib.CODEC_TILE}" in text and _lib.CODEC_TILE % 64 == 0
    assert "codec.hip" in open(os.path.join(ROOT, "interspeech_ser_amd", "csrc", "Makefile")).read()


def test_struct_layouts_match_c(built_library, tmp_path):
    from interspeech_ser_amd._lib import STRUCT_MIRRORS
    lines = ['printf("ser_gemm_args.sizeof %zu\\n", sizeof(ser_gemm_args));']
    for name in NEW:
        cname, cls = name + "_args", STRUCT_MIRRORS[name + "_args"]
        lines.append(f'printf("{cname}.sizeof %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, *_ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0; }\n' % (HEADER, "\n".join(lines)))
    subprocess.check_call(["gcc", str(src), "-o", str(tmp_path / "layout")])
    out = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    for name in NEW:
        cname, cls = name + "_args", STRUCT_MIRRORS[name + "_args"]
        assert int(out[cname + ".sizeof"]) == ctypes.sizeof(cls) <= int(out["ser_gemm_args.sizeof"])     # ser_cmd does not grow
        for f, *_ in cls._fields_:
            assert int(out[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_launchers_validate_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    L, err = _lib.lib, _lib.lib.ser_last_error
    # ---- the unit
    assert L.ser_codec_unit_v(None, None) == -1 and b"ser_codec_unit: null pointer" in err()
    u = _lib.CodecUnitArgs()
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -1
    for i, f in enumerate(("x", "y", "row_offs", "taps", "ea1", "ib1", "w7", "b7", "ea2", "ib2", "w1", "b1")):
        setattr(u, f, 4096 * (i + 1))                                                  # never dereferenced
    u.B, u.C, u.k, u.dilation, u.max_rows, u.rows = 1, 12, 7, 1, 10, 10
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -2 and b"C=12" in err()
    u.C = 40
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -2 and b"C=40" in err()
    u.C, u.k = 32, 6
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -2 and b"k=6" in err()
    u.k, u.rows = 7, -1
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -2 and b"rows=-1" in err()
    u.rows, u.dilation = 10, 27
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -2 and b"dilation=27" in err()
    u.dilation, u.y = 9, u.x
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -3 and b"must not be x" in err()
    u.y, u.ea1 = 8192, None
    assert L.ser_codec_unit_v(ctypes.byref(u), None) == -1
    # ---- the narrow convolution
    assert L.ser_codec_conv_v(None, None) == -1 and b"ser_codec_conv: null pointer" in err()
    c = _lib.CodecConvArgs()
    c.x, c.in_offs, c.out_offs, c.w, c.bias, c.y = 4096, 8192, 12288, 16384, 20480, 24576
    c.B, c.C_in, c.C_out, c.k, c.stride, c.pad, c.max_out_rows, c.rows, c.ldy = 1, 12, 16, 4, 2, 1, 5, 5, 16
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -2 and b"C_in=12" in err()
    c.C_in = 64
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -2 and b"C_in=64" in err()
    c.C_in, c.C_out = 8, 12
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -2 and b"C_out=12" in err()
    c.C_out, c.rows = 16, -3
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -2 and b"rows=-3" in err()
    c.rows, c.stride = 5, 9
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -2 and b"stride=9" in err()
    c.stride, c.ea = 2, 28672
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -1 and b"needs ea, ib and taps" in err()
    c.ea, c.ldy = None, 8
    assert L.ser_codec_conv_v(ctypes.byref(c), None) == -3 and b"ldy=8" in err()
    # ---- the wide activation
    assert L.ser_snake_v(None, None) == -1 and b"ser_snake: null pointer" in err()
    s = _lib.SnakeArgs()
    s.x, s.row_offs, s.taps, s.ea, s.ib, s.out_act = 4096, 8192, 12288, 16384, 20480, 24576
    s.ldx = s.ldo_act = 64
    s.B, s.C, s.max_rows, s.rows, s.mode = 1, 32, 3, 3, _lib.MODE_FP16X
    assert L.ser_snake_v(ctypes.byref(s), None) == -2 and b"C=32" in err()
    s.C, s.rows = 64, -1
    assert L.ser_snake_v(ctypes.byref(s), None) == -2 and b"rows=-1" in err()
    s.rows, s.mode = 3, _lib.MODE_FP16M
    assert L.ser_snake_v(ctypes.byref(s), None) == -4 and b"bad mode" in err()
    s.mode, s.ldx = _lib.MODE_BF16, 62
    assert L.ser_snake_v(ctypes.byref(s), None) == -3
    s.ldx, s.out_act = 64, None
    assert L.ser_snake_v(ctypes.byref(s), None) == -1
    cmds = (_lib.Cmd * 1)()
    for op, name in ((_lib.OP_CODEC_UNIT, b"ser_codec_unit"), (_lib.OP_CODEC_CONV, b"ser_codec_conv"), (_lib.OP_SNAKE, b"ser_snake")):
        cmds[0].op = op                                                                # the command list reaches the new launchers
        assert L.ser_run(cmds, 1, None, None) == -1 and name in err()


# ------------------------------------------------------------------------------------------------------------- driver and command lines
class _StubEncoder:
    """what the driver needs of engine.SpeakerProsodyEncoder: rows [M, 2 D] = (file's first sample, frame index) pattern"""
    D = 4

    def forward(self, waves):
        if min(len(w) for w in waves) < 400:
            raise ValueError("utterance shorter than 400 samples: it cannot be reflect-padded (the reference fails such a file)")
        T = [len(w) // 200 + 1 for w in waves]
        rows = torch.cat([torch.full((t, 2 * self.D), float(w[0])) + torch.arange(t)[:, None] for t, w in zip(T, waves)])
        offs = [0] + [int(v) for v in np.cumsum(T)]
        return type("F", (), dict(rows=rows, frame_offs=offs, take_range_bits=lambda self: 0))()


def _write_wav(path, samples):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.asarray(samples, dtype=np.int16).tobytes())


def test_driver_end_to_end_around_a_stub(built_library, tmp_path, monkeypatch, capsys):
    from interspeech_ser_amd import prosody as P
    wavs, out = tmp_path / "wav", tmp_path / "out"
    wavs.mkdir()
    lengths = {"a.wav": 400, "b.wav": 1234, "c.wav": 399, "d.wav": 4000}
    for i, (name, n) in enumerate(lengths.items()):
        _write_wav(wavs / name, np.full(n, 1000 * (i + 1)))
    (wavs / "e.wav").write_bytes(b"not a wave file")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    assert P.run_speaker(["--wav_dir", str(wavs), "--save_path", str(out), "--num_workers", "2", "--batch_size", "3"], encoder=_StubEncoder()) == 0
    text = capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["a.pt", "b.pt", "d.pt"]
    for i, name in ((0, "a"), (1, "b"), (3, "d")):
        t = torch.load(out / f"{name}.pt")
        T = lengths[name + ".wav"] // 200 + 1
        assert t.dtype == torch.float32 and tuple(t.shape) == (T, 2 * _StubEncoder.D)
        assert torch.equal(t[:, 0], 1000 * (i + 1) / 32768.0 + torch.arange(T, dtype=torch.float32))
    assert f"Failed to process {wavs / 'c.wav'}: utterance shorter than 400 samples" in text
    assert f"Failed to process {wavs / 'e.wav'}" in text and "3 files processed, 2 failed" in text
    assert "Extracting prosody codes from NaturalSpeech3" in text and "5 file are going to be processed..." in text


def test_driver_command_line(tmp_path):
    from interspeech_ser_amd import prosody as P
    a = P.build_parser(speaker=True).parse_args(["--wav_dir", "W", "--save_path", "S", "--num_workers", "3"])
    assert (a.wav_dir, a.save_path, a.num_workers, a.seed, a.checkpoint, a.encoder_checkpoint, a.mode, a.batch_size) == ("W", "S", 3, 7, "", "", "f16x", 16)
    a = P.build_parser(speaker=True).parse_args(["--checkpoint", "ckpt", "--encoder_checkpoint", "enc.bin", "--mode", "bf16", "--synthetic_weights"])
    assert (a.checkpoint, a.encoder_checkpoint, a.mode, a.synthetic_weights) == ("ckpt", "enc.bin", "bf16", True)
    with pytest.raises(SystemExit):
        P.build_parser().parse_args(["--encoder_checkpoint", "x"])                    # the plain stream's command line is what it was
    assert "interspeech_ser_amd.prosody import run_speaker" in open(os.path.join(ROOT, "preprocessing", "preprocess_ns3_prosody_speaker.py")).read()
    d = tmp_path / "ns3"
    assert P.encoder_checkpoint_path(str(d / P.CHECKPOINT_FILE)) == str(d / P.ENCODER_CHECKPOINT_FILE)
    d.mkdir()
    assert P.encoder_checkpoint_path(str(d)) == str(d / P.ENCODER_CHECKPOINT_FILE)
    assert P.encoder_checkpoint_path(str(d), "other.bin") == "other.bin" and P.encoder_checkpoint_path("", str(d)) == str(d / P.ENCODER_CHECKPOINT_FILE)
    with pytest.raises(OSError, match="no codec encoder checkpoint"):
        P.load_encoder_state_dict(str(d))


def test_stream_kinds_report_the_512_wide_stream(gold, tmp_path):
    from interspeech_ser_amd import predictor as PR
    from interspeech_ser_amd import prosody as P
    dec = dict(gold["prosody"]["sd"])
    dec.update(gold["dec"])
    torch.save(dec, tmp_path / P.CHECKPOINT_FILE)
    torch.save(gold["enc"], tmp_path / P.ENCODER_CHECKPOINT_FILE)
    enc, ck = ["microsoft/wavlm-large", "roberta-large", P.NS3_PROSODY_SPEAKER], ["", "", ""]
    cfg = {"feat1_dim": 1024, "feat2_dim": 1024, "feat3_dim": 512}
    geos = PR._stream_kinds(cfg, enc, ck, synthetic=True)
    assert geos[2] == P.CodecSpec() and geos[2].family == P.NS3_PROSODY_SPEAKER == "ns3-prosody-speaker" and geos[2].hidden == 512
    with pytest.raises(ValueError, match="feat3_dim = 256 in the config, but ns3-prosody-speaker has hidden size 512"):
        PR._stream_kinds(dict(cfg, feat3_dim=256), enc, ck, synthetic=True)
    with pytest.raises(ValueError, match="heads of 64"):                              # the tiny pair has heads of 64 only with 2 heads
        PR._stream_kinds(cfg, enc, ["", "", str(tmp_path)])
    assert P.resolve_codec_spec(str(tmp_path), heads=2) == P.TINY_CODEC
