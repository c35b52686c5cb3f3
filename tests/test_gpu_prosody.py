"""GPU: the prosody stream -- ser_prosody_mel_v, ser_fvq_v, ser_act_rows_v through the C ABI and engine.ProsodyEncoder, the
FusionPredictor's ProsodyStream, the extraction driver and the scoring command -- against the float64 statement tests/prosody_ref.py and
the reference's own run (tests/golden/tiny_prosody_d128h2.npz).  Each test prints its numbers (lines starting PROSODY).

Bounds.  Log-mel: the fp32 torch.stft path's own distance from the statement on the same wave (the kernel accumulates in float64 and may
not be farther).  z: tests/test_gpu_e2e.py's gates (1e-3; bf16 3e-2), error form max|a - b| / max(1, max|b|).  Codes: a code may differ
from the float64 statement's only where the statement's top-2 gap is <= 1e-5 (the fp32 storage of eight normalised code components moves
a distance by about 2e-6), and then the chosen code's float64 distance is within 1e-5 of the best.  The fourth end-to-end property of the
issue ("the share of differing frames is no larger than the fixture's share under that gap") is read as continuing the sentence before it:
asserted in f16x and fp32x, printed in bf16, whose 3e-2 gate on z promises no code."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import prosody_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HEADS = 2
TOL = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}          # tests/test_gpu_e2e.py TOL
GAP_SURE, GAP_SLACK = 1e-5, 1e-5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def fx(built_library, golden_dir):
    """the fixture, the float64 statement and the fp32 twin of every wave (computed once), and one f16x encoder"""
    from interspeech_ser_amd.engine import ProsodyEncoder
    gold = R.load_golden(golden_dir)
    gold["stated"] = [R.forward(gold["sd"], w, HEADS) for w in gold["waves"]]
    gold["twin_mel"] = [R.torch_log_mel(w).numpy() for w in gold["waves"]]
    gold["sd64"] = R._f64(gold["sd"])
    gold["enc"] = ProsodyEncoder(gold["sd"], DEV, "f16x", heads=HEADS)
    return gold


def _check_codes(what, codes, gaps_dev, z_dev, sd64):
    """the device's codes / gaps against the statement's quantizer on the rows the device quantized; returns the statement's result"""
    q = R.quantize(sd64, np.asarray(z_dev, dtype=np.float64))
    sure = q["gaps"] > GAP_SURE
    chosen = q["dist"][np.arange(len(codes)), codes]
    slack = float((chosen - q["dist"].min(axis=1)).max())
    gap_err = float(np.abs(np.asarray(gaps_dev, dtype=np.float64) - q["gaps"]).max())
    print(f"PROSODY {what}: {int((codes != q['codes']).sum())} of {len(codes)} codes differ from the statement's ({int((~sure).sum())} frames "
          f"with a gap <= {GAP_SURE:g}); worst chosen-minus-best distance {slack:.2e}; gap error {gap_err:.2e}")
    assert np.array_equal(codes[sure], q["codes"][sure])
    assert slack <= GAP_SLACK and gap_err <= GAP_SLACK
    return q


# ----------------------------------------------------------------------------------------------------------------------- log-mel
def test_log_mel_every_value_against_the_statement(fx):
    enc, waves, offs = fx["enc"], fx["waves"], fx["offs"]
    mel = enc.log_mel(waves).cpu().numpy()
    assert mel.shape == (offs[-1], 20) and mel.dtype == np.float32
    for j, st in enumerate(fx["stated"]):
        got, ref = mel[offs[j]: offs[j + 1]], st["mel"]
        bound = R.rel_err(fx["twin_mel"][j], ref)
        err = R.rel_err(got, ref)
        edge = [0, 1, len(ref) - 2, len(ref) - 1]                          # the frames reflection touches
        e_edge, b_edge = R.rel_err(got[edge], ref[edge]), R.rel_err(fx["twin_mel"][j][edge], ref[edge])
        print(f"PROSODY log-mel wave {j} ({len(waves[j])} samples, {len(ref)} frames): {err:.3e} (torch.stft path {bound:.3e}); "
              f"reflected frames {e_edge:.3e} ({b_edge:.3e})")
        assert err <= bound and e_edge <= b_edge
        alone = enc.log_mel([waves[j]], slot=1).cpu().numpy()              # batched equals batch-of-one, bit for bit
        assert np.array_equal(_bits(alone), _bits(got))


def test_log_mel_of_silence_through_the_c_abi(fx):
    """an all-zero wave gives log(1e-5) exactly, in every bin of every frame; launched through ser_prosody_mel_v itself"""
    from interspeech_ser_amd import _lib
    enc = fx["enc"]
    lengths = [400, 1000, 3400]
    T = [n // 200 + 1 for n in lengths]
    wav = torch.zeros(sum(lengths), dtype=torch.float32, device=DEV)
    so = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=DEV)
    fo = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=DEV)
    out = torch.full((sum(T), 20), float("nan"), dtype=torch.float32, device=DEV)
    a = _lib.ProsodyMelArgs()
    a.wav, a.sample_offs, a.frame_offs, a.dft, a.mel = wav.data_ptr(), so.data_ptr(), fo.data_ptr(), enc.dft.data_ptr(), enc.melw.data_ptr()
    a.mel_out, a.B, a.max_frames, a.n_bins, a.n_mels = out.data_ptr(), 3, max(T), enc.n_bins, 20
    _lib.check(_lib.lib.ser_prosody_mel_v(ctypes.byref(a), _stream()), "ser_prosody_mel_v")
    torch.cuda.synchronize()
    want = np.float32(np.log(1e-5))
    assert want == np.float32(np.log(np.float64(np.float32(1e-5))))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(np.full((sum(T), 20), want)))


# --------------------------------------------------------------------------------------------------------------------- ser_fvq_v
def gpu_fvq(z, w, codes=None, table=None, mode=None):
    """ser_fvq_v on fp32 rows -> (idx, gap, out rows, planes as raw words or None, range bits, error word)"""
    from interspeech_ser_amd import _lib
    codes = w["codes"] if codes is None else codes
    table = w["table"] if table is None else table
    M, D = z.shape
    zd, wi, bi, cd, td = _dev(z), w["w_in"].to(DEV), w["b_in"].to(DEV), codes.to(DEV).contiguous(), table.to(DEV).contiguous()
    idx = torch.full((M,), -1, dtype=torch.int32, device=DEV)
    gap = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((M, D), float("nan"), dtype=torch.float32, device=DEV)
    flag, err = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    a = _lib.FvqArgs()
    a.z, a.ldz, a.w_in, a.b_in, a.codes, a.table, a.ld_table = zd.data_ptr(), D, wi.data_ptr(), bi.data_ptr(), cd.data_ptr(), td.data_ptr(), D
    a.idx, a.gap, a.out_f32, a.ldo_f32, a.range_flag, a.err = idx.data_ptr(), gap.data_ptr(), out.data_ptr(), D, flag.data_ptr(), err.data_ptr()
    a.rows, a.D, a.n_codes, a.code_dim, a.mode = M, D, codes.shape[0], 8, _lib.MODE_BF16
    act = None
    if mode is not None:
        act = torch.zeros((1 if mode == _lib.MODE_BF16 else 2, M, D), dtype=torch.int16, device=DEV)
        a.out_act, a.ldo_act, a.out_plane_stride, a.mode = act.data_ptr(), D, M * D, mode
    _lib.check(_lib.lib.ser_fvq_v(ctypes.byref(a), _stream()), "ser_fvq_v")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), gap.cpu().numpy(), out.cpu().numpy(), (None if act is None else act.cpu()), int(flag.item()), int(err.item())


def test_fvq_on_rows_handed_in(fx):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd import prosody as P
    w = P.prepare(fx["sd"], HEADS)
    z = fx["g"]["z"]                                                        # the reference's own fp32 rows: 283 x 128
    idx, gap, out, act, bits, err = gpu_fvq(z, w, mode=_lib.MODE_FP16X)
    _check_codes("ser_fvq_v on the fixture's z", idx, gap, z, fx["sd64"])
    assert (bits, err) == (0, 0)
    table = w["table"].numpy()
    assert np.array_equal(_bits(out), _bits(table[idx]))                    # the output row is the table row, bit for bit
    planes = act.view(torch.float16).float().sum(dim=0).numpy()             # hi + lo fp16 planes
    assert np.abs(planes - out).max() <= 2.0 ** -21 * max(1.0, float(np.abs(out).max()))
    sure = fx["g"]["gaps"] > GAP_SURE
    assert np.array_equal(idx[sure], fx["g"]["codes"][sure])               # ... and the reference's own codes
    # bf16 planes, one plane; no planes at all
    _, _, out_b, act_b, bits_b, _ = gpu_fvq(z[:9], w, mode=_lib.MODE_BF16)
    assert bits_b == 0 and np.array_equal(act_b.view(torch.bfloat16)[0].float().numpy(), torch.from_numpy(out_b).bfloat16().float().numpy())


def test_fvq_ties_go_to_the_lowest_index(fx):
    """The codebook twice over (code n + 64 = code n: the same lane meets both, 64 codes apart) with codes 20 and 50 -- which no frame
    of the fixture takes -- overwritten by code 18, which many take (three lanes hold one code): every row ties, the lowest index wins
    and the gap is exactly 0."""
    from interspeech_ser_amd import prosody as P
    w = P.prepare(fx["sd"], HEADS)
    codes = torch.cat([w["codes"], w["codes"]]).clone()
    for n in (20, 50, 64 + 20, 64 + 50):
        codes[n] = codes[18]
    table = torch.arange(128, dtype=torch.float32)[:, None].repeat(1, 128).contiguous()      # row n holds n: the lookup shows the index
    z = fx["g"]["z"][:130]
    idx, gap, out, _, _, err = gpu_fvq(z, w, codes=codes, table=table)
    c = codes.double().numpy()
    e = R.quantize(fx["sd64"], z.astype(np.float64))["e"]
    dist = (e ** 2).sum(axis=1, keepdims=True) - 2.0 * e @ c.T + (c ** 2).sum(axis=1)[None, :]
    canon = np.arange(128) % 64                                             # the lowest index that holds the same code
    canon[np.isin(canon, (20, 50))] = 18
    best = dist.min(axis=1)
    near = dist <= best[:, None] + GAP_SURE                                 # float64 distances of one code differ by ~1e-16 between its copies
    lo, hi = np.where(near, canon[None, :], 128).min(axis=1), np.where(near, canon[None, :], -1).max(axis=1)
    sure = lo == hi                                                         # only copies of ONE code are that near
    print(f"PROSODY ties: {int(sure.sum())} of {len(idx)} rows with one nearest code; {int((lo == 18).sum())} rows nearest to code 18")
    assert err == 0 and sure.sum() >= 100 and (lo[sure] == 18).sum() >= 5 and (gap == 0.0).all()
    assert np.array_equal(idx[sure], lo[sure])
    assert (dist[np.arange(len(idx)), idx] - best <= GAP_SLACK).all() and (idx < 64).all() and not np.isin(idx, (20, 50)).any()
    assert np.array_equal(out[:, 0].astype(np.int64), idx)


def test_fvq_nan_row_sets_the_error_word(fx):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd import prosody as P
    w = P.prepare(fx["sd"], HEADS)
    z = fx["g"]["z"][:10].copy()
    clean = gpu_fvq(z, w)
    assert clean[5] == 0
    z[3, 17] = np.nan
    idx, gap, out, _, _, err = gpu_fvq(z, w)
    assert err & _lib.FVQ_ERR_NONFINITE and 0 <= idx[3] < 64
    keep = np.arange(10) != 3
    assert np.array_equal(idx[keep], clean[0][keep]) and np.array_equal(_bits(out[keep]), _bits(clean[2][keep]))
    z[3, 17] = np.inf
    assert gpu_fvq(z, w)[5] & _lib.FVQ_ERR_NONFINITE


# ----------------------------------------------------------------------------------------------------------------- ser_act_rows_v
@pytest.mark.parametrize("mode_name", ["f16x", "bf16"])
def test_act_rows_relu_rowmap_and_range_guard(built_library, mode_name):
    from interspeech_ser_amd import _lib
    mode = {"f16x": _lib.MODE_FP16X, "bf16": _lib.MODE_BF16}[mode_name]
    rng = np.random.default_rng(4)
    M, D = 7, 132                                                           # more than one block of 4 rows; D no multiple of 256
    x = rng.standard_normal((M, D)).astype(np.float32) * 3
    rowmap = np.array([2, 3, 4, 7, 8, 11, 12], dtype=np.int32)
    planes = 2 if mode == _lib.MODE_FP16X else 1
    dt = torch.float16 if mode == _lib.MODE_FP16X else torch.bfloat16

    def run(xs, relu, rm):
        xd = _dev(xs)
        act = torch.zeros((planes, 14, D), dtype=torch.int16, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        a = _lib.ActRowsArgs()
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = xd.data_ptr(), D, act.data_ptr(), D, 14 * D
        a.out_rowmap = None if rm is None else _dev(rm, np.int32).data_ptr()
        a.range_flag, a.relu, a.mode, a.rows, a.D = flag.data_ptr(), relu, mode, M, D
        _lib.check(_lib.lib.ser_act_rows_v(ctypes.byref(a), _stream()), "ser_act_rows_v")
        torch.cuda.synchronize()
        return act.view(dt).float().sum(dim=0).cpu().numpy(), int(flag.item())

    def want(v):
        t = torch.from_numpy(v)
        hi = t.to(dt)
        return (hi.float() + ((t - hi.float()).to(dt).float() if planes == 2 else 0)).numpy()

    got, bits = run(x, 1, rowmap)
    assert bits == 0 and np.array_equal(got[rowmap], want(np.maximum(x, 0))) and not got[np.setdiff1d(np.arange(14), rowmap)].any()
    got, bits = run(x, 0, None)
    assert bits == 0 and np.array_equal(got[:M], want(x)) and not got[M:].any()
    x[5, 130] = 7.0e4
    assert run(x, 1, None)[1] == (3 if mode == _lib.MODE_FP16X else 0)      # the fp16 range guard, as in every kernel that writes such planes
    x[5, 130] = -7.0e4
    assert run(x, 1, None)[1] == 0                                          # ... of the values written: ReLU leaves 0
    x[5, 130] = np.nan
    assert run(x, 1, None)[1] == (3 if mode == _lib.MODE_FP16X else 0)


# -------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_end_to_end_against_the_statement(fx, mode):
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.engine import ProsodyEncoder
    g, offs, waves = fx["g"], fx["offs"], fx["waves"]
    enc = fx["enc"] if mode == "f16x" else ProsodyEncoder(fx["sd"], DEV, mode, heads=HEADS)
    out = enc.forward(waves)
    assert out.frame_offs == [int(v) for v in offs] and out.batch == 5 and [out.frames(b) for b in range(5)] == [3, 4, 65, 81, 130]
    z, codes, gaps, rows = out.z.cpu().numpy(), out.codes.cpu().numpy(), out.gaps.cpu().numpy(), out.rows.cpu().numpy()
    assert out.take_range_bits() == 0 and tuple(rows.shape) == (283, 128)
    z_ref = np.concatenate([st["z"] for st in fx["stated"]])
    err = max(R.rel_err(z[offs[j]: offs[j + 1]], st["z"]) for j, st in enumerate(fx["stated"]))
    print(f"PROSODY {mode} z against the statement: {err:.3e} (gate {TOL[mode]:.0e})")
    assert err < TOL[mode]
    # the device's codes are the statement's quantizer applied to the device's own z
    q_dev = _check_codes(f"{mode} codes on the device's z", codes, gaps, z, fx["sd64"])
    assert np.array_equal(_bits(rows), _bits(P.prepare(fx["sd"], HEADS)["table"].numpy()[codes]))
    # against the reference's run
    e_ref = R.quantize(fx["sd64"], z_ref)["e"]
    de = float(np.sqrt(((q_dev["e"] - e_ref) ** 2).sum(axis=1)).max())
    wide = g["gaps"] > 1e-3
    differ = codes != g["codes"]
    share, allowed = float(differ.mean()), float((~wide).mean())
    print(f"PROSODY {mode}: max |e_dev - e_ref| {de:.3e} (4x = {4 * de:.3e} against the 1e-3 gap); {int(differ.sum())} of {len(codes)} frames "
          f"differ from the fixture's codes (share {share:.4f}, fixture's share under the gap {allowed:.4f})")
    if mode != "bf16":
        assert 4 * de <= 1e-3, "the z accuracy is what failed: a latent moved by more than a quarter of the 1e-3 gap"
        assert not differ[wide].any()
        assert share <= allowed


def test_full_geometry_on_two_short_waves(built_library):
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.engine import ProsodyEncoder
    sd = P.synthetic_state_dict(seed=11)
    rng = np.random.default_rng(12)
    waves = [(0.3 * np.sin(np.arange(n) * f) + 0.05 * rng.standard_normal(n)).astype(np.float32) for n, f in ((1000, 0.11), (3333, 0.07))]
    enc = ProsodyEncoder(sd, DEV, "f16x")
    assert enc.spec == P.ProsodySpec() and (enc.spec.hidden, enc.spec.num_layers, enc.spec.n_codes, enc.spec.ffn) == (256, 4, 1024, 1024)
    out = enc.forward(waves)
    z, codes, gaps, rows = out.z.cpu().numpy(), out.codes.cpu().numpy(), out.gaps.cpu().numpy(), out.rows.cpu().numpy()
    assert out.frame_offs == [0, 6, 23] and out.take_range_bits() == 0
    sd64 = R._f64(sd)
    for j, w in enumerate(waves):
        st = R.forward(sd, w, 4)
        sl = slice(out.frame_offs[j], out.frame_offs[j + 1])
        err = R.rel_err(z[sl], st["z"])
        print(f"PROSODY full geometry wave {j}: z {err:.3e} (gate {TOL['f16x']:.0e}); mel {R.rel_err(out.mel.cpu().numpy()[sl], st['mel']):.3e}")
        assert err < TOL["f16x"]
        sure = st["gaps"] > 1e-3
        assert np.array_equal(codes[sl][sure], st["codes"][sure])
    _check_codes("full geometry codes on the device's z", codes, gaps, z, sd64)
    assert np.array_equal(_bits(rows), _bits(P.prepare(sd)["table"].numpy()[codes]))


def test_replay_equals_a_fresh_eager_forward(fx):
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import ProsodyEncoder
    waves = fx["waves"]
    eager = ProsodyEncoder(fx["sd"], DEV, "f16x", heads=HEADS)
    eager.use_tape = False
    taped = ProsodyEncoder(fx["sd"], DEV, "f16x", heads=HEADS)
    # slot 0: recorded on the first batch, the largest, sizes patched for the others.  Slot 1 starts small: the arena grows under a recorded
    # list (which must be recorded again over the new buffers), then holds a subset and the full batch again
    runs = [(batch, 0) for batch in (waves, [waves[3], waves[0]], [waves[1]], waves)]
    runs += [(batch, 1) for batch in ([waves[1]], waves, [waves[3], waves[0]], waves)]
    for batch, slot in runs:
        a, b = eager.forward(batch, slot=slot), taped.forward(batch, slot=slot)
        lens = [len(w) for w in batch]
        assert taped.recorded_tape(lens, slot).n > 0
        with pytest.raises(_lib.SerHipError, match="no recorded command list"):
            eager.recorded_tape(lens, slot)
        for name in ("mel", "z", "rows", "gaps"):
            assert np.array_equal(_bits(getattr(a, name).cpu().numpy()), _bits(getattr(b, name).cpu().numpy())), name
        assert torch.equal(a.codes, b.codes) and a.frame_offs == b.frame_offs
        assert a.take_range_bits() == 0 and b.take_range_bits() == 0


def test_short_wave_fails_alone(fx):
    enc = fx["enc"]
    with pytest.raises(ValueError, match="400 samples"):
        enc.forward([fx["waves"][0], fx["short"]])
    assert enc.forward([fx["waves"][0]]).frame_offs == [0, 3]


# --------------------------------------------------------------------------------------------------------------------- predictor
def test_prosody_stream_equals_rows_handed_in(fx, golden_dir):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder, TextEncoder, TrimodalHead
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, ProsodyStream, RowsStream, TextStream
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle.fusion_head import seeded_head_weights
    import fusion3_ref as R3
    import fusion_ref as RF
    gt = np.load(os.path.join(golden_dir, "tiny_roberta_d128h2.npz"))
    ids = torch.from_numpy(np.stack([gt[f"ids_{j}"] for j in range(2)]))
    mask = torch.from_numpy(np.stack([gt[f"mask_{j}"] for j in range(2)]))
    hubert = SpeechEncoder(C.TINY_HUBERT, synthetic_state_dict(C.TINY_HUBERT, 3), DEV, mode="f16x")
    roberta = TextEncoder(C.TINY_ROBERTA, synthetic_state_dict(C.TINY_ROBERTA, int(gt["seed"])), DEV, mode="f16x")
    enc, waves = fx["enc"], [fx["waves"][1], fx["waves"][2]]
    feats = enc.forward(waves)
    rows = [feats.rows[feats.frame_offs[b]: feats.frame_offs[b + 1]].cpu().clone() for b in range(2)]
    sd3 = seeded_head_weights(R3.head_shapes(320, 128, 128, h=64), 9)
    got = FusionPredictor([AudioStream(hubert, state=1), TextStream(roberta), ProsodyStream(enc)], sd3).predict(waves, ids, mask)
    pred = FusionPredictor([AudioStream(hubert, state=1), TextStream(roberta), RowsStream(128)], sd3)
    want = pred.predict(waves, ids, mask, rows)
    assert isinstance(pred.head, TrimodalHead) and got.shape == (2, 8) and np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(want))
    # any position: first of two
    sd2 = seeded_head_weights(RF.head_shapes(128, 320, h=64), 8)
    got = FusionPredictor([ProsodyStream(enc), AudioStream(hubert, state=1)], sd2).predict(waves)
    head_rows = FusionPredictor([AudioStream(hubert, state=1), ProsodyStream(enc)], seeded_head_weights(RF.head_shapes(320, 128, h=64), 8))
    assert got.shape == (2, 8) and np.isfinite(got).all() and head_rows.predict(waves).shape == (2, 8)
    with pytest.raises(ValueError, match="prosody encoder"):
        FusionPredictor([AudioStream(hubert, state=1), ProsodyStream(roberta)], sd2)
    with pytest.raises(ValueError, match="400 samples"):
        head_rows.predict([fx["waves"][1], fx["short"]])


def _write_wav(path, x):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.round(np.asarray(x, dtype=np.float64) * 32768.0).astype("<i2").tobytes())


def test_driver_writes_the_reference_files(fx, tmp_path, capsys):
    from interspeech_ser_amd import prosody as P
    wav_dir, out = tmp_path / "Audios", tmp_path / "ns3"
    wav_dir.mkdir()
    picks = {"a.wav": fx["waves"][1], "b.wav": fx["waves"][3], "short.wav": fx["short"], "c.wav": fx["waves"][0]}
    for name, w in picks.items():
        _write_wav(wav_dir / name, w)                                       # int16 PCM / 32768: the fixture's waves exactly
    (wav_dir / "broken.wav").write_bytes(b"RIFF")
    assert P.run(["--wav_dir", str(wav_dir), "--save_path", str(out), "--num_workers", "2", "--batch_size", "3"], encoder=fx["enc"]) == 0
    log = capsys.readouterr().out
    assert sorted(os.listdir(out)) == ["a.pt", "b.pt", "c.pt"], log
    assert log.count("Failed to process") == 2 and f"Failed to process {wav_dir / 'short.wav'}" in log and "broken.wav" in log, log
    assert "3 files processed, 2 failed" in log
    for name, w in picks.items():
        if name == "short.wav":
            continue
        t = torch.load(out / name.replace(".wav", ".pt"), weights_only=True)
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(w) // 200 + 1, 128)
        alone = fx["enc"].forward([w]).rows.cpu()
        assert torch.equal(t, alone)                                        # (the head's rows: table rows, whatever the batch around them)


def test_scoring_from_wav_equals_the_route_through_the_drivers_files(built_library, tmp_path, capsys):
    """bin/predict_cat_from_wav.py --encoder3 ns3-prosody on synthetic weights writes, byte for byte, the results/test.csv that the
    driver's .pt files give through --encoder3 files in the same modes."""
    import pandas as pd
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.predictor import score_from_wav
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import synth_wave
    import fusion3_ref as R3
    geo, max_len = C.TINY_ROBERTA, 16
    wav_dir, lazy3 = tmp_path / "Audios", tmp_path / "ns3"
    wav_dir.mkdir()
    lengths = (4800, 12800, 399, 9000)
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(len(lengths))]
    for i, (name, n) in enumerate(zip(names, lengths)):
        _write_wav(wav_dir / name, 0.5 * synth_wave(40 + i, n))
    texts = ["hello there", "a longer sentence with more words", "too short to pad", "yes no"]
    pd.DataFrame({"FileName": names, "transcription": texts}).to_csv(tmp_path / "text.csv", index=False)
    pd.DataFrame({"FileName": names}).to_csv(tmp_path / "test.csv", index=False)

    def fake_tokenize(batch):
        ids = torch.full((len(batch), max_len), geo.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((len(batch), max_len), dtype=torch.int64)
        for i, t in enumerate(batch):
            toks = ([0] + [3 + (len(w) * 7 + j) % (geo.vocab_size - 4) for j, w in enumerate(t.split())])[: max_len - 1] + [2]
            ids[i, : len(toks)] = torch.tensor(toks)
            mask[i, : len(toks)] = 1
        return ids, mask

    sd = seeded_head_weights(R3.head_shapes(320, 128, 256, h=64), 31)
    cfgs = []
    for tag in ("files", "wav"):
        cfg = {"wav_dir": str(wav_dir), "txt_dir": str(tmp_path / "text.csv"), "lazy_dir3": str(lazy3), "feat1_dim": 320, "feat2_dim": 128,
               "feat3_dim": 256, "model_path": str(tmp_path / f"exp_{tag}")}
        os.makedirs(cfg["model_path"])
        torch.save(sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
        cfgs.append(cfg)
    C._REGISTRY["tiny-hubert-prosody"], C._REGISTRY["tiny-roberta-prosody"] = C.TINY_HUBERT, geo
    common = dict(test_csv=str(tmp_path / "test.csv"), mode="f16x", text_mode="f16x", head_mode="f16x", batch_size=2, max_len=max_len,
                  synthetic_weights=True, tokenize=fake_tokenize)               # batches [0, 1], [2, 3]: file 3 runs alone on both routes
    try:
        assert P.run(["--wav_dir", str(wav_dir), "--save_path", str(lazy3), "--synthetic_weights", "--mode", "f16x"]) == 0
        assert sorted(os.listdir(lazy3)) == [n.replace(".wav", ".pt") for n in names if n != names[2]]
        assert tuple(torch.load(lazy3 / "MSP-PODCAST_0001.pt", weights_only=True).shape) == (65, 256)
        capsys.readouterr()
        a = score_from_wav(cfgs[0], ["tiny-hubert-prosody", "tiny-roberta-prosody", "files"], **common)
        log_a = capsys.readouterr().out
        b = score_from_wav(cfgs[1], ["tiny-hubert-prosody", "tiny-roberta-prosody", P.NS3_PROSODY], **common)
        log_b = capsys.readouterr().out
        with pytest.raises(ValueError, match="feat3_dim = 128 in the config, but ns3-prosody has hidden size 256"):
            score_from_wav(dict(cfgs[1], feat3_dim=128), ["tiny-hubert-prosody", "tiny-roberta-prosody", P.NS3_PROSODY], **common)
    finally:
        C._REGISTRY.pop("tiny-hubert-prosody")
        C._REGISTRY.pop("tiny-roberta-prosody")
    for res, log in ((a, log_a), (b, log_b)):
        assert res["n"] == 3 and res["failed"] == 1, log
        assert log.count("Failed to process") == 1 and "Failed to process MSP-PODCAST_0002.wav" in log, log
    assert "Stream 3: ns3-prosody (synthetic weights (seed 7); numerics mode f16x)" in log_b
    with open(a["csv"], "rb") as f:
        by_files = f.read()
    with open(b["csv"], "rb") as f:
        from_wav = f.read()
    assert from_wav == by_files
    assert [ln.split(",")[0] for ln in from_wav.decode().splitlines()[1:]] == [names[0], names[1], names[3]]
