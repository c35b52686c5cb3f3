"""GPU: attentive statistics pooling + head (csrc/pool.hip, engine.PoolHead, baseline.py) against the float64 statement in
tests/asp_ref.py.  Every bound is computed from the inputs: a multiple of the error of the reference's own fp32 arithmetic
(torch CPU fp32 in pooling.py's / ser.py's order, restated here) and, where a GEMM operand format is involved, of the error that
rounding the operands to that format causes.  Each test prints its measured error next to its bound (lines starting POOLHEAD)."""
import csv
import ctypes
import json
import os
import pickle
import wave as _wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import asp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RAGGED = ((1, 2, 70, 333), (5, 130))


def _offs(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _report(what, err, bound):
    print(f"POOLHEAD {what}: error {err:.3e}  bound {bound:.3e}")


# ------------------------------------------------------------------------------- the reference's arithmetic, fp32 on the CPU
def ref32_pool(x, offs, a, hlin=None, W=None, b=None):
    """The reference's arithmetic order in torch fp32 on [T, D] tensors, one utterance at a time: tanh of the linear map, its dot
    with a, softmax over the frames, the weighted first and second moments, m2 - mu^2, the clamp at 1e-5, the root."""
    f32 = torch.float32
    x = torch.as_tensor(x, dtype=f32)
    a = torch.as_tensor(a, dtype=f32).reshape(-1)
    out = torch.empty((len(offs) - 1, 2 * x.shape[1]), dtype=f32)
    for i, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        frames = x[lo:hi]                                              # [T, D]
        if hlin is not None:
            lin = torch.as_tensor(hlin[lo:hi], dtype=f32)
        else:
            lin = frames @ torch.as_tensor(W, dtype=f32).T + torch.as_tensor(b, dtype=f32)
        weight = torch.softmax(torch.tanh(lin) @ a, dim=0)[:, None]    # [T, 1]
        mu = (frames * weight).sum(dim=0)
        m2 = (frames * frames * weight).sum(dim=0)
        out[i, : x.shape[1]] = mu
        out[i, x.shape[1]:] = (m2 - mu * mu).clamp_min(1e-5).sqrt()
    return out.numpy()


def ref32_head(p, sd):
    t = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in sd.items()}
    h = F.linear(torch.as_tensor(p, dtype=torch.float32), t["fc.0.0.weight"], t["fc.0.0.bias"])
    h = F.relu(F.layer_norm(h, (h.shape[1],), t["fc.0.1.weight"], t["fc.0.1.bias"], 1e-5))
    return F.linear(h, t["out.0.weight"], t["out.0.bias"]).numpy()


# ------------------------------------------------------------------------------- kernel launches
def _dev_rows(v, ld=None):
    """fp32 rows on the device at row pitch ``ld`` (default: contiguous); the padding columns hold NaN"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if ld is None or v.ndim < 2:
        return torch.from_numpy(v).to(DEV)
    t = torch.full((v.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    t[:, : v.shape[1]] = torch.from_numpy(v).to(DEV)
    return t


def gpu_asp_pool(x, hlin, a, lengths, ldx=None, ldh=None):
    from interspeech_ser_amd import _lib
    offs = _offs(lengths)
    rows, D, B = offs[-1], x.shape[1], len(lengths)
    xd, hd, ad = _dev_rows(x, ldx), _dev_rows(hlin, ldh), _dev_rows(a.reshape(-1))
    od = torch.tensor(offs, dtype=torch.int32, device=DEV)
    scores = torch.empty(rows, dtype=torch.float32, device=DEV)
    out = torch.full((B, 2 * D), float("nan"), dtype=torch.float32, device=DEV)
    p = _lib.AspPoolArgs()
    p.x, p.ldx, p.hlin, p.ldh, p.a = xd.data_ptr(), ldx or D, hd.data_ptr(), ldh or D, ad.data_ptr()
    p.frame_offs, p.scores, p.out, p.ldo = od.data_ptr(), scores.data_ptr(), out.data_ptr(), 2 * D
    p.B, p.D, p.rows, p.max_frames = B, D, rows, max(lengths)
    _lib.check(_lib.lib.ser_asp_pool_v(ctypes.byref(p), torch.cuda.current_stream().cuda_stream), "ser_asp_pool_v")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def gpu_mlp_head(p, sd, ldp=None):
    from interspeech_ser_amd import _lib
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV) for k, v in sd.items()}
    pd = _dev_rows(p, ldp)
    B, K = p.shape
    H, n_out = t["fc.0.0.weight"].shape[0], t["out.0.weight"].shape[0]
    hidden = torch.empty((B, H), dtype=torch.float32, device=DEV)
    out = torch.full((B, n_out), float("nan"), dtype=torch.float32, device=DEV)
    h = _lib.MlpHeadArgs()
    h.p, h.ldp, h.W1, h.b1 = pd.data_ptr(), ldp or K, t["fc.0.0.weight"].data_ptr(), t["fc.0.0.bias"].data_ptr()
    h.gamma, h.beta, h.W2, h.b2 = t["fc.0.1.weight"].data_ptr(), t["fc.0.1.bias"].data_ptr(), t["out.0.weight"].data_ptr(), t["out.0.bias"].data_ptr()
    h.hidden, h.out, h.eps, h.B, h.K, h.H, h.n_out = hidden.data_ptr(), out.data_ptr(), 1e-5, B, K, H, n_out
    _lib.check(_lib.lib.ser_mlp_head_v(ctypes.byref(h), torch.cuda.current_stream().cuda_stream), "ser_mlp_head_v")
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------- ser_asp_pool_v alone
def _pool_inputs(D, lengths, case):
    rng = np.random.default_rng(1000 * D + sum(lengths) + len(case))
    rows = sum(lengths)
    x = rng.standard_normal((rows, D)).astype(np.float32)
    if case == "mean30":
        x = (30.0 + 0.1 * rng.standard_normal((rows, D))).astype(np.float32)
    if case == "constcol":
        x[:, 5] = np.float32(1.7)
    W = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    b = (0.1 * rng.standard_normal(D)).astype(np.float32)
    a = rng.standard_normal(D).astype(np.float32) * (8.0 if case == "a8" else 1.0)
    if case == "mean30":
        W = W - W.mean(axis=1, keepdims=True)              # keep x W^T inside tanh's live range for the offset rows
    hlin = (x.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)).astype(np.float32)      # float64, rounded once
    return x, hlin, a.astype(np.float32)


@pytest.mark.parametrize("case", ["plain", "a8", "mean30", "constcol"])
@pytest.mark.parametrize("lengths", RAGGED, ids=["1-2-70-333", "5-130"])
@pytest.mark.parametrize("D", [64, 192])
def test_asp_pool_kernel(built_library, D, lengths, case):
    _check_asp_pool(D, lengths, case)


# D = 1024 (WavLM-large): four 256-column steps per lane in the scores kernel, 16 slabs; D = 68: a last slab with one live column quad
@pytest.mark.parametrize("D", [1024, 68])
def test_asp_pool_kernel_wide_and_partial_slab(built_library, D):
    _check_asp_pool(D, RAGGED[0], "plain")


def _check_asp_pool(D, lengths, case):
    x, hlin, a = _pool_inputs(D, lengths, case)
    offs = _offs(lengths)
    ref = R.asp_pool_from_scores(x, R.asp_scores(hlin, a), offs)
    scale = max(1.0, float(np.abs(ref).max()))
    e_ref32 = R.rel_err(ref32_pool(x, offs, a, hlin=hlin), ref)
    # two-ulp tanhf errors per element move a score by <= 2^-22 ||a||_1 and through it the weights, hence mu by that times max|x|
    bound = max(4.0 * e_ref32, 2.0 ** -22 * float(np.abs(a).sum()) * float(np.abs(x).max()) / scale)
    got = gpu_asp_pool(x, hlin, a, lengths)
    err = R.rel_err(got, ref)
    _report(f"asp_pool D={D} lengths={lengths} {case} (e_ref32 {e_ref32:.2e})", err, bound)
    assert np.isfinite(got).all()
    assert err <= bound
    if case == "a8":
        assert R.asp_scores(hlin, a).max() > 89.0, "the scores should exceed what expf takes without the max subtraction"
    if case == "constcol":
        want = np.sqrt(np.float32(1e-5))
        assert np.all(np.abs(got[:, D + 5].view(np.int32) - want.view(np.int32)) <= 1)
    if lengths[0] == 1:                                       # one frame: mu = x, rh = sqrt(1e-5f)
        assert np.array_equal(got[0, :D], x[0])
        assert np.all(np.abs(got[0, D:].view(np.int32) - np.sqrt(np.float32(1e-5)).view(np.int32)) <= 1)
    for i, n in enumerate(lengths):                           # batch of one: bit-equal to its batched row
        one = gpu_asp_pool(x[offs[i]: offs[i + 1]], hlin[offs[i]: offs[i + 1]], a, (n,))
        assert np.array_equal(one[0].view(np.uint32), got[i].view(np.uint32)), (i, n)


def test_asp_pool_padded_rows_are_bit_equal(built_library):
    """row pitches beyond D (ldx = D + 4, ldh = D + 8): the same bits as contiguous rows.  D = 68: a last slab with one live quad; 17
    frames: two frames in row group 0; one frame: mu = x"""
    D, lengths = 68, (1, 17)
    x, hlin, a = _pool_inputs(D, lengths, "plain")
    flat = gpu_asp_pool(x, hlin, a, lengths)
    padded = gpu_asp_pool(x, hlin, a, lengths, ldx=D + 4, ldh=D + 8)
    assert np.isfinite(flat).all() and np.array_equal(flat[0, :D], x[0])
    assert np.array_equal(padded.view(np.uint32), flat.view(np.uint32))


# ------------------------------------------------------------------------------- ser_mlp_head_v alone
@pytest.mark.parametrize("n_out", [8, 3])
@pytest.mark.parametrize("K,H", [(128, 96), (384, 64)])
def test_mlp_head_kernel(built_library, K, H, n_out):
    _check_mlp_head(K, H, n_out)


# the register-resident W1 row has one instantiation per K range: 1024 -> 4 chunks a lane, 2048 (WavLM-large, H = 1024) -> 8, 4096 -> 16
@pytest.mark.parametrize("K,H", [(1024, 96), (2048, 1024), (4096, 64)])
def test_mlp_head_kernel_wide(built_library, K, H):
    _check_mlp_head(K, H, 8)


def _check_mlp_head(K, H, n_out):
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    _, sd = synthetic_head_state_dicts(K // 2, H, n_out, seed=K + n_out)
    sd = {k: v.numpy() for k, v in sd.items()}
    rng = np.random.default_rng(K * H + n_out)
    p = rng.standard_normal((5, K)).astype(np.float32)
    ref = R.mlp_head(p, sd)
    e_ref32 = R.rel_err(ref32_head(p, sd), ref)
    got = gpu_mlp_head(p, sd)
    err = R.rel_err(got, ref)
    _report(f"mlp_head K={K} H={H} n_out={n_out}", err, 4.0 * e_ref32)
    assert err <= 4.0 * e_ref32
    for i in range(p.shape[0]):
        assert np.array_equal(gpu_mlp_head(p[i: i + 1], sd)[0].view(np.uint32), got[i].view(np.uint32))


def test_mlp_head_padded_rows_are_bit_equal(built_library):
    """input pitch beyond K (ldp = K + 8): the same bits as contiguous rows.  K = 384: two chunks a lane, the second partly dead"""
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    K, H, n_out = 384, 64, 3
    _, sd = synthetic_head_state_dicts(K // 2, H, n_out, seed=K + n_out)
    sd = {k: v.numpy() for k, v in sd.items()}
    p = np.random.default_rng(K * H + n_out).standard_normal((3, K)).astype(np.float32)
    flat = gpu_mlp_head(p, sd)
    assert np.isfinite(flat).all()
    assert np.array_equal(gpu_mlp_head(p, sd, ldp=K + 8).view(np.uint32), flat.view(np.uint32))


# ------------------------------------------------------------------------------- PoolHead behind an encoder
def _round_planes(t, mode):
    """the mode's GEMM operand planes on the CPU: hi = cast, lo = cast of the remainder (oracle/numerics_whatif.py)"""
    t = torch.as_tensor(t, dtype=torch.float32)
    if mode == "bf16":
        return t.bfloat16().double()
    dt = torch.bfloat16 if mode == "fp32x" else torch.float16
    hi = t.to(dt)
    lo = (t - hi.float()).to(dt)
    return hi.double() + lo.double()


def _waves(seed=0):
    rng = np.random.default_rng(seed)
    return [(0.5 * rng.standard_normal(n)).astype(np.float32) for n in (16000, 23457)]


@pytest.mark.parametrize("n_out", [8, 3])
@pytest.mark.parametrize("geo_name,mode", [("TINY_WAVLM", "f16mf"), ("TINY_WAVLM", "f16x"), ("TINY_WAVLM", "fp32x"), ("TINY_WAVLM", "bf16"),
                                           ("TINY_WAVLM_BASE", "f16x"), ("TINY_WAVLM_BASE", "fp32x"), ("TINY_WAVLM_BASE", "bf16")])
def test_pool_head_on_encoder_output(built_library, geo_name, mode, n_out):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    from interspeech_ser_amd.engine import PoolHead, SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, geo_name)
    D = geo.hidden
    enc = SpeechEncoder(geo, synthetic_state_dict(geo, 11), DEV, mode=mode, normalize=False)
    pool_sd, ser_sd = synthetic_head_state_dicts(D, 96, n_out, seed=5)
    head = PoolHead(enc, pool_sd, ser_sd)
    waves = _waves()
    lengths = [len(w) for w in waves]
    hs0 = enc.forward(enc.upload(waves), lengths)
    torch.cuda.synchronize()
    plain = hs0.states.clone()                                # a forward without a head
    hs = enc.forward(enc.upload(waves), lengths)
    got = head.forward(hs).cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(hs.states, plain), "the head must leave the hidden states as the forward wrote them"
    assert hs.take_range_bits() == 0
    x = hs.states[-1].cpu().numpy()
    offs = hs.frame_offs
    pool_np = {k: v.numpy() for k, v in pool_sd.items()}
    ser_np = {k: v.numpy() for k, v in ser_sd.items()}
    ref = R.logits(x, offs, pool_np, ser_np)
    e_ref32 = R.rel_err(ref32_head(ref32_pool(x, offs, pool_np["attention"], W=pool_np["sap_linear.weight"], b=pool_np["sap_linear.bias"]), ser_np), ref)
    op = mode if mode in ("bf16", "fp32x") else "f16x"
    hl = (_round_planes(x, op) @ _round_planes(pool_np["sap_linear.weight"], op).T).numpy() + pool_np["sap_linear.bias"].astype(np.float64)
    e_emul = R.rel_err(R.mlp_head(R.asp_pool(x, offs, pool_np, hlin=hl), ser_np), ref)
    bound = 4.0 * max(e_ref32, e_emul)
    err = R.rel_err(got, ref)
    _report(f"PoolHead {geo_name} {mode} n_out={n_out} (e_ref32 {e_ref32:.2e}, e_emul {e_emul:.2e})", err, bound)
    assert got.shape == (2, n_out) and err <= bound
    for i, w in enumerate(waves):                             # batch of one: bit-equal logits
        hs1 = enc.forward(enc.upload([w]), [len(w)])
        one = head.forward(hs1).cpu().numpy()
        assert np.array_equal(one[0].view(np.uint32), got[i].view(np.uint32)), i
        if i == 0:
            first = head.forward(hs1, slot=1).cpu().numpy()   # a slot of the head that meets the smaller batch first ...
            assert np.array_equal(first.view(np.uint32), one.view(np.uint32))
    grown = head.forward(enc.forward(enc.upload(waves), lengths), slot=1).cpu().numpy()    # ... and grows for the ragged one
    assert np.array_equal(grown.view(np.uint32), got.view(np.uint32))


def test_pool_head_refuses_what_it_cannot_run(built_library):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    from interspeech_ser_amd.engine import PoolHead, WhisperEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    enc = WhisperEncoder(C.TINY_WHISPER, synthetic_state_dict(C.TINY_WHISPER, 1), DEV, mode="bf16")
    with pytest.raises(ValueError, match="speech encoders"):
        PoolHead(enc, *synthetic_head_state_dicts(128, 96, 8))


# ------------------------------------------------------------------------------- the drivers on files
def _write_wav(path, x):
    with _wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())


def synth_file(rng, i, t):
    tone, noise = ((0.2, 0.1), (0.02, 0.3), (0.6, 0.01), (0.0, 0.05), (0.2, 0.1))[i]
    return tone * np.sin(2 * np.pi * rng.uniform(90, 400) * t) + noise * rng.standard_normal(len(t))


SSL_NAME = "tiny-wavlm-baseline-test"
FILES = {"u1_test3.wav": 16000, "u0_test3.wav": 23457, "long_test3.wav": 13 * 16000, "u2_test3.wav": 9000, "other_dev.wav": 12000}
WAV_MEAN, WAV_STD = np.float64(0.0123), np.float64(0.21)
SEED = 7


@pytest.fixture(scope="module")
def model_dir(tmp_path_factory, built_library):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = C.TINY_WAVLM
    root = tmp_path_factory.mktemp("baseline")
    wav_dir = root / "Audios"
    wav_dir.mkdir()
    rng = np.random.default_rng(17)
    for i, (name, n) in enumerate(FILES.items()):             # tones and noise at different levels, so the files differ in class
        t = np.arange(n) / 16000.0
        _write_wav(wav_dir / name, synth_file(rng, i, t))
    cfg = root / "config.json"
    cfg.write_text(json.dumps({"wav_dir": str(wav_dir), "label_path": "unused.csv"}))
    sd = synthetic_state_dict(geo, SEED)
    heads = {}
    for kind, n_out in (("cat", 8), ("dim", 3)):
        d = root / kind
        d.mkdir()
        pool_sd, ser_sd = synthetic_head_state_dicts(geo.hidden, 96, n_out, seed=SEED)
        torch.save(sd, str(d / "final_ssl.pt"))
        torch.save(pool_sd, str(d / "final_pool.pt"))
        torch.save(ser_sd, str(d / "final_ser.pt"))
        with open(d / "train_norm_stat.pkl", "wb") as f:
            pickle.dump((WAV_MEAN, WAV_STD), f)
        heads[kind] = (pool_sd, ser_sd)
    C._REGISTRY[SSL_NAME] = geo
    yield dict(root=root, wav_dir=wav_dir, cfg=str(cfg), sd=sd, heads=heads, geo=geo)
    C._REGISTRY.pop(SSL_NAME)


def _raw(path):
    from interspeech_ser_amd.frontend import decode_wav
    return decode_wav(str(path))[0]


@pytest.mark.parametrize("kind", ["cat", "dim"])
def test_driver_on_files(model_dir, kind, capsys):
    from interspeech_ser_amd import baseline as BL
    from oracle import ssl_oracle as O
    m = model_dir
    mdir = str(m["root"] / kind)
    fn = BL.run_eval_cat if kind == "cat" else BL.run_eval_dim
    assert fn(["--ssl_type", SSL_NAME, "--model_path", mdir, "--config_path", m["cfg"], "--head_dim", "96", "--batch_size", "3"]) == 0
    log = capsys.readouterr().out
    assert "4 rows written" in log and "0 files failed" in log, log
    with open(os.path.join(mdir, "results", "test3.csv"), newline="") as f:
        rows = list(csv.reader(f))
    names = sorted(n for n in FILES if "test3" in n)
    assert [r[0] for r in rows[1:]] == names
    pool_sd, ser_sd = m["heads"][kind]
    pred = BL.BaselinePredictor(m["geo"], m["sd"], pool_sd, ser_sd, WAV_MEAN, WAV_STD, DEV, "f16mf")
    pool_np, ser_np = {k: v.numpy() for k, v in pool_sd.items()}, {k: v.numpy() for k, v in ser_sd.items()}
    for row in rows[1:]:
        raw = _raw(m["wav_dir"] / row[0])
        alone = BL.predict(pred, [raw])[0]                    # the file alone: batch independence makes this an equality
        _, want = BL.format_rows(kind, [row[0]], alone[None])
        assert row == [str(v) for v in want[0]], (row, want)
        if kind == "cat":                                     # ... and the CPU chain picks the same class
            x = np.ascontiguousarray(BL.scale_wave(BL.cut_wave(raw), WAV_MEAN, WAV_STD))
            assert len(x) == min(len(raw), 192000)
            last = O.speech_hidden_states(m["geo"], m["sd"], torch.from_numpy(x))[-1].numpy()
            lg = R.logits(last, [0, last.shape[0]], pool_np, ser_np)[0]
            top = np.sort(lg)[::-1]
            gap = (top[0] - top[1]) / np.abs(lg).max()
            print(f"POOLHEAD driver {row[0]}: oracle top-two gap {gap:.3e} of max|logit| (must exceed 1e-2); "
                  f"logits vs oracle chain {R.rel_err(alone, lg):.3e}")
            assert gap > 1e-2, "choose another seed: the oracle's top two logits are too close on this file"
            assert row[1] == BL.CAT_LETTERS[int(np.argmax(lg))]


def test_driver_fails_files_through_the_range_guard(model_dir, capsys):
    """encoder.layer_norm.bias carries a 1e6 outlier: the last hidden state exceeds fp16's range, the head's operand copy reports it
    into the slot's guard word, and in f16x every file fails (batch, then one by one) instead of getting a row; fp32x writes them."""
    from interspeech_ser_amd import baseline as BL
    m = model_dir
    d = m["root"] / "outlier"
    d.mkdir()
    sd = {k: v.clone() for k, v in m["sd"].items()}
    sd["encoder.layer_norm.bias"][3] = 1.0e6
    pool_sd, ser_sd = m["heads"]["cat"]
    torch.save(sd, str(d / "final_ssl.pt"))
    torch.save(pool_sd, str(d / "final_pool.pt"))
    torch.save(ser_sd, str(d / "final_ser.pt"))
    with open(d / "train_norm_stat.pkl", "wb") as f:
        pickle.dump((WAV_MEAN, WAV_STD), f)
    common = ["--ssl_type", SSL_NAME, "--model_path", str(d), "--config_path", m["cfg"], "--head_dim", "96", "--batch_size", "2"]
    assert BL.run_eval_cat(common + ["--mode", "f16x"]) == 0
    log = capsys.readouterr().out
    assert log.count("Failed to process") == 4 and "fp16 operand range" in log and "0 rows written" in log and "4 files failed" in log, log
    with open(d / "results" / "test3.csv", newline="") as f:
        assert list(csv.reader(f)) == [["FileName", "EmoClass"]]
    assert BL.run_eval_cat(common + ["--mode", "fp32x"]) == 0
    assert "4 rows written" in capsys.readouterr().out
