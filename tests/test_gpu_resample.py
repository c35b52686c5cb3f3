"""-m gpu: ser_resample_v (the Kaiser polyphase resampler, ABI 18) through ctypes against the float64 statement of tests/resample_ref.py,
engine.upload_resampled against the host filter for files on disk, and the drivers with --resample over a directory of mixed rates.

The gate of every sample: |got - ref| <= spacing_fp32(|ref|) + 1e-13 max|x| (resample_ref.within_one_ulp): one fp32 ulp plus 4 x the
float64 accumulation bound; no share of samples is exempt."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_kernel(items):
    """[(fp32 samples, rate)] -> [fp32 16 kHz samples]: one ser_resample_v launch over the ragged, mixed-rate batch."""
    from interspeech_ser_amd import _lib
    B = len(items)
    ratios = [R.ratio(sr) for _, sr in items]
    n_in = [len(x) for x, _ in items]
    n_out = [R.out_len(len(x), sr) for x, sr in items]
    banks, bank_off, halves = [np.zeros(1)], [], []                          # element 0: what a 16 kHz member points at (never read)
    where = {}
    for (x, sr), (up, down) in zip(items, ratios):
        if up == down == 1:
            bank_off.append(0)
            halves.append(0)
            continue
        if sr not in where:
            h, half = R.bank(sr)
            where[sr] = (sum(len(b) for b in banks), half)
            banks.append(h)
        bank_off.append(where[sr][0])
        halves.append(where[sr][1])

    def dev(a, dt):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(DEV)

    wav = dev(np.concatenate([x for x, _ in items]), np.float32)
    in_offs, out_offs = dev(np.concatenate([[0], np.cumsum(n_in)]), np.int64), dev(np.concatenate([[0], np.cumsum(n_out)]), np.int64)
    ups, downs, halves_d = dev([u for u, _ in ratios], np.int32), dev([d for _, d in ratios], np.int32), dev(halves, np.int32)
    boff, bank = dev(bank_off, np.int64), dev(np.concatenate(banks), np.float64)
    out = torch.full((sum(n_out) + 64,), float("nan"), dtype=torch.float32, device=DEV)      # the tail must stay untouched
    a = _lib.ResampleArgs()
    a.wav, a.in_offs, a.out_offs, a.up, a.down, a.half = wav.data_ptr(), in_offs.data_ptr(), out_offs.data_ptr(), ups.data_ptr(), downs.data_ptr(), halves_d.data_ptr()
    a.bank_off, a.bank, a.out = boff.data_ptr(), bank.data_ptr(), out.data_ptr()
    a.total_in, a.total_out, a.max_out, a.B = sum(n_in), sum(n_out), max(n_out), B
    _lib.check(_lib.lib.ser_resample_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "ser_resample_v")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.isnan(host[sum(n_out):]).all(), "ser_resample_v wrote beyond the packed output"
    offs = np.concatenate([[0], np.cumsum(n_out)])
    return [host[offs[b]: offs[b + 1]].copy() for b in range(B)]


def tile_lengths(sr):
    """Input lengths whose output is the longest one short of a tile boundary and the shortest one past it."""
    from interspeech_ser_amd._lib import RESAMPLE_TILE
    n = 1
    while R.out_len(n + 1, sr) < RESAMPLE_TILE:
        n += 1
    short = n
    while R.out_len(n, sr) <= RESAMPLE_TILE:
        n += 1
    assert R.out_len(short, sr) < RESAMPLE_TILE < R.out_len(n, sr)
    return short, n


def signals(sr, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    imp0, imp1 = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    imp0[0], imp1[-1] = 1.0, 1.0
    return {"noise": rng.standard_normal(n).astype(np.float32),
            "sine": np.sin(2 * np.pi * 0.45 * min(sr, 16000) * t).astype(np.float32),          # full scale, just below the new Nyquist
            "impulse@0": imp0, "impulse@last": imp1}


@pytest.mark.parametrize("sr", R.RATES)
def test_kernel_equals_the_float64_statement_to_one_ulp(sr):
    short, past = tile_lengths(sr)
    items, names = [], []
    for n in (1, 2, short, past, 10 * sr):
        for name, x in signals(sr, n, 1000 + n % 97).items():
            items.append((x, sr))
            names.append(f"{name} n={n}")
    got = run_kernel(items)
    worst = -1.0
    for (x, _), name, y in zip(items, names, got):
        ref = R.resample(x, sr)
        assert len(y) == len(ref) == R.out_len(len(x), sr), name
        excess = R.within_one_ulp(y, ref, float(np.abs(x).max()))
        err = float(np.abs(y.astype(np.float64) - ref).max())
        print(f"{sr} Hz {name}: {len(ref)} samples, max |got - ref| {err:.3e}, excess over the bound {excess:.3e}")
        worst = max(worst, excess)
        assert excess <= 0.0, (sr, name, excess)


def test_mixed_rate_batch_equals_its_utterances_one_by_one():
    rng = np.random.default_rng(5)
    items = [(rng.standard_normal(n).astype(np.float32), sr)
             for n, sr in ((16000, 16000), (44100 + 37, 44100), (3 * 48000 - 5, 48000), (9001, 8000), (777, 16000), (2 * 44100, 44100), (1500, 48000))]
    batch = run_kernel(items)
    for (x, sr), y in zip(items, batch):
        alone = run_kernel([(x, sr)])[0]
        assert len(y) == R.out_len(len(x), sr)
        assert np.array_equal(y.view(np.uint32), alone.view(np.uint32)), sr                  # bit for bit
        if sr == 16000:
            assert np.array_equal(y.view(np.uint32), x.view(np.uint32))                      # a copy


def _write(path, x, sr, kind):
    """mono fp32 x in [-1, 1] -> a file of the given kind; stereo writes (x, 0.5 x)."""
    if kind == "float":
        from scipy.io import wavfile
        wavfile.write(str(path), sr, x.astype(np.float32))
        return
    ch = 2 if kind == "stereo" else 1
    if ch == 2:
        x = np.stack([x, 0.5 * x], axis=1).reshape(-1)
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(ch)
        wf.setframerate(sr)
        if kind == "pcm24":
            v = (np.clip(x, -1, 1) * 8388607).astype(np.int32)
            wf.setsampwidth(3)
            wf.writeframes(b"".join(int(s).to_bytes(3, "little", signed=True) for s in v))
        else:
            wf.setsampwidth(2)
            wf.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _synth(seed, n, sr):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(sr)
    return 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220 * t)


@pytest.mark.parametrize("family", ["speech", "whisper"])
def test_upload_resampled_equals_the_host_filter_for_files_on_disk(tmp_path, family):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import build_encoder
    from interspeech_ser_amd.frontend import decode_wav, load_wav_16k, resampled_len
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = C.TINY_WAVLM if family == "speech" else C.TINY_WHISPER
    enc = build_encoder(geo, synthetic_state_dict(geo, 3), DEV, "fp32x")
    files = [("a.wav", 44100, "pcm16", 30011), ("b.wav", 48000, "pcm24", 20000), ("c.wav", 22050, "float", 12345),
             ("d.wav", 32000, "stereo", 18000), ("e.wav", 16000, "pcm16", 9000)]
    for name, sr, kind, n in files:
        _write(tmp_path / name, _synth(len(name) + n, n, sr), sr, kind)
    for pinned in (False, True):
        decoded = [decode_wav(str(tmp_path / name), pinned) for name, *_ in files]
        assert [sr for _, sr in decoded] == [sr for _, sr, _, _ in files]
        dev, lengths = enc.upload_resampled([x for x, _ in decoded], [sr for _, sr in decoded])
        torch.cuda.synchronize()
        assert lengths == [resampled_len(len(x), sr) for x, sr in decoded] and dev.numel() == sum(lengths)
        got = dev.cpu().numpy()
        o = 0
        for (name, sr, kind, n), (x, _), L in zip(files, decoded, lengths):
            host = load_wav_16k(str(tmp_path / name), resample=True)
            assert len(host) == L, name
            y = got[o: o + L]
            o += L
            if sr == 16000:
                assert np.array_equal(y, host)
                continue
            excess = R.within_one_ulp(y, host, float(np.abs(x).max()))
            print(f"{family} {name} ({kind}, {sr} Hz, pinned={pinned}): max |gpu - host| {float(np.abs(y.astype(np.float64) - host).max()):.3e}, excess {excess:.3e}")
            assert excess <= 0.0, (name, excess)
    # a batch at 16 kHz alone is the plain upload
    x16 = decoded[-1][0]
    dev, lengths = enc.upload_resampled([x16, x16[:5000]], [16000, 16000])
    torch.cuda.synchronize()
    assert lengths == [9000, 5000] and np.array_equal(dev.cpu().numpy(), np.concatenate([x16, x16[:5000]]))
    hs = enc.forward(*enc.upload_resampled([x for x, _ in decoded], [sr for _, sr in decoded]))   # what forward takes
    torch.cuda.synchronize()
    assert hs.batch == len(files)


MIXED = [("a16.wav", 16000, 16000), ("b44.wav", 44100, 30011), ("c48.wav", 48000, 52000), ("d16.wav", 16000, 9000), ("e44.wav", 44100, 61111)]


def _mixed_dir(tmp_path):
    wav_dir = tmp_path / "wav"
    wav_dir.mkdir()
    for i, (name, sr, n) in enumerate(MIXED):
        _write(wav_dir / name, _synth(80 + i, n, sr), sr, "pcm16")
    return wav_dir


def test_speech_driver_resamples_on_the_gpu(tmp_path, capsys):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.frontend import decode_wav, load_wav_16k, resampled_len
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle import ssl_oracle as O
    geo = C.TINY_WAVLM
    wav_dir = _mixed_dir(tmp_path)
    _write(wav_dir / "f44_tiny.wav", _synth(99, 700, 44100), 44100, "pcm16")      # 254 samples at 16 kHz: below the receptive field;
    out, out_plain = tmp_path / "pt", tmp_path / "pt_plain"                       # its batch is retried file by file
    C._REGISTRY["tiny-resample-test"] = geo
    try:
        common = ["--ssl_type", "tiny-resample-test", "--wav_dir", str(wav_dir), "--synthetic_weights", "--use_n_layer", "--n_layer", "-1",
                  "--batch_size", "2", "--timing"]
        assert driver.run_speech(common + ["--save_path", str(out), "--resample"]) == 0
        log = capsys.readouterr().out
        assert log.count("Failed to process") == 1 and "f44_tiny.wav" in log and "receptive field" in log, log
        assert "upload_resample" in log                                           # --timing names the step
        assert sorted(os.listdir(out)) == [n.replace(".wav", ".pt") for n, _, _ in MIXED]
        assert driver.run_speech(common + ["--save_path", str(out_plain)]) == 0
        log = capsys.readouterr().out
    finally:
        C._REGISTRY.pop("tiny-resample-test")
    sd = synthetic_state_dict(geo, 7)                                             # --seed default
    for name, sr, n in MIXED:
        raw, got_sr = decode_wav(str(wav_dir / name))
        assert got_sr == sr and len(raw) == n
        host = load_wav_16k(str(wav_dir / name), resample=True)                   # the HOST-resampled wave
        assert len(host) == resampled_len(n, sr)
        got = torch.load(out / name.replace(".wav", ".pt"))
        assert tuple(got.shape) == (geo.frames_for(resampled_len(n, sr)), geo.hidden), name
        with torch.no_grad():
            ref = O.speech_hidden_states(geo, sd, torch.from_numpy(O.zero_mean_unit_var(host)))[-1]
        err = float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))
        print(f"speech driver {name}: rel err vs the oracle on the host-resampled wave {err:.2e}")
        assert err < 1e-3, (name, err)
        # without --resample: exactly the non-16 kHz files fail, the others are written as before
        plain = out_plain / name.replace(".wav", ".pt")
        if sr == 16000:
            assert torch.equal(torch.load(plain), got), name
        else:
            assert not plain.exists() and f"Failed to process {wav_dir / name}" in log and f"sample rate {sr} Hz" in log
    assert log.count("Failed to process") == 4 and sorted(os.listdir(out_plain)) == ["a16.pt", "d16.pt"]      # + the tiny file, refused for its rate


def test_whisper_driver_resamples_on_the_gpu(tmp_path, capsys):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.frontend import load_wav_16k, resampled_len, whisper_saved_rows
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle import ssl_oracle as O
    geo = C.TINY_WHISPER
    wav_dir = _mixed_dir(tmp_path)
    out, out_plain = tmp_path / "pt", tmp_path / "pt_plain"
    C._REGISTRY["tiny-whisper-resample-test"] = geo
    try:
        common = ["--ssl_type", "tiny-whisper-resample-test", "--wav_dir", str(wav_dir), "--synthetic_weights", "--mode", "fp32x",
                  "--n_layer", "-1", "--batch_size", "2"]
        assert driver.run_whisper(common + ["--save_path", str(out), "--resample"]) == 0
        log = capsys.readouterr().out
        assert "Failed to process" not in log, log
        assert driver.run_whisper(common + ["--save_path", str(out_plain)]) == 0
        log = capsys.readouterr().out
    finally:
        C._REGISTRY.pop("tiny-whisper-resample-test")
    sd = synthetic_state_dict(geo, 7)
    seen_uncapped = False
    for name, sr, n in MIXED:
        host = load_wav_16k(str(wav_dir / name), resample=True)
        rows = whisper_saved_rows(resampled_len(n, sr), geo.hidden)               # the saved-row rule on the 16 kHz length
        seen_uncapped |= rows < geo.hidden and sr != 16000
        got = torch.load(out / name.replace(".wav", ".pt"))
        assert tuple(got.shape) == (rows, geo.hidden), name
        with torch.no_grad():
            ref = O.whisper_hidden_states(geo, sd, torch.from_numpy(O.whisper_log_mel(host, geo.n_mels)))[-1]
        err = float((got - ref[:rows]).abs().max() / max(1.0, float(ref.abs().max())))
        print(f"whisper driver {name}: rel err vs the oracle on the host-resampled wave {err:.2e}")
        assert err < 1e-3, (name, err)
        plain = out_plain / name.replace(".wav", ".pt")
        if sr == 16000:
            assert torch.equal(torch.load(plain), got), name
        else:
            assert not plain.exists() and f"sample rate {sr} Hz" in log
    assert seen_uncapped                                                          # the row count depended on the resampled length somewhere
    assert log.count("Failed to process") == 3 and sorted(os.listdir(out_plain)) == ["a16.pt", "d16.pt"]
