"""CPU: the host side of the GPU resampler (frontend.resample_ratio / resampled_len / polyphase_bank / decode_wav) and the validation of
ser_resample_v (ABI 18).  The float64 statement of the filter is tests/resample_ref.py; scipy's resample_poly is the yardstick here."""
import ctypes
import os
import wave

import numpy as np
import pytest

import resample_ref as R
from interspeech_ser_amd import frontend


@pytest.mark.parametrize("sr", R.RATES)
def test_polyphase_bank_equals_firwin(sr):
    """<= 1e-14 absolute against scipy.signal.firwin(2 half + 1, 1 / R, kaiser 14) * up: float64 rounding noise (3.4e-16 measured), eight
    orders below an fp32 ulp."""
    from scipy.signal import firwin
    up, down = frontend.resample_ratio(sr)
    assert (up, down) == R.ratio(sr)
    h, half = frontend.polyphase_bank(up, down)
    assert half == 10 * max(up, down) and h.dtype == np.float64 and h.shape == (2 * half + 1,)
    ref = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 14.0)) * up
    worst = float(np.abs(h - ref).max())
    print(f"bank {sr} Hz: max |h - firwin| {worst:.2e}; own statement {float(np.abs(R.bank(sr)[0] - ref).max()):.2e}")
    assert worst <= 1e-14
    assert float(np.abs(R.bank(sr)[0] - ref).max()) <= 1e-14
    assert frontend.polyphase_bank(up, down)[0] is h                         # cached


@pytest.mark.parametrize("sr", R.RATES)
def test_float64_statement_equals_resample_poly(sr):
    """Equal length and <= 1e-13 max|x| (1.8e-15 measured) against resample_poly for lengths 1, 2, half / up, 3 001 and a 10 s clip."""
    from scipy.signal import resample_poly
    up, down = R.ratio(sr)
    half = 10 * max(up, down)
    rng = np.random.default_rng(sr)
    for n in (1, 2, max(1, half // up), 3001, 160000 * sr // 16000):
        x = rng.standard_normal(n).astype(np.float32)
        ref = resample_poly(x.astype(np.float64), up, down, window=("kaiser", 14.0))
        got = R.resample(x, sr)
        assert len(got) == len(ref) == frontend.resampled_len(n, sr) == R.out_len(n, sr), (sr, n)
        worst = float(np.abs(got - ref).max())
        print(f"{sr} Hz n={n}: max |statement - resample_poly| {worst:.2e}")
        assert worst <= 1e-13 * float(np.abs(x).max()), (sr, n, worst)


def test_resampled_len_is_the_exact_ceiling():
    for sr in R.RATES + (16000, 44101, 7, 192000):
        for n in (0, 1, 2, 3, 159, 160, 161, 441, 44100, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1):
            want = -((-n * 16000) // sr)                                     # Python integers: exact
            assert frontend.resampled_len(n, sr) == want, (sr, n)
            assert isinstance(frontend.resampled_len(n, sr), int)
    assert frontend.resampled_len(12345, 16000) == 12345 and frontend.resample_ratio(16000) == (1, 1)
    assert frontend.resample_ratio(44100) == (160, 441) and frontend.resample_ratio(48000) == (1, 3)
    assert max(frontend.resample_ratio(44101)) > frontend.RESAMPLE_MAX_R      # the driver keeps such a rate on the host


def _write_pcm16(path, x, sr, ch=1):
    pcm = (np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(ch)
        wf.setsampwidth(2)
        wf.setframerate(sr)
        wf.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def test_decode_wav_returns_the_files_own_rate_and_decodes_once(tmp_path, monkeypatch):
    rng = np.random.default_rng(3)
    for sr in (16000, 44100, 8000):
        x = _write_pcm16(tmp_path / f"r{sr}.wav", 0.1 * rng.standard_normal(2000), sr)
        y, got_sr = frontend.decode_wav(str(tmp_path / f"r{sr}.wav"))
        assert got_sr == sr and y.dtype == np.float32 and np.array_equal(y, x)
    calls = []
    native = frontend._native_wav

    def counting(path, pinned=False):
        calls.append(path)
        return native(path, pinned)

    def python_decoder_not_expected(*a, **k):
        raise AssertionError("a 44.1 kHz PCM file was handed to the Python decoder as well")

    monkeypatch.setattr(frontend, "_native_wav", counting)
    monkeypatch.setattr(frontend._wave, "open", python_decoder_not_expected)
    p = str(tmp_path / "r44100.wav")
    y, sr = frontend.decode_wav(p)
    assert sr == 44100 and calls == [p]
    z = frontend.load_wav_16k(p, resample=True)                               # the host path: decoded once as well
    assert calls == [p, p] and len(z) == frontend.resampled_len(len(y), 44100)
    with pytest.raises(frontend.UnsupportedAudio):
        frontend.load_wav_16k(p)                                              # still refused without resample=True


def test_decode_wav_python_decoder_when_the_native_reader_declines(tmp_path, monkeypatch):
    x = _write_pcm16(tmp_path / "s.wav", 0.1 * np.random.default_rng(4).standard_normal(2 * 1500), 22050, ch=2)
    monkeypatch.setattr(frontend, "_native_wav", lambda p, pinned=False: None)
    y, sr = frontend.decode_wav(str(tmp_path / "s.wav"))
    assert sr == 22050 and np.array_equal(y, x.reshape(-1, 2).mean(axis=1).astype(np.float32))


def test_ser_resample_is_exported_and_validates_before_any_launch(built_library):
    from interspeech_ser_amd import _lib
    assert _lib.lib.ser_version() == 18 == _lib.ABI_VERSION
    assert "ser_resample_v" in _lib.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(built_library), "ser_resample_v")
    assert _lib.lib.ser_resample_v(None, None) == -1
    a = _lib.ResampleArgs()
    assert _lib.lib.ser_resample_v(ctypes.byref(a), None) == -1
    assert b"ser_resample: null pointer" in _lib.lib.ser_last_error()
    for f in ("wav", "in_offs", "out_offs", "up", "down", "half", "bank_off", "bank", "out"):
        setattr(a, f, 256)                                                    # never dereferenced: validation comes first
    a.B, a.total_in, a.total_out, a.max_out = 2, 1000, 400, 300
    for field, bad in (("B", 0), ("B", -1), ("total_in", 0), ("total_in", -5), ("total_out", 0), ("max_out", 0), ("max_out", 401)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert _lib.lib.ser_resample_v(ctypes.byref(a), None) == -2, (field, bad)
        assert b"ser_resample: bad" in _lib.lib.ser_last_error()
        setattr(a, field, keep)
    a.wav = None
    assert _lib.lib.ser_resample_v(ctypes.byref(a), None) == -1


def test_driver_hands_raw_samples_and_rates_to_an_extractor_that_resamples(tmp_path, capsys):
    """With --resample the workers decode at the file's own rate and the batch carries (samples, rate) to an extractor that has
    upload_resampled; a rate whose bank would be too large (44 101 Hz: max(up, down) > 1 024) is resampled on the host for that file;
    an extractor without upload_resampled (the stubs of the host tests) gets host-resampled 16 kHz samples as before."""
    import torch
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    seen = {}

    class Stub:
        pipelined = False

        def __init__(self, args, whisper, device):
            self.geo = C.TINY_WAVLM
            self.weight_source = "stub"

        def extract(self, waves, layer_index, rates=None):
            for w, r in zip(waves, rates if rates is not None else [None] * len(waves)):
                seen[len(seen)] = (np.array(w), r)
            return [torch.zeros(3, 4) for _ in waves]

    class GpuStub(Stub):
        def upload_resampled(self, waves, rates, slot=0):
            raise AssertionError("the stub's extract does the bookkeeping")

    wav_dir = tmp_path / "wav"
    wav_dir.mkdir()
    rng = np.random.default_rng(9)
    raw = {name: _write_pcm16(wav_dir / name, 0.1 * rng.standard_normal(n), sr)
           for name, sr, n in (("a.wav", 16000, 3000), ("b.wav", 44100, 5000), ("c.wav", 44101, 5000))}
    common = ["--wav_dir", str(wav_dir), "--batch_size", "1", "--resample"]
    assert driver._run(common + ["--save_path", str(tmp_path / "p1")], whisper=False, extractor_factory=GpuStub) == 0
    assert "Failed to process" not in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "p1")) == ["a.pt", "b.pt", "c.pt"]
    by_len = {len(w): (w, r) for w, r in seen.values()}                                              # the driver orders files by size
    (a, ra), (b, rb), (c, rc) = by_len[3000], by_len[5000], by_len[frontend.resampled_len(5000, 44101)]
    assert (ra, rb, rc) == (16000, 44100, 16000)
    assert np.array_equal(a, raw["a.wav"]) and np.array_equal(b, raw["b.wav"])                       # raw samples at the file's rate
    host_c = frontend.load_wav_16k(str(wav_dir / "c.wav"), resample=True)
    assert len(c) == frontend.resampled_len(5000, 44101) and np.array_equal(c, host_c)               # the host filter, same numbers
    seen.clear()
    assert driver._run(common + ["--save_path", str(tmp_path / "p2")], whisper=False, extractor_factory=Stub) == 0
    assert [r for _, r in seen.values()] == [None, None, None]
    host_b = frontend.load_wav_16k(str(wav_dir / "b.wav"), resample=True)
    assert any(len(w) == len(host_b) and np.array_equal(w, host_b) for w, _ in seen.values())
