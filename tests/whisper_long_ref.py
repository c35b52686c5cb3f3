"""Whisper long-form transcription, stated once more for the tests (tests/test_whisper_longform_host.py,
tests/test_gpu_whisper_longform.py): the whole-file log-mel in float64 numpy and the seek loop over scripted windows.  It leans neither on
the kernels nor on interspeech_ser_amd.transcribe.

    log_mel_long64: x = the file's fp32 samples, ANY length >= 201;  F = len // 160 frames
                    p = reflect-pad 200 about the file's own first and last sample;  frames, Hann, rfft as frontend_ref.power64
                    frame F (the STFT's last) is dropped BEFORE the maximum;  L = log10(max(mel^T P^T, 1e-10))
                    out = (max(L, max(L) - 8) + 4) / 4                                                       [n_mels, F]
                    -- what WhisperFeatureExtractor(...)(wave, truncation=False, padding="longest") returns
    loop:           HF's WhisperGenerationMixin.generate, long-form, one file at batch size 1 (generation_whisper.py:649-903):
                    seek = 0; while seek < F: nf = min(3000, F - seek); time_offset = float64(seek) * 0.02 / 2; ids = decode(window, seek, nf);
                    segments, advance = segments_of(ids, ts_begin, nf, time_offset); seek += advance
"""
import numpy as np

import frontend_ref as FR
import whisper_seg_ref as SR

N_WINDOW = 3000


def frames_of(n_samples: int) -> int:
    return int(n_samples) // FR.HOP


def power_long64(wave_f32):
    """[F, 201] float64 power spectrum of the file's F = len // 160 kept frames"""
    x = np.asarray(wave_f32, dtype=np.float64).reshape(-1)
    assert len(x) > FR.N_FFT // 2, "numpy's reflect pad of 200 needs at least 201 samples"
    F = frames_of(len(x))
    p = np.pad(x, FR.N_FFT // 2, mode="reflect")
    n = np.arange(FR.N_FFT, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / FR.N_FFT)
    frames = np.lib.stride_tricks.sliding_window_view(p, FR.N_FFT)[::FR.HOP]        # [F + 1, 400]
    assert frames.shape == (F + 1, FR.N_FFT)
    spec = np.fft.rfft(frames[:F] * hann, axis=-1)                                 # frame F is dropped
    return spec.real ** 2 + spec.imag ** 2


def log_mel_long_raw64(wave_f32, mel_filters):
    mel = np.asarray(mel_filters, dtype=np.float64)
    assert mel.ndim == 2 and mel.shape[0] == FR.N_BINS, mel.shape
    return np.log10(np.maximum(mel.T @ power_long64(wave_f32).T, 1e-10))


def log_mel_long64(wave_f32, mel_filters):
    """[n_mels, len // 160] float64 long-form input features of one file's fp32 samples: one floor, the file's"""
    raw = log_mel_long_raw64(wave_f32, mel_filters)
    return (np.maximum(raw, FR.clamp_floor(raw)) + 4.0) / 4.0


def window_of(features, seek: int, nf: int):
    """[n_mels, 3000]: the features at [seek, seek + nf), then 3000 - nf columns of exactly 0.0"""
    out = np.zeros((features.shape[0], N_WINDOW), dtype=features.dtype)
    out[:, :nf] = features[:, seek: seek + nf]
    return out


def loop(features_len: int, decode, ts_begin: int, max_windows: int = 1000):
    """The seek loop of one file of ``features_len`` frames.  ``decode(window_index, seek, nf) -> ids`` (prompt, pads and the closing eos
    removed).  Returns dict(windows [(seek, nf, advance)], offsets [time_offset], segments [(start_s, end_s, ids)], sequence (the
    segments' ids: what HF's generate returns), seek (the final one), stuck (a window whose advance was 0: HF would not end))."""
    seek, k = 0, 0
    windows, offsets, segments, sequence = [], [], [], []
    while seek < features_len:
        assert k < max_windows
        nf = min(N_WINDOW, features_len - seek)
        off = float(seek) * SR.TIME_PRECISION / SR.INPUT_STRIDE
        ids = [int(t) for t in decode(k, seek, nf)]
        segs, adv = SR.segments_of(ids, ts_begin, nf, off)
        windows.append((seek, nf, int(adv)))
        offsets.append(off)
        if adv <= 0:
            return dict(windows=windows, offsets=offsets, segments=segments, sequence=sequence, seek=seek, stuck=True)
        segments.extend(segs)
        sequence.extend(t for _, _, part in segs for t in part)
        seek += int(adv)
        k += 1
    return dict(windows=windows, offsets=offsets, segments=segments, sequence=sequence, seek=seek, stuck=False)


# ------------------------------------------------------------------------------------------------- the end-to-end fixture (tests/golden)
FIXTURE = "tiny_whisper_long_d128h2.npz"
EOS, START, TRANSLATE, TASK, NO_TS = 470, 471, 476, 477, 481
LANG_IDS = (472, 473, 474, 475)
TS_BEGIN = NO_TS + 1
N_TS = 1501                                          # <|0.00|> .. <|30.00|>
V = TS_BEGIN + N_TS
SUPPRESS = tuple(range(30, 70)) + (START, TRANSLATE, TASK, 478, 479, 480) + LANG_IDS
BEGIN_SUPPRESS = (220, EOS)
MAX_LENGTH, MAX_INITIAL, MAX_TARGET = 24, 50, 64
ENCODER_WEIGHT_SEED = 14


def fixture_geo():
    import dataclasses
    from interspeech_ser_amd import config as C
    return C.with_decoder(dataclasses.replace(C.TINY_WHISPER, name="tiny-whisper-long-d128h2"), 2, 2, 512, V, MAX_TARGET)


def fixture_spec(language=None):
    from interspeech_ser_amd import config as C
    return C.GenerationSpec(decoder_start_token_id=START, eos_token_id=EOS, pad_token_id=EOS, suppress_tokens=SUPPRESS,
                            begin_suppress_tokens=BEGIN_SUPPRESS, no_timestamps_token_id=NO_TS, lang_ids=LANG_IDS, task_id=TASK,
                            max_length=MAX_LENGTH, max_initial_timestamp_index=MAX_INITIAL, language=language)


def fixture_wave(seed: int, n_samples: int):
    """Seeded noise whose level changes every 2 to 12 s (10^-3 .. 10^-0.5): the windows of one file look different to the encoder"""
    g = np.random.default_rng(seed)
    x = g.standard_normal(n_samples)
    at = 0
    while at < n_samples:
        n = int(g.uniform(2.0, 12.0) * 16000)
        x[at: at + n] *= 10.0 ** g.uniform(-3.0, -0.5)
        at += n
    return np.clip(x, -1.0, 1.0).astype(np.float32)


_FIXTURE = {}


def load_fixture(golden_dir):
    """(gold npz, geometry, state dict of encoder and decoder, GenerationSpec, waves) of the long-form fixture: weights and waves
    regenerated from the recorded seeds and checked against the recorded digest.  Loaded once and shared; nobody writes to it."""
    if "v" not in _FIXTURE:
        import os
        from interspeech_ser_amd import config as C
        from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
        gold = np.load(os.path.join(golden_dir, FIXTURE))
        geo = fixture_geo()
        dec_sd = SR.fixture_state_dict(geo, int(gold["decoder_seed"]), TS_BEGIN, float(gold["ts_scale"]))
        assert state_dict_digest(dec_sd) == str(gold["digest"]), "the decoder weights are not the ones the fixture was recorded with"
        sd = dict(synthetic_state_dict(C.TINY_WHISPER, int(gold["encoder_seed"])))
        sd.update(dec_sd)
        waves = [fixture_wave(int(s), int(n)) for s, n in zip(gold["wave_seeds"], gold["wave_lengths"])]
        _FIXTURE["v"] = (gold, geo, sd, fixture_spec(), waves)
    return _FIXTURE["v"]
