"""CPU: the float64 statements of tests/frontend_ref.py against what already pins this project's front ends -- the committed Hugging Face
log-mel probes, oracle.whisper_log_mel and base_oracle.normalize_wave -- and the stress waves of tests/test_gpu_frontends.py against the
dynamic range they are named for.  The GPU gates rest on what is checked here."""
import os

import numpy as np
import pytest

import base_oracle as BO
import frontend_ref as R
from interspeech_ser_amd.frontend import whisper_mel_filters
from oracle import ssl_oracle as O

U32 = 2.0 ** -24                                     # unit roundoff of fp32


@pytest.fixture(scope="module")
def logmel_pairs():
    """{(case, index in its batch, n_mels): (float64 statement before the clamp, statement, oracle)}, computed once."""
    out = {}
    for name in R.LOGMEL_CASES:
        for i, w in enumerate(R.logmel_case(name)):
            power = R.power64(w)
            for n_mels in (80, 128):
                mel = whisper_mel_filters(n_mels)
                out[name, i, n_mels] = (R.log_mel_raw64(w, mel, power), R.log_mel64(w, mel, power), O.whisper_log_mel(w, n_mels))
    return out


def test_log_mel64_matches_the_hugging_face_probes(golden_dir):
    """Every 50th frame of WhisperFeatureExtractor's own output, at the bound tests/test_oracle_golden.py holds the oracle to."""
    def synth_wave(seed, n):                                          # the fixture's waves (oracle/make_golden.py)
        rng = np.random.default_rng(seed)
        t = np.arange(n, dtype=np.float64) / 16000.0
        return np.clip(0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t), -1, 1).astype(np.float32)

    gold = np.load(os.path.join(golden_dir, "tiny_whisper_d128h2.npz"))
    mel = whisper_mel_filters(128)
    for j, n in enumerate(int(x) for x in gold["lengths"]):
        got = R.log_mel64(synth_wave(int(gold[f"wave_seed_{j}"]), n), mel)
        assert got.shape == (128, 3000) and got.dtype == np.float64
        err = float(np.abs(got[:, ::50] - gold[f"mel_probe_{j}"]).max())
        print(f"log_mel64 vs the HF probe {j} ({n} samples): {err:.3e}")
        assert err < 1e-5, (j, err)


def test_log_mel64_matches_the_oracle_on_every_gpu_case(logmel_pairs):
    """Element by element.  The oracle's STFT is fp32: window rounding and an fp32 FFT of 400 points leave an amplitude error of up to
    c u32 times the LARGEST amplitude of the frame, c = 2 log2(400) = 17.3 (log2 N butterfly stages, twice for the window product and the
    mel sum that follow).  An element whose mel power lies D decades below the utterance maximum has 10^(-D/2) of its amplitude, so its
    amplitude is off by at most c u32 10^(D/2) relatively, its power by twice that, its log10 by that / ln 10, the feature by a quarter
    (D <= 8: the clamp).  On top of it the fp32 rounding of log10, of the clamp and of (v + 4) / 4: 4 u32 ulp-of-16 terms, 1e-6.
    At D = 8 this allows 2.2e-3, at the maximum 1.2e-6."""
    c = 2.0 * np.log2(400.0)
    for (name, i, n_mels), (raw, ref, got) in logmel_pairs.items():
        assert got.shape == ref.shape == (n_mels, 3000)
        depth = np.minimum(raw.max() - raw, R.CLAMP_DECADES)
        tol = 2.0 * c * U32 * 10.0 ** (depth / 2.0) / np.log(10.0) / 4.0 + 1e-6
        err = np.abs(got - ref)
        print(f"{name}[{i}] n_mels {n_mels}: max |oracle - log_mel64| {float(err.max()):.3e}, worst err / bound {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (name, i, n_mels, float((err / tol).max()))


@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_stress_cases_exercise_the_range_they_are_named_for(logmel_pairs, n_mels):
    """From the float64 statement alone: the share of elements within one decade above the utterance's clamp floor."""
    def near_floor(raw):
        floor = R.clamp_floor(raw)
        return float(((raw >= floor) & (raw <= floor + 1.0)).mean()), float((raw < floor).mean())

    for name in ("tone over floor", "DC offset"):
        near, clamped = near_floor(logmel_pairs[name, 0, n_mels][0])
        print(f"{name} n_mels {n_mels}: {100 * near:.2f} % within a decade of the floor, {100 * clamped:.2f} % clamped")
        assert near >= 0.01, (name, near)
    raw = logmel_pairs["noise", 0, n_mels][0]
    inside = (100000 - 200) // 160                                   # frames 0 .. inside - 1 hold no zero padding
    assert not (raw[:, :inside] < R.clamp_floor(raw)).any()
    padded = -(-(100000 + 200) // 160)                               # frames from here on hold nothing else: the 1e-10 guard, clamped
    assert (raw[:, padded:] == -10.0).all()
    raw = logmel_pairs["30 s truncated", 0, n_mels][0]
    assert not (raw < R.clamp_floor(raw)).any()
    raw = logmel_pairs["loud then quiet", 0, n_mels][0]              # the quiet part straddles the floor that the loud part sets
    quiet = raw[:, 60:540]
    assert (quiet > R.clamp_floor(raw)).any() and (quiet < R.clamp_floor(raw)).any() and quiet.max() < raw.max() - 7.0
    assert (logmel_pairs["silence", 0, n_mels][1] == -1.5).all()


def test_log_mel64_truncates_and_reflects_where_it_says():
    """The length edges, against the statement's own definition on a hand-built frame: sample 480000 and later never matter; the last
    kept frame (2999) reads p[479840 .. 480239] = x[479640 .. 479999], then x[479998 .. 479960] mirrored."""
    rng = np.random.default_rng(5)
    x = (0.1 * rng.standard_normal(480200)).astype(np.float32)
    mel = whisper_mel_filters(80)
    assert np.array_equal(R.log_mel64(x, mel), R.log_mel64(x[:480000], mel))
    xd = x[:480000].astype(np.float64)
    frame = np.concatenate([xd[479640:], xd[479998:479958:-1]])
    assert len(frame) == 400
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(400) / 400)
    k = np.arange(201)[:, None] * np.arange(400)[None, :]
    spec = (np.exp(-2j * np.pi * k / 400) * (frame * hann)[None, :]).sum(axis=1)              # the plain DFT sum
    assert np.allclose(R.power64(x)[2999], np.abs(spec) ** 2, rtol=1e-9, atol=1e-18)
    first = np.concatenate([xd[200:0:-1], xd[:200]])                                         # frame 0: p[0 .. 399] = x[200 .. 1], x[0 .. 199]
    spec = (np.exp(-2j * np.pi * k / 400) * (first * hann)[None, :]).sum(axis=1)
    assert np.allclose(R.power64(x)[0], np.abs(spec) ** 2, rtol=1e-9, atol=1e-18)


def test_wave_norm64_matches_the_oracle():
    """base_oracle.normalize_wave is numpy fp32: its mean carries up to u32 |mean| (pairwise sum, one rounding at this size class), the
    difference x - mean one rounding, the quotient one more, the deviation's relative error half the variance's (a few u32).  In units of
    the output: (u32 |mean| + 2 u32 max|x - mean|) / std + 4 u32 max|out|."""
    for name in R.WAVE_CASES:
        for i, w in enumerate(R.wave_case(name)):
            ref = R.wave_norm64(w)
            got = BO.normalize_wave(w).astype(np.float64)
            x = w.astype(np.float64)
            std = np.sqrt(x.var() + 1e-7)
            tol = (U32 * abs(x.mean()) + 2 * U32 * np.abs(x - x.mean()).max()) / std + 4 * U32 * np.abs(ref).max() + 1e-12
            err = float(np.abs(got - ref).max())
            print(f"{name}[{i}] ({len(w)} samples): max |normalize_wave - wave_norm64| {err:.3e}, bound {tol:.3e}")
            assert err <= tol, (name, i, err, tol)
            assert abs(ref.mean()) < 1e-9 and (name in ("constant 0.25", "zeros") or abs(ref.var() - x.var() / (x.var() + 1e-7)) < 1e-9)
    assert (R.wave_norm64(np.full(4000, 0.25, dtype=np.float32)) == 0.0).all()


def test_frames64_is_the_im2col_of_conv_layer_0():
    x = np.arange(1, 28, dtype=np.float32)
    f = R.frames64(x, 10, 5)
    assert f.shape == (4, 64) and R.n_frames(27, 10, 5) == 4 and R.n_frames(9, 10, 5) == 0 and R.frames64(x[:9], 10, 5).shape == (0, 64)
    for t in range(4):
        assert np.array_equal(f[t, :10], x[5 * t: 5 * t + 10]) and not f[t, 10:].any()
