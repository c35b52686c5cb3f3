"""The two waveform front ends, stated once more in float64 numpy for the tests (tests/test_frontend_ref_host.py,
tests/test_gpu_frontends.py): they lean neither on the oracle nor on the kernels.

    log_mel64:   x = fp32 samples, zero-padded / truncated to 480000;  p = reflect-pad 200 (p[i] = x[|i - 200|], mirrored at the end too)
                 F[t, n] = p[160 t + n] w[n],  w[n] = 0.5 - 0.5 cos(2 pi n / 400)  (periodic Hann),  t = 0 .. 3000,  n = 0 .. 399
                 P[t, k] = |rfft(F[t])[k]|^2,  k = 0 .. 200;  frame 3000 is dropped
                 L = log10(max(mel^T P^T, 1e-10));  out = (max(L, max(L) - 8) + 4) / 4            [n_mels, 3000]
    wave_norm64: (x - mean) / sqrt(var + 1e-7), population variance (Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm)
    frames64:    row t = [x[stride t .. stride t + k - 1], 0 ...] padded to 64 columns, T = (len - k) // stride + 1 rows
"""
import numpy as np

N_SAMPLES, N_FFT, HOP, N_FRAMES, N_BINS = 480000, 400, 160, 3000, 201
CLAMP_DECADES = 8.0


def power64(wave_f32):
    """[3000, 201] float64 power spectrum of the 3000 kept frames."""
    w = np.asarray(wave_f32, dtype=np.float64).reshape(-1)[:N_SAMPLES]
    x = np.zeros(N_SAMPLES, dtype=np.float64)
    x[: len(w)] = w
    p = np.pad(x, N_FFT // 2, mode="reflect")
    n = np.arange(N_FFT, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)
    frames = np.lib.stride_tricks.sliding_window_view(p, N_FFT)[::HOP]          # [3001, 400]
    assert frames.shape == (N_FRAMES + 1, N_FFT)
    spec = np.fft.rfft(frames[:N_FRAMES] * hann, axis=-1)                       # frame 3000 is dropped
    return spec.real ** 2 + spec.imag ** 2


def log_mel_raw64(wave_f32, mel_filters, power=None):
    """[n_mels, 3000] float64: log10(max(mel^T |STFT|^2, 1e-10)) before the per-utterance clamp (what the GPU tests compare when they
    have to name the stage an error comes from).  ``power`` = power64(wave_f32), for callers that project one wave on several matrices."""
    mel = np.asarray(mel_filters, dtype=np.float64)
    assert mel.ndim == 2 and mel.shape[0] == N_BINS, mel.shape
    if power is None:
        power = power64(wave_f32)
    return np.log10(np.maximum(mel.T @ power.T, 1e-10))


def clamp_floor(raw):
    """The per-utterance floor: max - 8 decades."""
    return float(raw.max()) - CLAMP_DECADES


def log_mel64(wave_f32, mel_filters, power=None):
    """[n_mels, 3000] float64 Whisper input features of one utterance's fp32 samples for the [201, n_mels] filter matrix given."""
    raw = log_mel_raw64(wave_f32, mel_filters, power)
    return (np.maximum(raw, clamp_floor(raw)) + 4.0) / 4.0


def wave_norm64(wave_f32):
    x = np.asarray(wave_f32, dtype=np.float64).reshape(-1)
    mean = x.sum() / len(x)
    var = ((x - mean) ** 2).sum() / len(x)
    return (x - mean) / np.sqrt(var + 1e-7)


def n_frames(n, k, stride):
    return (int(n) - k) // stride + 1 if n >= k else 0


def frames64(x, k, stride):
    """[T, 64] float64 rows of conv layer 0's im2col: columns k .. 63 are zero."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T = n_frames(len(x), k, stride)
    out = np.zeros((T, 64), dtype=np.float64)
    if T:
        out[:, :k] = np.lib.stride_tricks.sliding_window_view(x, k)[::stride][:T]
    return out


# ------------------------------------------------------------------------------------------------- the waves both test modules run
EDGE_LENGTHS = (0, 1, 199, 200, 201, 479840, 479999, 480000, 480001, 480200)
LOGMEL_CASES = ("noise", "tone over floor", "DC offset", "loud then quiet", "30 s truncated", "edges", "silence")


def logmel_case(name):
    """name -> list of fp32 waves (one, except "edges": the ragged batch of EDGE_LENGTHS).  Seeded; |x| <= 1."""
    rng = np.random.default_rng(1000 + LOGMEL_CASES.index(name))
    if name == "noise":
        return [(0.1 * rng.standard_normal(100000)).astype(np.float32)]
    if name == "tone over floor":
        t = np.arange(160000, dtype=np.float64) / 16000.0
        return [(0.5 * np.sin(2.0 * np.pi * 1000.0 * t) + 10.0 ** -3.5 * rng.standard_normal(160000)).astype(np.float32)]
    if name == "DC offset":
        return [(0.5 + 1e-3 * rng.standard_normal(64000)).astype(np.float32)]
    if name == "loud then quiet":
        return [np.concatenate([np.clip(0.9 * rng.standard_normal(8000), -1.0, 1.0), 1e-4 * rng.standard_normal(80000)]).astype(np.float32)]
    if name == "30 s truncated":
        return [(0.1 * rng.standard_normal(500000)).astype(np.float32)]
    if name == "edges":
        return [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in EDGE_LENGTHS]
    if name == "silence":
        return [np.zeros(16000, dtype=np.float32)]
    raise KeyError(name)


WAVE_CASES = ("sigma 0.1 offset 0.03", "DC 0.5 sigma 1e-3", "near-silent", "constant 0.25", "zeros", "short ragged", "long + three short",
              "one long")


def wave_case(name):
    """name -> list of fp32 clips, one ragged batch of ser_wave_frames_v."""
    rng = np.random.default_rng(2000 + WAVE_CASES.index(name))

    def noise(n, sigma, offset=0.0):
        return (offset + sigma * rng.standard_normal(n)).astype(np.float32)

    if name == "sigma 0.1 offset 0.03":
        return [noise(16000, 0.1, 0.03)]
    if name == "DC 0.5 sigma 1e-3":
        return [noise(64000, 1e-3, 0.5)]
    if name == "near-silent":
        return [noise(16000, 1e-4)]
    if name == "constant 0.25":
        return [np.full(4000, 0.25, dtype=np.float32)]
    if name == "zeros":
        return [np.zeros(4000, dtype=np.float32)]
    if name == "short ragged":                                  # fewer samples than the 64 statistics chunks, one more, and a few frames
        return [noise(n, 0.1, 0.03) for n in (10, 14, 15, 63, 64, 65, 401)]
    if name == "long + three short":                            # the grid follows the AVERAGE rows per utterance: several passes for the long one
        return [noise(n, 0.1, 0.03) for n in (480000, 10, 10, 10)]
    if name == "one long":                                      # 95999 rows: more than 1024 blocks of 32
        return [noise(480000, 0.1, 0.03)]
    raise KeyError(name)
