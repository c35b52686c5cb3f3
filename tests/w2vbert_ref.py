"""float64 statement of w2v-BERT 2.0 (HF Wav2Vec2BertModel behind SeamlessM4TFeatureExtractor, one utterance alone): the Kaldi fbank
front end and the conformer encoder with its relative-key attention bias.  Test infrastructure, like tests/data2vec_oracle.py: written
from the model's description, pinned to the HF classes by the fixtures of tools/make_golden_w2vbert.py, and the reference the GPU tests
compare kernels with.  numpy / torch on the CPU only."""
import math

import numpy as np
import torch

MEL_FLOOR = 1.192092955078125e-07


def synth_wave(seed: int, n: int) -> np.ndarray:
    """Seeded noise with a slow envelope, in [-1, 1] fp32 (numpy PCG64: the same samples on every host).  The first 640 samples fade in
    over e^8: an utterance of two to five frames then has frames of clearly different energy in every mel bin, so the per-bin standard
    deviation its normalisation divides by stays far above the fp32 rounding of a log-mel value (two noise frames of EQUAL level leave
    some of 80 bins with a difference of a few 1e-3, and a normalised value there amplifies HF's own fp32 rounding past any bound)."""
    g = np.random.default_rng(int(seed))
    x = g.standard_normal(n).astype(np.float64)
    t = np.arange(n)
    env = (0.25 + 0.2 * np.sin(t * (2 * np.pi / 3700.0) + 0.3)) * np.exp(8.0 * np.minimum(t, 640) / 640.0 - 8.0)
    y = np.convolve(x, [0.5, 0.3, 0.2], mode="same") * env
    return np.clip(y, -1.0, 1.0).astype(np.float32)


def mel_frames(n: int) -> int:
    return 1 + (n - 400) // 160 if n >= 400 else 0


def frames(n: int, stride: int = 2) -> int:
    return mel_frames(n) // stride


def mel_filters(n_mels: int = 80) -> np.ndarray:
    """[257, n_mels]: Kaldi mel scale, 20 .. 8000 Hz, triangles in mel space, no norm."""
    def mel(f):
        return 1127.0 * np.log(1.0 + f / 700.0)
    edges = np.linspace(mel(20.0), mel(8000.0), n_mels + 2)
    bins = mel(np.arange(257) * 31.25)
    fb = np.zeros((257, n_mels))
    for m in range(n_mels):
        lo, mid, hi = edges[m], edges[m + 1], edges[m + 2]
        fb[:, m] = np.maximum(0.0, np.minimum((bins - lo) / (mid - lo), (hi - bins) / (hi - mid)))
    return fb


def log_mel(wave: np.ndarray, n_mels: int = 80) -> np.ndarray:
    """[n_frames, n_mels] float64 log-mel energies before the per-bin normalisation."""
    x = np.asarray(wave, dtype=np.float32).astype(np.float64) * 32768.0
    F = mel_frames(len(x))
    window = np.hanning(400) ** 0.85
    fb = mel_filters(n_mels)
    out = np.zeros((F, n_mels))
    for f in range(F):
        fr = x[160 * f: 160 * f + 400].copy()
        fr -= fr.mean()
        z = np.empty(400)
        z[1:] = fr[1:] - 0.97 * fr[:-1]
        z[0] = fr[0] * (1.0 - 0.97)
        spec = np.abs(np.fft.rfft(z * window, 512)) ** 2
        out[f] = np.log(np.maximum(spec @ fb, MEL_FLOOR))
    return out


def fbank_rows(wave: np.ndarray, n_mels: int = 80, stride: int = 2) -> np.ndarray:
    """[T, stride n_mels] float64: normalised per mel bin over ALL frames (unbiased variance), `stride` frames to a row; an odd last
    frame counts for the statistics and has no row."""
    lm = log_mel(wave, n_mels)
    lm = (lm - lm.mean(0, keepdims=True)) / np.sqrt(lm.var(0, ddof=1, keepdims=True) + 1e-7)
    T = lm.shape[0] // stride
    return lm[: T * stride].reshape(T, stride * n_mels)


def _ln(x, sd, p, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p, bias=True):
    w = sd[p + ".weight"]
    w = w.reshape(w.shape[0], -1)
    y = x @ w.T
    return y + sd[p + ".bias"] if bias else y


def swish(x):
    return x * torch.sigmoid(x)


def relkey_bias(q: torch.Tensor, E: torch.Tensor, Lm: int, Rm: int) -> torch.Tensor:
    """q [H, T, dh], E [Lm + Rm + 1, dh] -> [H, T, T]: q . E[clamp(k - q, -Lm, Rm) + Lm]"""
    T = q.shape[1]
    pos = torch.arange(T)
    dist = torch.clamp(pos[None, :] - pos[:, None], -Lm, Rm) + Lm                  # [T(q), T(k)]
    return torch.einsum("hqd,qkd->hqk", q, E[dist])


def attention(x, sd, p, heads, Lm, Rm):
    T, D = x.shape
    dh = D // heads
    q = _lin(x, sd, p + ".linear_q").view(T, heads, dh).transpose(0, 1)
    k = _lin(x, sd, p + ".linear_k").view(T, heads, dh).transpose(0, 1)
    v = _lin(x, sd, p + ".linear_v").view(T, heads, dh).transpose(0, 1)
    s = (q @ k.transpose(1, 2) + relkey_bias(q, sd[p + ".distance_embedding.weight"], Lm, Rm)) / math.sqrt(dh)
    ctx = (torch.softmax(s, dim=-1) @ v).transpose(0, 1).reshape(T, D)
    return _lin(ctx, sd, p + ".linear_out")


def conv_module(x, sd, p, K, eps):
    """LN -> pointwise D -> 2D -> GLU -> causal depthwise (K - 1 zero rows on the left) -> LN -> swish -> pointwise D -> D"""
    T, D = x.shape
    h = _lin(_ln(x, sd, p + ".layer_norm", eps), sd, p + ".pointwise_conv1", bias=False)
    g = h[:, :D] * torch.sigmoid(h[:, D:])
    w = sd[p + ".depthwise_conv.weight"].reshape(D, K)
    gp = torch.cat([torch.zeros(K - 1, D, dtype=g.dtype), g], 0)
    u = torch.zeros_like(g)
    for k in range(K):
        u = u + gp[k: k + T] * w[:, k][None, :]
    u = swish(_ln(u, sd, p + ".depthwise_layer_norm", eps))
    return _lin(u, sd, p + ".pointwise_conv2", bias=False)


def ffn(x, sd, p):
    return _lin(swish(_lin(x, sd, p + ".intermediate_dense")), sd, p + ".output_dense")


def hidden_states(geo, sd, rows: torch.Tensor):
    """The L + 1 hidden states [T, D] (float64) of the stacked fbank rows [T, 160]; no norm behind the last layer."""
    sd = {k: v.double() for k, v in sd.items()}
    eps = geo.layer_norm_eps
    x = _lin(_ln(rows.double(), sd, "feature_projection.layer_norm", eps), sd, "feature_projection.projection")
    states = [x]
    for i in range(geo.num_layers):
        p = f"encoder.layers.{i}"
        x = x + 0.5 * ffn(_ln(x, sd, p + ".ffn1_layer_norm", eps), sd, p + ".ffn1")
        x = x + attention(_ln(x, sd, p + ".self_attn_layer_norm", eps), sd, p + ".self_attn", geo.heads,
                          geo.left_max_positions, geo.right_max_positions)
        x = x + conv_module(x, sd, p + ".conv_module", geo.conv_depthwise_kernel, eps)
        x = x + 0.5 * ffn(_ln(x, sd, p + ".ffn2_layer_norm", eps), sd, p + ".ffn2")
        x = _ln(x, sd, p + ".final_layer_norm", eps)
        states.append(x)
    return states


def forward(geo, sd, wave: np.ndarray):
    return hidden_states(geo, sd, torch.from_numpy(fbank_rows(wave, geo.fbank_mels, geo.fbank_stride)))
