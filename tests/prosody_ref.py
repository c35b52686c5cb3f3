"""Float64 statement of the reference's prosody stream (preprocessing/preprocess_ns3_prosody.py:41-60), one utterance at a time:
FACodecEncoderV2.get_prosody_feature's 20-bin log-mel (src/ns3/melspec.py), then of FACodecDecoderV2.get_processed_style_embedding
melspec_linear, melspec_encoder (src/ns3/transformer.py) and the first layer of quantizer[0] (src/ns3/quantize/fvq.py).  Written from
what those files compute, on the checkpoint's own key names; nothing of the product's ``prosody.prepare`` is used, so the folds it makes
(weight norm, the position-0 vector in the bias, the [codes, D] table, the FC1 weight layout) are checked against this.

``torch_twin`` is the same computation in fp32 torch ops the way the reference composes them (torch.stft, nn.functional): the
"reference-style" CPU path whose distance from the statement bounds what a faithful implementation may differ by.
Error form as everywhere: max|a - b| / max(1, max|b|)."""
import numpy as np
import torch

HOP, WIN, NFFT, PAD, KEEP = 200, 800, 1024, 412, 20
ENC, VQ = "melspec_encoder", "quantizer.0.layers.0"


def rel_err(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, float(np.abs(b).max())))


def frames(n: int) -> int:
    return n // HOP + 1


def mel_basis() -> np.ndarray:
    """[20, 513] float64 of the fp32 Slaney basis rows the reference keeps (the product's restatement, pinned to transformers' in
    tests/test_prosody_host.py)"""
    from interspeech_ser_amd.frontend import whisper_mel_filters
    return whisper_mel_filters(80, NFFT).T[:KEEP].astype(np.float64)


def padded(wave) -> np.ndarray:
    y = np.asarray(wave, dtype=np.float64)
    y = np.concatenate([y, np.zeros(HOP - len(y) % HOP)])
    if PAD >= len(y):
        raise ValueError(f"a wave of {len(wave)} samples cannot be reflect-padded by {PAD}")
    return np.pad(y, (PAD, PAD), mode="reflect")


def log_mel(wave) -> np.ndarray:
    """[T, 20] float64"""
    y = padded(wave)
    T = 1 + (len(y) - NFFT) // HOP
    win = np.zeros(NFFT)
    win[(NFFT - WIN) // 2: (NFFT + WIN) // 2] = torch.hann_window(WIN, dtype=torch.float32).double().numpy()
    fr = np.stack([y[t * HOP: t * HOP + NFFT] for t in range(T)]) * win
    spec = np.fft.rfft(fr, axis=1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return np.log(np.maximum(mag @ mel_basis().T, np.float64(np.float32(1e-5))))


def _f64(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items()}


def layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def weight_norm(sd, p):
    g, v = sd[p + ".weight_g"], sd[p + ".weight_v"]
    return g.reshape(-1, 1) * v / np.sqrt((v ** 2).sum(axis=1, keepdims=True))


def encoder(sd, mel, heads: int, real_positions: bool = False) -> np.ndarray:
    """[T, 20] log-mel -> z [T, D]: melspec_linear, the positional encoding as the reference applies it, the layers, last_ln.
    ``real_positions``: what PositionalEncoding would add on (T, B, d) input -- NOT the reference (a test's counter-example)."""
    x = mel @ sd["melspec_linear.weight"].T + sd["melspec_linear.bias"]
    T, D = x.shape
    div = np.exp(np.arange(0, D, 2) * (-np.log(10000.0) / D))
    pos = np.arange(T)[:, None] if real_positions else np.zeros((T, 1))      # pe[:1] broadcast over the frames: position 0 everywhere
    x[:, 0::2] += np.sin(pos * div)
    x[:, 1::2] += np.cos(pos * div)
    dh = D // heads
    L = 0
    while f"{ENC}.layers.{L}.ln_1.weight" in sd:
        L += 1
    for i in range(L):
        p = f"{ENC}.layers.{i}"
        y = layer_norm(x, sd[p + ".ln_1.weight"], sd[p + ".ln_1.bias"])
        qkv = y @ sd[p + ".self_attn.in_proj_weight"].T + sd[p + ".self_attn.in_proj_bias"]
        ctx = np.empty((T, D))
        for h in range(heads):
            q, k, v = (qkv[:, j * D + h * dh: j * D + (h + 1) * dh] for j in range(3))
            s = (q * dh ** -0.5) @ k.T
            s = np.exp(s - s.max(axis=1, keepdims=True))
            ctx[:, h * dh:(h + 1) * dh] = (s / s.sum(axis=1, keepdims=True)) @ v
        x = x + ctx @ sd[p + ".self_attn.out_proj.weight"].T + sd[p + ".self_attn.out_proj.bias"]
        y = layer_norm(x, sd[p + ".ln_2.weight"], sd[p + ".ln_2.bias"])
        w = sd[p + ".ffn.ffn_1.weight"]                                      # [F, D, k]
        k = w.shape[2]
        yp = np.concatenate([np.zeros((k // 2, D)), y, np.zeros((k // 2, D))])
        f = sum(yp[j: j + T] @ w[:, :, j].T for j in range(k)) + sd[p + ".ffn.ffn_1.bias"]
        x = x + np.maximum(f, 0.0) @ sd[p + ".ffn.ffn_2.weight"].T + sd[p + ".ffn.ffn_2.bias"]
    return layer_norm(x, sd[ENC + ".last_ln.weight"], sd[ENC + ".last_ln.bias"])


def quantize(sd, z):
    """z [T, D] -> dict(e [T, 8], dist [T, N], codes [T], gaps [T], rows [T, D])"""
    z_e = z @ weight_norm(sd, VQ + ".in_proj").T + sd[VQ + ".in_proj.bias"]
    e = z_e / np.maximum(np.sqrt((z_e ** 2).sum(axis=1, keepdims=True)), 1e-12)
    cb = sd[VQ + "._codebook.weight"]
    c = cb / np.maximum(np.sqrt((cb ** 2).sum(axis=1, keepdims=True)), 1e-12)
    dist = (e ** 2).sum(axis=1, keepdims=True) - 2.0 * e @ c.T + (c ** 2).sum(axis=1)[None, :]
    codes = dist.argmin(axis=1)                                              # the first minimum: the lowest index on a tie
    srt = np.sort(dist, axis=1)
    gaps = srt[:, 1] - srt[:, 0] if dist.shape[1] > 1 else np.full(len(z), np.inf)
    rows = cb[codes] @ weight_norm(sd, VQ + ".out_proj").T + sd[VQ + ".out_proj.bias"]
    return dict(e=e, dist=dist, codes=codes.astype(np.int64), gaps=gaps, rows=rows)


def forward(sd, wave, heads: int) -> dict:
    sd = _f64(sd)
    mel = log_mel(wave)
    z = encoder(sd, mel, heads)
    out = quantize(sd, z)
    out.update(mel=mel, z=z)
    return out


# ---------------------------------------------------------------------------------------------- the fp32 torch twin (reference-style)
def torch_log_mel(wave) -> torch.Tensor:
    """[T, 20] fp32 through torch.stft, as src/ns3/melspec.py composes it"""
    y = torch.as_tensor(np.asarray(wave, dtype=np.float32))
    y = torch.nn.functional.pad(y, (0, HOP - len(y) % HOP))[None]
    y = torch.nn.functional.pad(y.unsqueeze(1), (PAD, PAD), mode="reflect").squeeze(1)
    spec = torch.stft(y, NFFT, hop_length=HOP, win_length=WIN, window=torch.hann_window(WIN), center=False, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    spec = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    basis = torch.from_numpy(mel_basis()).float()
    return torch.log(torch.clamp(torch.matmul(basis, spec), min=1e-5))[0].T.contiguous()


def torch_twin(sd, wave, heads: int) -> dict:
    """mel, z, codes, rows in fp32 torch ops (nn.functional.multi_head_attention_forward, conv1d), batch of one"""
    F = torch.nn.functional
    sd = {k: torch.as_tensor(v).float() for k, v in sd.items()}
    mel = torch_log_mel(wave)
    x = F.linear(mel, sd["melspec_linear.weight"], sd["melspec_linear.bias"])[None]      # (1, T, D)
    D = x.shape[-1]
    pe0 = torch.zeros(D)
    pe0[1::2] = 1.0
    x = x + pe0
    L = 0
    while f"{ENC}.layers.{L}.ln_1.weight" in sd:
        L += 1
    for i in range(L):
        p = f"{ENC}.layers.{i}"
        y = F.layer_norm(x, (D,), sd[p + ".ln_1.weight"], sd[p + ".ln_1.bias"], 1e-5)
        yt = y.transpose(0, 1)
        a, _ = F.multi_head_attention_forward(yt, yt, yt, D, heads, sd[p + ".self_attn.in_proj_weight"], sd[p + ".self_attn.in_proj_bias"],
                                              None, None, False, 0.0, sd[p + ".self_attn.out_proj.weight"],
                                              sd[p + ".self_attn.out_proj.bias"], training=False, need_weights=False)
        x = x + a.transpose(0, 1)
        y = F.layer_norm(x, (D,), sd[p + ".ln_2.weight"], sd[p + ".ln_2.bias"], 1e-5)
        w = sd[p + ".ffn.ffn_1.weight"]
        f = F.conv1d(y.permute(0, 2, 1), w, sd[p + ".ffn.ffn_1.bias"], padding=w.shape[2] // 2).permute(0, 2, 1)
        x = x + F.linear(F.relu(f), sd[p + ".ffn.ffn_2.weight"], sd[p + ".ffn.ffn_2.bias"])
    z = F.layer_norm(x, (D,), sd[ENC + ".last_ln.weight"], sd[ENC + ".last_ln.bias"], 1e-5)[0]

    def wn(p):
        g, v = sd[p + ".weight_g"], sd[p + ".weight_v"]
        return g * v / v.norm(dim=1, keepdim=True)
    z_e = F.linear(z, wn(VQ + ".in_proj"), sd[VQ + ".in_proj.bias"])
    e, c = F.normalize(z_e), F.normalize(sd[VQ + "._codebook.weight"])
    dist = e.pow(2).sum(1, keepdim=True) - 2 * e @ c.t() + c.pow(2).sum(1, keepdim=True).t()
    codes = (-dist).max(1)[1]
    rows = F.linear(sd[VQ + "._codebook.weight"][codes], wn(VQ + ".out_proj"), sd[VQ + ".out_proj.bias"])
    return dict(mel=mel.numpy(), z=z.numpy(), codes=codes.numpy(), rows=rows.numpy())


def load_golden(golden_dir: str) -> dict:
    """tests/golden/tiny_prosody_d128h2.npz as (state dict of fp32 tensors, waves, packed frame offsets, the 399-sample wave, arrays)"""
    import os
    g = np.load(os.path.join(golden_dir, "tiny_prosody_d128h2.npz"))
    sd = {str(k): torch.from_numpy(g["w." + str(k)].astype(np.float32)) for k in g["keys"]}
    waves = [g[f"wave_{j}"].astype(np.float32) / 32768.0 for j in range(len(g["lengths"]))]
    offs = np.concatenate([[0], np.cumsum([frames(len(w)) for w in waves])])
    return dict(g=g, sd=sd, waves=waves, offs=offs, short=g["short_wave"].astype(np.float32) / 32768.0)
