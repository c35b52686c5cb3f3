"""Writes tests/golden/tiny_prosody_d128h2.npz: what the reference's own modules (src/ns3: MelSpectrogram, TransformerEncoder,
ResidualVQ, with nn.Linear for melspec_linear) compute in fp32 on the CPU at a tiny geometry, composed utterance by utterance the way
FACodecEncoderV2.get_prosody_feature and FACodecDecoderV2.get_processed_style_embedding compose them.  Arrays only.

    python tools/make_prosody_golden.py /path/to/interspeech_ser

Run where the reference checkout exists.  The modules melspec.py imports and does not need for this (pyworld, soundfile, torchaudio,
librosa) are stubbed where they are absent; ``librosa.filters.mel`` is bound to transformers' Slaney filter bank (parity with
librosa's own table is not pinned offline).  Weights are PyTorch's default initialisation under a seed, rounded to fp16 values (stored as fp16: half the bytes,
exactly the fp32 weights the modules ran with); waves are int16 PCM / 32768.  tests/test_prosody_host.py compares tests/prosody_ref.py
to the fixture, tests/test_gpu_prosody.py the device.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, HEADS, LAYERS, FILTER, KERNEL, CODES_LOG2, CODE_DIM = 128, 2, 2, 128, 5, 6, 8
LENGTHS = (400, 799, 12800, 16000, 25999)        # T = 3 (the shortest legal wave), 4, 65 (a multiple of 200), 81, 130
SHORT = 399                                      # must fail alone


def stub_modules() -> None:
    from transformers.audio_utils import mel_filter_bank

    def mel(sr, n_fft, n_mels, fmin, fmax):
        return mel_filter_bank(1 + n_fft // 2, n_mels, fmin, fmax, sr, norm="slaney", mel_scale="slaney").T

    for name in ("pyworld", "soundfile", "torchaudio", "torchaudio.functional", "librosa", "librosa.filters"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchaudio.functional"].pitch_shift = None
    sys.modules["torchaudio"].functional = sys.modules["torchaudio.functional"]
    sys.modules["librosa.filters"].mel = mel
    sys.modules["librosa"].filters = sys.modules["librosa.filters"]


def waves(rng) -> list:
    """voiced-looking test signals: a few harmonics of a gliding pitch under a slow envelope, plus noise; int16 PCM"""
    out = []
    for n in LENGTHS + (SHORT,):
        t = np.arange(n) / 16000.0
        f0 = rng.uniform(90, 220) * (1.0 + 0.3 * np.sin(2 * np.pi * rng.uniform(1, 4) * t + rng.uniform(0, 6)))
        ph = 2 * np.pi * np.cumsum(f0) / 16000.0
        x = sum(rng.uniform(0.2, 1.0) / h * np.sin(h * ph + rng.uniform(0, 6)) for h in range(1, 9))
        x = x * (0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2, 6) * t + rng.uniform(0, 6))) + 0.05 * rng.standard_normal(n)
        out.append(np.round(x / np.abs(x).max() * 0.5 * 32767).astype(np.int16))
    return out


def main(reference_dir: str) -> None:
    stub_modules()
    sys.path.insert(0, os.path.join(reference_dir, "src", "ns3"))
    from melspec import MelSpectrogram
    from quantize.rvq import ResidualVQ
    from transformer import TransformerEncoder
    from tests import prosody_ref as R
    torch.manual_seed(20251)
    mel_transform = MelSpectrogram(n_fft=1024, num_mels=80, sampling_rate=16000, hop_size=200, win_size=800, fmin=0, fmax=8000)
    melspec_linear = torch.nn.Linear(20, D)
    melspec_encoder = TransformerEncoder(encoder_layer=LAYERS, encoder_hidden=D, encoder_head=HEADS, conv_filter_size=FILTER,
                                         conv_kernel_size=KERNEL, encoder_dropout=0.1, use_cln=False, cfg=None)
    quantizer = ResidualVQ(num_quantizers=1, dim=D, codebook_size=CODES_LOG2, codebook_dim=CODE_DIM, threshold_ema_dead_code=2,
                           commitment=0.005, weight_init=False, full_commit_loss=False, quantizer_dropout=0.0, dropout_type="linear")
    mods = {"melspec_linear": melspec_linear, "melspec_encoder": melspec_encoder, "quantizer.0": quantizer}
    sd = {}
    for prefix, m in mods.items():
        m.eval()
        part = {k: v.half().float() for k, v in m.state_dict().items()}       # fp16 values: what the fixture stores
        m.load_state_dict(part)
        sd.update({f"{prefix}.{k}": v for k, v in part.items() if not k.endswith("position_emb.pe")})
    pcm = waves(np.random.default_rng(20252))
    out = {"w." + k: v.numpy().astype(np.float16) for k, v in sd.items()}
    out["keys"] = np.array(list(sd.keys()))
    out["lengths"] = np.array(LENGTHS, dtype=np.int64)
    out["short_wave"] = pcm[-1]
    mels, zs, codes, rows, gaps = [], [], [], [], []
    with torch.no_grad():
        for j, p in enumerate(pcm[:-1]):
            out[f"wave_{j}"] = p
            y = p.astype(np.float32) / 32768.0
            y = np.pad(y, (0, 200 - len(y) % 200))                           # preprocess_ns3_prosody.py:45
            y = torch.tensor(y).float().unsqueeze(0).unsqueeze(0)
            prosody = mel_transform(y.squeeze(1))[:, :20, :]                 # get_prosody_feature
            f0_input = melspec_encoder(melspec_linear(prosody.transpose(1, 2)), None, None)
            o, q, _, _ = quantizer(f0_input.transpose(1, 2), n_quantizers=None)
            feats = o.squeeze(0).permute(1, 0)
            T = R.frames(len(p))
            assert tuple(feats.shape) == (T, D) and prosody.shape[-1] == T, (feats.shape, T)
            mels.append(prosody[0].T.numpy())
            zs.append(f0_input[0].numpy())
            codes.append(q[0, 0].numpy())
            rows.append(feats.numpy())
            qz = R.quantize(R._f64(sd), zs[-1].astype(np.float64))           # float64 distances on the reference's own fp32 z
            assert np.array_equal(qz["codes"], codes[-1]), "fp32 and float64 disagree on a code"
            gaps.append(qz["gaps"])
        y = torch.tensor(np.pad(pcm[-1].astype(np.float32) / 32768.0, (0, 200 - SHORT % 200))).float()[None]
        try:
            mel_transform(y)
            raise AssertionError("the 399-sample wave went through")
        except RuntimeError as e:
            print(f"{SHORT} samples: {e}")
    out.update(mel=np.concatenate(mels).astype(np.float32), z=np.concatenate(zs).astype(np.float32),
               codes=np.concatenate(codes).astype(np.int32), rows=np.concatenate(rows).astype(np.float32),
               gaps=np.concatenate(gaps).astype(np.float64))
    n_codes, close = len(np.unique(out["codes"])), float((out["gaps"] <= 1e-3).mean())
    print(f"{len(out['codes'])} frames, {n_codes} distinct codes, {100 * close:.2f} % of frames with a gap <= 1e-3")
    assert n_codes >= 8 and close <= 0.05
    path = os.path.join(ROOT, "tests", "golden", "tiny_prosody_d128h2.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main(sys.argv[1])
