"""Writes tests/golden/tiny_codec_ngf8.npz: what the reference's own FACodecEncoderV2(ngf=8, out_channels=128) and a TransformerEncoder
(2 layers, hidden 128, 2 heads, filter 64, kernel 5: the timbre encoder) compute in fp32 on the CPU for the five waves of
tests/golden/tiny_prosody_d128h2.npz, composed utterance by utterance as preprocessing/preprocess_ns3_prosody_speaker.py and
FACodecDecoderV2.get_processed_style_speaker_embedding compose them.  Arrays only.

    python tools/make_codec_golden.py /path/to/interspeech_ser

Run where the reference checkout exists; absent modules are stubbed as tools/make_prosody_golden.py stubs them.  The codec's weights are
``prosody.synthetic_codec_state_dict``'s recipe (levels of order 1; the reference's own initialisation leaves max|encoded| ~ 0.03), the
timbre encoder's PyTorch's default initialisation under a seed; both rounded to fp16 values and stored as fp16 -- exactly the fp32 weights
the modules ran with.  Stored: the weights, ``encoded`` and the timbre rows of all five waves (packed), conv_in's and every level's output
for the 400- and 799-sample waves.  The fixture is two files, each under the repository's 1 MiB limit for a committed file:
tiny_codec_ngf8.npz holds the codec's weights and ``encoded``, tiny_codec_ngf8_timbre.npz the timbre encoder's weights, the timbre rows and
the level outputs (tests/codec_ref.py load_golden reads both as one set of arrays).  tests/test_codec_host.py compares tests/codec_ref.py
to the fixture, tests/test_gpu_codec.py the device."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SEED, LEVELS_OF = 2, (0, 1)                      # the waves whose per-level outputs are stored (400 and 799 samples)
SIZE_LIMIT = 1 << 20                             # per file: no committed file may be larger than 1 MiB
FILES = ("tiny_codec_ngf8.npz", "tiny_codec_ngf8_timbre.npz")


def main(reference_dir: str, seed: int = SEED) -> None:
    from make_prosody_golden import SHORT, stub_modules
    stub_modules()
    sys.path.insert(0, os.path.join(reference_dir, "src"))
    from ns3.facodec import FACodecEncoderV2
    from ns3.transformer import TransformerEncoder
    import codec_ref as R
    from interspeech_ser_amd import prosody as P
    spec = P.TINY_CODEC
    ts = spec.timbre
    import prosody_ref
    pg = prosody_ref.load_golden(os.path.join(ROOT, "tests", "golden"))
    torch.manual_seed(20261)
    encoder = FACodecEncoderV2(ngf=spec.ngf, up_ratios=spec.strides, out_channels=spec.out_channels).eval()
    timbre = TransformerEncoder(encoder_layer=ts.num_layers, encoder_hidden=ts.hidden, encoder_head=ts.heads, conv_filter_size=ts.ffn,
                                conv_kernel_size=ts.kernel, encoder_dropout=0.1, use_cln=False, cfg=None).eval()
    own = {k: v for k, v in encoder.state_dict().items() if k.startswith("block.")}
    enc_sd = {k: v.half().float() for k, v in P.synthetic_codec_state_dict(spec, seed).items()}
    assert set(enc_sd) == set(own), sorted(set(enc_sd) ^ set(own))
    for k, v in enc_sd.items():
        if k.endswith(".filter"):                                            # the module's own buffers, as a checkpoint carries them
            enc_sd[k] = own[k].clone()
            assert float((own[k].reshape(-1).double() - torch.from_numpy(P.kaiser_sinc_taps())).abs().max()) <= 1e-6
        else:
            assert tuple(v.shape) == tuple(own[k].shape), k
    encoder.load_state_dict(enc_sd, strict=False)
    dec_part = {k: v.half().float() for k, v in timbre.state_dict().items()}
    timbre.load_state_dict(dec_part)
    dec_sd = {f"{P.TIMBRE}.{k}": v for k, v in dec_part.items() if not k.endswith("position_emb.pe")}
    out = {"e." + k: (v.numpy().astype(np.float32) if k.endswith(".filter") else v.numpy().astype(np.float16)) for k, v in enc_sd.items()}
    out.update({"d." + k: v.numpy().astype(np.float16) for k, v in dec_sd.items()})
    out["enc_keys"], out["dec_keys"] = np.array(list(enc_sd.keys())), np.array(list(dec_sd.keys()))
    encoded, rows = [], []
    taps = {}
    hooks = [encoder.block[0].register_forward_hook(lambda m, i, o: taps.__setitem__("conv_in", o))]
    for i in range(1, len(spec.strides) + 1):
        for j in range(3):
            hooks.append(encoder.block[i].block[j].register_forward_hook(lambda m, a, o, key=f"u{i}_{j}": taps.__setitem__(key, o)))
        hooks.append(encoder.block[i].register_forward_hook(lambda m, a, o, key=f"level_{i}": taps.__setitem__(key, o)))
    with torch.no_grad():
        for b, w in enumerate(pg["waves"]):
            y = np.pad(w.astype(np.float32), (0, 200 - len(w) % 200))         # preprocess_ns3_prosody_speaker.py:45
            y = torch.tensor(y).float().unsqueeze(0).unsqueeze(0)
            enc = encoder(y)
            x_timbre = timbre(enc.transpose(1, 2), None, None)                # get_processed_style_speaker_embedding
            T = R.frames(len(w))
            assert tuple(enc.shape) == (1, spec.out_channels, T) and tuple(x_timbre.shape) == (1, T, ts.hidden), (enc.shape, x_timbre.shape)
            peak = float(enc.abs().max())
            print(f"wave {b}: {len(w)} samples, {T} frames, max|encoded| = {peak:.3f}, " +
                  ", ".join(f"{k} {float(v.abs().max()):.2f}" for k, v in taps.items() if k.startswith("level")))
            assert peak >= 1.0, "choose another seed: max|encoded| < 1 on this wave"
            encoded.append(enc[0].T.numpy())
            rows.append(x_timbre[0].numpy())
            if b in LEVELS_OF:
                for k, v in taps.items():
                    if k.startswith("u"):                                     # the units' outputs would take the file past its limit
                        continue
                    out[f"lv{b}.{k}"] = v[0].T.contiguous().numpy().astype(np.float32)
            # the statement agrees with the run it is about to be pinned to
            ref = R.forward(enc_sd, dec_sd, w, ts.heads)
            print(f"    statement vs reference: encoded {R.rel_err(encoded[-1], ref['encoded']):.2e}, timbre {R.rel_err(rows[-1], ref['timbre']):.2e}")
        short = torch.tensor(np.pad(pg["short"], (0, 200 - SHORT % 200))).float()[None, None]
        try:
            encoder.get_prosody_feature(short)
            raise AssertionError("the 399-sample wave went through")
        except RuntimeError as e:
            print(f"{SHORT} samples: {e}")
    for h in hooks:
        h.remove()
    out["encoded"], out["timbre"] = np.concatenate(encoded).astype(np.float32), np.concatenate(rows).astype(np.float32)
    first = {k: v for k, v in out.items() if k.startswith("e.") or k in ("enc_keys", "encoded")}
    for name, part in zip(FILES, (first, {k: v for k, v in out.items() if k not in first})):
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **part)
        size = os.path.getsize(path)
        print(f"wrote {path} ({size} bytes, {len(part)} arrays)")
        assert size < SIZE_LIMIT, "narrow the timbre filter, not the codec"


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else SEED)
