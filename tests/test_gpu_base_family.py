"""-m gpu: the *-base speech encoders (GroupNorm-over-time conv stem, post-LayerNorm encoder layers): wavlm-base, wav2vec2-base,
hubert-base.  The stem's statistics kernel against fp64 torch, batch independence, the HF fixtures end to end in every supported
mode, the drivers at full geometry against tests/base_oracle.py, command-list replay and the fp16 range guard."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import base_oracle as BO

pytestmark = pytest.mark.gpu

TOL = {"f16x": 2e-5, "fp32x": 1e-3, "bf16": 3e-2}        # tests/test_gpu_e2e.py's gates
CASES = (("tiny_wavlm_base_d128h2", "TINY_WAVLM_BASE"), ("tiny_wav2vec2_base_d128h2", "TINY_WAV2VEC2_BASE"),
         ("tiny_hubert_base_d128h2", "TINY_HUBERT_BASE"))


def synth_wave(seed, n):               # tools/make_golden_base.py's recipe
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.05 + 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def rel_err(got, ref):
    return float((got - ref).abs().max() / max(1.0, float(ref.abs().max())))


def write_wav(path, x):
    pcm = (np.clip(x, -1, 1) * 32767).astype("<i2")
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / 32768.0


def _stem_geo():
    from interspeech_ser_amd import config as C
    return C.tiny_geometry(C.FAMILY_WAVLM, hidden=128, heads=2, ffn=256, conv_dim=512, layers=1, base=True)


def _gn_stats(enc, lengths):
    """Re-launch ser_gn_stats_v over the slot's last batch with stat_out: per-(utterance, channel) (mean, rstd) [B, C, 2]."""
    from interspeech_ser_amd import _lib
    pl = enc._plan(lengths, 0)
    B, C0 = len(lengths), enc.geo.conv_dim[0]
    out = torch.zeros((B, C0, 2), dtype=torch.float32, device=enc.device)
    a = _lib.GnStatsArgs()
    a.wav, a.sample_offs, a.frame_offs = enc._last_wave.data_ptr(), pl["sample_offs"].data_ptr(), pl["frame_offs0"].data_ptr()
    a.w, a.bias, a.gamma, a.beta = enc.conv0_w.data_ptr(), None, enc.gn0[0].data_ptr(), enc.gn0[1].data_ptr()
    a.wave_stats, a.scale, a.shift, a.stat_out, a.work = (pl["wave_work"].data_ptr(), pl["gn_scale"].data_ptr(), pl["gn_shift"].data_ptr(),
                                                          out.data_ptr(), pl["gn_work"].data_ptr())
    a.B, a.C, a.k, a.stride, a.ld, a.no_norm, a.eps = B, C0, 10, 5, C0, 0 if enc.normalize else 1, 1e-5
    _lib.check(_lib.lib.ser_gn_stats_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "ser_gn_stats_v")
    torch.cuda.synchronize()
    return out.cpu()


def _stem_forward(enc, waves):
    """conv layer 0's output (layer 1's operand planes) for a ragged batch: the stem of a forward, then conv 0 once more on its own --
    conv layers 2 and 4 reuse that buffer (ping-pong)"""
    lengths = [len(w) for w in waves]
    enc.use_tape = False
    enc._last_wave = enc.upload(waves)
    enc.forward(enc._last_wave, lengths, last_state=0)
    pl = enc._plan(lengths, 0)
    enc._st = torch.cuda.current_stream().cuda_stream
    enc._guard_word(pl)
    try:
        enc._groupnorm_stem(pl, enc._last_wave)
    finally:
        enc._st = None
    torch.cuda.synchronize()
    return pl, pl["conv_act"][0].float()[: pl["rows"][0]].cpu()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_groupnorm_stem_statistics_and_output(mode, normalize):
    """Ragged batch (0.03 s / 1 s / 3.3 s / 10 s), C = 512: the statistics from frame moments match fp64 torch's GroupNorm statistics
    of the conv output to 1e-6 relative, and layer 1's operand input (GELU of the normalised conv 0) is right to the mode's rounding."""
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = _stem_geo()
    sd = synthetic_state_dict(geo, 5)
    waves = [synth_wave(300 + i, n) for i, n in enumerate((480, 16000, 52800, 160000))]
    enc = SpeechEncoder(geo, sd, "cuda:0", mode=mode, normalize=normalize)
    pl, act = _stem_forward(enc, waves)
    st = _gn_stats(enc, [len(w) for w in waves])
    w0 = sd["feature_extractor.conv_layers.0.conv.weight"].double()
    g, b = sd["feature_extractor.conv_layers.0.layer_norm.weight"].double(), sd["feature_extractor.conv_layers.0.layer_norm.bias"].double()
    worst_act = 0.0
    for j, wv in enumerate(waves):
        x = torch.from_numpy(wv).double()
        if normalize:
            x = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
        mean, rstd = BO.conv0_groupnorm_stats(geo, {"feature_extractor.conv_layers.0.conv.weight": w0}, x)
        got_mean, got_rstd = st[j, :, 0].double(), st[j, :, 1].double()
        assert float(((got_rstd - rstd) / rstd).abs().max()) < 1e-6, j
        assert float(((got_mean - mean) * rstd).abs().max()) < 1e-6, j          # relative to the channel's spread
        y = F.conv1d(x[None, None], w0, stride=5)[0]
        ref = F.gelu(F.group_norm(y[None], y.shape[0], g, b, eps=1e-5)[0]).T.float()
        r0, r1 = int(np.sum([geo.frame_chain(len(v))[0] for v in waves[:j]])), int(np.sum([geo.frame_chain(len(v))[0] for v in waves[: j + 1]]))
        worst_act = max(worst_act, rel_err(act[r0:r1], ref))
    assert worst_act < {"f16x": 1e-5, "fp32x": 1e-4, "bf16": 1e-2}[mode], worst_act


def test_groupnorm_stem_is_batch_independent():
    """Each utterance's stem output is bit-equal between the ragged batch and its own batch-of-one launch."""
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = _stem_geo()
    sd = synthetic_state_dict(geo, 6)
    waves = [synth_wave(400 + i, n) for i, n in enumerate((480, 16000, 52800, 160000))]
    enc = SpeechEncoder(geo, sd, "cuda:0", mode="f16x")
    _, act = _stem_forward(enc, waves)
    r0 = 0
    for wv in waves:
        enc1 = SpeechEncoder(geo, sd, "cuda:0", mode="f16x")
        _, one = _stem_forward(enc1, [wv])
        assert torch.equal(act[r0: r0 + one.shape[0]], one)
        r0 += one.shape[0]


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_base_fixtures_end_to_end(golden_dir, mode, case):
    """The three fixture utterances in ONE ragged batch reproduce HF's batch-of-one states (every hidden state, the e2e gates)."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict, state_dict_digest
    tag, gname = CASES[case]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    sd = synthetic_state_dict(geo, int(gold["seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    lengths = [int(n) for n in gold["lengths"]]
    waves = [synth_wave(int(gold[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
    enc = SpeechEncoder(geo, sd, "cuda:0", mode=mode)
    hs = enc.forward(enc.upload(waves), lengths)
    torch.cuda.synchronize()
    assert hs.take_range_bits() & 1 == 0
    worst = 0.0
    for j, n in enumerate(lengths):
        ref = torch.from_numpy(gold[f"states_{j}"])
        assert hs.frames(j) == ref.shape[1] == geo.frames_for(n)
        for layer in range(ref.shape[0]):
            worst = max(worst, rel_err(hs.utterance(j, layer).cpu(), ref[layer]))
    print(f"{tag} {mode}: worst rel err {worst:.3e}")
    assert worst < TOL[mode], worst


def test_unsupported_modes_are_refused():
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(C.TINY_WAVLM_BASE, 1)
    for mode in ("f16mf", "f16m", "f16a", "f16q", "f16"):
        with pytest.raises(ValueError):
            SpeechEncoder(C.TINY_WAVLM_BASE, sd, "cuda:0", mode=mode)


@pytest.mark.parametrize("case", [0, 1, 2])
def test_command_list_replay_equals_eager(case):
    """The recorded command list (GN statistics op included, sizes patched per batch) equals the launch-by-launch forward bit for
    bit, for two batches of different shapes; early exit stops after states[N]."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, CASES[case][1])
    sd = synthetic_state_dict(geo, 9)
    enc = SpeechEncoder(geo, sd, "cuda:0", mode="f16x")
    for lens in ((16000, 7000, 24000), (9000, 400 + 5 * 3)):
        waves = [synth_wave(500 + i, n) for i, n in enumerate(lens)]
        dev = enc.upload(waves)
        enc.use_tape = False
        ref = enc.forward(dev, list(lens)).states.clone()
        enc.use_tape = True
        enc.forward(dev, list(lens))                 # records on the first call (the arena's tape), replays afterwards
        got = enc.forward(dev, list(lens)).states.clone()
        assert torch.equal(got, ref)
        for n in range(geo.num_layers + 1):
            for use_tape in (True, False):
                enc.use_tape = use_tape
                hs = enc.forward(dev, list(lens), last_state=n)
                assert torch.equal(hs.states[: n + 1], ref[: n + 1]), (n, use_tape)


def _driver_case(tmp_path, capsys, ssl_type, geo, lengths, n_check):
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.weights import synthetic_state_dict
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    waves = {}
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        waves[f"u{i:03d}"] = write_wav(wav_dir / f"u{i:03d}.wav", synth_wave(700 + i, n) * float(rng.uniform(0.5, 2.0)))
    sd = synthetic_state_dict(geo, 7)                                    # the driver's --seed default
    check = list(waves)[:: max(1, len(waves) // n_check)][:n_check]
    refs = {}
    with torch.no_grad():
        for name in check:
            refs[name] = BO.hidden_states(geo, sd, torch.from_numpy(BO.normalize_wave(waves[name])))
    # fresh directory, default mode: hidden_states[0] (the reference's rule) and the f16x fallback line
    out0 = tmp_path / "h0"
    assert driver.run_speech(["--ssl_type", ssl_type, "--wav_dir", str(wav_dir), "--save_path", str(out0), "--synthetic_weights"]) == 0
    log = capsys.readouterr().out
    assert "is not implemented for post-LayerNorm encoders" in log and "using f16x" in log, log
    assert "Layer rule: hidden_states[0]" in log and len(os.listdir(out0)) == len(lengths)
    out1 = tmp_path / "last"
    assert driver.run_speech(["--ssl_type", ssl_type, "--wav_dir", str(wav_dir), "--save_path", str(out1), "--synthetic_weights",
                              "--use_n_layer", "--n_layer", "-1", "--mode", "f16x"]) == 0
    out2 = tmp_path / "avg"
    assert driver.run_speech(["--ssl_type", ssl_type, "--wav_dir", str(wav_dir), "--save_path", str(out2), "--synthetic_weights",
                              "--use_average", "y", "--mode", "f16x"]) == 0
    capsys.readouterr()
    for name in check:
        r = refs[name]
        for d, ref in ((out0, r[0]), (out1, r[-1]), (out2, torch.stack(r[-4:]).mean(0))):
            got = torch.load(d / f"{name}.pt")
            assert tuple(got.shape) == (geo.frames_for(len(waves[name])), geo.hidden)
            assert rel_err(got, ref) < 1e-3, (d, name)


def test_wavlm_base_driver_full_geometry(tmp_path, capsys):
    """preprocess_speech.py --ssl_type microsoft/wavlm-base --synthetic_weights on 16 ragged 3-10 s files."""
    from interspeech_ser_amd import config as C
    lengths = [int(x) for x in np.linspace(48000, 160000, 16)]
    _driver_case(tmp_path, capsys, "microsoft/wavlm-base", C.WAVLM_BASE, lengths, 3)


@pytest.mark.parametrize("ssl_type", ["facebook/wav2vec2-base", "facebook/hubert-base-ls960"])
def test_wav2vec2_and_hubert_base_driver(tmp_path, capsys, ssl_type):
    from interspeech_ser_amd import config as C
    _driver_case(tmp_path, capsys, ssl_type, C.geometry_for(ssl_type), [24000, 31000, 40000, 17000], 2)


def test_range_guard_sees_the_groupnorm_affine(tmp_path, capsys):
    """An fp16-range overflow planted in the GroupNorm affine (conv 0's epilogue writes layer 1's fp16 planes) fails the batch's files
    with the existing message in f16x; fp32x extracts them."""
    from safetensors.torch import save_file
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = C.TINY_WAVLM_BASE
    sd = synthetic_state_dict(geo, 41)
    sd["feature_extractor.conv_layers.0.layer_norm.bias"][3] = 1.0e6
    ck = tmp_path / "huge.safetensors"
    save_file({k: v.contiguous() for k, v in sd.items()}, str(ck))
    wav_dir = tmp_path / "wav"
    wav_dir.mkdir()
    for i, n in enumerate((16000, 9000, 12000)):
        write_wav(wav_dir / f"u{i}.wav", synth_wave(80 + i, n))
    C._REGISTRY["tiny-base-range-test"] = geo
    try:
        out = tmp_path / "pt_f16x"
        assert driver.run_speech(["--ssl_type", "tiny-base-range-test", "--wav_dir", str(wav_dir), "--save_path", str(out),
                                  "--checkpoint", str(ck), "--mode", "f16x", "--use_n_layer", "--n_layer", "-1"]) == 0
        log = capsys.readouterr().out
        assert log.count("Failed to process") == 3 and "fp16 operand range" in log and "--mode fp32x" in log, log
        assert os.listdir(out) == []
        out2 = tmp_path / "pt_fp32x"
        assert driver.run_speech(["--ssl_type", "tiny-base-range-test", "--wav_dir", str(wav_dir), "--save_path", str(out2),
                                  "--checkpoint", str(ck), "--mode", "fp32x", "--use_n_layer", "--n_layer", "-1"]) == 0
        assert len(os.listdir(out2)) == 3
    finally:
        C._REGISTRY.pop("tiny-base-range-test")
