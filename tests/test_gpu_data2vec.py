"""-m gpu: the data2vec-audio speech encoders (layer-norm conv stem, post-LayerNorm encoder, a stack of LayerNorm'd positional convs).
ser_pos_ln_v against a float64 statement in both forms, its fp16 range guard, the HF fixtures end to end in every supported mode, the
exactness of batching / command-list replay / concurrent graph capture, and the speech driver at full geometry against
tests/data2vec_oracle.py."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import data2vec_oracle as DO

pytestmark = pytest.mark.gpu

TOL = {"f16x": 1e-3, "fp32x": 1e-3, "bf16": 3e-2}        # tests/test_gpu_e2e.py's gates
CASES = (("tiny_data2vec_audio_d128h2", "TINY_DATA2VEC_AUDIO"), ("tiny_data2vec_audio_d192h3g48", "TINY_DATA2VEC_AUDIO_G48"))
HALF = 9                                                 # halo rows between utterances: conv_pos_kernel_size 19 // 2


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


# ------------------------------------------------------------------------------------------------ ser_pos_ln_v
def _mode(name):
    from interspeech_ser_amd import _lib
    return {"bf16": (_lib.MODE_BF16, 1, torch.bfloat16), "fp32x": (_lib.MODE_FP32X, 2, torch.bfloat16),
            "f16x": (_lib.MODE_FP16X, 2, torch.float16)}[name]


def _halo_map(frames):
    """row m of the packed batch -> its row in the zero-halo'd layout [9 zero rows][utt 0][9 zero rows][utt 1] ... [9 zero rows];
    also the layout's row count"""
    rows, first = [], 0
    for b, t in enumerate(frames):
        rows += [HALF * (b + 1) + first + i for i in range(t)]
        first += t
    return torch.tensor(rows, dtype=torch.int32), first + HALF * (len(frames) + 1)


def _run_pos_ln(x, rows, D, mode, *, out, rowmap=None, residual=None, g=None, b=None, out_f32=None, flag=None):
    from interspeech_ser_amd import _lib
    a = _lib.PosLnArgs()
    a.x, a.ldx = x.data_ptr(), D
    a.out_act, a.ldo_act, a.out_plane_stride = out.data_ptr(), D, out.shape[1] * D
    a.out_rowmap = None if rowmap is None else rowmap.data_ptr()
    last = residual is not None
    a.residual, a.ldr = (residual.data_ptr(), D) if last else (None, 0)
    a.g, a.b = (g.data_ptr(), b.data_ptr()) if last else (None, None)
    a.out_f32, a.ldo_f32 = (out_f32.data_ptr(), D) if last else (None, 0)
    a.eps_pos, a.eps, a.last, a.mode, a.rows, a.D = 1e-5, 1e-5, int(last), mode, rows, D
    a.range_flag = None if flag is None else flag.data_ptr()
    _lib.check(_lib.lib.ser_pos_ln_v(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "ser_pos_ln_v")
    torch.cuda.synchronize()


def _ref_inner(x64):
    return F.gelu(F.layer_norm(x64, (x64.shape[1],), eps=1e-5))


def _ref_last(x64, r64, g64, b64):
    t = _ref_inner(x64) + r64
    return F.layer_norm(t, (t.shape[1],), g64, b64, eps=1e-5)


def _planes(out):
    return out.double().sum(dim=0).cpu()


def _inputs(D, frames, seed):
    gen = torch.Generator().manual_seed(seed)
    M = sum(frames)
    # rows of a conv output with a large mean (the reason for the two-pass statistics) and a spread that varies per row
    x = (3.0 * torch.randn(M, D, generator=gen) * torch.rand(M, 1, generator=gen) + 0.2 + 40.0 * torch.randn(M, 1, generator=gen))
    r = 2.0 * torch.randn(M, D, generator=gen) + 5.0
    g = 1.0 + 0.3 * torch.randn(D, generator=gen)
    b = 0.2 * torch.randn(D, generator=gen)
    return x.float(), r.float(), g.float(), b.float()


@pytest.mark.parametrize("D", [192, 1024])
@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
def test_pos_ln_intermediate_form(mode, D):
    """gelu(LN(x)) of every row lands at its halo'd row in the mode's planes; every halo row (and the spare row) stays zero."""
    code, planes, dt = _mode(mode)
    frames = [1, 37, 120, 5]                                                       # ragged, with a 1-frame utterance
    x, _, _, _ = _inputs(D, frames, 1 + D)
    rowmap, halo_rows = _halo_map(frames)
    out = torch.zeros((planes, halo_rows + 1, D), dtype=dt, device="cuda")
    _run_pos_ln(x.cuda(), len(rowmap), D, code, out=out, rowmap=rowmap.cuda())
    got = _planes(out)
    ref = _ref_inner(x.double())
    inner = torch.zeros(halo_rows + 1, dtype=torch.bool)
    inner[rowmap.long()] = True
    assert int(inner.sum()) == sum(frames)
    assert torch.count_nonzero(out[:, ~inner.cuda()]) == 0, "a halo row was written"
    err = rel_err(got[rowmap.long()], ref)
    assert err < {"bf16": 4e-3, "fp32x": 2e-5, "f16x": 2e-5}[mode], err


@pytest.mark.parametrize("D", [192, 1024])
@pytest.mark.parametrize("mode", ["bf16", "fp32x", "f16x"])
def test_pos_ln_last_form(mode, D):
    """LN(gelu(LN(x)) + residual) * g + b: fp32 state and its operand copy at row m."""
    code, planes, dt = _mode(mode)
    frames = [1, 37, 120, 5]
    M = sum(frames)
    x, r, g, b = _inputs(D, frames, 2 + D)
    out = torch.zeros((planes, M, D), dtype=dt, device="cuda")
    of = torch.full((M, D), float("nan"), dtype=torch.float32, device="cuda")
    _run_pos_ln(x.cuda(), M, D, code, out=out, residual=r.cuda(), g=g.cuda(), b=b.cuda(), out_f32=of)
    ref = _ref_last(x.double(), r.double(), g.double(), b.double())
    assert rel_err(of.double().cpu(), ref) < 2e-5
    err = rel_err(_planes(out), ref)
    assert err < {"bf16": 4e-3, "fp32x": 2e-5, "f16x": 2e-5}[mode], err


def _expected_bits(stored64):
    a = stored64.abs()
    if bool(torch.isnan(a).any()) or float(a.max()) > 65504.0:
        return 3
    return 2 if float(a.max()) > 32752.0 else 0


# the intermediate form has no affine and no residual: its values are bounded by sqrt(D), so only a NaN can trip it
@pytest.mark.parametrize("last,plant", [(False, "none"), (False, "nan_x"), (False, "unread_nan"), (True, "none"), (True, "nan_x"),
                                        (True, "half_b"), (True, "over_b"), (True, "nan_residual"), (True, "unread_nan")])
def test_pos_ln_range_guard(last, plant):
    """f16x: the guard word gets the bits a float64 statement of the STORED values requires (a NaN counts, a value in a row past
    ``rows`` does not); a run with a NULL flag stores the same bytes."""
    code, planes, dt = _mode("f16x")
    D, frames = 192, [1, 7, 30]
    M = sum(frames)
    x, r, g, b = _inputs(D, frames, 7)
    x = torch.cat([x, torch.zeros(4, D)], 0)                                       # 4 rows the launch must not read
    if plant == "nan_x":
        x[3, 17] = float("nan")
    elif plant == "unread_nan":
        x[M + 1, 5] = float("nan")
    elif plant == "half_b":
        b[11] = 40000.0
    elif plant == "over_b":
        b[11] = 1.0e5
    elif plant == "nan_residual":
        r[8, 2] = float("nan")
    xs = x[:M].double()
    if last:
        ref = _ref_last(xs, r.double(), g.double(), b.double())
        rowmap, rows_out = None, M
    else:
        ref = _ref_inner(xs)
        rowmap, rows_out = _halo_map(frames)
    outs = []
    for with_flag in (True, False):
        out = torch.zeros((planes, rows_out + 1, D), dtype=dt, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda") if with_flag else None
        kw = dict(residual=r.cuda(), g=g.cuda(), b=b.cuda(), out_f32=torch.empty((M, D), device="cuda")) if last else \
            dict(rowmap=rowmap.cuda())
        _run_pos_ln(x.cuda(), M, D, code, out=out, flag=flag, **kw)
        outs.append(out.view(torch.int16).cpu())
        if with_flag:
            assert int(flag.item()) == _expected_bits(ref), (plant, int(flag.item()))
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ end to end
def _fixture(golden_dir, case):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict, state_dict_digest
    tag, gname = CASES[case]
    geo = getattr(C, gname)
    gold = np.load(os.path.join(golden_dir, tag + ".npz"))
    sd = synthetic_state_dict(geo, int(gold["seed"]))
    assert state_dict_digest(sd) == str(gold["digest"])
    lengths = [int(n) for n in gold["lengths"]]
    waves = [DO.synth_wave(int(gold[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
    return geo, sd, gold, lengths, waves


@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
@pytest.mark.parametrize("case", [0, 1])
def test_data2vec_fixtures_end_to_end(golden_dir, mode, case):
    """The three fixture utterances in ONE ragged batch reproduce HF's batch-of-one states (every hidden state, the e2e gates)."""
    from interspeech_ser_amd.engine import SpeechEncoder
    geo, sd, gold, lengths, waves = _fixture(golden_dir, case)
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
    print(f"{CASES[case][0]} {mode}: worst rel err {worst:.3e}")
    assert worst < TOL[mode], worst


@pytest.mark.parametrize("mode", ["fp32x", "f16x"])
def test_batched_equals_batch_of_one(mode):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = C.TINY_DATA2VEC_AUDIO_G48
    sd = synthetic_state_dict(geo, 12)
    lengths = [4000, 16000, 401, 9000]                                            # 401 samples: one frame
    waves = [DO.synth_wave(60 + i, n) for i, n in enumerate(lengths)]
    enc = SpeechEncoder(geo, sd, "cuda:0", mode=mode)
    hs = enc.forward(enc.upload(waves), lengths)
    batched = [[hs.utterance(b, l).cpu().clone() for l in range(len(hs))] for b in range(len(waves))]
    assert hs.frames(2) == 1
    for b, w in enumerate(waves):
        one = enc.forward(enc.upload([w]), [len(w)])
        for l in range(len(one)):
            assert torch.equal(one.utterance(0, l).cpu(), batched[b][l]), (b, l)


@pytest.mark.parametrize("case", [0, 1])
def test_command_list_replay_equals_eager(case):
    """The recorded command list (ser_pos_ln_v entries included, rows patched per batch) equals the launch-by-launch forward bit for
    bit, for two batches of different shapes, and every early exit stops after states[N]."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = getattr(C, CASES[case][1])
    sd = synthetic_state_dict(geo, 9)
    enc = SpeechEncoder(geo, sd, "cuda:0", mode="f16x")
    for lens in ((16000, 7000, 24000), (9000, 400 + 5 * 3)):
        waves = [DO.synth_wave(500 + i, n) for i, n in enumerate(lens)]
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
    tape = enc.recorded_tape(list(lens), 0)
    from interspeech_ser_amd import _lib
    assert sum(tape.cmds[i].op == _lib.OP_POS_LN for i in range(tape.n)) == geo.pos_conv_layers


def test_concurrent_capture_replays_the_eager_forward():
    """Two utterance groups captured as parallel branches of one hipGraph, replayed twice, equal the eager forward bit for bit."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    geo = C.TINY_DATA2VEC_AUDIO_G48
    sd = synthetic_state_dict(geo, 13)
    enc = SpeechEncoder(geo, sd, "cuda:0", mode="f16x")
    spans = ([12000, 30000, 500], [22000, 8000])
    groups = [(enc.upload([DO.synth_wave(900 + 10 * s + i, n) for i, n in enumerate(lens)], slot=s), list(lens))
              for s, lens in enumerate(spans)]
    torch.cuda.synchronize()
    graph, hs = enc.capture_concurrent(groups)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    kept = [h.states.clone() for h in hs]
    eager = [enc.forward(w, l, slot=s) for s, (w, l) in enumerate(groups)]
    torch.cuda.synchronize()
    for k, e, h in zip(kept, eager, hs):
        assert e.frame_offs == h.frame_offs
        assert torch.equal(k, e.states)


def test_unsupported_modes_are_refused():
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(C.TINY_DATA2VEC_AUDIO, 1)
    for mode in ("f16mf", "f16m", "f16a", "f16q", "f16"):
        with pytest.raises(ValueError):
            SpeechEncoder(C.TINY_DATA2VEC_AUDIO, sd, "cuda:0", mode=mode)


def test_data2vec_audio_large_driver_full_geometry(tmp_path, capsys):
    """preprocess_speech.py --ssl_type facebook/data2vec-audio-large --synthetic_weights on 16 ragged 3-10 s files."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd.weights import synthetic_state_dict
    ssl_type, geo = "facebook/data2vec-audio-large", C.DATA2VEC_AUDIO_LARGE
    lengths = [int(x) for x in np.linspace(48000, 160000, 16)]
    wav_dir = tmp_path / "wavs"
    wav_dir.mkdir()
    waves = {}
    rng = np.random.default_rng(3)
    for i, n in enumerate(lengths):
        waves[f"u{i:03d}"] = write_wav(wav_dir / f"u{i:03d}.wav", DO.synth_wave(700 + i, n) * float(rng.uniform(0.5, 2.0)))
    sd = synthetic_state_dict(geo, 7)                                    # the driver's --seed default
    check = list(waves)[::6][:3]
    refs = {}
    with torch.no_grad():
        for name in check:
            refs[name] = DO.hidden_states(geo, sd, torch.from_numpy(DO.normalize_wave(waves[name])))
    del sd
    out0 = tmp_path / "h0"
    assert driver.run_speech(["--ssl_type", ssl_type, "--wav_dir", str(wav_dir), "--save_path", str(out0), "--synthetic_weights"]) == 0
    log = capsys.readouterr().out
    assert "is not implemented for post-LayerNorm encoders" in log and "using f16x" in log, log
    assert "Layer rule: hidden_states[0]" in log and len(os.listdir(out0)) == len(lengths)
    for name, x in waves.items():
        assert tuple(torch.load(out0 / f"{name}.pt").shape) == (geo.frames_for(len(x)), geo.hidden)
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
            assert rel_err(got, ref) < 1e-3, (d, name, rel_err(got, ref))


def test_fp16_modes_refuse_an_oversized_positional_weight():
    """Weight loading checks every positional conv of the stack like any other weight (weights.check_f16_weight): f16x names the
    tensor it refuses, fp32x (bf16 planes, fp32 range) loads it."""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    sd = synthetic_state_dict(C.TINY_DATA2VEC_AUDIO, 4)
    sd["encoder.pos_conv_embed.layers.3.conv.weight"][5, 2, 7] = 1.0e5
    with pytest.raises(ValueError, match=r"encoder\.pos_conv_embed\.layers\.3\.conv\.weight"):
        SpeechEncoder(C.TINY_DATA2VEC_AUDIO, sd, "cuda:0", mode="f16x")
    SpeechEncoder(C.TINY_DATA2VEC_AUDIO, sd, "cuda:0", mode="fp32x")
