"""GPU: the device heads reading rows in place (engine.RowSource), predictor.FusionPredictor behind Whisper, two audio encoders and three
streams, and predictor.score_from_wav against the route through the extraction drivers' files.

Bit-equal wherever two routes make the same launches; the one float gate is the head's own, as in tests/test_gpu_fusion.py:
device error against float64 <= 2 x (e_ref + e_split), with the float64 statement evaluated on the device's own rows."""
import copy
import os
import wave

import numpy as np
import pytest
import torch

import fusion3_ref as R3
import fusion_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _offs(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _report(what, err, e_ref, e_split):
    print(f"FUSION {what}: error {err:.3e}  e_ref {e_ref:.3e}  e_split {e_split:.3e}  gate {2.0 * (e_ref + e_split):.3e}")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scatter(xs, starts, rows, seed, n=1):
    """n seeded fp32 [rows, D] matrices, on the device at row pitch D + 8 with NaN in the pitch columns; for n = 1 the rows from
    starts[b] on hold xs[b].  Returns (the [rows, D] device views, the host copies)"""
    D = xs[0].shape[1]
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal((rows, D)).astype(np.float32) for _ in range(n)]
    if n == 1:
        for x, s in zip(xs, starts):
            host[0][s:s + len(x)] = x
    views = []
    for h in host:
        t = torch.full((rows, D + 8), float("nan"), dtype=torch.float32, device=DEV)
        t[:, :D] = _dev(h)
        views.append(t[:, :D])
    return views, host


# --------------------------------------------------------------------------------------------------------- RowSource == tensor
@pytest.mark.parametrize("mode", ["f16x", "fp32x", "bf16"])
def test_fusion_head_row_source_equals_the_gathered_tensor(built_library, mode):
    from interspeech_ser_amd.engine import FusionHead, RowSource
    l1, l2 = (1, 37, 12), (5, 16, 9)
    sd, xs1, _ = R.seeded_case(128, 64, l1, 3, h=64)
    xs2 = [np.random.default_rng(40 + i).standard_normal((t, 64)).astype(np.float32) for i, t in enumerate(l2)]
    head = FusionHead(sd, 128, 64, DEV, mode)
    want = head.forward(_dev(np.concatenate(xs1)), _offs(l1), _dev(np.concatenate(xs2)), _offs(l2)).cpu().numpy().copy()
    assert head.status() == (0, 0)
    s1, s2 = (200, 3, 100), (40, 0, 20)                                    # not ascending
    v1, _ = _scatter(xs1, s1, 260, 1)
    v2, _ = _scatter(xs2, s2, 64, 2)
    got = head.forward(RowSource(v1[0], s1), _offs(l1), RowSource(v2, s2), _offs(l2)).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert np.array_equal(_bits(got), _bits(want))
    mixed = head.forward(_dev(np.concatenate(xs1)), _offs(l1), RowSource(v2, s2), _offs(l2)).cpu().numpy()
    assert np.array_equal(_bits(mixed), _bits(want))
    with pytest.raises(ValueError, match="of a 260-row source"):
        head.forward(RowSource(v1[0], (260, 3, 100)), _offs(l1), RowSource(v2, s2), _offs(l2))
    with pytest.raises(ValueError, match="source offsets"):
        head.forward(RowSource(v1[0], s1[:2]), _offs(l1), RowSource(v2, s2), _offs(l2))
    with pytest.raises(ValueError, match="fp32"):
        head.forward(RowSource(v1[0].double(), s1), _offs(l1), RowSource(v2, s2), _offs(l2))
    with pytest.raises(ValueError, match="fp32"):                          # the width of dims_in
        head.forward(RowSource(v2, s2), _offs(l2), RowSource(v2, s2), _offs(l2))
    with pytest.raises(ValueError, match="fp32"):                          # a row pitch that is no multiple of 4
        t = torch.zeros((260, 130), device=DEV)
        head.forward(RowSource(t[:, :128], s1), _offs(l1), RowSource(v2, s2), _offs(l2))
    with pytest.raises(ValueError, match="on cuda:0"):
        head.forward(RowSource(v1[0].cpu(), s1), _offs(l1), RowSource(v2, s2), _offs(l2))


def test_trimodal_head_row_source_with_a_mean_of_four(built_library):
    from interspeech_ser_amd.engine import RowSource, TrimodalHead
    dims, lengths = (64, 128, 64), ((1, 37, 12), (5, 16, 9), (7, 2, 33))
    sd, xs1, xs2, _ = R3.seeded_case(dims, lengths, 4, h=64)
    s3 = (50, 0, 10)
    v3, h3 = _scatter([np.zeros((t, 64), np.float32) for t in lengths[2]], s3, 90, 5, n=4)
    mean = (((h3[0] + h3[1]) + h3[2]) + h3[3]) / np.float32(4)           # float32, mean_last4's order
    xs3 = [mean[s:s + t] for s, t in zip(s3, lengths[2])]
    head = TrimodalHead(sd, *dims, DEV, "f16x")
    cat = lambda xs: _dev(np.concatenate(xs))
    want = head.forward(cat(xs1), _offs(lengths[0]), cat(xs2), _offs(lengths[1]), cat(xs3), _offs(lengths[2])).cpu().numpy().copy()
    assert head.status() == (0, 0)
    s1 = (60, 0, 40)
    v1, _ = _scatter(xs1, s1, 100, 6)
    got = head.forward(RowSource(v1, s1), _offs(lengths[0]), cat(xs2), _offs(lengths[1]), RowSource(v3, s3), _offs(lengths[2])).cpu().numpy()
    assert head.status() == (0, 0)
    assert np.array_equal(_bits(got), _bits(want))
    with pytest.raises(ValueError, match="one state, or four"):
        head.forward(RowSource(v1, s1), _offs(lengths[0]), cat(xs2), _offs(lengths[1]), RowSource(v3[:3], s3), _offs(lengths[2]))


# --------------------------------------------------------------------------------------------------------- the tiny fixtures
@pytest.fixture(scope="module")
def tiny(built_library, golden_dir):
    """the committed Whisper / RoBERTa / HuBERT fixtures' encoders (f16x) and inputs: two utterances"""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import SpeechEncoder, TextEncoder, WhisperEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    from test_gpu_e2e import synth_wave
    gw, gt = np.load(os.path.join(golden_dir, "tiny_whisper_d128h2.npz")), np.load(os.path.join(golden_dir, "tiny_roberta_d128h2.npz"))
    gh = np.load(os.path.join(golden_dir, "tiny_hubert_d320h4.npz"))
    lengths = [int(n) for n in gw["lengths"]]
    assert lengths == [16000, 100000]
    waves = [synth_wave(int(gw[f"wave_seed_{j}"]), n) for j, n in enumerate(lengths)]
    ids = torch.from_numpy(np.stack([gt[f"ids_{j}"] for j in range(2)]))
    mask = torch.from_numpy(np.stack([gt[f"mask_{j}"] for j in range(2)]))
    return dict(gw=gw, gt=gt, waves=waves, ids=ids, mask=mask,
                whisper=WhisperEncoder(C.TINY_WHISPER, synthetic_state_dict(C.TINY_WHISPER, int(gw["seed"])), DEV, mode="f16x"),
                roberta=TextEncoder(C.TINY_ROBERTA, synthetic_state_dict(C.TINY_ROBERTA, int(gt["seed"])), DEV, mode="f16x"),
                hubert=SpeechEncoder(C.TINY_HUBERT, synthetic_state_dict(C.TINY_HUBERT, int(gh["seed"])), DEV, mode="f16x"))


def _per_utterance(rows, offs):
    host = rows.cpu().numpy()
    return [host[a:b].copy() for a, b in zip(offs[:-1], offs[1:])]


def test_whisper_and_roberta_on_the_tiny_fixtures(tiny):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.engine import FusionHead
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, TextStream, gather_rows
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import TOL
    gw, waves, ids, mask = tiny["gw"], tiny["waves"], tiny["ids"], tiny["mask"]
    N = C.TINY_WHISPER.num_layers
    sd = seeded_head_weights(R.head_shapes(128, 128), 31)
    pred = FusionPredictor([AudioStream(tiny["whisper"], state=N), TextStream(tiny["roberta"])], sd)
    assert pred.head.mode_name == "f16x" and isinstance(pred.head, FusionHead)
    got = pred.predict(waves, ids, mask)
    assert got.shape == (2, 8) and got.dtype == np.float32
    (src1, o1, hs1), (src2, o2, hs2) = pred.features(waves, ids, mask)
    # 1. the row counts the head sees: the reference's crop
    assert [b - a for a, b in zip(o1[:-1], o1[1:])] == [int(gw["rows_0"]), int(gw["rows_1"])] == [50, 128]
    assert src1.src_offs == [0, 1500] and o2 == [0, 80, 160]
    # 2. the rows it reads against the HF fixture, at the bound the Whisper fixture test holds the forward to
    xs1, xs2 = _per_utterance(gather_rows(src1, o1), o1), _per_utterance(gather_rows(src2, o2), o2)
    for j in range(2):
        ref = gw[f"states_{j}"][N]
        err = float(np.abs(xs1[j] - ref).max() / max(1.0, float(np.abs(ref).max())))
        print(f"FUSION whisper rows of utterance {j}: {err:.3e} of the fixture's (bound {TOL['f16x']:.0e})")
        assert xs1[j].shape == ref.shape and err < TOL["f16x"]
        assert np.array_equal(_bits(xs1[j]), _bits(hs1.utterance(j, N)[: len(ref)].cpu().numpy()))
    # 3. a head of its own, fed those rows cropped on the host
    head = FusionHead(sd, 128, 128, DEV, "f16x")
    direct = head.forward(_dev(np.concatenate(xs1)), o1, _dev(np.concatenate(xs2)), o2).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert np.array_equal(_bits(direct), _bits(got))
    # 4. the head's own gate, the float64 statement on the device's rows
    ref = R.batch_logits(sd, xs1, xs2)
    e_ref = R.rel_err(R.oracle_logits(sd, xs1, xs2), ref)
    e_split = R.rel_err(R.batch_logits(sd, xs1, xs2, "f16x"), ref)
    err = R.rel_err(got, ref)
    _report("FusionPredictor f16x Whisper + RoBERTa (statement on the device rows)", err, e_ref, e_split)
    assert err <= 2.0 * (e_ref + e_split)
    # 5. behind the crop: the window's other rows never reach the head or its range guard
    hs1.states[N][50:1500] = 7.0e4
    again = head.forward(src1, o1, src2, o2).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert np.array_equal(_bits(again), _bits(got))
    hs1.states[N][49, 3] = 7.0e4                                           # the last row inside the crop does
    head.forward(src1, o1, src2, o2)
    assert head.status()[0] & 1


def test_same_arguments_same_bits_as_the_bimodal_predictor(tiny):
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.bimodal import BimodalPredictor
    from interspeech_ser_amd.engine import SpeechEncoder
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, TextStream
    from interspeech_ser_amd.weights import synthetic_state_dict
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import synth_wave
    sd = seeded_head_weights(R.head_shapes(320, 128, h=64), 31)
    waves = [synth_wave(1, 8000), synth_wave(2, 4000)]
    ids, mask = tiny["ids"], tiny["mask"]
    want = BimodalPredictor(tiny["hubert"], tiny["roberta"], sd, 1).predict(waves, ids, mask)
    got = FusionPredictor([AudioStream(tiny["hubert"], state=1), TextStream(tiny["roberta"])], sd).predict(waves, ids, mask)
    assert np.array_equal(_bits(got), _bits(want))
    neg = FusionPredictor([AudioStream(tiny["hubert"], state=-2), TextStream(tiny["roberta"])], sd).predict(waves, ids, mask)
    assert np.array_equal(_bits(neg), _bits(want))                         # three states: -2 is 1
    geo = C.tiny_geometry(C.FAMILY_HUBERT, hidden=320, heads=4, ffn=384, pos_groups=4, layers=4)
    speech4 = SpeechEncoder(geo, synthetic_state_dict(geo, 3), DEV, mode="f16x")
    want = BimodalPredictor(speech4, tiny["roberta"], sd, 0, use_average=True).predict(waves, ids, mask)
    got = FusionPredictor([AudioStream(speech4, average=True), TextStream(tiny["roberta"])], sd).predict(waves, ids, mask)
    assert np.array_equal(_bits(got), _bits(want))


def test_two_audio_encoders_and_no_text(tiny):
    from interspeech_ser_amd.engine import FusionHead
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, gather_rows
    from oracle.fusion_head import seeded_head_weights
    sd = seeded_head_weights(R.head_shapes(128, 320, h=64), 8)
    waves = [w[:24000] for w in tiny["waves"]]
    waves[0] = waves[0][:9000]
    pred = FusionPredictor([AudioStream(tiny["whisper"]), AudioStream(tiny["hubert"], state=1)], sd)
    got = pred.predict(waves)
    assert got.shape == (2, 8) and np.isfinite(got).all()
    (src1, o1, _), (src2, o2, _) = pred.features(waves)
    assert o1 == [0, 29, 104] and o2[-1] == o2[1] + 74                    # ceil(9000 / 320), ceil(24000 / 320); 24 000 samples -> 74 frames
    x1, x2 = gather_rows(src1, o1), gather_rows(src2, o2)
    head = FusionHead(sd, 128, 320, DEV, "f16x")
    direct = head.forward(x1, o1, x2, o2).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert np.array_equal(_bits(direct), _bits(got))
    for j in range(2):
        assert np.array_equal(_bits(pred.predict(waves[j:j + 1])[0]), _bits(got[j])), j


def test_three_streams(tiny):
    from interspeech_ser_amd.engine import TrimodalHead
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, RowsStream, TextStream, gather_rows
    from oracle.fusion_head import seeded_head_weights
    sd = seeded_head_weights(R3.head_shapes(128, 128, 64, h=64), 9)
    rng = np.random.default_rng(10)
    rows = [rng.standard_normal((7, 64)).astype(np.float32), rng.standard_normal((21, 64, 1)).astype(np.float32)]
    waves, ids, mask = tiny["waves"], tiny["ids"], tiny["mask"]
    pred = FusionPredictor([AudioStream(tiny["whisper"]), TextStream(tiny["roberta"]), RowsStream(64)], sd)
    assert isinstance(pred.head, TrimodalHead) and pred.head.heads == (1, 1, 2)
    got = pred.predict(waves, ids, mask, rows)
    (src1, o1, _), (src2, o2, _), (x3, o3, none) = pred.features(waves, ids, mask, rows)
    assert none is None and o3 == [0, 7, 28] and tuple(x3.shape) == (28, 64)
    head = TrimodalHead(sd, 128, 128, 64, DEV, "f16x")
    direct = head.forward(gather_rows(src1, o1), o1, gather_rows(src2, o2), o2, x3, o3).cpu().numpy().copy()
    assert head.status() == (0, 0)
    assert got.shape == (2, 8) and np.array_equal(_bits(direct), _bits(got))


def test_predictor_refuses_what_it_cannot_run(tiny):
    from interspeech_ser_amd._lib import SerHipError
    from interspeech_ser_amd.predictor import AudioStream, FusionPredictor, RowsStream, TextStream
    from oracle.fusion_head import seeded_head_weights
    sd2 = seeded_head_weights(R.head_shapes(128, 128, h=64), 31)
    sd3 = seeded_head_weights(R3.head_shapes(128, 128, 64, h=64), 9)
    wh, ro, hu = tiny["whisper"], tiny["roberta"], tiny["hubert"]
    with pytest.raises(IndexError, match="tuple index out of range"):
        FusionPredictor([AudioStream(wh, state=3), TextStream(ro)], sd2)
    with pytest.raises(IndexError, match="tuple index out of range"):
        FusionPredictor([AudioStream(wh, state=-4), TextStream(ro)], sd2)
    with pytest.raises(ValueError, match="last four hidden states"):       # two layers: three states
        FusionPredictor([AudioStream(wh, average=True), TextStream(ro)], sd2)
    with pytest.raises(ValueError, match="last four hidden states"):
        FusionPredictor([AudioStream(wh), TextStream(ro, average=True)], sd2)
    elsewhere = copy.copy(ro)
    elsewhere.device = torch.device("cuda:1")
    with pytest.raises(ValueError, match="one device"):
        FusionPredictor([AudioStream(wh), TextStream(elsewhere)], sd2)
    with pytest.raises(ValueError, match="two streams .* or three"):
        FusionPredictor([AudioStream(wh), TextStream(ro), AudioStream(hu), RowsStream(64)], sd3)
    with pytest.raises(ValueError, match="speech_projection.weight has shape"):   # a stream width the state dict contradicts
        FusionPredictor([AudioStream(hu), TextStream(ro)], sd2)
    with pytest.raises(ValueError, match="text encoder"):
        FusionPredictor([AudioStream(wh), TextStream(hu)], sd2)
    pred = FusionPredictor([AudioStream(wh), TextStream(ro), RowsStream(64)], sd3)
    waves, ids, mask = tiny["waves"], tiny["ids"], tiny["mask"]
    with pytest.raises(ValueError, match="needs rows"):
        pred.predict(waves, ids, mask)
    rows = [np.ones((3, 64), np.float32), np.ones((4, 64), np.float32)]
    rows[1][2, 5] = 7.0e4
    with pytest.raises(SerHipError, match="fp16 operand range"):
        pred.predict(waves, ids, mask, rows)
    rows[1][2, 5] = 1.0
    assert np.isfinite(pred.predict(waves, ids, mask, rows)).all()


# --------------------------------------------------------------------------------------------------------- score_from_wav on files
def _write_wav(path, x):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(16000)
        f.writeframes(np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype("<i2").tobytes())


def test_score_from_wav_equals_the_route_through_feature_files(built_library, tmp_path, capsys):
    import pandas as pd
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd import driver
    from interspeech_ser_amd import head as HD
    from interspeech_ser_amd.predictor import score_from_wav
    from oracle.fusion_head import seeded_head_weights
    from test_gpu_e2e import synth_wave
    geo = C.TINY_ROBERTA
    max_len = 16
    wav_dir, lazy1, lazy2 = tmp_path / "Audios", tmp_path / "whisper", tmp_path / "roberta"
    wav_dir.mkdir()
    seconds = (0.3, 2.0, 0.71, 1.2, 0.5)
    names = [f"MSP-PODCAST_{i:04d}.wav" for i in range(len(seconds))]
    for i, (name, s) in enumerate(zip(names, seconds)):
        _write_wav(wav_dir / name, synth_wave(20 + i, int(16000 * s)))
    listed = names[:3] + ["MSP-PODCAST_9999.wav"] + names[3:]              # a sixth name, with a transcript and no wav file
    texts = ["hello there", "a much longer sentence with several more words in it", "ok", "nobody recorded this", "one two three", "yes no"]
    pd.DataFrame({"FileName": listed, "transcription": texts}).to_csv(tmp_path / "text.csv", index=False)
    pd.DataFrame({"FileName": listed}).to_csv(tmp_path / "test.csv", index=False)

    def fake_tokenize(batch):
        ids = torch.full((len(batch), max_len), geo.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((len(batch), max_len), dtype=torch.int64)
        for i, t in enumerate(batch):
            toks = ([0] + [3 + (len(w) * 7 + j) % (geo.vocab_size - 4) for j, w in enumerate(t.split())])[: max_len - 1] + [2]
            ids[i, : len(toks)] = torch.tensor(toks)
            mask[i, : len(toks)] = 1
        return ids, mask

    sd = seeded_head_weights(R.head_shapes(128, 128, h=64), 31)
    cfgs = []
    for tag in ("files", "wav"):
        cfg = {"wav_dir": str(wav_dir), "txt_dir": str(tmp_path / "text.csv"), "lazy_dir1": str(lazy1), "lazy_dir2": str(lazy2),
               "feat1_dim": 128, "feat2_dim": 128, "model_path": str(tmp_path / f"exp_{tag}")}
        os.makedirs(cfg["model_path"])
        torch.save(sd, os.path.join(cfg["model_path"], "multimodal_ser.pt"))
        cfgs.append(cfg)
    C._REGISTRY["tiny-whisper-from-wav"], C._REGISTRY["tiny-roberta-from-wav"] = C.TINY_WHISPER, geo
    try:
        assert driver.run_whisper(["--ssl_type", "tiny-whisper-from-wav", "--wav_dir", str(wav_dir), "--save_path", str(lazy1),
                                   "--synthetic_weights", "--mode", "f16x", "--batch_size", "16"]) == 0
        assert driver.run_roberta(["--roberta_type", "tiny-roberta-from-wav", "--df_path", str(tmp_path / "text.csv"), "--save_path", str(lazy2),
                                   "--synthetic_weights", "--mode", "f16x", "--max_len", str(max_len), "--batch_size", "16"],
                                  tokenize=fake_tokenize) == 0
        capsys.readouterr()
        a = HD.score(cfgs[0], engine="hip", mode="f16x", test_csv=str(tmp_path / "test.csv"))
        log_a = capsys.readouterr().out
        b = score_from_wav(cfgs[1], ["tiny-whisper-from-wav", "tiny-roberta-from-wav"], test_csv=str(tmp_path / "test.csv"), mode="f16x",
                           text_mode="f16x", head_mode="f16x", batch_size=16, max_len=max_len, synthetic_weights=True, tokenize=fake_tokenize)
        log_b = capsys.readouterr().out
    finally:
        C._REGISTRY.pop("tiny-whisper-from-wav")
        C._REGISTRY.pop("tiny-roberta-from-wav")
    for res, log in ((a, log_a), (b, log_b)):
        assert res["n"] == 5 and res["failed"] == 1, log
        assert log.count("Failed to process") == 1 and "Failed to process MSP-PODCAST_9999.wav" in log, log
        assert "5 rows written, 1 files failed" in log, log
    with open(a["csv"], "rb") as f:
        by_files = f.read()
    with open(b["csv"], "rb") as f:
        from_wav = f.read()
    assert from_wav == by_files
    lines = from_wav.decode().splitlines()
    assert lines[0].split(",") == ["FileName", "Prediction"] + [f"class_{i}_prob" for i in range(8)]
    assert [ln.split(",")[0] for ln in lines[1:]] == names and all(ln.split(",")[1] in HD.CLASS_LETTERS for ln in lines[1:])
