"""CPU: the x-vector head around its kernels -- the float64 statement against HF, HF's masked branch at batch size 1, the config and
weight plumbing, the per-layer offset tables, the launchers' refusals (validation comes before any launch) and the command line with a
stub in place of the model."""
import csv
import ctypes
import json
import wave

import numpy as np
import pytest
import torch

import xvector_ref as R
from interspeech_ser_amd import classify as CL
from interspeech_ser_amd import config as C
from interspeech_ser_amd import weights as W
from interspeech_ser_amd import xvector as XV


@pytest.fixture(scope="module", params=R.FIXTURES)
def fx(request):
    return R.Fixture(request.param)


# ------------------------------------------------------------------------------- the statement
def test_statement_reproduces_hf_float64(fx):
    """tests/xvector_ref.py on the fixture's float64 hidden states gives HF's float64 embeddings and logits to 1e-10 (measured when the
    fixtures were made: <= 6.3e-16), on every waveform that has an output; the T' = 1 waveform has none"""
    assert fx.one not in fx.emb64 and len(fx.good) == 5
    for j in fx.good:
        emb, logits = fx.outputs(j)
        assert emb.shape == fx.emb64[j].shape == (fx.spec().xvector_output_dim,)
        assert np.abs(emb - fx.emb64[j]).max() <= 1e-10 * np.abs(fx.emb64[j]).max(), (fx.name, j)
        assert np.abs(logits - fx.logits64[j]).max() <= 1e-10 * np.abs(fx.logits64[j]).max(), (fx.name, j)


def test_fixture_waves_have_the_row_counts_they_are_named_for(fx):
    geo, spec = fx.geometry(), fx.spec()
    assert geo.frames_for(fx.lengths[fx.two]) - spec.context == 2 and geo.frames_for(fx.lengths[fx.one]) - spec.context == 1
    assert fx.states64[fx.two].shape[1] == spec.min_frames
    assert all(geo.frames_for(fx.lengths[j]) == fx.states64[j].shape[1] for j in fx.good)


def test_hf_masked_branch_equals_unmasked_at_batch_size_one():
    """The batch-1 claim: HF's masked branch slices by _get_tdnn_output_lengths, which ignores the dilation (T - sum(k - 1) > T'), so at
    batch size 1 the slice clamps to all T' rows and an all-ones attention_mask changes nothing (layer-norm stem: the mask reaches the
    encoder too).  Shown on HF itself, not assumed."""
    import transformers as tf
    fx = R.Fixture("tiny_xvec_wavlm")
    model = tf.WavLMForXVector(tf.WavLMConfig(**{k: v for k, v in fx.config.items() if k not in ("architectures", "model_type", "transformers_version")})).eval()
    res = model.load_state_dict(fx.hf_state_dict(), strict=False)
    assert not res.unexpected_keys and all("masked_spec_embed" in k for k in res.missing_keys)
    model.double()
    spec = fx.spec()
    for j in (0, 3, fx.two):
        fe = tf.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True)
        x = fe(R.synth_wave(fx.wave_seeds[j], fx.lengths[j]), sampling_rate=16000, return_tensors="pt")["input_values"].double()
        with torch.no_grad():
            plain = model(input_values=x)
            masked = model(input_values=x, attention_mask=torch.ones(x.shape, dtype=torch.long))
        T = fx.states64[j].shape[1]
        sliced = int(model._get_tdnn_output_lengths(torch.tensor(T)))
        assert sliced == T - sum(k - 1 for k in spec.tdnn_kernel) > T - spec.context      # the slice is longer than the tensor
        assert torch.equal(plain.embeddings, masked.embeddings) and torch.equal(plain.logits, masked.logits)
        assert np.abs(plain.embeddings[0].numpy() - fx.emb64[j]).max() <= 1e-9 * np.abs(fx.emb64[j]).max()


# ------------------------------------------------------------------------------- config
def test_xvector_spec_from_each_fixture(fx):
    spec, cfg = fx.spec(), fx.config
    assert spec is not None and spec.architecture == cfg["architectures"][0] and spec.architecture in C.XVECTOR_ARCHITECTURES
    assert list(spec.tdnn_dim) == cfg["tdnn_dim"] and list(spec.tdnn_kernel) == cfg["tdnn_kernel"] and list(spec.tdnn_dilation) == cfg["tdnn_dilation"]
    assert spec.xvector_output_dim == cfg["xvector_output_dim"] == fx.head["feature_extractor.weight"].shape[0]
    assert spec.use_weighted_layer_sum == cfg["use_weighted_layer_sum"] == ("layer_weights" in fx.head)
    assert spec.context == sum(d * (k - 1) for k, d in zip(cfg["tdnn_kernel"], cfg["tdnn_dilation"])) and spec.min_frames == spec.context + 2


def test_the_four_architectures_and_the_defaults():
    assert C.XVECTOR_ARCHITECTURES == ("Wav2Vec2ForXVector", "WavLMForXVector", "Data2VecAudioForXVector", "Wav2Vec2BertForXVector")
    for arch in C.XVECTOR_ARCHITECTURES:
        spec = C.XVectorSpec.from_config({"architectures": [arch]})
        assert spec.tdnn_dim == (512, 512, 512, 512, 1500) and spec.tdnn_kernel == (5, 3, 3, 1, 1) and spec.tdnn_dilation == (1, 2, 3, 1, 1)
        assert spec.xvector_output_dim == 512 and not spec.use_weighted_layer_sum and spec.min_frames == 16
    assert C.XVectorSpec.from_config({"architectures": ["WavLMModel"]}) is None
    assert C.XVectorSpec.from_config({"architectures": ["WavLMForSequenceClassification"]}) is None
    assert C.XVectorSpec.from_config({"model_type": "wavlm"}) is None


def test_refusals_are_one_oserror_each():
    base = {"architectures": ["WavLMForXVector"]}
    with pytest.raises(OSError, match=r"tdnn_dim, tdnn_kernel and tdnn_dilation have 5, 4 and 5 entries"):
        C.XVectorSpec.from_config(dict(base, tdnn_kernel=[5, 3, 3, 1]), name="x")
    with pytest.raises(OSError, match=r"have 2, 2 and 3 entries"):
        C.XVectorSpec.from_config(dict(base, tdnn_dim=[64, 64], tdnn_kernel=[3, 1], tdnn_dilation=[1, 1, 1]), name="x")
    for arch in ("UniSpeechSatForXVector", "Wav2Vec2ConformerForXVector"):
        with pytest.raises(OSError, match=arch + " is not supported"):
            C.XVectorSpec.from_config({"architectures": [arch]}, name="x")
    with pytest.raises(OSError, match="add_adapter"):
        C.XVectorSpec.from_config(dict(base, add_adapter=True), name="x")


def test_resolve_xvector_reads_the_snapshot(tmp_path):
    fx = R.Fixture("tiny_xvec_w2v_bert")
    (tmp_path / "config.json").write_text(json.dumps(fx.config))
    assert C.resolve_xvector(str(tmp_path)) == fx.spec()
    assert C.resolve_xvector(str(tmp_path / "nowhere")) is None


# ------------------------------------------------------------------------------- weights
def test_weight_split(fx):
    """the encoder gets what a bare-encoder snapshot gives it, the head its tensors, and objective.* goes nowhere"""
    sd = fx.hf_state_dict()
    assert "objective.weight" in sd
    enc, head = W.split_xvector_head(W.normalize_names(sd))
    bare = W.normalize_names(W.synthetic_state_dict(fx.geometry(), fx.seed))
    assert sorted(enc) == sorted(bare) and all(torch.equal(enc[k], bare[k]) for k in bare)
    spec = fx.spec()
    assert sorted(head) == sorted(W.xvector_head_keys(len(spec.tdnn_dim), spec.use_weighted_layer_sum))
    assert not any(k.startswith("objective") for k in list(enc) + list(head))
    W.check_xvector_head(head, fx.geometry().hidden, spec, fx.geometry().num_layers + 1)


def test_snapshot_without_a_head_comes_back_whole():
    sd = W.synthetic_state_dict(C.TINY_WAVLM, 3)
    enc, head = W.split_xvector_head(sd)
    assert head == {} and sorted(enc) == sorted(sd)


@pytest.mark.parametrize("key,shape", [("projector.weight", (64, 64)), ("tdnn.0.kernel.weight", (64, 5 * 32)), ("tdnn.4.kernel.bias", (64,)),
                                       ("feature_extractor.weight", (24, 100)), ("classifier.weight", (24, 20)), ("layer_weights", (4,))])
def test_wrong_shaped_or_missing_head_tensor_is_refused_by_name(key, shape):
    fx = R.Fixture("tiny_xvec_wavlm")
    head = {k: torch.from_numpy(np.array(v)) for k, v in fx.head.items() if not k.startswith("objective")}
    head[key] = torch.zeros(shape)
    with pytest.raises(ValueError) as e:
        W.check_xvector_head(head, 128, fx.spec(), 3)
    assert key in str(e.value) and str(tuple(shape)) in str(e.value)
    del head[key]
    with pytest.raises(ValueError, match=key.replace(".", r"\.") + " is missing"):
        W.check_xvector_head(head, 128, fx.spec(), 3)


# ------------------------------------------------------------------------------- the per-layer offsets and row tables
def test_layout_matches_a_loop_and_no_window_crosses_an_utterance():
    spec = C.XVectorSpec.from_config({"architectures": ["WavLMForXVector"]})
    kernel, dilation = (5, 3, 3, 1, 1), (1, 2, 3, 1, 1)
    lengths = [16, 17, 40, 15]
    with pytest.raises(ValueError, match=r"utterance 3: 15 encoder frames leave 1 TDNN output rows"):
        spec.layout(np.concatenate([[0], np.cumsum(lengths)]))
    lengths = lengths[:3]
    lay = spec.layout(np.concatenate([[0], np.cumsum(lengths)]))
    T = list(lengths)
    want = [[0, 16, 33, 73]]
    for k, d in zip(kernel, dilation):                                   # the T_i chain and the packed offsets, by a loop of the test's own
        T = [t - d * (k - 1) for t in T]
        offs = [0]
        for t in T:
            offs.append(offs[-1] + t)
        want.append(offs)
    assert T == [2, 3, 26] and [list(o) for o in lay.offs] == want
    for i, (k, d) in enumerate(zip(kernel, dilation), start=1):
        first = lay.first_rows(i)
        src, dst = lay.offs[i - 1], lay.offs[i]
        assert len(first) == dst[-1] and (np.diff(first) >= 0).all()     # non-decreasing: what ser_gemm's row map needs
        for b in range(3):
            rows = first[dst[b]: dst[b + 1]]
            assert rows[0] == src[b] and (np.diff(rows) == 1).all()
            assert rows[-1] + d * (k - 1) == src[b + 1] - 1              # the last tap of the last window is the utterance's last row:
            assert rows.max() + d * (k - 1) < src[b + 1]                 # no row index of utterance b reaches utterance b + 1


def test_layout_of_the_fixtures(fx):
    spec = fx.spec()
    lay = spec.layout([0, spec.min_frames, 2 * spec.min_frames + 30])
    assert lay.offs[-1] == (0, 2, 34)
    with pytest.raises(ValueError, match="utterance 1"):
        spec.layout([0, spec.min_frames, 2 * spec.min_frames - 1, 3 * spec.min_frames])


# ------------------------------------------------------------------------------- launchers (no GPU: validation comes first)
def _stat_args(offs, **over):
    from interspeech_ser_amd import _lib
    a = _lib.StatPoolArgs()
    host = (ctypes.c_int32 * len(offs))(*offs)
    a.x, a.frame_offs, a.work, a.out = 256, 768, 1024, 2048                               # never dereferenced
    a.frame_offs_host = ctypes.cast(host, ctypes.c_void_p)
    a.ldx, a.ldo, a.work_elems = 104, 200, 1 << 20
    a.B, a.D, a.rows, a.max_frames, a.relu = len(offs) - 1, 100, 100, max(int(np.diff(offs).max()), 1), 1
    for k, v in over.items():
        setattr(a, k, v)
    return a, host


@pytest.mark.parametrize("over,offs,word", [
    (dict(D=98), [0, 5, 9], b"D=98"),
    (dict(), [0, 5, 6, 9], b"utterance 1 has 1 rows"),
    (dict(), [0, 5, 5, 9], b"utterance 1 has 0 rows"),
    (dict(), [0, 5, 3, 9], b"utterance 1 owns rows 5..3"),
    (dict(max_frames=96), [0, 5, 101], b"outside [0, 100]"),
    (dict(max_frames=3), [0, 5, 9], b"utterance 0 has 5 rows, max_frames=3"),
    (dict(work_elems=10), [0, 5, 9], b"work holds 10"),
    (dict(ldx=98), [0, 5, 9], b"ldx=98"),
    (dict(ldo=199), [0, 5, 9], b"ldo=199"),
    (dict(relu=2), [0, 5, 9], b"relu=2"),
    (dict(x=260), [0, 5, 9], b"16-byte"),
    (dict(B=65536), [0, 5, 9], b"B=65536"),
])
def test_stat_pool_refusals(built_library, over, offs, word):
    from interspeech_ser_amd import _lib
    a, keep = _stat_args(offs, **over)
    assert _lib.lib.ser_stat_pool_v(ctypes.byref(a), None) == -2
    msg = _lib.lib.ser_last_error()
    assert msg.startswith(b"ser_stat_pool:") and word in msg, msg


def test_launchers_refuse_null_pointers_and_sizes(built_library):
    from interspeech_ser_amd import _lib
    lib = _lib.lib
    for fn, name, args in ((lib.ser_stat_pool_v, b"ser_stat_pool", _lib.StatPoolArgs), (lib.ser_layer_mix_v, b"ser_layer_mix", _lib.LayerMixArgs),
                           (lib.ser_xvec_tail_v, b"ser_xvec_tail", _lib.XvecTailArgs)):
        assert fn(None, None) == -1 and name + b": null pointer" in lib.ser_last_error()
        assert fn(ctypes.byref(args()), None) == -1
    m = _lib.LayerMixArgs()
    m.s, m.w, m.out_act = 256, 512, 1024
    m.state_stride, m.lds, m.ldo_act, m.out_plane_stride, m.n_states, m.mode, m.rows, m.D = 128 * 10, 128, 128, 1280, 3, _lib.MODE_FP16X, 10, 128
    for over, code, word in ((dict(n_states=0), -2, b"n_states=0"), (dict(D=126), -2, b"D=126"), (dict(D=2052, lds=2052, ldo_act=2052), -2, b"D=2052"),
                             (dict(lds=124), -3, b"lds=124"), (dict(s=260), -3, b"16-byte"), (dict(mode=_lib.MODE_FP16M), -4, b"bad mode 6")):
        a = _lib.LayerMixArgs.from_buffer_copy(m)
        for k, v in over.items():
            setattr(a, k, v)
        assert lib.ser_layer_mix_v(ctypes.byref(a), None) == code and word in lib.ser_last_error(), (over, lib.ser_last_error())
    t = _lib.XvecTailArgs()
    t.stats, t.F, t.bf, t.C, t.bc, t.emb, t.logits = (256 * i for i in range(1, 8))
    t.lds, t.lde, t.ldo, t.B, t.D, t.dim, t.n_labels = 200, 24, 5, 2, 200, 2049, 5
    assert lib.ser_xvec_tail_v(ctypes.byref(t), None) == -2 and b"dim=2049" in lib.ser_last_error()
    t.dim, t.D = 24, 198
    assert lib.ser_xvec_tail_v(ctypes.byref(t), None) == -2 and b"D=198" in lib.ser_last_error()
    t.D, t.lde = 200, 23
    assert lib.ser_xvec_tail_v(ctypes.byref(t), None) == -2 and b"lde=23" in lib.ser_last_error()
    assert _lib.STAT_POOL_FC == 32 and "#define SER_STAT_POOL_FC 32" in open(_lib._HERE + "/../include/ser_hip.h").read()


def test_pt_vector_writer_round_trips(built_library, tmp_path):
    v = (np.random.default_rng(3).standard_normal(40) * 7).astype(np.float32)
    XV.save_embedding(v, str(tmp_path / "utt.pt"))
    t = torch.load(str(tmp_path / "utt.pt"))
    assert t.shape == (40,) and t.dtype == torch.float32 and np.array_equal(t.numpy().view(np.uint32), v.view(np.uint32))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["utt.pt"]                       # no temporary file stays


# ------------------------------------------------------------------------------- the command line, with a stub model
class _Stub:
    """rows by length: what the head would return ([embedding | logits]), keyed by the number of samples; short inputs fail alone"""
    SLOTS = 2
    dim = 4
    weight_source, mode = "stub", "f16x"

    def __init__(self, table):
        self.table, self.batches = table, []

    def _rows(self, waves):
        self.batches.append([len(w) for w in waves])
        if any(len(w) < 400 for w in waves):
            raise ValueError("utterance 0: 1 encoder frames leave 0 TDNN output rows")
        return np.stack([np.asarray(self.table[len(w)] + [9.0, 9.0], dtype=np.float32) for w in waves])

    def submit(self, waves, layer_index, slot=0, rates=None):
        return dict(rows=self._rows(waves))

    def collect(self, ticket):
        return ticket["rows"]

    def extract(self, waves, layer_index=None, rates=None):
        return self._rows(waves)


def _write_wav(path, n, sr=16000, seed=0):
    pcm = (np.random.default_rng(seed).standard_normal(n) * 3000).astype(np.int16)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


TABLE = {4000: [0.25, -1.5, 3.0, 1.0], 5000: [2.0, 0.125, -0.5, 0.0], 7000: [-1.0, 0.5, 0.0, 2.0]}


@pytest.fixture
def wav_dir(tmp_path):
    d = tmp_path / "wavs"
    d.mkdir()
    _write_wav(d / "b.wav", 5000, seed=1)
    _write_wav(d / "a.wav", 4000, seed=2)
    _write_wav(d / "c.wav", 7000, seed=3)
    return d


def test_cli_writes_one_vector_per_file_and_scores_trials(built_library, wav_dir, tmp_path, capsys):
    _write_wav(wav_dir / "short.wav", 100)
    stub = _Stub(TABLE)
    save = tmp_path / "emb"
    trials = tmp_path / "trials.txt"
    trials.write_text("a.wav b.wav\nc.wav a.wav\n\nb.wav short.wav\n")
    scores = tmp_path / "out" / "scores.csv"
    rc = XV.run_embed(["--model", "stub", "--wav_dir", str(wav_dir), "--save_path", str(save), "--trials", str(trials), "--scores_csv", str(scores)],
                      embedder_factory=lambda a, d: stub)
    out = capsys.readouterr().out
    assert rc == 0 and sorted(p.name for p in save.iterdir()) == ["a.pt", "b.pt", "c.pt"]
    for name, n in (("a", 4000), ("b", 5000), ("c", 7000)):
        t = torch.load(str(save / f"{name}.pt"))
        assert t.shape == (4,) and t.dtype == torch.float32 and t.tolist() == TABLE[n]    # the embedding columns only, not the logits
    assert stub.batches == [[4000, 5000, 7000, 100], [4000], [5000], [7000], [100]]       # sorted order; the batch whole, then file by file
    assert f"Failed to process {wav_dir / 'short.wav'}: utterance 0" in out and "3 embeddings written" in out and "1 files failed" in out
    with open(scores, newline="") as f:
        rows = list(csv.reader(f))
    assert [r[:2] for r in rows] == [["a.wav", "b.wav"], ["c.wav", "a.wav"]] and "Failed to score b.wav short.wav" in out
    for r in rows:
        a, b = (np.array(TABLE[{"a.wav": 4000, "b.wav": 5000, "c.wav": 7000}[n]], dtype=np.float64) for n in r[:2])
        assert float(r[2]) == pytest.approx(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), abs=1e-15)
    assert "2 trials scored" in out


def test_cli_set_up_errors_exit_0(wav_dir, tmp_path, capsys):
    def factory(args, device):
        raise OSError("no local checkpoint for stub")
    rc = XV.run_embed(["--model", "stub", "--wav_dir", str(wav_dir), "--save_path", str(tmp_path / "e")], embedder_factory=factory)
    assert rc == 0 and "No pretrained model found with the name stub" in capsys.readouterr().out
    rc = XV.run_embed(["--model", "stub", "--wav_dir", str(wav_dir), "--save_path", str(tmp_path / "e"), "--trials", "t.txt"], embedder_factory=factory)
    assert rc == 0 and "--trials and --scores_csv go together" in capsys.readouterr().out


def test_load_path_names_what_it_refuses(tmp_path):
    fx = R.Fixture("tiny_xvec_wavlm")
    args = XV.build_parser().parse_args(["--model", str(tmp_path), "--wav_dir", ".", "--save_path", "x"])
    (tmp_path / "config.json").write_text(json.dumps(dict(fx.config, architectures=["WavLMModel"])))
    with pytest.raises(OSError, match="not an x-vector checkpoint"):
        XV._build_embedder(args, "cpu")
    (tmp_path / "config.json").write_text(json.dumps(dict(fx.config, architectures=["UniSpeechSatForXVector"], model_type="unispeech-sat")))
    with pytest.raises(OSError, match="UniSpeechSatForXVector is not supported"):
        XV._build_embedder(args, "cpu")


def test_head_mode_fallback_says_so_in_one_line(capsys):
    assert XV.head_mode("f16mf", "m") == "f16x"
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "--mode f16mf is not implemented for the x-vector head (m): using f16x" in out
    assert [XV.head_mode(m, "m") for m in ("f16x", "fp32x", "bf16")] == ["f16x", "fp32x", "bf16"] and capsys.readouterr().out == ""


def test_classify_on_an_xvector_snapshot_still_says_what_it_said(tmp_path):
    """bin/classify_from_wav.py refuses an x-vector snapshot with the words it had before this head existed"""
    fx = R.Fixture("tiny_xvec_wavlm")
    (tmp_path / "config.json").write_text(json.dumps(fx.config))
    args = CL.build_parser().parse_args(["--model", str(tmp_path), "--wav_dir", ".", "--out_csv", "x.csv"])
    with pytest.raises(OSError, match="is not an audio-classification checkpoint \\(its config.json names none of Wav2Vec2ForSequenceClassification"):
        CL._build_classifier(args, "cpu")
    assert C.ClassifierSpec.from_config(fx.config) is None
