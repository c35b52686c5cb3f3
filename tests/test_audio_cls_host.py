"""CPU: the audio-classification head around its kernels -- the float64 statement against HF, the config and weight plumbing, the
launchers' refusals (validation comes before any launch) and the command line with a stub in place of the model."""
import csv
import ctypes
import wave

import numpy as np
import pytest
import torch

import audio_cls_ref as R
from interspeech_ser_amd import classify as CL
from interspeech_ser_amd import config as C
from interspeech_ser_amd import weights as W


@pytest.fixture(scope="module", params=R.FIXTURES)
def fx(request):
    return R.Fixture(request.param)


# ------------------------------------------------------------------------------- the statement
def test_pool_first_statement_reproduces_hf_float64(fx):
    """mean_t(projector(x_t)) = projector(mean_t x_t): the float64 statement on the fixture's float64 hidden states gives HF's float64
    logits to 1e-10 relative (measured when the fixtures were made: <= 2.3e-15).  Whisper's fixture keeps the row means of its states."""
    for j in range(3):
        got = R.head_logits(fx.states64[j], fx.head, fx.weighted)
        want = fx.logits64[j]
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (fx.name, j)


def test_fixture_margins(fx):
    """the property the GPU test's argmax check stands on: at least two of the three waveforms have a top-two margin beyond twice the
    f16x / fp32x logit bound (regression fixtures, one output, have no argmax)"""
    if fx.spec().num_labels == 1:
        return
    wide = 0
    for j in range(3):
        top = np.sort(fx.logits64[j])[::-1]
        wide += top[0] - top[1] > 2 * fx.logit_bound(1e-3, j).max()
    assert wide >= 2


# ------------------------------------------------------------------------------- config
def test_classifier_spec_from_each_fixture(fx):
    spec = fx.spec()
    cfg = fx.config
    assert spec is not None and spec.architecture == cfg["architectures"][0]
    assert spec.use_weighted_layer_sum == cfg["use_weighted_layer_sum"] and spec.classifier_proj_size == cfg["classifier_proj_size"]
    assert spec.num_labels == len(cfg["id2label"]) == fx.head["classifier.weight"].shape[0]
    assert list(spec.labels) == [cfg["id2label"][str(i)] for i in range(spec.num_labels)]
    geo = fx.geometry()
    assert geo.hidden == fx.head["projector.weight"].shape[1]


def test_labels_of_the_wavlm_fixture_are_the_configs_names():
    assert R.Fixture("tiny_cls_wavlm").spec().labels == ("angry", "happy", "neutral", "sad", "surprised")


def test_plain_encoder_config_has_no_classifier():
    cfg = dict(R.Fixture("tiny_cls_wavlm").config, architectures=["WavLMModel"])
    assert C.ClassifierSpec.from_config(cfg) is None
    assert C.ClassifierSpec.from_config({"model_type": "wavlm"}) is None
    assert C.ClassifierSpec.from_config(dict(cfg, architectures=["WavLMForCTC"])) is None


def test_add_adapter_is_refused():
    cfg = dict(R.Fixture("tiny_cls_wav2vec2").config, add_adapter=True)
    with pytest.raises(OSError, match="add_adapter"):
        C.ClassifierSpec.from_config(cfg, name="x")


def test_label_fallback():
    cfg = {k: v for k, v in R.Fixture("tiny_cls_wavlm").config.items() if k not in ("id2label", "label2id")}
    cfg["num_labels"] = 3
    spec = C.ClassifierSpec.from_config(cfg)
    assert spec.labels == ("LABEL_0", "LABEL_1", "LABEL_2") and spec.num_labels == 3


def test_resolve_classifier_reads_the_snapshot(tmp_path):
    import json
    fx = R.Fixture("tiny_cls_w2v_bert")
    (tmp_path / "config.json").write_text(json.dumps(fx.config))
    assert C.resolve_classifier(str(tmp_path)) == fx.spec()
    assert C.resolve_classifier(str(tmp_path / "nowhere")) is None


# ------------------------------------------------------------------------------- weights
def test_weight_split(fx):
    """the encoder gets what a bare-encoder snapshot gives it, the head its five (four without the weighted sum)"""
    full = W.normalize_names(fx.hf_state_dict())
    enc, head = W.split_classifier_head(full)
    bare = W.normalize_names(W.synthetic_state_dict(fx.geometry(), fx.seed))
    assert sorted(enc) == sorted(bare)
    assert all(torch.equal(enc[k], bare[k]) for k in bare)
    want = [k for k in W.CLASSIFIER_HEAD_KEYS if fx.weighted or k != "layer_weights"]
    assert sorted(head) == sorted(want)
    geo, spec = fx.geometry(), fx.spec()
    W.check_classifier_head(head, geo.hidden, spec.classifier_proj_size, spec.num_labels, geo.num_layers + 1, spec.use_weighted_layer_sum)


def test_snapshot_without_a_head_comes_back_whole():
    sd = W.synthetic_state_dict(C.TINY_WAVLM, 3)
    enc, head = W.split_classifier_head(sd)
    assert head == {} and sorted(enc) == sorted(sd)


@pytest.mark.parametrize("key,shape", [("projector.weight", (48, 64)), ("classifier.weight", (5, 40)), ("layer_weights", (4,)),
                                       ("classifier.bias", (6,))])
def test_wrong_shaped_head_tensor_is_refused_by_name(key, shape):
    fx = R.Fixture("tiny_cls_wavlm")
    head = {k: torch.from_numpy(np.array(v)) for k, v in fx.head.items()}
    head[key] = torch.zeros(shape)
    with pytest.raises(ValueError) as e:
        W.check_classifier_head(head, 128, 48, 5, 3, True)
    assert key in str(e.value) and str(tuple(shape)) in str(e.value)
    del head[key]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        W.check_classifier_head(head, 128, 48, 5, 3, True)


# ------------------------------------------------------------------------------- launchers (no GPU: validation comes first)
def _pool_args(offs, **over):
    from interspeech_ser_amd import _lib
    a = _lib.LayerPoolArgs()
    host = (ctypes.c_int32 * len(offs))(*offs)
    a.s, a.w, a.frame_offs, a.work, a.out = 256, 512, 768, 1024, 2048                     # never dereferenced
    a.frame_offs_host = ctypes.cast(host, ctypes.c_void_p)
    a.state_stride, a.lds, a.ldo, a.work_elems = 64 * 100, 64, 64, 1 << 20
    a.n_states, a.B, a.D, a.rows, a.max_frames = 3, len(offs) - 1, 64, 100, max(np.diff(offs).max(), 1)
    for k, v in over.items():
        setattr(a, k, v)
    return a, host


@pytest.mark.parametrize("over,offs,word", [
    (dict(D=62), [0, 5, 9], b"D=62"),
    (dict(n_states=0), [0, 5, 9], b"n_states=0"),
    (dict(), [0, 5, 5, 9], b"utterance 1 is empty"),
    (dict(max_frames=101), [0, 5, 9], b"max_frames=101"),
    (dict(B=65536), [0, 5, 9], b"B=65536"),
    (dict(max_frames=3), [0, 5, 9], b"utterance 0 has 5 frames"),
    (dict(max_frames=96), [0, 5, 101], b"outside [0, 100]"),
    (dict(work_elems=10), [0, 5, 9], b"work holds 10"),
    (dict(lds=62), [0, 5, 9], b"lds=62"),
    (dict(s=260), [0, 5, 9], b"16-byte"),
])
def test_layer_pool_refusals(built_library, over, offs, word):
    """the refusals of ser_layer_pool_v return a negative code with a message and launch nothing (a null stream on a box without a GPU:
    a launch would fail differently)"""
    from interspeech_ser_amd import _lib
    a, keep = _pool_args(offs, **over)
    assert _lib.lib.ser_layer_pool_v(ctypes.byref(a), None) == -2
    msg = _lib.lib.ser_last_error()
    assert msg.startswith(b"ser_layer_pool:") and word in msg, msg


def test_launchers_refuse_null_pointers_and_tail_sizes(built_library):
    from interspeech_ser_amd import _lib
    lib = _lib.lib
    assert lib.ser_layer_pool_v(None, None) == -1 and b"ser_layer_pool: null pointer" in lib.ser_last_error()
    assert lib.ser_layer_pool_v(ctypes.byref(_lib.LayerPoolArgs()), None) == -1
    assert lib.ser_cls_tail_v(None, None) == -1 and b"ser_cls_tail: null pointer" in lib.ser_last_error()
    t = _lib.ClsTailArgs()
    assert lib.ser_cls_tail_v(ctypes.byref(t), None) == -1
    t.pooled, t.P, t.bp, t.C, t.bc, t.out = (256 * i for i in range(1, 7))
    t.ldp, t.ldo, t.B, t.D, t.proj, t.n_labels = 128, 5, 2, 128, 2049, 5
    assert lib.ser_cls_tail_v(ctypes.byref(t), None) == -2 and b"proj=2049" in lib.ser_last_error()
    t.proj, t.n_labels = 48, 0
    assert lib.ser_cls_tail_v(ctypes.byref(t), None) == -2 and b"n_labels=0" in lib.ser_last_error()
    t.n_labels, t.D = 5, 126
    assert lib.ser_cls_tail_v(ctypes.byref(t), None) == -2 and b"D=126" in lib.ser_last_error()
    t.D, t.ldo = 128, 4
    assert lib.ser_cls_tail_v(ctypes.byref(t), None) == -2 and b"ldo=4" in lib.ser_last_error()
    assert _lib.LAYER_POOL_FC == 32 and "#define SER_LAYER_POOL_FC 32" in open(_lib._HERE + "/../include/ser_hip.h").read()


# ------------------------------------------------------------------------------- the command line, with a stub model
class _Stub:
    """logits by length: what the head would return, keyed by the number of samples; 100-sample inputs fail like a short waveform"""
    SLOTS = 2
    labels = ("neg", "neu", "pos")
    weight_source, mode = "stub", "f16x"

    def __init__(self, table, fail_batches=False):
        self.table, self.batches, self.fail_batches = table, [], fail_batches

    def _rows(self, waves):
        self.batches.append([len(w) for w in waves])
        if any(len(w) < 400 for w in waves):
            raise ValueError("waveform shorter than the receptive field (400 samples)")
        if self.fail_batches and len(waves) > 1:
            raise ValueError("a value beyond the fp16 operand range")
        return np.stack([np.asarray(self.table[len(w)], dtype=np.float32) for w in waves])

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


TABLE = {4000: [0.25, -1.5, 3.0], 5000: [2.0, 0.125, -0.5], 7000: [-1.0, 0.5, 0.0]}


@pytest.fixture
def wav_dir(tmp_path):
    d = tmp_path / "wavs"
    d.mkdir()
    _write_wav(d / "b.wav", 5000, seed=1)
    _write_wav(d / "a.wav", 4000, seed=2)
    _write_wav(d / "c.wav", 7000, seed=3)
    return d


def _run(wav_dir, tmp_path, stub, extra=()):
    out = tmp_path / "out" / "preds.csv"
    rc = CL.run_classify(["--model", "stub", "--wav_dir", str(wav_dir), "--out_csv", str(out), *extra], classifier_factory=lambda a, d: stub)
    with open(out, newline="") as f:
        return rc, list(csv.reader(f))


def test_csv_header_rows_and_labels(wav_dir, tmp_path):
    rc, rows = _run(wav_dir, tmp_path, _Stub(TABLE))
    assert rc == 0
    assert rows[0] == ["FileName", "label", "neg", "neu", "pos"]
    assert [r[:2] for r in rows[1:]] == [["a.wav", "pos"], ["b.wav", "neg"], ["c.wav", "neu"]]
    assert [[np.float32(v) for v in r[2:]] for r in rows[1:]] == [[np.float32(v) for v in TABLE[n]] for n in (4000, 5000, 7000)]


def test_a_short_and_a_44k_file_fail_alone_and_leave_the_rows(wav_dir, tmp_path, capsys):
    _write_wav(wav_dir / "short.wav", 100)
    _write_wav(wav_dir / "hi.wav", 12000, sr=44100)
    stub = _Stub(TABLE)
    rc, rows = _run(wav_dir, tmp_path, stub)
    out = capsys.readouterr().out
    assert rc == 0 and [r[0] for r in rows[1:]] == ["a.wav", "b.wav", "c.wav"]
    assert f"Failed to process {wav_dir / 'short.wav'}: waveform shorter" in out
    assert f"Failed to process {wav_dir / 'hi.wav'}: sample rate 44100 Hz" in out
    assert "3 rows written" in out and "2 files failed" in out
    assert stub.batches == [[4000, 5000, 7000, 100], [4000], [5000], [7000], [100]]         # the batch whole first, then file by file


def test_a_failed_batch_is_retried_file_by_file(wav_dir, tmp_path, capsys):
    stub = _Stub(TABLE, fail_batches=True)
    rc, rows = _run(wav_dir, tmp_path, stub)
    assert rc == 0 and len(rows) == 4 and "0 files failed" in capsys.readouterr().out
    assert sorted(b[0] for b in stub.batches if len(b) == 1) == [4000, 5000, 7000]


def test_resample_flag_brings_the_44k_file_in(wav_dir, tmp_path, capsys):
    _write_wav(wav_dir / "hi.wav", 11025, sr=44100)                     # 0.25 s -> 4000 samples at 16 kHz
    rc, rows = _run(wav_dir, tmp_path, _Stub(TABLE), extra=["--resample"])
    assert rc == 0 and [r[0] for r in rows[1:]] == ["a.wav", "b.wav", "c.wav", "hi.wav"] and rows[4][1] == "pos"


def test_a_missing_model_is_a_set_up_error_with_exit_0(wav_dir, tmp_path, capsys):
    def factory(args, device):
        raise OSError("no local checkpoint for stub")
    rc = CL.run_classify(["--model", "stub", "--wav_dir", str(wav_dir), "--out_csv", str(tmp_path / "p.csv")], classifier_factory=factory)
    out = capsys.readouterr().out
    assert rc == 0 and "No pretrained model found with the name stub" in out and not (tmp_path / "p.csv").exists()


def test_a_bare_encoder_snapshot_is_refused_by_the_load_path(tmp_path):
    import json
    cfg = dict(R.Fixture("tiny_cls_wavlm").config, architectures=["WavLMModel"])
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    args = CL.build_parser().parse_args(["--model", str(tmp_path), "--wav_dir", ".", "--out_csv", "x.csv"])
    with pytest.raises(OSError, match="not an audio-classification checkpoint"):
        CL._build_classifier(args, "cpu")
