"""CPU: the CTC path around the kernels -- the spec of config.json, the head's tensors, the numpy restatement against HF's ids and offsets
on the fixtures, the vocabulary against Wav2Vec2CTCTokenizer, ser_ctc_greedy_v's refusals, the command line around a stub."""
import csv
import ctypes
import json
import wave

import numpy as np
import pytest
import torch

import ctc_ref as R
from interspeech_ser_amd import config as C
from interspeech_ser_amd import ctc as CT
from interspeech_ser_amd import weights as W


# ------------------------------------------------------------------------------- spec
@pytest.mark.parametrize("arch", ["Wav2Vec2ForCTC", "HubertForCTC", "WavLMForCTC", "Data2VecAudioForCTC", "Wav2Vec2BertForCTC"])
def test_spec_of_the_five_classes(arch):
    assert arch in C.CTC_ARCHITECTURES
    spec = C.CTCSpec.from_config({"architectures": [arch], "vocab_size": 32, "pad_token_id": 0})
    assert spec == C.CTCSpec(vocab_size=32, blank=0, architecture=arch)
    assert C.CTCSpec.from_config({"architectures": arch, "vocab_size": 12, "pad_token_id": 11}).blank == 11


def test_spec_is_none_for_other_classes():
    for arch in ("WavLMModel", "WavLMForXVector", "Wav2Vec2ForSequenceClassification", ""):
        assert C.CTCSpec.from_config({"architectures": [arch], "vocab_size": 32, "pad_token_id": 0}) is None
    assert C.CTCSpec.from_config({}) is None


@pytest.mark.parametrize("arch", ["UniSpeechForCTC", "UniSpeechSatForCTC", "Wav2Vec2ConformerForCTC", "SEWForCTC", "SEWDForCTC"])
def test_spec_refuses_the_unbuilt_encoders(arch):
    with pytest.raises(OSError, match=arch):
        C.CTCSpec.from_config({"architectures": [arch], "vocab_size": 32, "pad_token_id": 0}, name="x/y")


@pytest.mark.parametrize("cfg, what", [
    ({"vocab_size": 32, "pad_token_id": 0, "add_adapter": True}, "add_adapter"),
    ({"pad_token_id": 0}, "vocab_size"),
    ({"vocab_size": 32}, "pad_token_id"),
    ({"vocab_size": 32, "pad_token_id": None}, "pad_token_id"),
    ({"vocab_size": 32, "pad_token_id": 32}, "pad_token_id"),
])
def test_spec_refusals_name_the_class(cfg, what):
    with pytest.raises(OSError) as e:
        C.CTCSpec.from_config(dict(cfg, architectures=["HubertForCTC"]), name="x/y")
    assert "HubertForCTC" in str(e.value) and what in str(e.value)


def test_resolve_ctc_reads_config_json(tmp_path):
    assert C.resolve_ctc(str(tmp_path)) is None
    (tmp_path / "config.json").write_text(json.dumps({"architectures": ["Wav2Vec2ForCTC"], "vocab_size": 32, "pad_token_id": 0, "model_type": "wav2vec2"}))
    assert C.resolve_ctc(str(tmp_path)) == C.CTCSpec(32, 0, "Wav2Vec2ForCTC")
    (tmp_path / "config.json").write_text(json.dumps({"architectures": ["SEWForCTC"], "vocab_size": 32, "pad_token_id": 0}))
    with pytest.raises(OSError, match="SEWForCTC"):
        C.resolve_ctc(str(tmp_path))


# ------------------------------------------------------------------------------- head tensors
@pytest.mark.parametrize("name", R.FIXTURES)
def test_split_and_check_ctc_head(name):
    fx = R.Fixture(name)
    sd = fx.hf_state_dict()
    assert "lm_head.weight" not in W.normalize_names(sd)                  # the encoder drivers' view is unchanged
    enc, head = W.split_ctc_head(W.normalize_names(sd, keep=W.CTC_HEAD_PREFIXES))
    bare = W.normalize_names(W.synthetic_state_dict(fx.geometry(), fx.seed))
    assert sorted(enc) == sorted(bare) and sorted(head) == ["lm_head.bias", "lm_head.weight"]
    D = fx.geometry().hidden
    W.check_ctc_head(head, D, fx.V)
    with pytest.raises(ValueError, match="lm_head.weight"):
        W.check_ctc_head(head, D, fx.V + 1)
    with pytest.raises(ValueError, match="lm_head.bias is missing"):
        W.check_ctc_head({"lm_head.weight": head["lm_head.weight"]}, D, fx.V)
    whole, none = W.split_ctc_head(bare)
    assert sorted(whole) == sorted(bare) and none == {}


def test_load_checkpoint_keeps_lm_head_on_request(tmp_path):
    from safetensors.torch import save_file
    fx = R.Fixture("tiny_ctc_wavlm")
    save_file({k: v.contiguous() for k, v in fx.hf_state_dict().items()}, str(tmp_path / "model.safetensors"))
    assert "lm_head.weight" not in W.load_checkpoint(str(tmp_path))
    sd = W.load_checkpoint(str(tmp_path), keep=W.CTC_HEAD_PREFIXES)
    assert tuple(sd["lm_head.weight"].shape) == (fx.V, fx.geometry().hidden) and "encoder.layers.0.attention.q_proj.weight" in sd


# ------------------------------------------------------------------------------- the restatement and the fixtures' conditions
@pytest.mark.parametrize("name", R.FIXTURES)
def test_restatement_equals_hf_on_the_goldens(name):
    fx = R.Fixture(name)
    assert fx.spec() == C.CTCSpec(fx.V, fx.blank, fx.config["architectures"][0]) and fx.V == 12
    assert fx.geometry().frames_for(fx.lengths[-1]) == 1 and fx.geometry().frames_for(fx.lengths[-1] - 1) == 0    # the shortest the stem admits
    offs = np.concatenate([[0], np.cumsum([l.shape[0] for l in fx.logits64])])
    got = R.greedy(np.concatenate(fx.logits64).astype(np.float32), offs, fx.V, fx.blank)
    assert got["err"] == 0
    for j in range(len(fx.lengths)):
        assert np.array_equal(got["frame_ids"][offs[j]: offs[j + 1]], fx.frame_ids[j])
        assert np.array_equal(fx.frame_ids[j], np.argmax(fx.logits64[j], axis=1))
        assert got["ids"][j] == fx.ids[j]
        assert list(zip(got["starts"][j], got["ends"][j])) == fx.offsets[j]


@pytest.mark.parametrize("name", R.FIXTURES)
def test_goldens_meet_the_margin_and_collapse_conditions(name):
    """(a) every frame's float64 margin is at least 4 g: a device within g of HF's logits cannot choose another token, so no frame is
    left out of the token comparison; (b) at least 3 blank frames and 3 repeated non-blank frames: both collapse rules are exercised."""
    fx = R.Fixture(name)
    g = fx.gate()
    assert min(float(R.margins64(l).min()) for l in fx.logits64) >= 4 * g
    blanks = sum(int((f == fx.blank).sum()) for f in fx.frame_ids)
    repeats = sum(int(((f[1:] == f[:-1]) & (f[1:] != fx.blank)).sum()) for f in fx.frame_ids)
    assert blanks >= 3 and repeats >= 3
    assert sum(len(i) for i in fx.ids) < sum(len(f) for f in fx.frame_ids) - blanks          # the collapse removed repeats too


# ------------------------------------------------------------------------------- vocabulary
VOCAB = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, "E": 5, "T": 6, "A": 7, "O": 8, "'": 9}
FRAME_CASES = {
    "plain": [0, 6, 6, 0, 5, 5, 4, 4, 7, 0, 7, 8, 0],
    "blank between two delimiters": [6, 4, 0, 4, 7, 7],
    "leading and trailing delimiter": [4, 4, 6, 5, 0, 4],
    "unk": [6, 3, 3, 5, 0, 3],
    "special tokens are not skipped": [1, 6, 2, 2],
    "apostrophe": [6, 9, 0, 9, 5],
    "empty": [0, 0, 0],
    "only delimiters": [4, 0, 4],
    "no frames": [],
}


@pytest.fixture(scope="module")
def hf_tokenizer(tmp_path_factory):
    tf = pytest.importorskip("transformers")
    d = tmp_path_factory.mktemp("ctc_vocab")
    (d / "vocab.json").write_text(json.dumps(VOCAB))
    return tf.Wav2Vec2CTCTokenizer(str(d / "vocab.json")), d


@pytest.mark.parametrize("case", sorted(FRAME_CASES))
def test_vocab_text_and_offsets_equal_the_hf_tokenizer(hf_tokenizer, case):
    tok, d = hf_tokenizer
    frames = FRAME_CASES[case]
    ids, starts, ends = R.collapse(frames, VOCAB["<pad>"])
    vocab = CT.CTCVocab.from_dir(str(d))
    if not frames:
        assert tok.decode(frames) == "" and vocab.text(ids) == ""
        return
    want = tok.decode(frames, output_char_offsets=True)
    assert vocab.text(ids) == want.text == tok.decode(frames)
    got = vocab.char_offsets(ids, list(zip(starts, ends)))
    assert got == [{"char": o["char"], "start_offset": int(o["start_offset"]), "end_offset": int(o["end_offset"])} for o in want.char_offsets]
    if case == "blank between two delimiters":
        assert vocab.text(ids) == "T  A"
    if case == "leading and trailing delimiter":
        assert vocab.text(ids) == "TE" and [o["char"] for o in got] == [" ", "T", "E", " "]
    if case == "unk":
        assert vocab.text(ids) == "T<unk>E<unk>"


def test_vocab_reads_the_tokenizer_config(tmp_path):
    (tmp_path / "vocab.json").write_text(json.dumps({"en": {"[PAD]": 0, "_": 1, "A": 2, "B": 3, "[UNK]": 4}}))
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({"pad_token": "<pad>", "unk_token": {"content": "[UNK]"}}))
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"pad_token": {"content": "[PAD]"}, "word_delimiter_token": "_", "target_lang": "en",
                                                                 "do_lower_case": True}))
    v = CT.CTCVocab.from_dir(str(tmp_path))
    assert v.text([2, 1, 3, 0, 9]) == "a b[unk]"
    assert CT.CTCVocab.from_dir(str(tmp_path / "nothing")) is None
    assert CT.load_vocab(str(tmp_path / "nothing")) is None


# ------------------------------------------------------------------------------- the launcher's refusals (no GPU: validation comes first)
def _good_args():
    from interspeech_ser_amd import _lib
    a = _lib.CtcGreedyArgs()
    a.z, a.ldz, a.frame_offs, a.work, a.work_elems = 4096, 16, 8192, 12288, 200          # never dereferenced
    a.ids, a.starts, a.ends, a.ld_tok, a.counts, a.err = 16384, 20480, 24576, 50, 28672, 32768
    a.B, a.V, a.rows, a.blank, a.max_frames = 2, 12, 100, 0, 50
    return a


@pytest.mark.parametrize("field, value, rc", [
    ("z", None, -1), ("frame_offs", None, -1), ("work", None, -1), ("ids", None, -1), ("starts", None, -1), ("ends", None, -1),
    ("counts", None, -1), ("err", None, -1),
    ("B", 0, -2), ("B", 65536, -2), ("V", 0, -2), ("rows", 0, -2), ("blank", -1, -2), ("blank", 12, -2), ("max_frames", 0, -2), ("work_elems", 199, -2),
    ("ldz", 8, -3), ("ldz", 14, -3), ("ld_tok", 49, -3), ("z", 4100, -3),
])
def test_ctc_greedy_refuses_bad_arguments(built_library, field, value, rc):
    from interspeech_ser_amd import _lib
    a = _good_args()
    setattr(a, field, value)
    assert _lib.lib.ser_ctc_greedy_v(ctypes.byref(a), None) == rc
    assert b"ser_ctc_greedy" in _lib.lib.ser_last_error()


def test_ctc_greedy_refuses_null_arguments_and_exports_its_chunk(built_library):
    import os
    import re
    from interspeech_ser_amd import _lib
    assert _lib.lib.ser_ctc_greedy_v(None, None) == -1 and b"ser_ctc_greedy" in _lib.lib.ser_last_error()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ser_hip.h")).read()
    assert int(re.search(r"#define SER_CTC_CHUNK (\d+)", header).group(1)) == _lib.CTC_CHUNK
    assert int(re.search(r"#define SER_CTC_ERR_NONFINITE (\d+)", header).group(1)) == _lib.CTC_ERR_NONFINITE
    assert "ser_ctc_greedy_v" in _lib.EXPORTED_SYMBOLS and _lib.STRUCT_MIRRORS["ser_ctc_greedy_args"] is _lib.CtcGreedyArgs


def test_blob_layout_round_trip():
    from interspeech_ser_amd.engine import CTCHead
    B, Tm = 3, 5
    n = CTCHead.blob_words(B, Tm)
    w = np.arange(n, dtype=np.int32)
    w[B + 3 * B * Tm: 2 * B + 3 * B * Tm] = np.array([0.5, 1.5, np.inf], dtype=np.float32).view(np.int32)
    w[:B] = [0, 2, 5]
    w[-1] = 0
    p = CTCHead.unpack(w, B, Tm)
    assert p["counts"].tolist() == [0, 2, 5] and p["ids"].shape == (B, Tm) and p["ids"][1, 0] == B + Tm and p["starts"][0, 0] == B + B * Tm
    assert p["ends"][2, 4] == B + 3 * B * Tm - 1 and p["min_margin"].tolist() == [0.5, 1.5, np.inf] and p["err"] == 0
    got = CT.split_blob(w.view(np.float32).reshape(-1, 1), B, Tm)
    assert got[0].ids == [] and got[1].ids == [B + Tm, B + Tm + 1] and got[2].offsets[4] == (int(p["starts"][2, 4]), int(p["ends"][2, 4]))
    w[-1] = 1
    with pytest.raises(RuntimeError, match="error word"):
        CT.split_blob(w, B, Tm)


# ------------------------------------------------------------------------------- the command line around a stub
class _Stub:
    """per-frame ids by length: what the device would return, keyed by the number of samples; short inputs fail alone"""
    SLOTS = 2
    hop = 320
    weight_source, mode = "stub", "f16x"

    def __init__(self, table):
        self.table, self.batches = table, []

    def _rows(self, waves):
        self.batches.append([len(w) for w in waves])
        if any(len(w) < 400 for w in waves):
            raise ValueError("an utterance shorter than one frame")
        out = []
        for w in waves:
            ids, starts, ends = R.collapse(self.table[len(w)], 0)
            out.append(CT.Transcript(ids, list(zip(starts, ends)), 1.0))
        return out

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


TABLE = {4000: [0, 6, 6, 5, 4, 7, 0], 5000: [0, 0, 0], 7000: [4, 8, 8, 0, 8, 3]}


@pytest.fixture
def wav_dir(tmp_path):
    d = tmp_path / "wavs"
    d.mkdir()
    _write_wav(d / "b.wav", 5000, seed=1)
    _write_wav(d / "a.wav", 4000, seed=2)
    _write_wav(d / "c.wav", 7000, seed=3)
    _write_wav(d / "short.wav", 100)
    return d


def _read_table(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def test_cli_writes_the_table_failures_and_offsets(built_library, wav_dir, tmp_path, capsys):
    stub = _Stub(TABLE)
    out_csv, offs = tmp_path / "out" / "t.csv", tmp_path / "offs.json"
    rc = CT.run(["--model", "stub", "--wav_dir", str(wav_dir), "--out_csv", str(out_csv), "--offsets_json", str(offs)],
                transcriber_factory=lambda a, d: stub, vocab=CT.CTCVocab(VOCAB))
    out = capsys.readouterr().out
    assert rc == 0
    assert _read_table(out_csv) == [["FileName", "transcription"], ["a.wav", "TE A"], ["b.wav", ""], ["c.wav", "OO<unk>"]]
    assert stub.batches == [[4000, 5000, 7000, 100], [4000], [5000], [7000], [100]]       # sorted order; the batch whole, then file by file
    assert f"Failed to process {wav_dir / 'short.wav'}: an utterance shorter than one frame" in out and "Wrote 3 of 4 transcripts" in out
    got = json.loads(offs.read_text())
    assert sorted(got) == ["a.wav", "b.wav", "c.wav"] and got["b.wav"] == []
    assert got["a.wav"] == [["T", 1 * 0.02, 3 * 0.02], ["E", 3 * 0.02, 4 * 0.02], [" ", 4 * 0.02, 5 * 0.02], ["A", 5 * 0.02, 6 * 0.02]]
    from interspeech_ser_amd.transcribe import read_table
    assert read_table(str(out_csv))["a.wav"] == "TE A"                     # the loader of --df_path / txt_dir reads it


def test_cli_writes_decimal_ids_without_vocabulary_files(built_library, wav_dir, tmp_path, capsys):
    out_csv = tmp_path / "t.csv"
    rc = CT.run(["--model", str(tmp_path / "no_such_snapshot"), "--wav_dir", str(wav_dir), "--out_csv", str(out_csv)],
                transcriber_factory=lambda a, d: _Stub(TABLE))
    assert rc == 0 and "writing token ids instead of text" in capsys.readouterr().out
    assert _read_table(out_csv)[1:] == [["a.wav", "6 5 4 7"], ["b.wav", ""], ["c.wav", "4 8 8 3"]]


def test_cli_refuses_other_sample_rates_without_resample(built_library, tmp_path, capsys):
    d = tmp_path / "w"
    d.mkdir()
    _write_wav(d / "a.wav", 4000, seed=2)
    _write_wav(d / "k8.wav", 4000, sr=8000, seed=4)
    stub = _Stub({4000: [6], 8000: [5]})
    CT.run(["--model", "stub", "--wav_dir", str(d), "--out_csv", str(tmp_path / "t.csv")], transcriber_factory=lambda a, dv: stub, vocab=CT.CTCVocab(VOCAB))
    assert "k8.wav: sample rate 8000 Hz" in capsys.readouterr().out and _read_table(tmp_path / "t.csv")[1:] == [["a.wav", "T"]]
    CT.run(["--model", "stub", "--wav_dir", str(d), "--out_csv", str(tmp_path / "t.csv"), "--resample"], transcriber_factory=lambda a, dv: stub,
           vocab=CT.CTCVocab(VOCAB))
    assert _read_table(tmp_path / "t.csv")[1:] == [["a.wav", "T"], ["k8.wav", "E"]]      # resampled on the host for a stub: 8 000 samples


def test_cli_set_up_errors_exit_0(wav_dir, tmp_path, capsys):
    def factory(args, device):
        raise OSError("no local checkpoint for stub")
    rc = CT.run(["--model", "stub", "--wav_dir", str(wav_dir), "--out_csv", str(tmp_path / "t.csv")], transcriber_factory=factory)
    assert rc == 0 and "No pretrained model found with the name stub" in capsys.readouterr().out


def test_head_mode_falls_back_in_one_line(capsys):
    assert CT.head_mode("bf16", "m") == "bf16" and CT.head_mode("f16mf", "m") == "f16x"
    assert capsys.readouterr().out.count("\n") == 1
    assert CT.frame_hop(C.TINY_WAVLM) == int(np.prod(C.TINY_WAVLM.conv_stride)) and CT.frame_hop(C.WAVLM_LARGE) == 320
    assert CT.frame_hop(C.TINY_W2V_BERT) == 160 * C.TINY_W2V_BERT.fbank_stride


# ------------------------------------------------------------------------------- the predictor's flag and method (no GPU)
def test_scoring_command_line_takes_transcribe_ctc(tmp_path, monkeypatch):
    import os
    from interspeech_ser_amd import predictor as PR
    seen = {}
    monkeypatch.setattr(PR, "score_from_wav", lambda config, encoders, layers, averages, checkpoints, **kw: seen.update(encoders=encoders, kw=kw))
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({}))
    argv = ["--config_path", str(cfg), "--encoder1", "facebook/hubert-xlarge-ls960-ft", "--encoder2", "roberta-large"]
    assert PR.main(argv + ["--transcribe_ctc"]) == 0
    assert seen["kw"]["transcribe_ctc"] is True and seen["kw"]["transcribe"] is False
    assert PR.main(argv + ["--transcribe"]) == 0
    assert seen["kw"]["transcribe_ctc"] is False and seen["kw"]["transcribe"] is True
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "interspeech_ser_amd.ctc import run" in open(os.path.join(root, "preprocessing", "transcribe_ctc.py")).read()


def test_transcribe_with_ctc_is_a_method_of_its_own():
    import inspect
    from interspeech_ser_amd.predictor import FusionPredictor
    assert list(inspect.signature(FusionPredictor.transcribe_with_ctc).parameters) == ["self", "head", "detokenize", "tokenize"]
    assert list(inspect.signature(FusionPredictor.transcribe_with).parameters) == ["self", "decoder", "spec", "tokenize", "detokenize"]
    assert "transcription needs a Whisper audio stream and a text stream" in inspect.getsource(FusionPredictor.transcribe_with)
