"""CPU: CTC forced alignment -- the numpy rule (tests/ctc_align_ref.py) against brute force, the feasibility rule, the fixtures' own greedy
ids against HF's offsets, the vocabulary's encoding of foreign text, forward_align's blob, ser_ctc_align_v's struct and refusals, the
command line around a stub."""
import ctypes
import itertools
import json
import os
import re
import wave

import numpy as np
import pytest

import ctc_align_ref as A
import ctc_ref as R
from interspeech_ser_amd import ctc as CT

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ser_hip.h")


# ------------------------------------------------------------------------------- the rule against brute force
def _tiny_cases():
    """every (T, target) with T <= 7, L <= 3, V in {2, 3}, blank 0, that has a path"""
    for V in (2, 3):
        toks = list(range(1, V))
        for L in range(0, 4):
            for y in ([list(t) for t in itertools.product(toks, repeat=L)]):
                for T in range(1, 8):
                    if A.feasible(T, y):
                        yield V, T, y


def test_rule_equals_brute_force_on_integer_logits():
    """integer-level logits from {-1, 0, 1}, so ties occur in most cases: the score and the tie-broken path must both agree"""
    rng = np.random.default_rng(7)
    n = tied = 0
    for V, T, y in _tiny_cases():
        for _ in range(2):
            z = rng.integers(-1, 2, size=(T, V)).astype(np.float32)
            best, paths = A.brute_force(z, y, 0)
            got = A.align(z, y, V, 0)
            assert got["status"] == 0
            assert np.float64(got["path_logit"]) == best, (V, T, y)
            assert tuple(int(s) for s in got["states"]) == A.tie_broken(paths), (V, T, y, z)
            n += 1
            tied += len(paths) > 1
    assert n > 150 and tied > n // 3


def test_all_equal_logits_take_the_earliest_path():
    """every path ties: the end state is S - 2, and walking back from it stay beats step beats skip, so the path stays in the last token
    for as long as that state is reachable: one frame per token from frame 0 on (skips over the blanks), the last token to the end"""
    got = A.align(np.zeros((7, 4), dtype=np.float32), [1, 2, 3], 4, 0)
    assert got["states"].tolist() == [1, 3, 5, 5, 5, 5, 5] and got["pos"].tolist() == [0, 1, 2, 2, 2, 2, 2]
    assert got["starts"].tolist() == [0, 1, 2] and got["ends"].tolist() == [1, 2, 7]
    got = A.align(np.zeros((7, 4), dtype=np.float32), [1, 1, 3], 4, 0)                    # a repeat: no skip over the blank between
    assert got["states"].tolist() == [1, 2, 3, 5, 5, 5, 5]


@pytest.mark.parametrize("y", [[1], [1, 1], [1, 2, 2, 2, 3], [2, 2, 2, 2], [1, 2, 1, 2], []])
def test_feasibility_rule_at_its_edge(y):
    """at T = L + rep - 1 no path is finite, at L + rep exactly one is, at L + rep + 5 many are; the trellis itself is the witness"""
    rng = np.random.default_rng(len(y))
    need = len(y) + A.n_repeats(y)
    for T in (need - 1, need, need + 5):
        if T < 1:
            assert not A.feasible(T, y)
            continue
        z = rng.integers(-3, 4, size=(T, 4)).astype(np.float32)
        score, _ = A.trellis(z, y, 0)
        assert A.feasible(T, y) == bool(np.isfinite(score)) == (T >= max(need, 1))
        assert A.align(z, y, 4, 0)["status"] == (0 if T >= max(need, 1) else A.INFEASIBLE)


def test_status_rules():
    z = np.zeros((6, 5), dtype=np.float32)
    assert A.align(z, [1, 0], 5, 0)["status"] == A.BAD_TARGET and A.align(z, [5], 5, 0)["status"] == A.BAD_TARGET
    assert A.align(z, [1] * 3, 5, 0, max_tokens=2)["status"] == A.BAD_TARGET
    bad = z.copy()
    bad[2, 1] = np.nan
    assert A.align(bad, [1, 2], 5, 0)["status"] == A.NONFINITE and A.align(bad, [2, 3], 5, 0)["status"] == 0
    bad[2, 1] = np.inf
    assert A.align(bad, [1, 2], 5, 0)["status"] == A.NONFINITE
    bad[2, 1] = -np.inf
    assert A.align(bad, [1, 2], 5, 0)["status"] == 0
    noblank = z.copy()
    noblank[:, 0] = -np.inf
    assert A.align(noblank, [1, 1], 5, 0)["status"] == A.NONFINITE and A.align(noblank[:2], [1, 2], 5, 0)["status"] == 0


# ------------------------------------------------------------------------------- the fixtures: greedy ids -> HF's offsets
@pytest.mark.parametrize("name", R.FIXTURES)
def test_aligning_the_greedy_ids_gives_hf_offsets(name):
    """The greedy frame sequence is the unconstrained per-frame optimum and a valid path of its own collapse; with every margin positive
    it is the unique best path, so the rule's spans are HF's char offsets."""
    fx = R.Fixture(name)
    assert len(fx.ids) == 4
    for z64, ids, offsets, fid in zip(fx.logits64, fx.ids, fx.offsets, fx.frame_ids):
        z = np.asarray(z64, dtype=np.float32)
        assert R.margins64(z.astype(np.float64)).min() > 0
        got = A.align(z, ids, fx.V, fx.blank)
        assert got["status"] == 0
        assert list(zip(got["starts"].tolist(), got["ends"].tolist())) == offsets
        assert np.array_equal(A.labels(ids, fx.blank)[got["states"]], np.asarray(fid))
        assert got["path_logit"] == np.float64(z.astype(np.float64).max(axis=1).cumsum()[-1])


# ------------------------------------------------------------------------------- the vocabulary: text that is not its own
UPPER = {"<pad>": 0, "<s>": 1, "</s>": 2, "<unk>": 3, "|": 4, "E": 5, "T": 6, "A": 7, "O": 8, "N": 9, "'": 10, "S": 11}


def test_encode_words_cases():
    v = CT.CTCVocab(UPPER)
    assert v.encode_words("Tea's on") == [("Tea's", [6, 5, 7, 10, 11]), ("on", [8, 9])]                       # mixed case, an apostrophe
    assert v.encode("Tea's on") == [6, 5, 7, 10, 11, 4, 8, 9]
    assert v.encode_words("no, 2 teas!") == [("no,", [9, 8]), ("2", []), ("teas!", [6, 5, 7, 11])]            # digits and punctuation dropped
    assert v.encode("no, 2 teas!") == [9, 8, 4, 6, 5, 7, 11]                                                  # no delimiter doubled around "2"
    assert v.encode("42 tea") == [6, 5, 7] and v.encode("tea 42") == [6, 5, 7]                                # none at either end
    assert v.encode_words("") == [] and v.encode("") == [] and v.encode("  \n") == []
    assert v.encode_words("<s> | <unk>") == [("<s>", [11]), ("|", []), ("<unk>", [9])]                        # specials never match whole
    assert v.encode("straße") == [11, 6, 7, 11, 11, 5]                                                        # "ß".upper() == "SS"
    lower = CT.CTCVocab({"<pad>": 0, "a": 1, "t": 2})                                                         # no delimiter in the vocabulary
    assert lower.encode_words("At TA") == [("At", [1, 2]), ("TA", [2, 1])] and lower.encode("At TA") == [1, 2, 2, 1]
    assert v.text(v.encode("Tea's on")) == "TEA'S ON"                                                          # chars() inverts it


def test_words_from_token_means():
    v = CT.CTCVocab(UPPER)
    enc = v.encode_words("tea 7 on")
    ids = v.join(enc)
    spans = [(0, 2), (2, 3), (5, 6), (6, 7), (8, 11), (11, 12)]
    sc = [-1.0, -2.0, -4.0, -0.5, -1.0, -3.0]
    al = CT.Alignment(ids, spans, sc, -1.0, 0.0, None, None)
    got = CT.words(al, enc)
    assert got[0] == ("tea", 0, 6, (-1.0 * 2 - 2.0 - 4.0) / 4) and got[1] == ("7", None, None, None)
    assert got[2] == ("on", 8, 12, (-1.0 * 3 - 3.0) / 4)
    with pytest.raises(ValueError):
        CT.words(CT.Alignment(ids[:-1], spans[:-1], sc[:-1], 0.0, 0.0, None, None), enc)


# ------------------------------------------------------------------------------- the blob, the struct, the refusals
def test_align_blob_layout_round_trip():
    from interspeech_ser_amd.engine import CTCHead
    for B, Lm, rows in ((3, 4, 0), (2, 3, 7), (1, 0, 2)):
        n = CTCHead.align_words(B, Lm, rows)
        Lp = max(Lm, 1)
        w = np.arange(n, dtype=np.int32)
        o = B + 3 * B * Lp
        o += o & 1
        assert o % 2 == 0 and n == o + 2 * B + 2 * rows
        w[o: o + 2 * B] = np.arange(B, dtype=np.float64).view(np.int32) if B else []
        p = CTCHead.unpack_align(w, B, Lm, rows)
        assert p["status"].tolist() == list(range(B)) and p["starts"].shape == (B, Lp) and p["starts"][0, 0] == B
        assert p["ends"][0, 0] == B + B * Lp and p["tok_score"].dtype == np.float32 and p["tok_score"].view(np.int32)[0, 0] == B + 2 * B * Lp
        assert p["path_logit"].tolist() == [float(b) for b in range(B)]
        assert ("pos" in p) == bool(rows)
        if rows:
            assert p["pos"].tolist() == list(range(o + 2 * B, o + 2 * B + rows)) and p["frame_score"].shape == (rows,)


def test_split_align_blob_fails_an_utterance_alone():
    from interspeech_ser_amd import _lib
    from interspeech_ser_amd.engine import CTCHead
    targets, frame_offs = [[5, 6], [7], [5, 5]], [0, 4, 6, 8]
    w = np.zeros(CTCHead.align_words(3, 2, 8), dtype=np.int32)
    p = CTCHead.unpack_align(w, 3, 2, 8)
    p["status"][2] = _lib.CTC_ALIGN_INFEASIBLE
    p["starts"][0], p["ends"][0], p["starts"][1, 0], p["ends"][1, 0] = [0, 2], [2, 3], 1, 2
    p["tok_score"][0], p["path_logit"][1] = [-0.5, -1.5], 12.5
    p["frame_score"][:] = -np.arange(8, dtype=np.float32)
    p["pos"][:4] = [0, 0, 1, -1]
    got = CT.split_align_blob(w, frame_offs, targets)
    assert got[0].ids == [5, 6] and got[0].spans == [(0, 2), (2, 3)] and got[0].tok_scores == [-0.5, -1.5] and got[0].score == -1.5
    assert got[0].pos.tolist() == [0, 0, 1, -1] and got[1].spans == [(1, 2)] and got[1].path_logit == 12.5 and got[1].score == -4.5
    assert isinstance(got[2], CT.AlignmentError) and got[2].status == _lib.CTC_ALIGN_INFEASIBLE and "2 frames are too few" in str(got[2])


def _good_args():
    from interspeech_ser_amd import _lib
    a = _lib.CtcAlignArgs()
    a.z, a.ldz, a.frame_offs, a.targets, a.tgt_offs = 4096, 16, 8192, 12288, 16384                # never dereferenced
    a.work, a.work_bytes = 20480, _lib.lib.ser_ctc_align_work_bytes(100, 2, 50, 20)
    a.starts, a.ends, a.tok_score, a.ld_tok, a.status, a.path_logit = 24576, 28672, 32768, 20, 36864, 40960
    a.B, a.V, a.rows, a.blank, a.max_frames, a.max_tokens, a.n_targets = 2, 12, 100, 0, 50, 20, 30
    return a


@pytest.mark.parametrize("field, value, rc", [
    ("z", None, -1), ("frame_offs", None, -1), ("targets", None, -1), ("tgt_offs", None, -1), ("work", None, -1), ("starts", None, -1),
    ("ends", None, -1), ("tok_score", None, -1), ("status", None, -1), ("path_logit", None, -1),
    ("B", 0, -2), ("B", 65536, -2), ("V", 0, -2), ("rows", 0, -2), ("blank", -1, -2), ("blank", 12, -2), ("max_frames", 0, -2),
    ("max_tokens", -1, -2), ("max_tokens", 1024, -2), ("n_targets", -1, -2), ("work_bytes", 100 * 16 + 2 * 50 * 16 - 1, -2),
    ("ldz", 11, -3), ("ld_tok", 19, -3), ("z", 4098, -3), ("work", 20484, -3), ("path_logit", 40964, -3),
])
def test_ctc_align_refuses_bad_arguments(built_library, field, value, rc):
    """return codes only: validation comes before any launch (no GPU needed)"""
    from interspeech_ser_amd import _lib
    a = _good_args()
    setattr(a, field, value)
    assert _lib.lib.ser_ctc_align_v(ctypes.byref(a), None) == rc
    assert b"ser_ctc_align" in _lib.lib.ser_last_error()


def test_ctc_align_constants_and_work_rule(built_library):
    from interspeech_ser_amd import _lib
    assert _lib.lib.ser_ctc_align_v(None, None) == -1 and b"ser_ctc_align" in _lib.lib.ser_last_error()
    header = open(HEADER).read()
    for c in ("THREADS", "MAX_TOKENS", "INFEASIBLE", "NONFINITE", "BAD_TARGET"):
        assert int(re.search(rf"#define SER_CTC_ALIGN_{c} (\d+)", header).group(1)) == getattr(_lib, "CTC_ALIGN_" + c), c
    assert (_lib.CTC_ALIGN_INFEASIBLE, _lib.CTC_ALIGN_NONFINITE, _lib.CTC_ALIGN_BAD_TARGET) == (A.INFEASIBLE, A.NONFINITE, A.BAD_TARGET)
    assert _lib.CTC_ALIGN_MAX_TOKENS >= 1023 and _lib.CTC_ALIGN_THREADS % _lib.WAVE == 0
    assert "ser_ctc_align_v" in _lib.EXPORTED_SYMBOLS and _lib.STRUCT_MIRRORS["ser_ctc_align_args"] is _lib.CtcAlignArgs
    wb = _lib.lib.ser_ctc_align_work_bytes
    assert wb(100, 2, 50, 20) == 16 * 100 + 2 * 50 * 16 * 1 and wb(100, 2, 50, 32) == 16 * 100 + 2 * 50 * 16 * 2      # 41 and 65 states
    assert wb(8000, 16, 1500, 1023) == 16 * 8000 + 16 * 1500 * 16 * 32 and wb(8000, 16, 1500, 1023) < 16 * (1 << 20)   # under 1 MB per utterance
    assert wb(0, 1, 1, 1) == -1 and wb(1, 0, 1, 1) == -1 and wb(1, 1, 0, 1) == -1 and wb(1, 1, 1, 1024) == -1 and wb(1, 1, 1, 0) == 32


# ------------------------------------------------------------------------------- the command line around a stub
VOCAB = R.tiny_vocab(12, 0)                    # <pad> 0, | 1, <unk> 2, A 3, B 4, ...


class _Stub:
    """aligns with the numpy rule on logits made from the number of samples; short inputs fail their batch, then alone"""
    SLOTS = 2
    hop = 320
    weight_source, mode = "stub", "f16x"

    def __init__(self):
        self.batches = []

    def _rows(self, waves, targets):
        self.batches.append([len(w) for w in waves])
        if any(len(w) < 400 for w in waves):
            raise ValueError("an utterance shorter than one frame")
        out = []
        for w, y in zip(waves, targets):
            T = len(w) // 320
            z = np.random.default_rng(len(w)).integers(-4, 5, size=(T, 12)).astype(np.float32)
            r = A.align(z, y, 12, 0)
            if r["status"]:
                out.append(CT.AlignmentError(r["status"], T, len(y)))
                continue
            fs = r["frame_score"]
            out.append(CT.Alignment(list(y), list(zip(r["starts"].tolist(), r["ends"].tolist())), [float(v) for v in r["tok_score"]],
                                    float(fs.astype(np.float64).mean()), float(r["path_logit"]), r["pos"], fs))
        return out

    def submit(self, waves, targets, slot=0, rates=None):
        return dict(rows=self._rows(waves, targets))

    def collect(self, ticket):
        return ticket["rows"]

    def extract(self, waves, targets=None, rates=None):
        return self._rows(waves, targets)


def _write_wav(path, n, sr=16000, seed=0):
    pcm = (np.random.default_rng(seed).standard_normal(n) * 3000).astype(np.int16)
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


@pytest.fixture
def wav_dir(tmp_path):
    d = tmp_path / "wavs"
    d.mkdir()
    for name, n, seed in (("a.wav", 6400, 1), ("b.wav", 4800, 2), ("c.wav", 3200, 3), ("d.wav", 6400, 4), ("e.wav", 960, 5)):
        _write_wav(d / name, n, seed=seed)
    return d


def _table(path, rows):
    from interspeech_ser_amd.transcribe import write_table
    write_table(str(path), [n for n, _ in rows], [t for _, t in rows])


def test_run_align_writes_words_and_fails_files_alone(built_library, wav_dir, tmp_path, capsys):
    """a.wav aligns; b.wav has only digits; c.wav is missing from the table; d.wav aligns with an unalignable word inside; e.wav has 3
    frames for 5 tokens (status: fails alone, its batch mates are not run again)"""
    table = tmp_path / "t.csv"
    _table(table, [("a.wav", "Bad cab"), ("b.wav", "1234 56"), ("d.wav", "a 22 fee."), ("e.wav", "abcde")])
    stub, out_json = _Stub(), tmp_path / "out" / "a.json"
    rc = CT.run_align(["--model", "stub", "--wav_dir", str(wav_dir), "--df_path", str(table), "--out_json", str(out_json), "--chars"],
                      aligner_factory=lambda a, d: stub, vocab=CT.CTCVocab(VOCAB))
    out = capsys.readouterr().out
    assert rc == 0 and stub.batches == [[6400, 6400, 960]]                                   # one batch, nothing re-run
    assert f"Failed to process {wav_dir / 'b.wav'}:" in out and "has no word the vocabulary can spell" in out
    assert f"Failed to process {wav_dir / 'c.wav'}:" in out and "no row for it" in out
    assert f"Failed to process {wav_dir / 'e.wav'}: 3 frames are too few for a target of 5 tokens" in out
    assert "Wrote 2 of 5 alignments" in out and "3 files failed" in out
    got = json.loads(out_json.read_text())
    assert sorted(got) == ["a.wav", "d.wav"]
    a = got["a.wav"]
    assert sorted(a) == ["chars", "score", "words"] and [w[0] for w in a["words"]] == ["Bad", "cab"] and a["score"] < 0
    assert [c[0] for c in a["chars"]] == ["B", "A", "D", " ", "C", "A", "B"]
    ref = A.align(np.random.default_rng(6400).integers(-4, 5, size=(20, 12)).astype(np.float32), CT.CTCVocab(VOCAB).encode("Bad cab"), 12, 0)
    assert a["words"][0][1:3] == [ref["starts"][0] * 0.02, ref["ends"][2] * 0.02] and a["words"][1][1:3] == [ref["starts"][4] * 0.02, ref["ends"][6] * 0.02]
    assert a["chars"][3][1:3] == [ref["starts"][3] * 0.02, ref["ends"][3] * 0.02] and a["chars"][3][3] == pytest.approx(float(ref["tok_score"][3]))
    assert a["score"] == pytest.approx(float(ref["frame_score"].astype(np.float64).mean()))
    d = got["d.wav"]["words"]
    assert [w[0] for w in d] == ["a", "22", "fee."] and d[1][1:] == [None, None, None] and d[0][2] <= d[2][1]


def test_run_align_retries_a_failing_batch_file_by_file(built_library, tmp_path, capsys):
    d = tmp_path / "w"
    d.mkdir()
    _write_wav(d / "a.wav", 6400, seed=1)
    _write_wav(d / "short.wav", 100, seed=2)
    table = tmp_path / "t.csv"
    _table(table, [("a.wav", "cab"), ("short.wav", "cab")])
    stub, out_json = _Stub(), tmp_path / "a.json"
    assert CT.run_align(["--model", "stub", "--wav_dir", str(d), "--df_path", str(table), "--out_json", str(out_json)],
                        aligner_factory=lambda a, dev: stub, vocab=CT.CTCVocab(VOCAB)) == 0
    assert stub.batches == [[6400, 100], [6400], [100]]
    out = capsys.readouterr().out
    assert f"Failed to process {d / 'short.wav'}: an utterance shorter than one frame" in out
    got = json.loads(out_json.read_text())
    assert sorted(got) == ["a.wav"] and "chars" not in got["a.wav"]


def test_run_align_needs_a_vocabulary(built_library, wav_dir, tmp_path, capsys):
    table = tmp_path / "t.csv"
    _table(table, [("a.wav", "cab")])
    called = []
    rc = CT.run_align(["--model", str(tmp_path / "no_such_snapshot"), "--wav_dir", str(wav_dir), "--df_path", str(table),
                       "--out_json", str(tmp_path / "a.json")], aligner_factory=lambda a, d: called.append(1))
    out = capsys.readouterr().out
    assert rc == 0 and not called and "needs the checkpoint's vocabulary (vocab.json)" in out and not (tmp_path / "a.json").exists()
