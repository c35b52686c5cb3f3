"""CPU: Whisper token timestamps (include/ser_hip.h "a33").  The numpy rule (tests/whisper_ts_ref.py) against transformers' own
``_median_filter``, ``_dynamic_time_warping`` and ``_extract_token_timestamps``; the fixture's own conditions
(tools/make_whisper_timestamps_golden.py); the word grouping against HF's functions on a stub tokenizer; ``GenerationSpec``'s
``alignment_heads``; the JSON writer; the binding."""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import whisper_ts_ref as TS                                                                     # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gw = pytest.importorskip("transformers.models.whisper.generation_whisper")


# ------------------------------------------------------------------------------------------------------------------ the rule against HF
@pytest.mark.parametrize("F", [1, 3, 4, 7, 8, 33])
def test_median_filter_equals_hf(F):
    z = np.random.default_rng(F).standard_normal((3, 5, F))
    assert np.array_equal(TS.median_filter(z, 7), gw._median_filter(torch.from_numpy(z)[None], 7)[0].numpy())


def _dtw_cases():
    g = np.random.default_rng(11)
    cases = {"random 5x9": g.standard_normal((5, 9)), "random 7x24": g.standard_normal((7, 24)), "constant": np.full((4, 6), 0.25),
             "N > M": g.standard_normal((9, 4)), "N = 1": g.standard_normal((1, 7)), "quantised ties": g.integers(-1, 2, (6, 11)).astype(float)}
    for M in (1, 3, 4):
        cases[f"M = {M}"] = g.standard_normal((3, M))
    cases["1 x 1"] = g.standard_normal((1, 1))
    cases["NaN row"] = np.full((1, 5), np.nan)
    return cases


@pytest.mark.parametrize("name", list(_dtw_cases()))
def test_dtw_equals_hf(name):
    m = _dtw_cases()[name].astype(np.float32)
    text, time, _ = TS.dtw(m)
    with np.errstate(invalid="ignore"):
        ht, hi = gw._dynamic_time_warping(-m.astype(np.float64))
    assert np.array_equal(text, ht) and np.array_equal(time, hi)
    first = TS.first_frames(text, time)
    assert len(first) == m.shape[0] and first[0] == 0
    dt, di, dc = TS.dtw_diag(m)                                             # the anti-diagonal order the GPU tests' large cases use
    assert np.array_equal(dt, text) and np.array_equal(di, time) and np.array_equal(dc.view(np.uint32), TS.dtw(m)[2].view(np.uint32))


@pytest.mark.parametrize("n,F,heads", [(6, 20, [(0, 1), (1, 0), (1, 1)]), (8, 4, [(1, 0)]), (3, 3, [(0, 0), (1, 1)]), (2, 9, [(0, 1)]),
                                       (1, 9, [(0, 1)]), (5, 33, [(0, 0), (0, 1), (1, 0), (1, 1)])])
def test_rule_equals_hf_extract_token_timestamps(n, F, heads):
    """HF's method on a float64 'generate output' of batch 1 with num_frames given: the same token times as the rule, and a matrix that
    agrees to float64 rounding (HF's std / mean reduce in another order)."""
    from transformers.generation.utils import GenerateEncoderDecoderOutput
    P, S = 4, 40
    g = np.random.default_rng(100 * n + F)
    att = g.random((2, 1, 2, P + n - 1, S)).astype(np.float32)                # [layer][batch][head][position][key]
    att /= att.sum(-1, keepdims=True)
    go = GenerateEncoderDecoderOutput(sequences=torch.zeros((1, P + n), dtype=torch.long),
                                      cross_attentions=(tuple(torch.from_numpy(att[l]).double() for l in range(2)),))
    fake = SimpleNamespace(config=SimpleNamespace(decoder_layers=2, median_filter_width=7))
    seen = []
    orig = gw._dynamic_time_warping
    gw._dynamic_time_warping = lambda neg: (seen.append(-np.array(neg)), orig(neg))[1]
    try:
        with np.errstate(invalid="ignore"):
            ts = gw.WhisperGenerationMixin._extract_token_timestamps(fake, go, heads, num_frames=2 * F, num_input_ids=P)[0].numpy()
    finally:
        gw._dynamic_time_warping = orig
    w = np.stack([att[l, 0, h, P:, :F] for l, h in heads])
    if n == 1:
        assert not seen and np.all(ts == 0)
        assert np.all(TS.token_times(np.zeros(0), 1) == 0)
        return
    m64 = TS.matrix64(w)
    if n == 2:
        assert np.isnan(m64).all() and np.isnan(seen[0]).all()
    else:
        assert np.abs(m64 - seen[0]).max() <= 1e-9 * max(1.0, np.abs(m64).max())
    text, time, _ = TS.dtw(m64.astype(np.float32))
    assert np.array_equal(TS.token_times(TS.first_frames(text, time), n), ts[P:])


def test_weights_rule_is_the_softmax_over_all_keys():
    g = np.random.default_rng(2)
    q, k = g.standard_normal((2, 3, 64)).astype(np.float32), g.standard_normal((2, 50, 64)).astype(np.float32)
    w = TS.weights(q, k, 0.125, 20)
    ref = torch.softmax(torch.einsum("ard,asd->ars", torch.from_numpy(q).double() * 0.125, torch.from_numpy(k).double()), -1)[..., :20]
    assert w.shape == (2, 3, 20) and np.abs(w - ref.numpy()).max() < 1e-8 and w.sum(-1).max() < 1.0


# ------------------------------------------------------------------------------------------------------------------ the fixture
def test_fixture_conditions(golden_dir):
    """Token-time equality follows from the matrix gate: every item's margin mu covers twice the worst change of a path's cost under the
    gate plus the fp32 cost table's rounding; the rule on HF's matrix gives HF's times; the head list spans two layers with two heads in
    one; no item is left out."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    path = os.path.join(golden_dir, "tiny_whisper_ts_d128h2.npz")
    assert os.path.getsize(path) < 64 * 1024
    f = np.load(path)
    heads = [tuple(h) for h in f["alignment_heads"]]
    assert len({l for l, _ in heads}) >= 2 and max(sum(1 for l, _ in heads if l == q) for q in {l for l, _ in heads}) >= 2
    assert len(f["lengths"]) >= 3 and len(set(f["frames"].tolist())) == len(f["frames"])
    for b in range(len(f["lengths"])):
        n, F = int(f["n_tokens"][b]), int(f["frames"][b])
        assert n <= 8 and F <= 24 and (int(f["lengths"][b]) // 160) // 2 == F
        m = f["matrix"][b, : n - 1, :F]
        assert np.isfinite(m).all()
        g = 1e-3 * max(1.0, np.abs(m).max())
        need = 2 * ((n - 1 + F - 1) * g + (n - 1 + F) ** 2 * 2.0 ** -24 * np.abs(m).max())
        assert abs(g - f["g"][b]) < 1e-15 and f["mu"][b] >= need and abs(need - f["needed"][b]) < 1e-12
        text, time, _ = TS.dtw(m.astype(np.float32))
        first = TS.first_frames(text, time)
        assert np.array_equal(TS.token_times(first, n), f["token_timestamps"][b, 4: 4 + n])
        import make_whisper_timestamps_golden as tool
        assert abs(tool.margin(m, first) - f["mu"][b]) < 1e-12


# ------------------------------------------------------------------------------------------------------------------ words
class StubTokenizer:
    """Byte-level pieces: decode joins the pieces' bytes and decodes with replacement, as a byte-level BPE tokenizer does."""
    eos_token_id = 100
    language = None

    def __init__(self, pieces):
        self.pieces = [p if isinstance(p, bytes) else p.encode() for p in pieces]

    def decode(self, ids, decode_with_timestamps=False, **kw):
        return b"".join(self.pieces[i] if i < self.eos_token_id else b"<|s|>" for i in ids).decode("utf-8", errors="replace")


def _hf_words(tok, ids, language):
    from transformers.models.whisper import tokenization_whisper as tw
    return tw._combine_tokens_into_words(tok, list(ids), language)


@pytest.mark.parametrize("language", ["english", "japanese", None])
def test_word_grouping_equals_hf(language):
    from interspeech_ser_amd.transcribe import combine_tokens_into_words
    e = "é".encode()
    pieces = [" Hel", "lo", ",", " wor", "ld", "!", " (", "a", ")", " caf", e[:1], e[1:], " \"", "q", "\"", " -", "x", ".", " 3", ".", "5", " ¿", "no", "?"]
    tok = StubTokenizer(pieces)
    for ids in (list(range(len(pieces))), [0, 1, 2], [10, 11], [3, 100, 4, 5], [6, 7, 8, 2, 17], [2, 5, 0], []):
        got = combine_tokens_into_words(tok, ids, language)
        ref = _hf_words(tok, ids, language)
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2], (ids, got, ref)


def test_token_words_spans():
    from interspeech_ser_amd.transcribe import token_spans, token_words
    tok = StubTokenizer([" a", "b", " c", "."])
    assert token_spans([0.0, 0.5, 0.75]) == [(0.0, 0.5), (0.5, 0.75), (0.75, 0.75)]
    words = token_words(tok, [0, 1, 2, 3], [0.1, 0.2, 0.4, 0.9])
    assert words == [(" ab", 0.1, 0.4), (" c.", 0.4, 0.9)]              # a word ends where the token behind it starts; the last one where it starts


# ------------------------------------------------------------------------------------------------------------------ spec, JSON, binding
def _gen_cfg(**extra):
    cfg = dict(decoder_start_token_id=1, eos_token_id=2, no_timestamps_token_id=5, lang_to_id={"<|en|>": 3}, task_to_id={"transcribe": 4})
    cfg.update(extra)
    return cfg


def test_generation_spec_reads_or_refuses_alignment_heads():
    from interspeech_ser_amd.config import GenerationSpec
    spec = GenerationSpec.from_config(_gen_cfg(alignment_heads=[[7, 0], [10, 17], [10, 2]]))
    assert spec.alignment_heads == ((7, 0), (10, 17), (10, 2)) and spec.require_alignment_heads() == spec.alignment_heads
    assert spec.median_filter_width == 7 and spec.TIME_PRECISION == 0.02
    bare = GenerationSpec.from_config(_gen_cfg())
    assert bare.alignment_heads == ()
    with pytest.raises(ValueError, match="alignment_heads"):
        bare.require_alignment_heads()
    with pytest.raises(OSError, match="alignment_heads"):
        GenerationSpec.from_config(_gen_cfg(alignment_heads=[[1, 2, 3]]))


def test_times_json_writer(tmp_path):
    from interspeech_ser_amd.transcribe import times_entry, write_times_json
    tok = StubTokenizer([" a", "b", " c", "."])
    entries = {"x.wav": times_entry([0, 1, 2, 3], [0.1, 0.2, 0.4, 0.9], " ab c.", tok), "y.wav": times_entry([2], [0.0], "2", None)}
    p = tmp_path / "t.json"
    write_times_json(str(p), entries)
    back = json.loads(p.read_text())
    assert back["x.wav"] == {"text": " ab c.", "tokens": [[0, 0.1, 0.2], [1, 0.2, 0.4], [2, 0.4, 0.9], [3, 0.9, 0.9]],
                             "words": [[" ab", 0.1, 0.4], [" c.", 0.4, 0.9]]}
    assert back["y.wav"] == {"text": "2", "tokens": [[2, 0.0, 0.0]]} and "words" not in back["y.wav"]


def test_binding_and_refusals(built_library):
    """The four entry points are declared, bound and refuse bad arguments before any launch (no GPU needed)."""
    import ctypes
    from interspeech_ser_amd import _lib
    header = open(os.path.join(ROOT, "include", "ser_hip.h")).read()
    for name in ("ser_dec_keep_q_v", "ser_ts_weights_v", "ser_ts_matrix_v", "ser_dtw_v", "ser_dtw_work_bytes"):
        assert name + "(" in header and name in _lib.EXPORTED_SYMBOLS
    for c, v in (("THREADS", _lib.TS_THREADS), ("BAND", _lib.TS_BAND), ("MAX_KEYS", _lib.TS_MAX_KEYS), ("MAX_HEADS", _lib.TS_MAX_HEADS),
                 ("KEEP_HEADS", _lib.TS_KEEP_HEADS), ("NONFINITE", _lib.TS_NONFINITE), ("BAD_SHAPE", _lib.TS_BAD_SHAPE), ("NO_FRAMES", _lib.TS_NO_FRAMES)):
        assert f"#define SER_TS_{c} {v}\n" in header
    assert "#define SER_OP_DEC_KEEP_Q 24" in header and _lib.OP_DEC_KEEP_Q == 24
    lib = _lib.lib
    assert lib.ser_dtw_work_bytes(16, 443, 1500) == 8 * 16 * 443 * 47 and lib.ser_dtw_work_bytes(1, 513, 10) == -1
    d = _lib.DtwArgs()
    assert lib.ser_dtw_v(ctypes.byref(d), None) == -1 and b"ser_dtw: null pointer" in lib.ser_last_error()
    d.matrix = d.n_rows = d.n_frames = d.work = d.first_frame = d.status = 256            # never dereferenced: validation comes first
    d.B, d.max_rows, d.max_frames, d.ld_m, d.ld_t = 1, 513, 8, 8, 513
    assert lib.ser_dtw_v(ctypes.byref(d), None) == -2 and b"max_rows=513" in lib.ser_last_error()
    d.max_rows, d.work_bytes = 8, 8
    assert lib.ser_dtw_v(ctypes.byref(d), None) == -2 and b"ser_dtw_work_bytes" in lib.ser_last_error()
    d.work_bytes, d.ld_m = 64, 4
    assert lib.ser_dtw_v(ctypes.byref(d), None) == -3
    m = _lib.TsMatrixArgs()
    m.w = m.n_rows = m.n_frames = m.stats = m.matrix = m.status = 256
    m.B, m.n_align, m.max_rows, m.max_frames, m.width, m.ld_w, m.ld_m = 1, 2, 4, 8, 6, 8, 8
    assert lib.ser_ts_matrix_v(ctypes.byref(m), None) == -2 and b"median width 6" in lib.ser_last_error()
    k = _lib.DecKeepQArgs()
    k.q = k.pos = k.keep = 256
    k.B, k.H, k.max_pos, k.n_heads, k.n_align, k.ldq = 1, 2, 8, 1, 1, 128
    k.head[0] = 2
    assert lib.ser_dec_keep_q_v(ctypes.byref(k), None) == -2 and b"head[0]=2" in lib.ser_last_error()
    cmds = (_lib.Cmd * 1)()
    cmds[0].op = _lib.OP_DEC_KEEP_Q
    assert lib.ser_run(cmds, 1, None, None) < 0 and b"ser_dec_keep_q" in lib.ser_last_error()
    w = _lib.TsWeightsArgs()
    assert lib.ser_ts_weights_v(ctypes.byref(w), None) == -1
