"""CPU: the float64 statement of the Whisper decoder and of greedy generation (tests/whisper_dec_ref.py) against HF's recorded logits and
tokens (tests/golden/tiny_whisper_dec_d128h2.npz, tools/make_whisper_decoder_golden.py), the fixture's own conditions, and the host-side
pieces of the transcription path: geometry and GenerationSpec parsing, the transcript table, the C ABI's new names."""
import json
import os
from dataclasses import replace as dataclasses_replace

import numpy as np
import pytest

import whisper_dec_ref as R
from interspeech_ser_amd import config as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    return R.load_fixture(golden_dir)


@pytest.fixture(scope="module")
def ref_a(fx):
    gold, geo, sd, spec, enc = fx
    return R.generate(geo, sd, spec, enc)


def test_fixture_is_small_enough(golden_dir):
    size = os.path.getsize(os.path.join(golden_dir, "tiny_whisper_dec_d128h2.npz"))
    assert size <= 1 << 20 and size <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if "whisper_dec" not in f)


def test_reference_step_agrees_with_hf_logits_at_every_position(fx):
    """teacher-forced along HF's own greedy path: the float64 statement against HF's float64 logits (stored as fp32: 2^-24 relative)"""
    gold, geo, sd, spec, enc = fx
    for tag, e, seqs in (("a", enc, gold["a_sequences"]), ("l", enc, gold["l_sequences"])):
        for b in range(seqs.shape[0]):
            ours = R.teacher_forced(geo, sd, e[b], seqs[b])
            err = np.abs(ours - gold[tag + "_logits"][b]).max()
            assert err <= 1e-5, (tag, b, err)


def test_reference_loop_reproduces_hf_generation(fx, ref_a):
    gold, geo, sd, spec, enc = fx
    assert np.array_equal(ref_a["sequences"], gold["a_sequences"])          # tokens, eos / pad tails and the stop step (the length)
    assert np.array_equal(ref_a["languages"], gold["a_languages"])
    for b, lst in enumerate(ref_a["lists"]):
        row = gold["a_sequences"][b, spec.PROMPT_LEN:].tolist()
        assert lst == (row[:row.index(spec.eos_token_id)] if spec.eos_token_id in row else row)
    given = R.generate(geo, sd, spec, enc, language=int(gold["l_language"]))
    assert np.array_equal(given["sequences"], gold["l_sequences"])


def test_fixture_conditions_hold(fx, ref_a):
    gold, geo, sd, spec, enc = fx
    seq, logits = gold["a_sequences"], gold["a_logits"].astype(np.float64)
    m = R.masks(spec, geo.decoder_vocab_size)
    dec = R.decided(seq, spec)
    g = R.gate(logits, seq, spec)
    margins = [R.top2_margin(logits[b, p] + m[2 if p == 0 else 1 if p == 3 else 0]) for b, p in dec]
    assert min(margins) >= 4 * g, (min(margins), g)
    assert min(ref_a["margins"].values()) >= 4 * g                          # the reference's own margins: the same decisions
    assert sorted(ref_a["margins"]) == sorted(dec)
    gen = [tuple(seq[b, spec.PROMPT_LEN:]) for b in range(3)]
    assert len(set(gen)) == 3
    assert len({t for row in gen for t in row}) >= 12
    ends = sorted(row.index(spec.eos_token_id) if spec.eos_token_id in row else len(row) for row in gen)
    assert ends[0] + 3 <= ends[1] and ends[0] >= 3                          # one row finishes mid-sequence, >= 3 steps before the others
    b0 = int(np.argmin([row.index(spec.eos_token_id) if spec.eos_token_id in row else 99 for row in gen]))
    assert all(t == spec.pad_token_id for t in gen[b0][ends[0] + 1:])       # its pad tail
    assert any(int(np.argmax(logits[b, p])) in spec.suppress_tokens for b, p in dec if p >= 3)
    assert any(int(np.argmax(logits[b, 3] + m[0])) in spec.begin_suppress_tokens for b in range(3))
    assert (geo.decoder_vocab_size - 51866) % 8 == 0 and geo.decoder_vocab_size % 8 != 0     # the vocabulary padding path is live
    # case "b" (plumbing): the same margin bar; its rows may coincide
    seq_b, log_b = gold["b_sequences"], gold["b_logits"].astype(np.float64)
    gb = R.gate(log_b, seq_b, spec)
    assert min(R.top2_margin(log_b[b, p] + m[2 if p == 0 else 1 if p == 3 else 0]) for b, p in R.decided(seq_b, spec)) >= 4 * gb
    # the given-language path: every generated position
    seq_l, log_l = gold["l_sequences"], gold["l_logits"].astype(np.float64)
    gl = R.gate(log_l, seq_l, spec)
    assert min(R.top2_margin(log_l[b, p] + m[1 if p == 3 else 0]) for b, p in R.decided(seq_l, spec) if p > 0) >= 4 * gl


def test_geometry_and_generation_spec_parse(tmp_path):
    cfg = dict(model_type="whisper", d_model=1280, encoder_layers=32, encoder_attention_heads=20, encoder_ffn_dim=5120, num_mel_bins=128,
               max_source_positions=1500, decoder_layers=32, decoder_attention_heads=20, decoder_ffn_dim=5120, vocab_size=51866,
               max_target_positions=448)
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    geo = C.resolve_geometry(str(tmp_path))
    want = C.WHISPER_LARGE_V3
    assert (geo.decoder_layers, geo.decoder_attention_heads, geo.decoder_ffn_dim, geo.decoder_vocab_size, geo.max_target_positions) == (32, 20, 5120, 51866, 448)
    assert (want.decoder_layers, want.decoder_attention_heads, want.decoder_ffn_dim, want.decoder_vocab_size, want.max_target_positions) == (32, 20, 5120, 51866, 448)
    assert C.TINY_WHISPER.decoder is None and C.TINY_WHISPER.decoder_layers == 0 and C.TINY_WHISPER.max_target_positions == 448   # additive
    assert geo == dataclasses_replace(geo) and dataclasses_replace(geo).decoder is None          # an encoder geometry compares as before
    gen = dict(decoder_start_token_id=50258, eos_token_id=50257, pad_token_id=50257, suppress_tokens=[1, 2, 7], begin_suppress_tokens=[220, 50257],
               no_timestamps_token_id=50364, lang_to_id={"<|en|>": 50259, "<|de|>": 50261}, task_to_id={"transcribe": 50360, "translate": 50359},
               max_length=448)
    (tmp_path / "generation_config.json").write_text(json.dumps(gen))
    spec = C.GenerationSpec.from_snapshot(str(tmp_path))
    assert (spec.decoder_start_token_id, spec.eos_token_id, spec.pad_token_id, spec.no_timestamps_token_id, spec.task_id) == (50258, 50257, 50257, 50364, 50360)
    assert spec.suppress_tokens == (1, 2, 7) and spec.begin_suppress_tokens == (220, 50257) and spec.lang_ids == (50259, 50261)
    assert spec.max_length == 448 and spec.language is None
    assert C.GenerationSpec.from_snapshot(str(tmp_path), "en").language == 50259
    assert C.GenerationSpec.from_snapshot(str(tmp_path / "model.safetensors"), "<|de|>").language == 50261
    with pytest.raises(ValueError):
        C.GenerationSpec.from_snapshot(str(tmp_path), "xx")
    (tmp_path / "generation_config.json").write_text(json.dumps({k: v for k, v in gen.items() if k != "lang_to_id"}))
    with pytest.raises(OSError):
        C.GenerationSpec.from_snapshot(str(tmp_path))


def test_transcript_table_round_trip(tmp_path):
    """what the driver's writer writes is what score_from_wav's / preprocess_roberta.py's reader reads"""
    from interspeech_ser_amd import transcribe as T
    names = ["a.wav", "b, c.wav", "d.wav"]
    texts = ["hello there", 'she said "no", twice', "12 7 99"]
    path = str(tmp_path / "whisper_transcripts.csv")
    T.write_table(path, names, texts)
    assert open(path).readline().strip() == "FileName,transcription"
    assert T.read_table(path) == dict(zip(names, texts))
    import inspect
    from interspeech_ser_amd import predictor
    assert "read_table(config[\"txt_dir\"])" in inspect.getsource(predictor.score_from_wav)      # score_from_wav's loader IS read_table


def test_new_symbols_are_declared_and_bound(built_library):
    from interspeech_ser_amd import _lib
    header = open(os.path.join(ROOT, "include", "ser_hip.h")).read()
    for name in ("ser_dec_embed_v", "ser_dec_attn_v", "ser_dec_select_v"):
        assert name + "(" in header and name in _lib.EXPORTED_SYMBOLS
    for op, val in (("DEC_EMBED", 10), ("DEC_ATTN", 11), ("DEC_SELECT", 12)):
        assert f"#define SER_OP_{op} {val}" in header and getattr(_lib, "OP_" + op) == val
    assert _lib.ABI_VERSION == 18
    import ctypes
    a = _lib.DecAttnArgs()
    assert _lib.lib.ser_dec_attn_v(ctypes.byref(a), None) < 0 and b"ser_dec_attn" in _lib.lib.ser_last_error()
    s = _lib.DecSelectArgs()
    assert _lib.lib.ser_dec_select_v(ctypes.byref(s), None) < 0 and b"ser_dec_select" in _lib.lib.ser_last_error()
    e = _lib.DecEmbedArgs()
    assert _lib.lib.ser_dec_embed_v(ctypes.byref(e), None) < 0 and b"ser_dec_embed" in _lib.lib.ser_last_error()
