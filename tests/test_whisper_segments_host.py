"""CPU: the segment-timestamp rule (tests/whisper_seg_ref.py) is HF's three logits processors in HF's order, ``transcribe.segments_of`` is
HF's ``_retrieve_segment``, the fixture meets the conditions it was searched for, and the host side of the feature (spec, refusals)."""
import os
import sys
import types

import numpy as np
import pytest

import whisper_dec_ref as R
import whisper_seg_ref as SR
from interspeech_ser_amd import config as C
from interspeech_ser_amd import transcribe as T
from interspeech_ser_amd.transcribe import segments_of, window_frames         # the feature's host entry points: the module needs them

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, EOS, NO_TS, TSB, P = 64, 40, 47, 48, 3                  # text < eos < specials < no_timestamps < 16 timestamp tokens
SUPPRESS, BEGIN = (5, 6, 41, 42, 43, 44, 45, 46), (7, EOS)
TS = lambda k: TSB + k


def hf_chain(scores, gen, max_initial):
    """HF's processors in ``generate``'s order on one row: float64 scores [V], the generated ids behind a prompt of 3."""
    import torch
    from transformers.generation.logits_process import (SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor,
                                                        WhisperTimeStampLogitsProcessor)
    gc = types.SimpleNamespace(no_timestamps_token_id=NO_TS, eos_token_id=EOS, bos_token_id=EOS + 1, max_initial_timestamp_index=max_initial)
    ids = torch.tensor([[EOS + 1, EOS + 2, EOS + 3] + [int(t) for t in gen]], dtype=torch.long)
    s = torch.from_numpy(np.asarray(scores, dtype=np.float64))[None].clone()
    for proc in (SuppressTokensAtBeginLogitsProcessor(list(BEGIN), begin_index=P), SuppressTokensLogitsProcessor(list(SUPPRESS)),
                 WhisperTimeStampLogitsProcessor(gc, begin_index=P)):
        s = proc(ids, s)
    return s[0].numpy()


def mask_row(first: bool) -> np.ndarray:
    m = np.zeros(V)
    m[list(SUPPRESS)] = -np.inf
    if first:
        m[list(BEGIN)] = -np.inf
    return m


def base_scores(seed: int) -> np.ndarray:
    return 2.0 * np.random.default_rng(seed).standard_normal(V)


def _cases():
    """(name, scores, generated ids, max_initial, what must hold of the rule's outcome)"""
    out = []
    z = base_scores(1)
    out.append(("n0", z, [], None, None))
    z = base_scores(2)
    z[TS(12)] = 9.0                                          # the raw winner lies behind max_initial
    out.append(("n0-max-initial", z, [], 5, lambda r: TSB <= r["tok"] <= TS(5)))
    out.append(("n1-text", base_scores(3), [10], None, None))
    out.append(("n1-timestamp", base_scores(4), [TS(2)], None, lambda r: r["tok"] < TSB))
    out.append(("text-text", base_scores(5), [TS(0), 10, 11], None, None))
    z = base_scores(6)
    z[12] = 9.0                                              # text would win; only a timestamp or eos may follow [text, timestamp]
    out.append(("text-timestamp", z, [TS(0), 10, TS(4)], None, lambda r: r["tok"] >= EOS))
    z = base_scores(7)
    z[TS(9)] = 9.0
    out.append(("timestamp-timestamp", z, [TS(0), 10, TS(4), TS(4)], None, lambda r: r["tok"] < TSB))
    out.append(("timestamp-text", base_scores(8), [TS(0), 10, TS(4), TS(4), 11], None, None))
    z = base_scores(9)
    z[TS(3)] = 12.0                                          # the raw winner is a timestamp before the last one
    out.append(("monotone-bound", z, [TS(0), 10, TS(6), TS(6), 11, 12], None, lambda r: r["tok"] != TS(3) and np.isneginf(r["x"][TS(3)])))
    z = base_scores(10)
    z[TS(6)] = 12.0                                          # [text, timestamp]: the bound is the last timestamp itself, which may repeat
    out.append(("bound-repeat", z, [TS(0), 10, TS(6)], None, lambda r: r["tok"] == TS(6)))
    z = np.full(V, -4.0)
    z[20], z[TSB:] = 1.0, 0.2                                # 16 timestamps of 0.2: L = 0.2 + log 15 > 1 (one is masked by the bound)
    out.append(("sum-fires", z, [TS(0), 10, 11], None, lambda r: r["fired"] and r["before"] == 20 and r["tok"] >= TSB))
    z = np.full(V, -4.0)
    z[20], z[TSB:] = 4.0, 0.2
    out.append(("sum-silent", z, [TS(0), 10, 11], None, lambda r: not r["fired"] and r["tok"] == 20 and np.isfinite(r["gap"])))
    z = base_scores(11)
    out.append(("not-monotone-row", z, [TS(8), 10, TS(2), TS(2), 11], None, lambda r: np.isneginf(r["x"][TS(2)]) and r["x"][TS(3)] > -np.inf))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_rule_equals_hf_processors(case):
    name, z, gen, max_initial, holds = case
    x, tok, margin, gap, fired, before = SR.rule(z, mask_row(len(gen) == 0), gen, TSB, NO_TS, EOS, max_initial)
    assert gap >= 1e-3, "the case must keep HF's fp32 comparison away from a tie"
    want = hf_chain(z, gen, max_initial)
    assert np.array_equal(np.isneginf(x), np.isneginf(want)), (name, np.nonzero(np.isneginf(x) != np.isneginf(want))[0])
    assert tok == int(np.argmax(want))
    live = ~np.isneginf(want)
    assert np.array_equal(x[live], want[live])
    if holds is not None:
        assert holds(dict(x=x, tok=tok, gap=gap, fired=fired, before=before)), name


def test_rule_cases_cover_both_outcomes_of_the_sum_rule():
    fired = [SR.rule(z, mask_row(len(gen) == 0), gen, TSB, NO_TS, EOS, mi)[4] for _, z, gen, mi, _ in CASES]
    assert any(fired) and not all(fired)


SEQUENCES = {
    "empty": [],
    "no-timestamp": [3, 4, 5],
    "only-zero": [TS(0)],
    "zero-and-text": [TS(0), 3, 4],
    "lone-later-timestamp": [TS(0), 3, 4, TS(7)],
    "lone-timestamp-mid": [3, TS(7), 4],
    "one-pair": [TS(0), 3, 4, TS(5), TS(5)],
    "one-pair-and-text": [TS(0), 3, TS(5), TS(5), 4, 6],
    "three-pairs-single-ending": [TS(0), 3, TS(2), TS(2), 4, 5, TS(6), TS(7), 6, TS(9), TS(9), 7, TS(12)],
    "pairs-unfinished-tail": [TS(1), 3, TS(4), TS(4), 5, TS(8), TS(8), 6, 7],
    "pairs-closed-at-end": [TS(1), 3, TS(4), TS(4), 5, TS(8), TS(8)],
    "three-timestamps-in-a-row": [TS(1), TS(2), TS(3), 4],
}


def hf_segments(tokens, num_frames, time_offset):
    import torch
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    segs, off = WhisperGenerationMixin._retrieve_segment(
        seek_sequence=torch.tensor(tokens, dtype=torch.long), seek_outputs=[{}], time_offset=torch.tensor([time_offset], dtype=torch.float64),
        timestamp_begin=TSB, seek_num_frames=torch.tensor([num_frames]), time_precision=0.02, time_precision_features=0.01, input_stride=2,
        prev_idx=0, idx=0, return_token_timestamps=False, decoder_input_ids=torch.zeros((1, 3), dtype=torch.long))
    return [(float(s["start"]), float(s["end"]), [int(t) for t in s["tokens"]], tuple(int(i) for i in s["idxs"])) for s in segs], int(off)


@pytest.mark.parametrize("name", list(SEQUENCES))
@pytest.mark.parametrize("frames,offset", [(3000, 0.0), (1234, 30.0)])
def test_segments_of_equals_hf(name, frames, offset):
    tokens = SEQUENCES[name]
    want, want_off = hf_segments(tokens, frames, offset)
    for fn in (segments_of, SR.segments_of):
        got, got_off = fn(tokens, TSB, frames, offset)
        assert got_off == want_off
        assert [(a, b, list(t)) for a, b, t in got] == [(a, b, t) for a, b, t, _ in want]
        at = 0
        for (_, _, t), (_, _, _, idxs) in zip(got, want):                     # the token slices are consecutive: HF's idxs behind the prompt
            assert idxs == (3 + at, 3 + at + len(t))
            at += len(t)


def test_segments_of_equals_its_twin_on_random_rows():
    g = np.random.default_rng(0)
    for _ in range(300):
        n = int(g.integers(0, 14))
        tokens = [int(TS(g.integers(0, 16))) if g.random() < 0.45 else int(g.integers(0, EOS)) for _ in range(n)]
        a, b = segments_of(tokens, TSB, 2800, 1.5), SR.segments_of(tokens, TSB, 2800, 1.5)
        assert a[1] == b[1] and [(x, y, list(t)) for x, y, t in a[0]] == [(x, y, list(t)) for x, y, t in b[0]], tokens


def test_window_frames():
    assert window_frames(None) == 3000 and window_frames(480000) == 3000 and window_frames(10 ** 6) == 3000
    assert window_frames(16000) == 100 and window_frames(159) == 0


# ---------------------------------------------------------------------------------------------------------------- the fixture
def _analyse(gold, spec):
    """per utterance: the numpy rule on the stored logits (dict per decided position), and the split of its tokens"""
    Vf = C.TINY_WHISPER_DEC.decoder_vocab_size
    m = R.masks(spec, Vf)
    seq, keep = gold["sequences"], gold["decided"]
    logits = np.zeros(keep.shape + (Vf,), dtype=np.float32)
    logits[keep] = gold["logits"]
    tsb = int(gold["ts_begin"])
    out = []
    for b in range(seq.shape[0]):
        steps = {}
        for p in np.nonzero(keep[b])[0]:
            _, tok, mg, gp, fired, before = SR.rule(logits[b, p], m[1 if p == SR.P - 1 else 0], seq[b, SR.P: p + 1], tsb, spec.no_timestamps_token_id,
                                                    spec.eos_token_id, spec.max_initial_timestamp_index)
            steps[int(p)] = dict(tok=tok, margin=mg, gap=gp, fired=fired, before=before, want=int(seq[b, p + 1]))
        gen = seq[b, SR.P:].tolist()
        cut = spec.eos_token_id not in gen
        out.append(dict(steps=steps, cut=cut, body=gen if cut else gen[: gen.index(spec.eos_token_id)]))
    return out, logits


def test_fixture_conditions(golden_dir):
    gold, geo, sd, spec, enc = SR.load_fixture(golden_dir)
    assert geo.decoder_vocab_size == 522 and (geo.decoder_vocab_size + 7) // 8 * 8 != geo.decoder_vocab_size, "the padded pitch is live"
    tsb = int(gold["ts_begin"])
    text_end = spec.eos_token_id
    assert text_end < spec.decoder_start_token_id < min(spec.lang_ids) <= max(spec.lang_ids) < spec.task_id < spec.no_timestamps_token_id < tsb
    assert 24 <= geo.decoder_vocab_size - tsb <= 60, "a few dozen timestamp tokens"
    info, logits = _analyse(gold, spec)
    assert len(info) >= 3 and len({tuple(i["body"]) for i in info}) == len(info), "pairwise different utterances"
    pairs = lambda body: sum(1 for i in range(len(body) - 1) if body[i] >= tsb and body[i + 1] >= tsb)
    assert any(pairs(i["body"]) >= 2 for i in info), "one utterance has at least 2 closed segments"
    assert any(not i["cut"] and len(i["body"]) >= 2 and i["body"][-2] < tsb <= i["body"][-1] for i in info), "one ends on a single timestamp before eos"
    assert any(i["cut"] for i in info) and gold["sequences"].shape[1] == spec.max_length, "one is cut by max_length"
    steps = [s for i in info for s in i["steps"].values()]
    assert all(s["tok"] == s["want"] for s in steps), "the numpy rule on HF's logits gives HF's tokens"
    assert any(s["fired"] and s["before"] != s["tok"] for s in steps), "step 5 changes the winner somewhere"
    assert any(not s["fired"] and np.isfinite(s["gap"]) for s in steps), "step 5 stays silent somewhere with timestamps allowed"
    g = 1e-3 * max(1.0, float(np.abs(logits[gold["decided"]]).max()))
    assert min(s["margin"] for s in steps) >= 4 * g and min(s["gap"] for s in steps) >= 4 * g, (g, min(s["margin"] for s in steps), min(s["gap"] for s in steps))
    assert os.path.getsize(os.path.join(golden_dir, "tiny_whisper_seg_d128h2.npz")) < 200 * 1024


def test_fixture_segments(golden_dir):
    """the split of the fixture's rows: the closed segments, the single-timestamp ending and the max_length cut give what HF gives"""
    gold, geo, sd, spec, enc = SR.load_fixture(golden_dir)
    info, _ = _analyse(gold, spec)
    import torch
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    for i in info:
        segs, off = segments_of(i["body"], spec.timestamp_begin, 3000)
        want, want_off = WhisperGenerationMixin._retrieve_segment(
            seek_sequence=torch.tensor(i["body"], dtype=torch.long), seek_outputs=[{}], time_offset=torch.zeros(1, dtype=torch.float64),
            timestamp_begin=spec.timestamp_begin, seek_num_frames=torch.tensor([3000]), time_precision=0.02, time_precision_features=0.01,
            input_stride=2, prev_idx=0, idx=0, return_token_timestamps=False, decoder_input_ids=torch.zeros((1, 3), dtype=torch.long))
        assert off == int(want_off) and [(a, b, t) for a, b, t in segs] == [(float(s["start"]), float(s["end"]), s["tokens"].tolist()) for s in want]


def test_reference_generate_reproduces_the_fixture(golden_dir):
    """the float64 numpy decoder under the rule walks HF's sequences (one utterance: the rest is the GPU suite's business)"""
    gold, geo, sd, spec, enc = SR.load_fixture(golden_dir)
    b = int(np.argmin([(row != spec.pad_token_id).sum() for row in gold["sequences"]]))                 # the shortest: seconds on a CPU
    sd64 = {k: v.double().numpy() for k, v in sd.items()}
    got = SR.generate(geo, sd64, spec, enc[b: b + 1], gold["languages"][b: b + 1], spec.max_initial_timestamp_index)
    want = gold["sequences"][b]
    assert got["sequences"][0].tolist() == want[: got["sequences"].shape[1]].tolist()
    assert all(t == spec.pad_token_id for t in want[got["sequences"].shape[1]:])


# ---------------------------------------------------------------------------------------------------------------- spec and refusals
def _cfg(**extra):
    cfg = dict(decoder_start_token_id=471, eos_token_id=470, no_timestamps_token_id=481, lang_to_id={"<|en|>": 472}, task_to_id={"transcribe": 477})
    cfg.update(extra)
    return cfg


def test_spec_max_initial_timestamp_index_and_prompt_length():
    assert C.GenerationSpec.from_config(_cfg()).max_initial_timestamp_index is None, "absent: None, as HF's processor reads it"
    spec = C.GenerationSpec.from_config(_cfg(max_initial_timestamp_index=50))
    assert spec.max_initial_timestamp_index == 50 and spec.timestamp_begin == 482
    for bad in (-1, 1.5, True, "50"):
        with pytest.raises(OSError, match="max_initial_timestamp_index"):
            C.GenerationSpec.from_config(_cfg(max_initial_timestamp_index=bad))
    assert C.GenerationSpec.PROMPT_LEN == 4 and spec.prompt_len() == 4 and spec.prompt_len(timestamps=True) == 3


def test_command_line_refusals_name_the_flags(capsys):
    base = ["--wav_dir", "w", "--out_csv", "o.csv", "--segments_json", "s.json"]
    assert T.parse_args(base).segments_json == "s.json" and T.parse_args(base[:4]).segments_json == ""
    for extra, names in ((["--times_json", "t.json"], ("--segments_json", "--times_json")), (["--num_beams", "2"], ("--segments_json", "--num_beams"))):
        with pytest.raises(SystemExit):
            T.parse_args(base + extra)
        err = capsys.readouterr().err
        assert all(n in err for n in names), err
    assert T.parse_args(base + ["--num_beams", "1"]).num_beams == 1


def test_transcriber_refusals_name_the_flags():
    spec = C.GenerationSpec.from_config(_cfg())
    tr = T.WhisperTranscriber(None, None, spec)
    with pytest.raises(ValueError, match="timestamps=True with token_times"):
        tr.transcribe([], timestamps=True, token_times=True)
    with pytest.raises(ValueError, match="timestamps=True with num_beams"):
        tr.transcribe([], timestamps=True, num_beams=2)
    import dataclasses
    with pytest.raises(ValueError, match="timestamps=True with num_beams"):
        T.WhisperTranscriber(None, None, dataclasses.replace(spec, num_beams=3)).transcribe([], timestamps=True)
    assert tr.transcribe([], timestamps=True) == [] and tr.segments == [] and tr.next_seek == []


def test_segments_entry_schema():
    e = T.segments_entry([(0.0, 0.1, [TS(0), 3, TS(5)]), (0.1, 0.24, [TS(5), 4, TS(12)])], 24, "3 4", TSB)
    assert e == {"text": "3 4", "segments": [[0.0, 0.1, "3"], [0.1, 0.24, "4"]], "next_seek_s": 0.24}
