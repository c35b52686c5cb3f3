"""CPU: Whisper transcript scores -- the float64 rule (tests/whisper_score_ref.py) against HF's own code (the three logits processors and
``F.log_softmax``, ``WhisperNoSpeechDetection``, ``_need_fallback``, ``_retrieve_compression_ratio``), the product's host rule
(``transcribe.need_fallback`` / ``compression_ratio``) against both, the skip in the window queue of ``transcribe_long`` over a fake
encoder and decoder, and the refusals."""
import dataclasses
import itertools
import types

import numpy as np
import pytest

import whisper_score_ref as QR
import whisper_seg_ref as SR
from interspeech_ser_amd import config as C
from interspeech_ser_amd import transcribe as TR
from interspeech_ser_amd.transcribe import compression_ratio, need_fallback       # the feature's host entry points: the module needs them
from test_whisper_longform_host import EOS, START, TASK, TSB, FakeDecoder, FakeEncoder, corpus, make_spec, scripted_ids, tag_of
from test_whisper_segments_host import CASES, NO_TS, V, hf_chain, mask_row
from test_whisper_segments_host import EOS as SEG_EOS
from test_whisper_segments_host import TSB as SEG_TSB

U64 = 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_logprob_equals_log_softmax_of_hf_processors(case):
    """every scripted branch of the timestamp rule (closed pair, opening timestamp, first step with max_initial, the outweigh case ...):
    the rule's log-probability of its token is F.log_softmax of HF's processed scores, gathered at that token.  Both are float64
    log-sum-exps of the same V = 64 values: (V + 8) ulps of the value's size apart at the most, two sides."""
    import torch
    transformers = pytest.importorskip("transformers")                        # noqa: F841
    name, z, gen, max_initial, _ = case
    x, tok, margin, gap, lp = QR.score_ts(z, mask_row(len(gen) == 0), gen, SEG_TSB, NO_TS, SEG_EOS, max_initial)
    want = torch.log_softmax(torch.from_numpy(hf_chain(z, gen, max_initial)), dim=-1)
    assert tok == int(torch.argmax(want)) and np.isfinite(lp) and lp <= 0.0
    assert abs(lp - float(want[tok])) <= 2 * U64 * (V + 8) * max(1.0, abs(lp), float(np.abs(z).max())), (name, lp, float(want[tok]))
    dead = np.isneginf(x)
    assert np.array_equal(dead, np.isneginf(want.numpy())), "the -inf columns of the processed row are HF's"
    for v in np.nonzero(~dead)[0][:8]:                                         # and so is every other column's log-probability
        assert abs(QR.logprob_of(x, int(v)) - float(want[v])) <= 2 * U64 * (V + 8) * max(1.0, abs(float(want[v])), float(np.abs(z).max()))


def test_cases_cover_the_branches_the_issue_names():
    fired = {c[0]: SR.rule(c[1], mask_row(len(c[2]) == 0), c[2], SEG_TSB, NO_TS, SEG_EOS, c[3])[4] for c in CASES}
    assert fired["sum-fires"] and not fired["sum-silent"]
    assert {"n0-max-initial", "timestamp-timestamp", "text-timestamp", "sum-fires"} <= set(fired)
    # in the outweigh case the normaliser runs over the live timestamp columns only: the value the select kernel calls L
    _, z, gen, mi, _ = [c for c in CASES if c[0] == "sum-fires"][0]
    x, tok, _, _, lp = QR.score_ts(z, mask_row(False), gen, SEG_TSB, NO_TS, SEG_EOS, mi)
    assert np.isneginf(x[:SEG_TSB]).all() and abs(lp - (x[tok] - SR.logsumexp(x[SEG_TSB:]))) < 1e-12


def test_plain_score_is_log_softmax_of_the_masked_row():
    import torch
    g = np.random.default_rng(3)
    z = (3.0 * g.standard_normal(V)).astype(np.float32)
    x, tok, margin, lp = QR.score_plain(z, mask_row(True))
    want = torch.log_softmax(torch.from_numpy(z.astype(np.float64) + mask_row(True)), dim=-1)
    assert tok == int(torch.argmax(want)) and abs(lp - float(want[tok])) <= 2 * U64 * (V + 8) * max(1.0, float(np.abs(z).max()))


@pytest.mark.parametrize("begin_index", [1, 3])
def test_no_speech_equals_hf_detection(begin_index):
    """WhisperNoSpeechDetection's probs[:, no_speech_token]: from the scores it is handed (begin_index 1) and from logits[:, 0] of its own
    forward over the whole prompt (begin_index 3; the model is a stand-in that returns scripted logits).  HF's softmax runs in fp32: V
    additions and an exp, (V + 8) fp32 ulps relatively."""
    import torch
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    g = np.random.default_rng(11)
    z = (3.0 * g.standard_normal((3, V))).astype(np.float32)
    z[1, NO_TS - 1] = 14.0                                                    # a silent row
    z[2, NO_TS - 1] = -30.0
    proc = WhisperNoSpeechDetection(no_speech_token=NO_TS - 1, begin_index=begin_index)
    later = torch.from_numpy((z + 5.0 * g.standard_normal(z.shape)).astype(np.float32))
    if begin_index > 1:
        whole = torch.stack([torch.from_numpy(z), later, later], dim=1)       # [B, 3, V]: position 0 is the one that counts
        proc.model = lambda **kw: types.SimpleNamespace(logits=whole)
        proc.inputs = {}
        proc(torch.zeros((3, begin_index), dtype=torch.long), later)
    else:
        proc(torch.zeros((3, 1), dtype=torch.long), torch.from_numpy(z))
    want = proc.no_speech_prob.numpy().astype(np.float64)
    for b in range(3):
        got = QR.no_speech(z[b], NO_TS - 1)
        assert abs(got - want[b]) <= (V + 8) * 2.0 ** -24 * want[b] + 1e-45, (b, got, want[b])
    assert QR.no_speech(z[1], NO_TS - 1) > 0.9 > 0.1 > QR.no_speech(z[2], NO_TS - 1)


# ---------------------------------------------------------------------------------------------------------------- the host rule
def hf_need_fallback(tokens, scores, no_speech_prob, limits, vocab_size):
    """HF's ``_need_fallback`` itself, on a stand-in for the model that carries HF's own two static helpers"""
    import torch
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    det = WhisperNoSpeechDetection(no_speech_token=0, begin_index=1)
    det._no_speech_prob = torch.tensor([no_speech_prob], dtype=torch.float64)
    me = types.SimpleNamespace(_retrieve_compression_ratio=M._retrieve_compression_ratio, _retrieve_avg_logprobs=M._retrieve_avg_logprobs)
    gc = types.SimpleNamespace(**limits)
    outs = [{"scores": tuple(torch.from_numpy(s)[None][0] for s in scores)}]
    return M._need_fallback(me, torch.tensor(tokens, dtype=torch.long), outs, 0, [det], gc, vocab_size, 0.0)


def test_need_fallback_equals_hf_over_every_combination_of_thresholds():
    pytest.importorskip("transformers")
    g = np.random.default_rng(5)
    Vv = 600
    plain = [int(t) for t in g.integers(0, 400, size=11)] + [EOS]            # hardly compressible
    loop = [7, 8, 9] * 20 + [EOS]                                              # a repetition loop: a high ratio
    checked = 0
    for tokens in (plain, loop):
        scores = [3.0 * g.standard_normal(Vv) for _ in tokens]
        lps = [QR.logprob_of(s, t) for s, t in zip(scores, tokens)]
        avg, ratio = QR.avg_logprob(lps), QR.compression_ratio(tokens, Vv)
        assert ratio == compression_ratio(tokens, Vv)
        for present in itertools.product((False, True), repeat=3):
            for side in itertools.product((-1, 1), repeat=3):                  # each threshold on both sides of the value it is compared with
                for ns in (0.2, 0.9):
                    limits = dict(logprob_threshold=avg + 0.25 * side[0] if present[0] else None,
                                  no_speech_threshold=ns + 0.1 * side[1] if present[1] else None,
                                  compression_ratio_threshold=ratio + 0.2 * side[2] if present[2] else None)
                    if present[1] and not present[0]:
                        with pytest.raises(UnboundLocalError):                 # HF's own end of this combination
                            hf_need_fallback(tokens, scores, ns, limits, Vv)
                        with pytest.raises(ValueError, match="no_speech_threshold without logprob_threshold"):
                            need_fallback(tokens, avg, ns, limits, Vv)
                        with pytest.raises(ValueError):
                            QR.need_fallback(tokens, avg, ns, vocab_size=Vv, **limits)
                        continue
                    want = tuple(bool(v) for v in hf_need_fallback(tokens, scores, ns, limits, Vv))
                    assert need_fallback(tokens, avg, ns, limits, Vv) == want == QR.need_fallback(tokens, avg, ns, vocab_size=Vv, **limits), limits
                    checked += 1
    assert checked == 2 * 6 * 8 * 2
    assert QR.compression_ratio(loop, Vv) > 2.0 * QR.compression_ratio(plain, Vv)


@pytest.mark.parametrize("vocab", [200, 256, 600, 51866, 65536])
def test_compression_ratio_equals_hf(vocab):
    """HF's function called here: no compressed length is stored, it belongs to this machine's zlib.  256 and 65536: the byte width steps."""
    import torch
    pytest.importorskip("transformers")
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    g = np.random.default_rng(vocab)
    for n in (1, 5, 60):
        for tokens in ([int(t) for t in g.integers(0, vocab, size=n)], [int(vocab - 1)] * n):
            want = M._retrieve_compression_ratio(torch.tensor(tokens, dtype=torch.long), vocab)
            assert compression_ratio(tokens, vocab) == want == QR.compression_ratio(tokens, vocab)


def test_avg_logprob_is_hf_sum_over_count():
    import torch
    pytest.importorskip("transformers")
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    g = np.random.default_rng(2)
    tokens = [int(t) for t in g.integers(0, V, size=9)]
    scores = [3.0 * g.standard_normal(V) for _ in tokens]
    want = float(M._retrieve_avg_logprobs(tuple(torch.from_numpy(s) for s in scores), torch.tensor(tokens), 0.0))
    got = QR.avg_logprob([QR.logprob_of(s, t) for s, t in zip(scores, tokens)])
    assert abs(got - want) <= 16 * 2.0 ** -24 * 20.0, "HF takes the log-softmax in fp32: a few fp32 ulps of logits of size ~10"


def test_spec_reads_thresholds_and_the_no_speech_token():
    cfg = dict(decoder_start_token_id=START, eos_token_id=EOS, no_timestamps_token_id=481, lang_to_id={"<|en|>": 472}, task_to_id={"transcribe": TASK})
    s = C.GenerationSpec.from_config(cfg)
    assert s.no_speech_token == 480 and s.thresholds == dict(logprob_threshold=None, no_speech_threshold=None, compression_ratio_threshold=None)
    s = C.GenerationSpec.from_config(dict(cfg, logprob_threshold=-1, no_speech_threshold=0.6, compression_ratio_threshold=1.35, no_speech_token_id=9))
    assert s.no_speech_token == 9 and s.thresholds == dict(logprob_threshold=-1.0, no_speech_threshold=0.6, compression_ratio_threshold=1.35)
    with pytest.raises(OSError, match="logprob_threshold"):
        C.GenerationSpec.from_config(dict(cfg, logprob_threshold="low"))


# ---------------------------------------------------------------------------------------------------------------- the queue
LIMITS = dict(logprob_threshold=-1.0, no_speech_threshold=0.6)


class ScoredFakeDecoder(FakeDecoder):
    """FakeDecoder whose windows in ``silent`` {(tag, seek)} score like silence: a low average and a high no-speech probability"""

    geo = types.SimpleNamespace(decoder_vocab_size=TSB + 1501)

    def __init__(self, silent=(), **kw):
        super().__init__(**kw)
        self.silent, self.scored_calls = set(silent), 0

    def generate(self, rows, B, spec, scores=False, **kw):
        res = super().generate(rows, B, spec, **kw)
        assert scores, "with thresholds every window goes through the scored plan"
        self.scored_calls += 1
        n = max(len(ids) for ids in res.lists) + 4
        res.sequences = np.full((B, n), EOS, dtype=np.int64)
        res.token_logprobs, res.avg_logprob, res.no_speech_prob = [], np.zeros(B), np.zeros(B)
        if res.segments is None:
            res.segments = [None] * B                                         # a timestamps run: the prompt is [start, language, task]
        for k, (tag, seek, nf) in enumerate(rows):
            quiet = (tag, seek) in self.silent
            res.sequences[k, :3] = [START, int(res.languages[k]), TASK]
            res.sequences[k, 3: 3 + len(res.lists[k])] = res.lists[k]
            res.avg_logprob[k], res.no_speech_prob[k] = (-2.5, 0.93) if quiet else (-0.4, 0.07)
            res.token_logprobs.append(np.full(len(res.lists[k]) + 1, res.avg_logprob[k]))
        return res


def loop_with_skips(F, tag, silent):
    """HF's seek loop on the script, a window in ``silent`` skipped whole: (windows [(seek, nf, advance, skipped)], segments)"""
    seek, windows, segments = 0, [], []
    while seek < F:
        nf = min(3000, F - seek)
        if (tag, seek) in silent:
            windows.append((seek, nf, nf, True))
            seek += nf
            continue
        segs, adv = SR.segments_of(scripted_ids(tag, seek, nf), TSB, nf, float(seek) * SR.TIME_PRECISION / SR.INPUT_STRIDE)
        windows.append((seek, nf, int(adv), False))
        segments += segs
        seek += int(adv)
    return windows, segments


def run_scored_queue(items, batch, silent, limits=LIMITS):
    enc, dec = FakeEncoder(), ScoredFakeDecoder(silent=silent)
    tr = TR.WhisperTranscriber(enc, dec, make_spec(**limits))
    return tr, dec, tr.transcribe_long(iter(items), batch=batch)


def middle_whole_window(items):
    """(item index, its tag, the seek) of a middle window, of a file of at least three, that the script consumes whole: skipping it leaves
    every later seek where it was"""
    for k, (name, w) in enumerate(items):
        wins, _ = loop_with_skips(len(w) // 160, tag_of(w), ())
        for seek, nf, adv, _ in wins[1:-1]:
            if adv == nf:
                return k, tag_of(w), seek
    raise AssertionError("the corpus has no such window")


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_queue_skips_a_silent_window_and_leaves_its_neighbours(batch):
    items = corpus()
    k, tag, at = middle_whole_window(items)
    whole_file = [i for i, (_, w) in enumerate(items) if TR.is_long(len(w)) and i != k][0]
    tag_all = tag_of(items[whole_file][1])
    short = [i for i, (_, w) in enumerate(items) if not TR.is_long(len(w))][0]
    silent = {(tag, at), (tag_of(items[short][1]), 0)} | {(tag_all, s) for s in range(0, len(items[whole_file][1]) // 160, 3000)}
    tr, dec, ids = run_scored_queue(items, batch, silent)
    assert tr.failed == [] and all(i is not None for i in ids) and dec.scored_calls == len(dec.calls) + len(dec.short_calls)
    for i, (name, w) in enumerate(items):
        wins, segs = loop_with_skips(len(w) // 160, tag_of(w), silent)
        got = tr.windows[i]
        assert [(s, nf, adv, e["skipped"]) for s, nf, adv, e in got] == wins, name
        assert all(sorted(e) == ["avg_logprob", "compression_ratio", "needs_fallback", "no_speech_prob", "skipped"] for *_, e in got)
        assert all(e["skipped"] == (e["avg_logprob"] < -1.0 and e["no_speech_prob"] > 0.6) and not (e["skipped"] and e["needs_fallback"]) for *_, e in got)
        assert [(a, b, list(t)) for a, b, t in tr.segments[i]] == [(a, b, list(t)) for a, b, t in segs], name
        assert ids[i] == [t for _, _, part in segs for t in part if t < TSB] and tr.next_seek[i] >= min(3000, len(w) // 160)
    # the victim: its neighbours' segments and absolute times are those of the run that skips nothing
    plain_wins, plain_segs = loop_with_skips(len(items[k][1]) // 160, tag, ())
    mine = [(a, b, list(t)) for a, b, t in tr.segments[k]]
    gone = [(a, b, list(t)) for a, b, t in SR.segments_of(scripted_ids(tag, at, 3000), TSB, 3000, float(at) * SR.TIME_PRECISION / SR.INPUT_STRIDE)[0]]
    assert [s for s in [(a, b, list(t)) for a, b, t in plain_segs] if s not in gone] == mine and len(gone) >= 1
    assert [(s, nf, adv) for s, nf, adv, _ in tr.windows[k]] == [w[:3] for w in plain_wins], "a skipped window advances by its whole nf"
    # a file whose windows were all skipped, a long one and a one-window one: the empty transcript, no failure
    for i in (whole_file, short):
        assert ids[i] == [] and tr.segments[i] == [] and tr.sequences[i] == [] and all(e["skipped"] for *_, e in tr.windows[i])
        assert tr.next_seek[i] == len(items[i][1]) // 160


def test_queue_results_do_not_depend_on_the_batch():
    items = corpus()
    k, tag, at = middle_whole_window(items)
    runs = [run_scored_queue(items, b, {(tag, at)}) for b in (1, 3, 16)]
    for tr, _, ids in runs[1:]:
        assert ids == runs[0][2] and tr.windows == runs[0][0].windows and tr.next_seek == runs[0][0].next_seek
        assert [[(a, b, list(t)) for a, b, t in s] for s in tr.segments] == [[(a, b, list(t)) for a, b, t in s] for s in runs[0][0].segments]


def test_queue_without_thresholds_is_the_unscored_queue():
    """no threshold, no scores: the decoder is called without the new argument (FakeDecoder.generate does not take it) and the window
    entries are the triples they were"""
    tr = TR.WhisperTranscriber(FakeEncoder(), FakeDecoder(), make_spec())
    ids = tr.transcribe_long(iter(corpus()), batch=16)
    assert all(i is not None for i in ids) and all(len(w) == 3 for wins in tr.windows for w in wins)
    tr2 = TR.WhisperTranscriber(FakeEncoder(), ScoredFakeDecoder(), make_spec())
    assert tr2.transcribe_long(iter(corpus()), batch=16, scores=True) == ids and all(len(w) == 4 for wins in tr2.windows for w in wins)
    assert not any(w[3]["skipped"] or w[3]["needs_fallback"] for wins in tr2.windows for w in wins)


def test_queue_refuses_no_speech_threshold_alone():
    tr = TR.WhisperTranscriber(FakeEncoder(), ScoredFakeDecoder(), make_spec(no_speech_threshold=0.6))
    with pytest.raises(ValueError, match="no_speech_threshold without logprob_threshold"):
        tr.transcribe_long(iter(corpus()))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_command_line_refusals(capsys):
    base = ["--wav_dir", "a", "--out_csv", "b.csv"]
    ok = TR.parse_args(base + ["--long_form", "--logprob_threshold", "-1", "--no_speech_threshold", "0.6", "--compression_ratio_threshold", "1.35",
                               "--scores_json", "q.json", "--segments_json", "s.json"])
    assert (ok.logprob_threshold, ok.no_speech_threshold, ok.compression_ratio_threshold, ok.scores_json) == (-1.0, 0.6, 1.35, "q.json")
    assert TR.parse_args(base + ["--scores_json", "q.json"]).scores_json == "q.json" and TR.parse_args(base).scores_json == ""
    refused = [(["--logprob_threshold", "-1"], ("--logprob_threshold", "--long_form")),
               (["--compression_ratio_threshold", "2"], ("--compression_ratio_threshold", "--long_form")),
               (["--no_speech_threshold", "0.6", "--logprob_threshold", "-1"], ("--long_form",)),
               (["--long_form", "--no_speech_threshold", "0.6"], ("--no_speech_threshold", "--logprob_threshold")),
               (["--scores_json", "q.json", "--times_json", "t.json"], ("--scores_json", "--times_json", "not built")),
               (["--scores_json", "q.json", "--num_beams", "2"], ("--scores_json", "--num_beams", "not built"))]
    for extra, words in refused:
        capsys.readouterr()
        with pytest.raises(SystemExit):
            TR.parse_args(base + extra)
        err = capsys.readouterr().err
        assert all(w in err for w in words), (extra, err)


def test_generate_refuses_scores_with_beams_and_token_times_by_name():
    """the engine's own refusals come before anything touches the device"""
    import inspect
    from interspeech_ser_amd.engine import DecodeResult, WhisperDecoder
    assert inspect.signature(WhisperDecoder.generate).parameters["scores"].default is False
    assert DecodeResult.token_logprobs is None and DecodeResult.avg_logprob is None and DecodeResult.no_speech_prob is None
    dec = WhisperDecoder.__new__(WhisperDecoder)
    dec.spec = dataclasses.replace(make_spec(), num_beams=1)
    for kw, words in ((dict(num_beams=2), "scores=True with num_beams > 1"), (dict(token_times=True, lengths=[16000]), "scores=True with token_times")):
        with pytest.raises(ValueError, match=words):
            WhisperDecoder.generate.__wrapped__(dec, None, 1, scores=True, **kw)      # the method behind the stream lookup: no device is touched
    tr = TR.WhisperTranscriber(FakeEncoder(), ScoredFakeDecoder(), make_spec())
    with pytest.raises(ValueError, match="scores=True with token_times"):
        tr.transcribe([np.zeros(16000, dtype=np.float32)], scores=True, token_times=True)
    with pytest.raises(ValueError, match="scores=True with num_beams > 1"):
        tr.transcribe([np.zeros(16000, dtype=np.float32)], scores=True, num_beams=2)


# ---------------------------------------------------------------------------------------------------------------- the end-to-end fixture
def test_fixture_conditions(golden_dir):
    """tests/golden/tiny_whisper_score_d128h2.npz (tools/make_whisper_scores_golden.py: HF's long-form loop with its thresholds on the
    float64 tiny model): the searched conditions hold on the stored file, the host rule fed HF's stored scores gives HF's skip and
    fallback decisions, and the seek loop with those skips gives HF's windows, sequence and segments"""
    import math
    import os
    gold, geo, sd, spec, waves = QR.load_fixture(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, QR.FIXTURE)) < 1024 * 1024
    g, limits, V = float(gold["g"]), spec.thresholds, geo.decoder_vocab_size
    assert limits["compression_ratio_threshold"] is None and spec.no_speech_token == int(gold["no_speech_token"])
    some_middle_skipped = False
    for i, w in enumerate(waves):
        wins = [tuple(int(x) for x in r) for r in gold[f"f{i}_windows"]]
        skipped, needs = gold[f"f{i}_skipped"].tolist(), gold[f"f{i}_needs_fallback"].tolist()
        rows = [r[r >= 0][SR.P:].tolist() for r in gold[f"f{i}_rows"]]
        avg, ns, lps = gold[f"f{i}_avg_logprob"], gold[f"f{i}_no_speech_prob"], gold[f"f{i}_token_logprobs"]
        assert len(wins) >= 3 and min(float(gold[f"f{i}_margins"].min()), float(gold[f"f{i}_gaps"].min()), float(gold[f"f{i}_lang_margin"])) >= 4 * g
        at = 0
        for k, row in enumerate(rows):
            assert need_fallback(row, avg[k], ns[k], limits, V) == (needs[k], skipped[k]) == QR.need_fallback(row, avg[k], ns[k], vocab_size=V, **limits)
            assert abs(avg[k] - limits["logprob_threshold"]) >= 4 * 2 * g, "the average lies four gates from its threshold"
            assert abs(ns[k] / limits["no_speech_threshold"] - 1.0) >= 4 * math.expm1(2 * g)
            mine = QR.avg_logprob(lps[at: at + len(row)])                     # HF takes its log-softmax in fp32: a few fp32 ulps of the logits
            assert abs(mine - avg[k]) <= 64 * 2.0 ** -24 * 20.0 and (lps[at: at + len(row)] <= 0.0).all()
            at += len(row)
        assert at == len(lps)
        some_middle_skipped |= any(skipped[1:-1])
        bodies = {seek: (r[: r.index(spec.eos_token_id)] if spec.eos_token_id in r else r) for (seek, _, _), r in zip(wins, rows)}
        seek, got_wins, segs = 0, [], []
        F = len(w) // 160
        while seek < F:                                                        # HF's loop: a skipped window advances by its nf, whole
            nf = min(3000, F - seek)
            k = [s for s, _, _ in wins].index(seek)
            if skipped[k]:
                got_wins.append((seek, nf, nf))
                seek += nf
                continue
            s, adv = TR.segments_of(bodies[seek], spec.timestamp_begin, nf, float(seek) * SR.TIME_PRECISION / SR.INPUT_STRIDE)
            got_wins.append((seek, nf, int(adv)))
            segs += s
            seek += int(adv)
        assert got_wins == wins and seek == int(gold[f"f{i}_seek"])
        assert [t for _, _, part in segs for t in part] == gold[f"f{i}_sequence"].tolist()
        assert [(a, b) for a, b, _ in segs] == [(float(a), float(b)) for a, b in gold[f"f{i}_seg_times"]]
        assert any(skipped) and not all(skipped), "a skipped and a kept window in every file"
    assert some_middle_skipped, "a middle window of a file of three windows is skipped"
