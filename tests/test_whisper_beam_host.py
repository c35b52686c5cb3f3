"""CPU: the beam search rule (tests/whisper_beam_ref.py) is HF's algorithm, and the host side of the feature.

HF is driven through ``_beam_search``'s own helper functions in its order around the float64 tiny model's forward
(tools/make_whisper_beam_golden.hf_beam; its docstring says why ``_beam_search`` itself is not: it keeps its scores in fp32 whatever the
model's dtype).  The rule fed HF's logits must give HF's sequences, per-step parents and tokens, finished sets and stop step exactly and
its scores within 1e-9."""
import json
import os
import sys

import numpy as np
import pytest

import whisper_beam_ref as BR
import whisper_dec_ref as R
from interspeech_ser_amd import beam as BM
from interspeech_ser_amd import config as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4
CASES = [(2, 1.0, 20), (3, 0.0, 20), (5, 2.0, 20), (2, 0.0, 12), (3, 2.0, 12), (5, 1.0, 12), (3, 1.0, 20)]


@pytest.fixture(scope="module")
def hf(golden_dir):
    """(model in float64, spec, encoder states [3, S, D] float64 tensor, languages) of the greedy decoder fixture"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_whisper_beam_golden as MB
    gold, geo, sd, spec, enc = R.load_fixture(golden_dir)
    torch.set_num_threads(4)
    return MB, MB.G.hf_model(sd), spec, torch.from_numpy(enc).double(), gold["a_languages"], geo.decoder_vocab_size


@pytest.fixture(scope="module")
def runs(hf):
    """HF and the rule on every case, computed once and shared"""
    MB, model, spec, enc, langs, V = hf
    out = {}
    for K, lp, max_length in CASES:
        h = MB.hf_beam(model, spec, enc, langs, K, lp, max_length)
        out[(K, lp, max_length)] = (h, [MB.rule_on(h, b, K, V, spec, lp, max_length) for b in range(enc.shape[0])])
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"K{c[0]}-lp{c[1]}-len{c[2]}")
def test_rule_equals_hf(hf, runs, case):
    MB, model, spec, enc, langs, V = hf
    K, lp, max_length = case
    h, beams = runs[case]
    assert h["stop_step"] == 1 + max(bm.done_step for bm in beams), "the batch stops when its last utterance is done"
    for b, bm in enumerate(beams):
        assert bm.err == 0 and bm.done
        for s, st in enumerate(bm.steps):
            hs = h["steps"][s]
            if st is not None:
                par, tok, sc = hs["cand"]
                assert list(zip(par[b].tolist(), tok[b].tolist())) == st["cand"], (b, s, "candidates")
                assert np.abs(sc[b] - np.array(st["cand_scores"])).max() <= 1e-9
                live = np.isfinite(st["run_scores"])
                par, tok, sc = hs["run"]
                assert [c for c, ok in zip(zip(par[b].tolist(), tok[b].tolist()), live) if ok] == [c for c, ok in zip(st["run"], live) if ok], (b, s, "running beams")
                assert np.abs(sc[b][live] - st["run_scores"][live]).max(initial=0.0) <= 1e-9
                assert (sc[b][~live] < -1e8).all()                            # HF's -1e9 is the rule's dead beam
                fin, flag = st["finished"], st["flag"]
            else:                                                             # the rule is frozen; HF's batch goes on, its finished set must not move
                fin, flag = bm.finished, bm.flag
            scores, mask, seqs, _ = hs["finished"]
            assert int(mask[b].sum()) == len(fin) and bool(hs["flag"][b]) == flag, (b, s, "finished count / flag")
            assert np.abs(scores[b][: len(fin)] - np.array([f[0] for f in fin])).max(initial=0.0) <= 1e-9
            for k, (_, handle) in enumerate(fin):
                want = bm.history(*handle)
                assert seqs[b, k, P: P + len(want)].tolist() == want, (b, s, k, "finished hypothesis")
        best = bm.nbest()[0]
        assert h["sequences"][b][P:] == best[0], (b, "the best hypothesis, cut to its own length")
        assert abs(h["scores"][b] - best[1]) <= 1e-9


def test_cases_cover_early_stop_and_max_length(runs):
    early = full = eos = shared = 0
    for (K, lp, max_length), (h, beams) in runs.items():
        for bm in beams:
            last = max_length - P - 1
            early += bm.done_step < last and not bm.flag
            full += bm.done_step == last
            eos += any(bm.steps[hd[0]]["cand"][hd[1]][1] == bm.eos for _, hd in bm.finished)
            shared += any(len({q for q, _ in st["run"]}) < K for st in bm.steps if st is not None and np.isfinite(st["run_scores"]).all())
    assert early >= 1, "no case stops early on the heuristic"
    assert full >= 1, "no case runs into max_length"
    assert eos >= 1 and shared >= 1


def test_rule_corners():
    """step 0 with only beam 0 alive; fewer than 2K candidates is an error; ties go to the lower flat index; nothing enters after the flag"""
    K, V = 2, 8
    z = np.zeros((K, V), dtype=np.float32)
    z[1] = 50.0
    bm = BR.Beam(K, V, eos=1, pad=0, prompt_len=P, max_length=P + 4)
    bm.step(z, P)
    assert [c for c in bm.steps[0]["cand"]] == [(0, 0), (0, 1), (0, 2), (0, 3)]          # all tie: flat index order, beam 0 only
    assert bm.finished[0][1] == (0, 1) and [t for _, t in bm.steps[0]["run"]] == [0, 2]   # eos at rank 1 < K enters; the survivors skip it
    few = BR.Beam(K, V, eos=1, pad=0, prompt_len=P, max_length=P + 4)
    few.step(z, P, banned=np.arange(V) >= 3)
    assert few.err == BR.ERR_CANDIDATES and few.done
    nan = BR.Beam(K, V, eos=1, pad=0, prompt_len=P, max_length=P + 4)
    bad = z.copy()
    bad[0, 5] = np.nan
    nan.step(bad, P)
    assert nan.err & BR.ERR_NONFINITE
    dead = BR.Beam(K, V, eos=1, pad=0, prompt_len=P, max_length=P + 4)
    bad = z.copy()
    bad[1, 5] = np.nan
    dead.step(bad, P)
    assert dead.err == 0
    # the heuristic: K strong finished hypotheses drop the flag; a frozen utterance takes nothing more
    h = BR.Beam(K, V, eos=1, pad=0, prompt_len=P, max_length=P + 6)
    strong = np.full((K, V), -5.0, dtype=np.float32)
    strong[:, 1] = 20.0
    strong[:, 2] = 1.0
    strong[:, 3] = 0.5
    h.step(strong, P)
    h.step(strong, P + 1)
    assert len(h.finished) == K and not h.flag and h.done and h.done_step == 1
    before = list(h.finished)
    h.step(strong, P + 2)
    assert h.finished == before and h.steps[-1] is None


# ---------------------------------------------------------------------------------------------------------------- the host side
def _trace():
    """two utterances, K = 2, three steps from position 3: hand-made (parent, token) tables"""
    run = np.full((8, 2, 2, 2), -1, dtype=np.int32)
    cand = np.full((8, 2, 4, 2), -1, dtype=np.int32)
    run[3, 0] = [[0, 10], [0, 11]]
    run[4, 0] = [[1, 12], [0, 13]]
    run[5, 0] = [[1, 14], [1, 15]]
    cand[3, 0] = [[0, 10], [0, 11], [0, 7], [0, 9]]
    cand[4, 0] = [[1, 12], [0, 7], [0, 13], [1, 9]]
    cand[5, 0] = [[1, 14], [1, 15], [0, 7], [0, 9]]
    run[3, 1] = [[0, 20], [0, 21]]
    cand[3, 1] = [[0, 7], [0, 20], [0, 21], [0, 22]]
    return run, cand


def test_backtracking_and_nbest_ordering():
    run, cand = _trace()
    assert BM.backtrack(run, cand, 0, 3, 2, 3) == [7]
    assert BM.backtrack(run, cand, 0, 4, 1, 3) == [10, 7]                                # rank 1 of step 4: parent 0 -> token 10
    assert BM.backtrack(run, cand, 0, 5, 2, 3) == [11, 12, 7]                            # parent 0 of step 5 is run[4][0] = (1, 12) -> run[3][1] = 11
    assert BM.backtrack(run, cand, 0, 5, 1, 3) == [10, 13, 15]
    assert BM.running_history(run, 0, 5, 0, 3) == [10, 13, 14]
    assert BM.running_history(run, 0, 4, 0, 3) == [11, 12]
    with pytest.raises(ValueError, match="no candidate"):
        BM.backtrack(run, cand, 1, 4, 0, 3)
    fin_score = np.array([[-0.5, -0.75], [-0.25, 0.0]])
    fin_handle = np.array([[[5, 2], [4, 1]], [[3, 0], [0, 0]]], dtype=np.int32)
    nb = BM.nbest(run, cand, fin_score, fin_handle, [2, 1], 3)
    assert nb == [[([11, 12, 7], -0.5), ([10, 7], -0.75)], [([7], -0.25)]]
    with pytest.raises(ValueError, match="descending"):
        BM.nbest(run, cand, fin_score[:, ::-1], fin_handle[:, ::-1], [2, 0], 3)
    assert BM.lenpow_table(4, 2.0).tolist() == [0.0, 1.0, 4.0, 9.0] and BM.lenpow_table(3, 0.0).tolist() == [1.0, 1.0, 1.0]
    assert all(BM.lenpow_table(30, 0.7)[n] == float(np.float64(n) ** np.float64(0.7)) for n in range(30))


def _generation_config(**extra):
    cfg = dict(decoder_start_token_id=1, eos_token_id=2, no_timestamps_token_id=20, lang_to_id={"<|en|>": 10}, task_to_id={"transcribe": 15})
    cfg.update(extra)
    return cfg


def test_generation_spec_reads_beams_and_refuses_what_is_not_built(tmp_path):
    spec = C.GenerationSpec.from_config(_generation_config())
    assert spec.num_beams == 1 and spec.length_penalty == 1.0
    spec = C.GenerationSpec.from_config(_generation_config(num_beams=5, length_penalty=0.6, early_stopping=False))
    assert spec.num_beams == 5 and spec.length_penalty == 0.6
    for early in (True, "never"):
        with pytest.raises(OSError, match="early_stopping"):
            C.GenerationSpec.from_config(_generation_config(num_beams=2, early_stopping=early))
    for beams in (0, 9, -1, 2.5, "4"):
        with pytest.raises(OSError, match="num_beams"):
            C.GenerationSpec.from_config(_generation_config(num_beams=beams))
    with pytest.raises(OSError, match="length_penalty"):
        C.GenerationSpec.from_config(_generation_config(length_penalty="long"))
    with open(tmp_path / "generation_config.json", "w") as f:
        json.dump(_generation_config(num_beams=3), f)
    assert C.GenerationSpec.from_snapshot(str(tmp_path)).num_beams == 3


def test_command_line_refusals(capsys):
    from interspeech_ser_amd import transcribe as T
    base = ["--wav_dir", "w", "--out_csv", "o.csv"]
    args = T.parse_args(base)
    assert args.num_beams is None and args.length_penalty is None
    args = T.parse_args(base + ["--num_beams", "5", "--length_penalty", "0.5"])
    assert args.num_beams == 5 and args.length_penalty == 0.5
    assert T.parse_args(base + ["--num_beams", "1", "--times_json", "t.json"]).num_beams == 1     # greedy with times is what it was
    for bad, text in ((["--num_beams", "3", "--times_json", "t.json"], "--times_json"), (["--num_beams", "9"], "--num_beams"),
                      (["--num_beams", "0"], "--num_beams"), (["--length_penalty", "2.0"], "--length_penalty")):
        with pytest.raises(SystemExit) as e:
            T.parse_args(base + bad)
        assert e.value.code == 2 and text in capsys.readouterr().err


def test_decode_result_and_transcriber_signatures():
    import inspect
    from interspeech_ser_amd.engine import DecodeResult, WhisperDecoder
    from interspeech_ser_amd.transcribe import WhisperTranscriber
    sig = inspect.signature(WhisperDecoder.generate).parameters
    assert sig["num_beams"].default is None and sig["length_penalty"].default is None
    assert inspect.signature(WhisperTranscriber.transcribe).parameters["num_beams"].default is None
    res = DecodeResult(np.zeros((1, 4), np.int64), np.zeros(1, np.int64), [[]], np.zeros((1, 3), np.float32), 0, 0)
    assert res.nbest is None and res.beam_scores is None and res.beam_trace is None and res.beam_gaps is None and not res.failed
