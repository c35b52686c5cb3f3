"""float64 statement of Whisper's transcript scores (numpy only), written from include/ser_hip.h's statement of ser_dec_select_score_v and
from HF's ``WhisperNoSpeechDetection``, ``_retrieve_avg_logprobs``, ``_retrieve_compression_ratio`` and ``_need_fallback``:

    logprob_of(x, tok)                    log-softmax of a processed row at a token
    score_plain(z, mask_row)              (x, token, margin, logprob) of a step without the timestamp rule
    score_ts(z, mask_row, gen, ...)       (x, token, margin, ts_gap, logprob) of a step with it (whisper_seg_ref.rule's masking)
    no_speech(z, token)                   softmax of the raw row at the no-speech token
    avg_logprob(logprobs)                 their sum in ascending order over their count
    compression_ratio / need_fallback     the host rule

tests/test_whisper_scores_host.py pins them to HF's own code; tests/test_gpu_whisper_scores.py pins the device to them.
"""
import math
import zlib

import numpy as np

import whisper_seg_ref as SR


def logprob_of(x: np.ndarray, tok: int) -> float:
    """x[tok] - log sum exp(x) around the row's maximum w, as (x[tok] - w) - log sum exp(x - w): the large parts cancel before anything is
    rounded, so the error is that of the sum and of one logarithm, whatever the size of the logits.  NaN when w is not finite."""
    x = np.asarray(x, dtype=np.float64)
    w = float(x.max())
    if not np.isfinite(w):
        return float("nan")
    with np.errstate(divide="ignore"):
        return float((x[tok] - w) - math.log(float(np.exp(x - w).sum())))


def score_plain(z, mask_row):
    """One row of a step without the rule (ser_dec_select_v's choice): x = z + mask, a NaN counting as +inf."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(z, dtype=np.float64) + np.asarray(mask_row, dtype=np.float64)
    x = np.where(np.isnan(x), np.inf, x)
    tok = int(np.argmax(x))
    a = np.sort(x)
    with np.errstate(invalid="ignore"):
        margin = float(a[-1] - a[-2])
    return x, tok, margin, logprob_of(x, tok)


def score_ts(z, mask_row, gen, ts_begin: int, no_ts: int, eos: int, max_initial=None):
    """One row of a step with the rule: whisper_seg_ref.rule's processed row (step 5's -inf text columns included) and the chosen
    token's log-softmax in it."""
    x, tok, margin, gap, fired, _ = SR.rule(z, mask_row, gen, ts_begin, no_ts, eos, max_initial)
    return x, tok, margin, gap, logprob_of(x, tok)


def no_speech(z, token: int) -> float:
    """softmax(raw logits)[token] in float64: no mask, no rule (HF's WhisperNoSpeechDetection on the first decoder position)"""
    z = np.asarray(z, dtype=np.float64)
    w = float(z.max())
    e = np.exp(z - w)
    return float(e[token] / e.sum())


def avg_logprob(logprobs) -> float:
    """HF's ``_retrieve_avg_logprobs`` behind the log-softmax: Python's ``sum`` from the first token on, over the count (eos included)"""
    total = 0.0
    for v in logprobs:
        total += float(v)
    return total / len(logprobs) if len(logprobs) else float("nan")


def compression_ratio(tokens, vocab_size: int) -> float:
    width = int(math.log2(vocab_size) / 8) + 1
    raw = b"".join(int(t).to_bytes(width, "little") for t in tokens)
    return len(raw) / len(zlib.compress(raw))


def need_fallback(tokens_with_eos, avg, no_speech_prob, logprob_threshold=None, no_speech_threshold=None, compression_ratio_threshold=None,
                  vocab_size=51866):
    """(needs_fallback, should_skip) as HF's ``_need_fallback`` decides them; ``no_speech_threshold`` without ``logprob_threshold`` is
    HF's unbound name: a ValueError here."""
    if no_speech_threshold is not None and logprob_threshold is None:
        raise ValueError("no_speech_threshold without logprob_threshold")
    needs = compression_ratio_threshold is not None and compression_ratio(tokens_with_eos, vocab_size) > compression_ratio_threshold
    low = logprob_threshold is not None and avg < logprob_threshold
    needs = needs or low
    if no_speech_threshold is not None and low and no_speech_prob > no_speech_threshold:
        return False, True
    return bool(needs), False


# ------------------------------------------------------------------------------------------------- the end-to-end fixture (tests/golden)
FIXTURE = "tiny_whisper_score_d128h2.npz"
_FIXTURE = {}


def load_fixture(golden_dir):
    """(gold npz, geometry, state dict of encoder and decoder, GenerationSpec with the recorded thresholds, waves) of the scores fixture
    (tools/make_whisper_scores_golden.py): the long-form fixture's geometry and token layout, weights and waves regenerated from the
    recorded seeds and checked against the recorded digest.  Loaded once and shared; nobody writes to it."""
    if "v" not in _FIXTURE:
        import dataclasses
        import os
        import whisper_long_ref as LR
        from interspeech_ser_amd import config as C
        from interspeech_ser_amd.weights import state_dict_digest, synthetic_state_dict
        gold = np.load(os.path.join(golden_dir, FIXTURE))
        geo = LR.fixture_geo()
        dec_sd = SR.fixture_state_dict(geo, int(gold["decoder_seed"]), LR.TS_BEGIN, float(gold["ts_scale"]))
        assert state_dict_digest(dec_sd) == str(gold["digest"]), "the decoder weights are not the ones the fixture was recorded with"
        sd = dict(synthetic_state_dict(C.TINY_WHISPER, int(gold["encoder_seed"])))
        sd.update(dec_sd)
        waves = [LR.fixture_wave(int(s), int(n)) for s, n in zip(gold["wave_seeds"], gold["wave_lengths"])]
        spec = dataclasses.replace(LR.fixture_spec(), logprob_threshold=float(gold["logprob_threshold"]),
                                   no_speech_threshold=float(gold["no_speech_threshold"]))
        _FIXTURE["v"] = (gold, geo, sd, spec, waves)
    return _FIXTURE["v"]
