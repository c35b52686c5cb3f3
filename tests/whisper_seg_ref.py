"""float64 statement of Whisper's segment-timestamp rule and of the split of a window's tokens into segments (numpy only), written from
the rule as include/ser_hip.h states it for ser_dec_select_ts_v -- HF's ``WhisperTimeStampLogitsProcessor`` behind the two suppress
processors -- and from HF's ``WhisperGenerationMixin._retrieve_segment``:

    rule(z, mask_row, gen, ...) -> (x, token, margin, ts_gap, fired, before) one row, one step; ``gen`` = the row's generated ids so far
    segments_of(tokens, ts_begin, num_frames, time_offset)                  the twin of ``transcribe.segments_of``
    generate(...)                                                           the greedy loop with the rule on the float64 decoder

tests/test_whisper_segments_host.py pins both to HF's own code; tests/test_gpu_whisper_segments.py pins the device path to them and to
HF's recorded result (tests/golden/tiny_whisper_seg_d128h2.npz, tools/make_whisper_segments_golden.py).
"""
import math

import numpy as np

import whisper_dec_ref as R

P = 3                           # the prompt of a timestamps run: [start, language, task]
TIME_PRECISION, TIME_PRECISION_FEATURES, INPUT_STRIDE = 0.02, 0.01, 2


def logsumexp(x: np.ndarray) -> float:
    """log sum exp in float64 around the maximum; -inf for an all-masked (or empty) set, the maximum itself when it is not finite"""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 0:
        return -np.inf
    m = float(x.max())
    if not np.isfinite(m):
        return m
    return m + math.log(float(np.exp(x - m).sum()))


def rule(z, mask_row, gen, ts_begin: int, no_ts: int, eos: int, max_initial=None):
    """One row of one step.  ``z`` [V] raw logits, ``mask_row`` [V] the additive static mask (0 / -inf), ``gen`` the generated ids of the
    row so far (n = len(gen)).  Returns (x [V] float64 after steps 1 to 5, token, margin, ts_gap, fired, before): token = the lowest index of
    the maximum, margin = top-1 minus top-2 of x, ts_gap = |L - M| (+inf when either is not finite), fired = step 5 masked the text
    columns, before = the winner of steps 1 to 4 alone (step 5 changed the winner when it differs from token)."""
    with np.errstate(invalid="ignore"):
        x = np.asarray(z, dtype=np.float64) + np.asarray(mask_row, dtype=np.float64)
    gen = [int(t) for t in gen]
    n = len(gen)
    x[no_ts] = -np.inf
    last_ts = n >= 1 and gen[-1] >= ts_begin
    pen_ts = n < 2 or gen[-2] >= ts_begin
    if last_ts and pen_ts:
        x[ts_begin:] = -np.inf
    if last_ts and not pen_ts:
        x[:eos] = -np.inf
    stamps = [t for t in gen if t >= ts_begin]
    if stamps:
        bound = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
        x[ts_begin:bound] = -np.inf
    if n == 0:
        x[:ts_begin] = -np.inf
        if max_initial is not None and max_initial >= 0:
            x[ts_begin + max_initial + 1:] = -np.inf
    L, M = logsumexp(x[ts_begin:]), float(x[:ts_begin].max())
    fired = bool(L > M)
    before = int(np.argmax(x))
    if fired:
        x[:ts_begin] = -np.inf
    gap = abs(L - M) if np.isfinite(L) and np.isfinite(M) else np.inf
    tok = int(np.argmax(x))
    a = np.sort(x)
    with np.errstate(invalid="ignore"):
        margin = float(a[-1] - a[-2])
    return x, tok, margin, float(gap), fired, before


def segments_of(tokens, ts_begin: int, num_frames: int, time_offset: float = 0.0):
    """(segments [(start_s, end_s, ids)], segment_offset in mel frames) of a window's generated tokens, written from HF's description:
    cut behind every pair of consecutive timestamps; [.., text, timestamp] at the end closes the last segment and consumes the window;
    else the tail behind the last pair is dropped and the offset is that pair's time; no pair: one segment, ending at the last timestamp
    unless there is none or it is <|0.00|>."""
    tok = [int(t) for t in tokens]
    ts = np.array([t >= ts_begin for t in tok], dtype=bool)
    pairs = [int(i) + 1 for i in np.nonzero(ts[:-1] & ts[1:])[0]] if len(tok) > 1 else []
    single = len(tok) >= 2 and (not ts[-2]) and bool(ts[-1])
    sec = lambda t: time_offset + float(t - ts_begin) * TIME_PRECISION
    if not pairs:
        stamps = [t for t in tok if t >= ts_begin]
        end = float(int(num_frames * TIME_PRECISION_FEATURES / TIME_PRECISION))
        if stamps and stamps[-1] != ts_begin:
            end = float(stamps[-1] - ts_begin)
        return [(float(time_offset), time_offset + end * TIME_PRECISION, tok)], int(num_frames)
    cuts = pairs + [len(tok)] if single else pairs[:-1] + [pairs[-1] + 1]
    out, at = [], 0
    for i, c in enumerate(cuts):
        part = tok[at:c]
        closing = part[-1] if (i < len(cuts) - 1 or single) else part[-2]
        out.append((sec(part[0]), sec(closing), part))
        at = c
    return out, int(num_frames) if single else (tok[at - 2] - ts_begin) * INPUT_STRIDE


def generate(geo, sd, spec, encs, languages, max_initial=None):
    """Greedy decoding with the rule on the float64 decoder, the languages given (the fixture records HF's).  Returns dict(sequences
    [B, n], lists, logits {(b, pos)}, margins, gaps, fired {(b, pos)})."""
    V = geo.decoder_vocab_size
    m = R.masks(spec, V)
    tsb = spec.no_timestamps_token_id + 1
    seqs, lists, logits, margins, gaps, fired = [], [], {}, {}, {}, {}
    for b, enc in enumerate(encs):
        d = R.Decoder(geo, sd, enc)
        seq = [spec.decoder_start_token_id, int(languages[b]), spec.task_id]
        for pos in range(P - 1):
            d.step(seq[pos], pos)
        pos = P - 1
        while len(seq) < spec.max_length:
            z = d.step(seq[pos], pos)
            _, tok, mg, gp, fr, _ = rule(z, m[1 if pos == P - 1 else 0], seq[P:], tsb, spec.no_timestamps_token_id, spec.eos_token_id, max_initial)
            logits[(b, pos)], margins[(b, pos)], gaps[(b, pos)], fired[(b, pos)] = z, mg, gp, fr
            seq.append(tok)
            pos += 1
            if tok == spec.eos_token_id:
                break
        seqs.append(seq)
        gen = seq[P:]
        lists.append(gen[:gen.index(spec.eos_token_id)] if spec.eos_token_id in gen else gen)
    n = max(len(s) for s in seqs)
    out = np.full((len(seqs), n), spec.pad_token_id, dtype=np.int64)
    for b, s in enumerate(seqs):
        out[b, : len(s)] = s
    return dict(sequences=out, lists=lists, logits=logits, margins=margins, gaps=gaps, fired=fired)


_FIXTURE = {}


def load_fixture(golden_dir):
    """(gold npz, geometry, decoder state dict, GenerationSpec, encoder states [B, 1500, 128] fp32) of tiny_whisper_seg_d128h2.npz: weights
    and encoder states regenerated from the recorded seeds (the one stored scalar put on embed_tokens' timestamp rows) and checked against
    the recorded digest.  Loaded once and shared; nobody writes to it."""
    if "v" not in _FIXTURE:
        import os
        from interspeech_ser_amd import config as C
        from interspeech_ser_amd.weights import state_dict_digest
        gold = np.load(os.path.join(golden_dir, "tiny_whisper_seg_d128h2.npz"))
        geo = C.TINY_WHISPER_DEC
        sd = fixture_state_dict(geo, int(gold["decoder_seed"]), int(gold["ts_begin"]), float(gold["ts_scale"]))
        assert state_dict_digest(sd) == str(gold["digest"]), "the decoder weights are not the ones the fixture was recorded with"
        mi = int(gold["max_initial"])
        spec = C.GenerationSpec(
            decoder_start_token_id=int(gold["start"]), eos_token_id=int(gold["eos"]), pad_token_id=int(gold["pad"]),
            suppress_tokens=tuple(int(t) for t in gold["suppress"]), begin_suppress_tokens=tuple(int(t) for t in gold["begin_suppress"]),
            no_timestamps_token_id=int(gold["no_timestamps"]), lang_ids=tuple(int(t) for t in gold["lang_ids"]), task_id=int(gold["task"]),
            max_length=int(gold["max_length"]), max_initial_timestamp_index=None if mi < 0 else mi)
        enc = np.concatenate([R.enc_states(int(s), 1, geo.max_source_positions, geo.hidden) for s in gold["enc_seeds"]])
        _FIXTURE["v"] = (gold, geo, sd, spec, enc)
    return _FIXTURE["v"]


def fixture_state_dict(geo, seed: int, ts_begin: int, ts_scale: float):
    """The seeded decoder weights with ``ts_scale`` on the timestamp rows of embed_tokens (the tied output projection: it moves the
    timestamp logits together, so that the sum rule neither always nor never fires)."""
    from interspeech_ser_amd.weights import synthetic_decoder_state_dict
    sd = dict(synthetic_decoder_state_dict(geo, seed))
    w = sd["decoder.embed_tokens.weight"].clone()
    w[ts_begin:] *= ts_scale
    sd["decoder.embed_tokens.weight"] = w
    return sd
