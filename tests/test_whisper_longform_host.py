"""CPU: Whisper long-form transcription -- the float64 statement of the whole-file log-mel against WhisperFeatureExtractor, the seek loop
(tests/whisper_long_ref.py) against HF's own static pieces called in ``generate``'s order, and the window queue of
``WhisperTranscriber.transcribe_long`` over a fake encoder and decoder."""
import dataclasses
import zlib

import numpy as np
import pytest

import frontend_ref as FR
import whisper_long_ref as LR
import whisper_seg_ref as SR
from interspeech_ser_amd import config as C
from interspeech_ser_amd import transcribe as TR
from interspeech_ser_amd.frontend import whisper_mel_filters

EOS, START, TASK, NO_TS = 470, 471, 477, 481
TSB = NO_TS + 1
LANGS = (472, 473, 474, 475)


def TS(k):
    return TSB + int(k)


def ulp32(v):
    return float(np.spacing(np.float32(v)))


def noise(seed, n, sigma=0.1):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the features
# With torch installed WhisperFeatureExtractor takes its torch path: an fp32 STFT.  The bound is the one tests/test_frontend_ref_host.py
# derives for an fp32 STFT against the float64 statement, restated: window rounding and an fp32 FFT of 400 points leave an amplitude
# error of up to c u32 times the LARGEST amplitude, c = 2 log2(400); an element whose mel power lies D decades below the file's maximum
# has 10^(-D/2) of its amplitude, so its power is off by 2 c u32 10^(D/2) relatively, its log10 by that / ln 10, the feature by a quarter
# (D <= 8: the clamp).  On top of it the fp32 rounding of log10, of the clamp and of (v + 4) / 4: 1e-6.
U32 = 2.0 ** -24


def fp32_stft_bound(raw):
    depth = np.minimum(raw.max() - raw, FR.CLAMP_DECADES)
    return 2.0 * (2.0 * np.log2(400.0)) * U32 * 10.0 ** (depth / 2.0) / np.log(10.0) / 4.0 + 1e-6


@pytest.mark.parametrize("n_mels", [80, 128])
def test_log_mel_long64_equals_the_feature_extractor(n_mels):
    from transformers import WhisperFeatureExtractor
    fe = WhisperFeatureExtractor(feature_size=n_mels)
    mel = np.asarray(fe.mel_filters, dtype=np.float64)
    assert mel.shape == (FR.N_BINS, n_mels)
    for k, n in enumerate((481000, 700123, 1121999)):
        w = noise(40 + k, n)
        w[n // 3: n // 3 + 8000] *= 1e-3                                       # a stretch deep below the file's maximum
        want = fe(w, sampling_rate=16000, truncation=False, padding="longest", return_tensors="np")["input_features"][0]
        got = LR.log_mel_long64(w, mel)
        assert want.shape == got.shape == (n_mels, n // 160), (want.shape, got.shape)
        err = np.abs(got - want.astype(np.float64))
        tol = fp32_stft_bound(LR.log_mel_long_raw64(w, mel))
        print(f"log_mel_long64 vs WhisperFeatureExtractor: {n} samples, {n_mels} mels: max {float(err.max()):.3e}, "
              f"worst err / bound {float((err / tol).max()):.3f}")
        assert (err <= tol).all(), (n, float((err / tol).max()))
        mine = LR.log_mel_long64(w, whisper_mel_filters(n_mels))              # the project's own filter matrix
        assert float(np.abs(mine - got).max()) < 1e-6


@pytest.mark.parametrize("n_mels", [80, 128])
def test_log_mel_long64_is_log_mel64_on_exactly_thirty_seconds(n_mels):
    w = noise(7, 480000)
    mel = whisper_mel_filters(n_mels)
    a, b = LR.log_mel_long64(w, mel), FR.log_mel64(w, mel)
    assert a.shape == b.shape == (n_mels, 3000) and a.tobytes() == b.tobytes()


def test_the_dropped_frame_is_in_no_maximum_and_the_floor_is_the_files():
    mel = whisper_mel_filters(80)
    F = 3100
    w = noise(3, 160 * F + 159, 1e-4)
    base = LR.log_mel_long64(w, mel)
    loud = w.copy()
    loud[-1] = 0.9                                                             # inside frame F alone: 160 F + 159 - 200 > 160 (F - 1) + 199
    assert LR.log_mel_long64(loud, mel).tobytes() == base.tobytes()
    quiet_then_loud = np.concatenate([noise(4, 480000, 1e-4), noise(5, 160000, 0.3)])
    whole = LR.log_mel_long64(quiet_then_loud, mel)
    assert float(np.abs(whole[:, :2990] - FR.log_mel64(quiet_then_loud[:480000], mel)[:, :2990]).max()) > 0.1, "a per-window maximum is another floor"
    raw = LR.log_mel_long_raw64(quiet_then_loud, mel)
    floor = (raw.max() - 8.0 + 4.0) / 4.0
    assert raw[:, :2990].max() < raw.max() - 6.0 and whole[:, :2990].min() == floor == whole.min(), "the quiet half sits on the file's floor"
    assert float((whole[:, :2990] == floor).mean()) > 0.5


# ---------------------------------------------------------------------------------------------------------------- the loop
SCRIPTS = {
    # a closed pair (partial advance of 1000 frames), pairs and a single-timestamp ending (the window consumed whole), no pair, then a
    # last window of 13 frames with a pair at 0.06 s and one of 7 frames
    "four-kinds": (7013, [[TS(0), 3, TS(500), TS(500), 4, 5], [TS(0), 3, TS(100), TS(100), 4, TS(900)], [TS(0), 3, 4],
                          [TS(0), 5, TS(3), TS(3)], [3]]),
    # exactly two windows; a lone timestamp that is not <|0.00|> ends the no-pair segment
    "two-whole-windows": (6000, [[TS(0), 3, 4, TS(1400)], [3, TS(7), 4]]),
    # 3001 frames: the route's boundary, a last window of one frame
    "one-frame-tail": (3001, [[TS(2), 9, TS(1500)], [TS(0)]]),
    # pairs all the way: every advance is a pair's time
    "pairs-only": (3407, [[TS(0), 3, TS(750), TS(750)], [TS(0), 4, TS(900), TS(900), 7], [TS(0), 4, TS(50), TS(50)], [5, 6]]),
}


def hf_loop(F, script):
    """HF's static pieces in ``generate``'s order (generation_whisper.py:649-903), one file at batch size 1, on an index-valued feature
    tensor: feature [m, t] = 1 + t + 10000 m, so that the slice and the zero pad of a window are visible."""
    import torch
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M
    feats = (1.0 + torch.arange(F, dtype=torch.float64)[None, None, :] + 10000.0 * torch.arange(2, dtype=torch.float64)[None, :, None])
    max_frames, seek = M._retrieve_max_frames_and_seek(batch_size=1, attention_mask=None, total_input_frames=F, is_shortform=False)
    cur_bsz, batch_idx_map = 1, [0]
    windows, offsets, segments, inputs = [], [], [], []
    k = 0
    while (seek < max_frames).any():
        feats, cur_bsz, batch_idx_map = M._maybe_reduce_batch(input_features=feats, seek=seek, max_frames=max_frames, cur_bsz=cur_bsz,
                                                              batch_idx_map=batch_idx_map)
        time_offset = seek.to(torch.float64) * 0.02 / 2
        seek_num_frames = (max_frames - seek).clamp(max=3000)
        seg_in = M._get_input_segment(input_features=feats, seek=seek, seek_num_frames=seek_num_frames, num_segment_frames=3000,
                                      cur_bsz=cur_bsz, batch_idx_map=batch_idx_map)
        segs, off = M._retrieve_segment(seek_sequence=torch.tensor(script[k], dtype=torch.long), seek_outputs=[{}], time_offset=time_offset,
                                        timestamp_begin=TSB, seek_num_frames=seek_num_frames, time_precision=0.02, time_precision_features=0.01,
                                        input_stride=2, prev_idx=0, idx=0, return_token_timestamps=False,
                                        decoder_input_ids=torch.zeros((1, 3), dtype=torch.long))
        windows.append((int(seek[0]), int(seek_num_frames[0]), int(off)))
        offsets.append(float(time_offset[0]))
        inputs.append(seg_in[0].numpy())
        segments += [(float(s["start"]), float(s["end"]), [int(t) for t in s["tokens"]]) for s in segs]
        seek[0] += off
        k += 1
    assert k == len(script), "the script has a window the loop never reached"
    return dict(windows=windows, offsets=offsets, segments=segments, inputs=inputs, sequence=[t for _, _, ids in segments for t in ids],
                seek=int(seek[0]))


@pytest.mark.parametrize("name", list(SCRIPTS))
def test_loop_equals_hf_pieces_in_generates_order(name):
    F, script = SCRIPTS[name]
    want = hf_loop(F, script)
    got = LR.loop(F, lambda k, seek, nf: script[k], TSB)
    assert not got["stuck"] and got["windows"] == want["windows"] and got["offsets"] == want["offsets"] and got["seek"] == want["seek"]
    assert [(a, b, list(t)) for a, b, t in got["segments"]] == want["segments"] and got["sequence"] == want["sequence"]
    feats = 1.0 + np.arange(F, dtype=np.float64)[None, :] + 10000.0 * np.arange(2, dtype=np.float64)[:, None]
    for (seek, nf, _), x in zip(got["windows"], want["inputs"]):
        mine = LR.window_of(feats, seek, nf)
        assert mine.tobytes() == x.tobytes() and (mine[:, nf:] == 0.0).all() and mine[0, 0] == 1.0 + seek
    if name == "four-kinds":
        adv = [w[2] for w in got["windows"]]
        assert adv[0] == 1000 and adv[1] == 3000 and adv[2] == 3000 and got["windows"][3][:2] == (7000, 13) and adv[3] == 6


def test_loop_reports_a_window_without_progress():
    got = LR.loop(5000, lambda k, seek, nf: [TS(0), 3, TS(80), TS(80)] if k == 0 else [TS(0), TS(0)], TSB)
    assert got["stuck"] and got["windows"] == [(0, 3000, 160), (160, 3000, 0)]


# ---------------------------------------------------------------------------------------------------------------- the queue
def make_spec(language=None, **kw):
    return C.GenerationSpec(decoder_start_token_id=START, eos_token_id=EOS, pad_token_id=EOS, suppress_tokens=(), begin_suppress_tokens=(),
                            no_timestamps_token_id=NO_TS, lang_ids=LANGS, task_id=TASK, max_length=24, language=language, **kw)


def tag_of(wave):
    return int(zlib.crc32(np.ascontiguousarray(wave[:64]).tobytes()))


def scripted_ids(tag, seek, nf):
    """a window's tokens as a function of the file and the seek alone: all four kinds of ending"""
    g = np.random.default_rng([tag & 0xffff, seek])
    kind = int(g.integers(0, 4))
    text = [int(t) for t in g.integers(0, 400, size=int(g.integers(1, 5)))]
    half = max(1, nf // 2 // 2)
    t1 = int(g.integers(1, half + 1))
    if kind == 0:
        return [TS(0)] + text + [TS(t1), TS(t1)] + text[:1]                    # a closed pair: advance 2 t1
    if kind == 1:
        return [TS(0)] + text + [TS(t1), TS(t1)] + text + [TS(min(t1 + 3, 1500))]      # pairs, then a single timestamp: the whole window
    if kind == 2:
        return text                                                            # no timestamp at all
    return [TS(0)] + text + [TS(t1)]                                           # [text, timestamp] without a pair


def lang_of(tag):
    return LANGS[tag % 4]


class FakeHandle:
    def __init__(self):
        self.files, self.released = [], []

    def __len__(self):
        return len(self.files)

    def release(self, f):
        assert f not in self.released
        self.released.append(f)


class FakeStates:
    def __init__(self, rows):
        self.states = [rows]

    def take_range_bits(self):
        return 0


class FakeResult:
    def __init__(self, lists, languages, failed):
        self.lists, self.languages, self.failed, self.err, self.range_bits = lists, np.array(languages), failed, 1 if failed else 0, 0
        self.segments, self.next_seek = None, None


class FakeEncoder:
    def __init__(self):
        self.admissions = []

    def upload(self, waves, slot=0):
        return list(waves)

    def log_mel_long(self, waves, lengths, into=None):
        h = into if into is not None else FakeHandle()
        assert [len(w) for w in waves] == list(lengths)
        self.admissions.append(len(waves))
        h.files += [(tag_of(w), len(w) // 160) for w in waves]
        return h

    def forward_windows(self, handle, rows, slot=0):
        for f, seek, nf in rows:
            assert f not in handle.released and 1 <= nf <= 3000 and seek + nf <= handle.files[f][1] and nf == min(3000, handle.files[f][1] - seek)
        return FakeStates([(handle.files[f][0], seek, nf) for f, seek, nf in rows])

    def forward(self, waves, lengths, slot=0):
        return FakeStates([(tag_of(w), 0, min(3000, len(w) // 160)) for w in waves])


class FakeDecoder:
    def __init__(self, bad=(), stuck=()):
        self.calls, self.short_calls, self.bad, self.stuck = [], [], set(bad), set(stuck)          # calls: the queue's rounds

    def generate(self, rows, B, spec, language=None, slot=0, timestamps=False, num_frames=None, lengths=None):
        assert timestamps and B == len(rows)
        language = spec.language if language is None else language
        if num_frames is not None:
            assert list(num_frames) == [nf for _, _, nf in rows]
        (self.calls if lengths is None else self.short_calls).append((language, list(rows)))
        lists = [[TS(0), TS(0)] if (tag, seek) in self.stuck else scripted_ids(tag, seek, nf) for tag, seek, nf in rows]
        res = FakeResult(lists, [lang_of(tag) if language is None else language for tag, _, _ in rows], any((tag, seek) in self.bad for tag, seek, _ in rows))
        if lengths is not None:                                                # the one-window path of a short file
            cut = [TR.segments_of(ids, TSB, nf) for ids, (_, _, nf) in zip(lists, rows)]
            res.segments, res.next_seek = [c[0] for c in cut], np.array([c[1] for c in cut])
        return res


LENGTHS = (500000, 1121999, 480160 + 7, 700123, 16000, 3 * 480000 + 11, 481000, 250000, 560000, 900001)


def corpus():
    return [(f"f{k}.wav", noise(900 + k, n)) for k, n in enumerate(LENGTHS)]


def expected(items):
    """per file: the loop of tests/whisper_long_ref.py on the same script"""
    out = {}
    for name, w in items:
        tag, F = tag_of(w), len(w) // 160
        out[name] = LR.loop(F, lambda k, seek, nf: scripted_ids(tag, seek, nf), TSB)
    return out


def run_queue(items, batch, language=None, **fake):
    enc, dec = FakeEncoder(), FakeDecoder(**fake)
    tr = TR.WhisperTranscriber(enc, dec, make_spec(language))
    ids = tr.transcribe_long(iter(items), batch=batch)
    return tr, enc, dec, ids


@pytest.mark.parametrize("batch", [1, 3, 16])
def test_queue_result_is_independent_of_batch_and_order(batch):
    items = corpus()
    want = expected(items)
    assert sum(len(w["windows"]) >= 3 for w in want.values()) >= 3 and not any(w["stuck"] for w in want.values())
    for order in (list(range(len(items))), list(reversed(range(len(items)))), [3, 0, 9, 4, 1, 8, 2, 7, 5, 6]):
        picked = [items[i] for i in order]
        tr, enc, dec, ids = run_queue(picked, batch)
        assert tr.failed == [] and len(ids) == len(picked)
        for k, (name, w) in enumerate(picked):
            if not TR.is_long(len(w)):
                assert tr.windows[k] == [(0, len(w) // 160, tr.next_seek[k])] and ids[k] == [t for t in scripted_ids(tag_of(w), 0, len(w) // 160) if t < TSB]
                continue
            e = want[name]
            assert tr.sequences[k] == e["sequence"] and ids[k] == [t for t in e["sequence"] if t < TSB]
            assert tr.windows[k] == e["windows"] and tr.next_seek[k] == e["seek"] >= len(w) // 160
            assert [(a, b, list(t)) for a, b, t in tr.segments[k]] == [(a, b, list(t)) for a, b, t in e["segments"]]
            assert tr.last_languages[k] == lang_of(tag_of(w))
        assert all(len(rows) <= batch for _, rows in dec.calls) and sum(enc.admissions) == sum(TR.is_long(n) for n in LENGTHS)
        assert max(enc.admissions) <= batch


def test_queue_rounds_are_homogeneous_and_the_language_is_detected_once():
    items = corpus()
    tr, enc, dec, ids = run_queue(items, 16)
    seen = set()
    for language, rows in dec.calls:
        if language is None:
            assert all(seek == 0 and tag not in seen for tag, seek, _ in rows), "only first windows are detected"
            seen |= {tag for tag, _, _ in rows}
        else:
            assert all(tag in seen and seek > 0 and lang_of(tag) == language for tag, seek, _ in rows), "a later window is forced to its file's language"
    assert len(seen) == sum(TR.is_long(n) for n in LENGTHS)
    assert len({language for language, _ in dec.calls}) >= 3, "several languages were met"
    forced_tr, _, forced_dec, forced_ids = run_queue(items, 16, language=LANGS[1])
    assert all(language == LANGS[1] for language, _ in forced_dec.calls) and forced_ids == ids
    assert all(l == LANGS[1] for l in forced_tr.last_languages)
    assert len(forced_dec.calls) < len(dec.calls), "one language: every pending window shares a round"


def test_queue_zero_advance_fails_its_file_alone(capsys):
    items = corpus()
    want = expected(items)
    victim = items[1]
    second = want[victim[0]]["windows"][1][0]
    tr, enc, dec, ids = run_queue(items, 16, stuck=[(tag_of(victim[1]), second)])
    assert tr.failed == [victim[0]] and ids[1] is None and tr.segments[1] is None and tr.windows[1] is None and tr.sequences[1] is None
    assert f"Failed to process {victim[0]}: window at {second * 0.01:g} s made no progress" in capsys.readouterr().out
    for k, (name, w) in enumerate(items):
        if k != 1 and TR.is_long(len(w)):
            assert tr.sequences[k] == want[name]["sequence"] and tr.windows[k] == want[name]["windows"]
    assert not any(tag == tag_of(victim[1]) and seek > second for _, rows in dec.calls for tag, seek, _ in rows), "its later windows never ran"


def test_queue_failing_round_is_retried_window_by_window(capsys):
    items = corpus()
    want = expected(items)
    victim = items[3]
    at = want[victim[0]]["windows"][1][0]
    tr, enc, dec, ids = run_queue(items, 16, bad=[(tag_of(victim[1]), at)])
    assert tr.failed == [victim[0]] and ids[3] is None
    assert f"Failed to process {victim[0]}: window at {at * 0.01:g} s: decoder error word 0x1" in capsys.readouterr().out
    hit = [i for i, (_, rows) in enumerate(dec.calls) if (tag_of(victim[1]), at) in [(t, s) for t, s, _ in rows]]
    assert len(hit) == 2 and len(dec.calls[hit[0]][1]) > 1 and len(dec.calls[hit[1]][1]) == 1, "the round, then the window alone"
    mates = dec.calls[hit[0]][1]
    alone = [rows[0] for _, rows in dec.calls[hit[0] + 1: hit[0] + 1 + len(mates)]]
    assert alone == mates, "every window of the failed round ran once more, alone, in order"
    for k, (name, w) in enumerate(items):
        if k != 3 and TR.is_long(len(w)):
            assert tr.sequences[k] == want[name]["sequence"] and tr.windows[k] == want[name]["windows"]


def test_queue_refuses_beams():
    tr = TR.WhisperTranscriber(FakeEncoder(), FakeDecoder(), dataclasses.replace(make_spec(), num_beams=2))
    with pytest.raises(ValueError, match="long-form with num_beams"):
        tr.transcribe_long(iter(corpus()))


def test_generate_takes_num_frames_in_place_of_lengths():
    import inspect
    from interspeech_ser_amd.engine import WhisperDecoder
    assert inspect.signature(WhisperDecoder.generate).parameters["num_frames"].default is None


def test_command_line_refusals(capsys):
    base = ["--wav_dir", "a", "--out_csv", "b.csv", "--long_form"]
    assert TR.parse_args(base).long_form and not TR.parse_args(base[:-1]).long_form
    assert TR.parse_args(base + ["--segments_json", "s.json", "--num_beams", "1"]).segments_json == "s.json"
    for extra, flag in ((["--times_json", "t.json"], "--times_json"), (["--num_beams", "2"], "--num_beams")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            TR.parse_args(base + extra)
        err = capsys.readouterr().err
        assert "--long_form" in err and flag in err and "not built" in err


# ---------------------------------------------------------------------------------------------------------------- the end-to-end fixture
def test_fixture_conditions(golden_dir):
    """tests/golden/tiny_whisper_long_d128h2.npz (tools/make_whisper_longform_golden.py): the searched conditions hold on the stored file,
    the numpy rule fed HF's stored logits gives HF's tokens, and the loop of this module over HF's recorded windows gives HF's seeks,
    segments and sequence"""
    import os
    import whisper_dec_ref as R
    gold, geo, sd, spec, waves = LR.load_fixture(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, LR.FIXTURE)) < 1024 * 1024
    assert geo.decoder_vocab_size - spec.timestamp_begin == 1501 and all(65 * 16000 <= len(w) <= 80 * 16000 + 160 for w in waves)
    g = float(gold["g"])
    m = R.masks(spec, geo.decoder_vocab_size)
    stored, at, zmax = gold["f0_logits"].astype(np.float64), 0, float(np.abs(gold["f0_lang_logits"]).max())
    for k, row in enumerate(gold["f0_rows"]):
        row = row[row >= 0]
        for p in range(SR.P - 1, len(row) - 1):
            _, tok, mg, gp, _, _ = SR.rule(stored[at], m[1 if p == SR.P - 1 else 0], row[SR.P: p + 1], spec.timestamp_begin, spec.no_timestamps_token_id,
                                           spec.eos_token_id, spec.max_initial_timestamp_index)
            assert tok == int(row[p + 1]), (k, p)
            assert abs(mg - gold["f0_margins"][at]) < 1e-4                     # the stored logits are HF's float64 ones rounded to fp32
            assert (np.isinf(gp) and np.isinf(gold["f0_gaps"][at])) or abs(gp - gold["f0_gaps"][at]) < 1e-4
            zmax = max(zmax, float(np.abs(stored[at]).max()))
            at += 1
    assert at == len(stored) and g >= 1e-3 * max(1.0, zmax) - 1e-9, "g is taken over both files: no smaller than the main file's own"
    assert int(np.argmax(gold["f0_lang_logits"] + m[2])) == int(gold["f0_language"]) and R.top2_margin(gold["f0_lang_logits"] + m[2]) >= 4 * g
    for i in range(len(waves)):
        assert min(float(gold[f"f{i}_margins"].min()), float(gold[f"f{i}_gaps"].min()), float(gold[f"f{i}_lang_margin"])) >= 4 * g
        rows = [r[r >= 0][SR.P:].tolist() for r in gold[f"f{i}_rows"]]
        bodies = [r[: r.index(spec.eos_token_id)] if spec.eos_token_id in r else r for r in rows]
        got = LR.loop(len(waves[i]) // 160, lambda k, seek, nf: bodies[k], spec.timestamp_begin)
        assert not got["stuck"] and got["windows"] == [tuple(int(x) for x in w) for w in gold[f"f{i}_windows"]]
        assert got["sequence"] == gold[f"f{i}_sequence"].tolist() and got["seek"] == int(gold[f"f{i}_seek"])
        assert [(a, b) for a, b, _ in got["segments"]] == [(float(a), float(b)) for a, b in gold[f"f{i}_seg_times"]]
        assert [len(t) for _, _, t in got["segments"]] == gold[f"f{i}_seg_lens"].tolist()
    w = [tuple(int(x) for x in r) for r in gold["f0_windows"]]
    assert len(w) >= 3 and w[-1][1] < 3000 and all(adv > 0 for _, _, adv in w)
    assert any(adv != nf and adv % 3000 != 0 for _, nf, adv in w), "a closed pair whose advance is no multiple of 3000"
    assert any(adv == nf for _, nf, adv in w), "a window consumed whole"
