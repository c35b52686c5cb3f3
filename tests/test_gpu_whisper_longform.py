"""GPU: Whisper long-form transcription (csrc/logmel_long.hip, include/ser_hip.h "a37").

A. ser_logmel_long_v through the C ABI against the float64 statement ``whisper_long_ref.log_mel_long64`` (pinned to
   WhisperFeatureExtractor by tests/test_whisper_longform_host.py): one ragged batch over the tile edges and the route's boundary, canaries
   and a NaN prefill; the floor is the FILE's; a file alone and in a batch gives the same bits; the refusals.
B. ser_mel_window_v equals slicing, bit for bit, and its refusals.
C. engine.WhisperEncoder.log_mel_long / forward_windows on the tiny Whisper geometry: window 0 of a file of exactly 480 000 samples is
   ``forward``'s input, bit for bit; a replay after changing only the row table equals a fresh plan.
D. WhisperTranscriber.transcribe_long on a tiny decoder with 1 501 timestamp tokens: every file alone, at batch 2 and at batch 16 gives the
   loop of tests/whisper_long_ref.py driven window by window through the engine; the default paths after a long-form run; the command line.
Lines that start with "LONGFORM" carry the measured figures.
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_ref as FR
import whisper_long_ref as LR
import whisper_seg_ref as SR
from interspeech_ser_amd._lib import LogmelLongArgs, MelWindowArgs            # the feature's bindings: the module needs them

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 12345.0
U32 = 2.0 ** -24


def ulp32(v):
    return float(np.spacing(np.float32(v)))


# tests/test_gpu_frontends.py's derivation, restated: what the fp32 stages that follow the fp64 DFT may add to a feature, from the formats
#   re, im rounded to fp32 (u32 each, 2 u32 on a square), one rounding per square and one for their sum       power bin: 4 u32 relative
#   201 FMAs into one accumulator, one rounding each, all terms non-negative (no cancellation)                 mel power: + 201 u32 relative
#   log10 of a value that is off by r relatively moves by r / ln 10                                            205 u32 / ln 10
#   log10f itself: 2 ulp (HIP math API), |v| <= 10                                                             + 2 ulp32(10)
#   the clamp max - 8 (|.| < 16: half an ulp) and v + 4 (|.| < 8: half an ulp); / 4 is exact and scales all of it
LOGMEL_FLOOR = ((4 + 201) * U32 / math.log(10.0) + 2 * ulp32(10.0) + 0.5 * ulp32(15.0) + 0.5 * ulp32(7.0)) / 4.0


def stream():
    return torch.cuda.current_stream().cuda_stream


def record(line):
    print("LONGFORM " + line)


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


@functools.lru_cache(maxsize=None)
def mel_matrix(n_mels):
    from interspeech_ser_amd.frontend import whisper_mel_filters
    return whisper_mel_filters(n_mels)


def noise(seed, n, sigma=0.1):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def fp32_log_mel_long(wave, mel):
    """the fp32 reference pipeline (oracle.whisper_log_mel's arithmetic) over a whole file: its distance from the statement is e_ref"""
    x = torch.from_numpy(np.asarray(wave, dtype=np.float32))
    frames = F.pad(x[None, None], (200, 200), mode="reflect")[0, 0].unfold(0, 400, 160)
    spec = torch.fft.rfft(frames * torch.hann_window(400, periodic=True, dtype=torch.float32), n=400, dim=-1)
    power = (spec.real ** 2 + spec.imag ** 2)[: len(wave) // 160].transpose(0, 1)
    log_spec = torch.clamp(torch.from_numpy(mel).transpose(0, 1) @ power, min=1e-10).log10()
    return ((torch.maximum(log_spec, log_spec.max() - 8.0) + 4.0) / 4.0).numpy()


# ---------------------------------------------------------------------------------------------------------------- ser_logmel_long_v
@functools.lru_cache(maxsize=None)
def init_table():
    from interspeech_ser_amd import _lib
    work = torch.zeros(_lib.lib.ser_workspace_bytes(_lib.WS_LOGMEL, 1, 0, 0, 0, 1), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib.ser_logmel_init(work.data_ptr(), 1, stream()), "ser_logmel_init")
    return work


def long_args(L, waves, n_mels, gap=64, scratch=None):
    """the tables of one launch, the files [n_mels][pitch] apart by ``gap`` canary floats in one NaN-prefilled buffer"""
    B = len(waves)
    lens = [len(w) for w in waves]
    Fs = [n // 160 for n in lens]
    pitches = [(f + 3) // 4 * 4 for f in Fs]
    counts = [(f + 31) // 32 for f in Fs]
    bases, at = [], gap
    for p in pitches:
        bases.append(at)
        at += n_mels * p + gap
    buf = torch.full((at,), CANARY, dtype=torch.float32, device=DEV)
    for b, p in zip(bases, pitches):
        buf[b: b + n_mels * p] = float("nan")
    offs_host = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    files = np.zeros((B, 4), dtype=np.int32)
    files[:, 0], files[:, 1], files[:, 3] = Fs, pitches, counts
    files[:, 2] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    tiles = np.stack([np.repeat(np.arange(B), counts), np.concatenate([np.arange(c) * 32 for c in counts])], axis=1).astype(np.int32)
    n_tiles = int(sum(counts))
    keep = dict(packed=torch.from_numpy(np.concatenate(list(waves) + [np.zeros(1, dtype=np.float32)])).to(DEV),
                offs=torch.from_numpy(offs_host).to(DEV), offs_host=offs_host, mel=torch.from_numpy(mel_matrix(n_mels)).to(DEV),
                bases=torch.tensor(bases, dtype=torch.int64, device=DEV), files=torch.from_numpy(files).to(DEV),
                tiles=torch.from_numpy(tiles).to(DEV), buf=buf, table=init_table(),
                scratch=torch.full((n_tiles + B,), float("nan"), dtype=torch.float32, device=DEV) if scratch is None else scratch)
    assert keep["scratch"].numel() >= n_tiles + B
    a = LogmelLongArgs()
    a.wav, a.sample_offs, a.sample_offs_host = keep["packed"].data_ptr(), keep["offs"].data_ptr(), offs_host.ctypes.data
    a.mel, a.out, a.bases = keep["mel"].data_ptr(), buf.data_ptr(), keep["bases"].data_ptr()
    a.tiles, a.files, a.table, a.scratch = keep["tiles"].data_ptr(), keep["files"].data_ptr(), keep["table"].data_ptr(), keep["scratch"].data_ptr()
    a.B, a.n_mels, a.n_tiles, a.max_pitch = B, n_mels, n_tiles, max(pitches)
    return a, keep, bases, pitches, Fs


def run_logmel_long(L, waves, n_mels, gap=64, scratch=None):
    """per file the [n_mels, F] fp32 features (numpy) of one launch; checks the canaries and that the first F columns were written"""
    a, keep, bases, pitches, Fs = long_args(L, waves, n_mels, gap, scratch)
    L.check(L.lib.ser_logmel_long_v(C.byref(a), stream()), "ser_logmel_long_v")
    torch.cuda.synchronize()
    host = keep["buf"].cpu().numpy()
    inside = np.zeros(host.shape, dtype=bool)
    out = []
    for b, p, f in zip(bases, pitches, Fs):
        inside[b: b + n_mels * p] = True
        rows = host[b: b + n_mels * p].reshape(n_mels, p)
        assert not np.isnan(rows[:, :f]).any(), "ser_logmel_long_v left part of a file's first F columns unwritten"
        out.append(rows[:, :f].copy())
    assert (host[~inside] == CANARY).all(), "ser_logmel_long_v wrote outside a file's [n_mels][pitch]"
    return out


RAGGED_F = (1, 31, 32, 33, 95, 3000, 3001, 7013)
RAGGED_R = (41, 159, 1, 80, 7, 159, 3, 119)                                   # len = 160 F + r: no multiple of 160, and >= 201 samples


@functools.lru_cache(maxsize=None)
def ragged_waves():
    return tuple(noise(500 + k, 160 * f + r) for k, (f, r) in enumerate(zip(RAGGED_F, RAGGED_R)))


@pytest.mark.parametrize("n_mels", [80, 128])
def test_logmel_long_equals_the_float64_statement(L, n_mels):
    """max |kernel - log_mel_long64| <= 2 e_ref + LOGMEL_FLOOR for every file of one ragged batch: e_ref is the fp32 reference's own
    distance from the statement on that file, LOGMEL_FLOOR (derived above) what the kernel's fp32 stages after the fp64 DFT may add"""
    waves = ragged_waves()
    got = run_logmel_long(L, waves, n_mels)
    mel = mel_matrix(n_mels)
    failures = []
    for w, g in zip(waves, got):
        ref = LR.log_mel_long64(w, mel)
        e_ref = float(np.abs(fp32_log_mel_long(w, mel).astype(np.float64) - ref).max())
        err = float(np.abs(g.astype(np.float64) - ref).max())
        gate = 2.0 * e_ref + LOGMEL_FLOOR
        record(f"logmel_long F {len(w) // 160} ({len(w)} samples) n_mels {n_mels}: kernel {err:.3e} e_ref {e_ref:.3e} gate {gate:.3e}")
        assert g.shape == ref.shape
        if not err <= gate:
            failures.append((len(w), err, gate))
    assert not failures, failures


def test_logmel_long_silence_is_exactly_the_guard(L):
    got = run_logmel_long(L, [np.zeros(160 * 40 + 9, dtype=np.float32)], 80)[0]
    assert (got == -1.5).all()


def test_logmel_long_the_clamp_is_the_files(L):
    n_mels = 80
    mel = mel_matrix(n_mels)
    quiet_then_loud = np.concatenate([noise(4, 480000, 1e-4), np.clip(noise(5, 160000 + 77, 0.3), -1, 1)]).astype(np.float32)
    F_dropped = 3100
    tail = noise(3, 160 * F_dropped + 159, 1e-4)
    loud_tail = tail.copy()
    loud_tail[-1] = 0.9                                                        # lies in the dropped frame alone
    got = run_logmel_long(L, [quiet_then_loud, tail, loud_tail], n_mels)
    ref = LR.log_mel_long64(quiet_then_loud, mel)
    raw = LR.log_mel_long_raw64(quiet_then_loud, mel)
    floor = (raw.max() - 8.0 + 4.0) / 4.0
    e_ref = float(np.abs(fp32_log_mel_long(quiet_then_loud, mel).astype(np.float64) - ref).max())
    first = got[0][:, :3000].astype(np.float64)
    assert float(np.abs(first - ref[:, :3000]).max()) <= 2.0 * e_ref + LOGMEL_FLOOR
    assert abs(float(first.min()) - floor) <= 2.0 * e_ref + LOGMEL_FLOOR and int((first == first.min()).sum()) > 1000, "the first window sits on the FILE's floor"
    per_window = FR.log_mel64(quiet_then_loud[:480000], mel)
    assert float(np.abs(first[:, :2990] - per_window[:, :2990]).max()) > 0.1, "a per-window maximum gives another floor"
    assert got[1].tobytes() == got[2].tobytes(), "a sample in the dropped frame alone moved the floor"


def test_logmel_long_alone_equals_batched_bit_for_bit(L):
    n_mels = 80
    waves = [ragged_waves()[k] for k in (0, 3, 4, 6)] + [np.concatenate([noise(4, 200000, 1e-4), noise(5, 300000 + 5, 0.3)])]
    n_tiles = sum((len(w) // 160 + 31) // 32 for w in waves)
    scratch = torch.full((n_tiles + len(waves) + 7,), float("nan"), dtype=torch.float32, device=DEV)
    both = run_logmel_long(L, waves, n_mels, scratch=scratch)
    for k in reversed(range(len(waves))):                                      # the same scratch buffer, never reset, across batch sizes
        alone = run_logmel_long(L, waves[k: k + 1], n_mels, scratch=scratch)
        assert alone[0].tobytes() == both[k].tobytes(), k
    pair = run_logmel_long(L, [waves[4], waves[1]], n_mels, gap=4, scratch=scratch)
    assert pair[0].tobytes() == both[4].tobytes() and pair[1].tobytes() == both[1].tobytes()


def test_logmel_long_refusals(L):
    waves = [noise(1, 5000), noise(2, 700)]
    for what, text in ((lambda a: setattr(a, "wav", None), "null pointer"), (lambda a: setattr(a, "sample_offs_host", None), "null pointer"),
                       (lambda a: setattr(a, "scratch", None), "null pointer"), (lambda a: setattr(a, "B", 0), "B = 0"),
                       (lambda a: setattr(a, "n_tiles", a.n_tiles + 1), "n_tiles"), (lambda a: setattr(a, "max_pitch", a.max_pitch + 4), "max_pitch")):
        a, keep, *_ = long_args(L, waves, 80)
        what(a)
        assert L.lib.ser_logmel_long_v(C.byref(a), stream()) != 0 and text.encode() in L.lib.ser_last_error(), text
        torch.cuda.synchronize()
        assert bool((keep["buf"][:64] == CANARY).all()) and bool(torch.isnan(keep["buf"][64:68]).all()), "a refused call launched"
    assert L.lib.ser_logmel_long_v(None, stream()) != 0
    a, keep, *_ = long_args(L, [noise(1, 5000), noise(2, 200)], 80)
    assert L.lib.ser_logmel_long_v(C.byref(a), stream()) != 0 and b"201" in L.lib.ser_last_error()
    a, keep, *_ = long_args(L, [noise(2, 201)], 80)
    L.check(L.lib.ser_logmel_long_v(C.byref(a), stream()), "201 samples is the shortest file")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- ser_mel_window_v
def run_window(L, src, rows, n_mels, mutate=None):
    """rows [(base, pitch, F, seek, nf)]; returns the [B, n_mels, 3000] output (numpy) or, with ``mutate``, the launcher's return code"""
    B = len(rows)
    table = np.array(rows, dtype=np.int64).reshape(B, 5)
    dev_rows = torch.from_numpy(table).to(DEV)
    n = B * n_mels * 3000
    buf = torch.full((64 + n + 64,), float("nan"), dtype=torch.float32, device=DEV)
    buf[:64] = CANARY
    buf[64 + n:] = CANARY
    a = MelWindowArgs()
    a.src, a.rows, a.rows_host, a.out, a.B, a.n_mels = src.data_ptr(), dev_rows.data_ptr(), table.ctypes.data, buf.data_ptr() + 256, B, n_mels
    if mutate is not None:
        mutate(a)
        rc = L.lib.ser_mel_window_v(C.byref(a), stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[64: 64 + n]).all()), "a refused call launched"
        return rc
    L.check(L.lib.ser_mel_window_v(C.byref(a), stream()), "ser_mel_window_v")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:64] == CANARY).all() and (host[64 + n:] == CANARY).all(), "ser_mel_window_v wrote outside [B, n_mels, 3000]"
    return host[64: 64 + n].reshape(B, n_mels, 3000)


def test_mel_window_equals_slicing_bit_for_bit(L):
    n_mels = 80
    g = np.random.default_rng(8)
    files = [(3000, 3000), (3001, 3004), (7013, 7016), (1, 4)]                # (F, pitch)
    bases, at = [], 8
    for _, p in files:
        bases.append(at)
        at += n_mels * p + 12
    host = g.standard_normal(at).astype(np.float32)
    host[host == 0.0] = 1.0
    src = torch.from_numpy(host).to(DEV)
    view = lambda k: host[bases[k]: bases[k] + n_mels * files[k][1]].reshape(n_mels, files[k][1])
    rows = [(0, 0, 3000), (1, 0, 3000), (1, 1, 3000), (1, 3000, 1), (2, 0, 3000), (2, 1001, 2999), (2, 4013, 3000), (2, 7012, 1),
            (2, 4014, 2999), (3, 0, 1), (2, 3, 1)]
    table = [(bases[k], files[k][1], files[k][0], seek, nf) for k, seek, nf in rows]
    got = run_window(L, src, table, n_mels)
    for b, (k, seek, nf) in enumerate(rows):
        want = np.zeros((n_mels, 3000), dtype=np.float32)
        want[:, :nf] = view(k)[:, seek: seek + nf]
        assert got[b].tobytes() == want.tobytes(), (k, seek, nf)
        assert not got[b][:, nf:].view(np.uint32).any(), "the pad is +0.0f: all-zero bits"
    one = run_window(L, src, table[5:6], n_mels)
    assert one[0].tobytes() == got[5].tobytes()
    good = table[2]
    for bad, text in (((good[0], good[1], good[2], 1, 0), "nf = 0"), ((good[0], good[1], good[2], 0, 3001), "nf = 3001"),
                      ((good[0], good[1], good[2], 2, 3000), "reads frames [2, 3002)"), ((good[0], good[1], good[2], -1, 5), "reads frames"),
                      ((good[0], good[2] - 1, good[2], 0, 5), "pitch")):
        assert run_window(L, src, [table[0], bad], n_mels, mutate=lambda a: None) != 0 and text.encode() in L.lib.ser_last_error(), text
    for what in (lambda a: setattr(a, "src", None), lambda a: setattr(a, "rows_host", None), lambda a: setattr(a, "B", 0), lambda a: setattr(a, "n_mels", 0)):
        assert run_window(L, src, table[:2], n_mels, mutate=what) != 0


# ---------------------------------------------------------------------------------------------------------------- the engine
@functools.lru_cache(maxsize=None)
def tiny_encoder(mode="f16x"):
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd.engine import WhisperEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    return WhisperEncoder(Cfg.TINY_WHISPER, synthetic_state_dict(Cfg.TINY_WHISPER, 14), DEV, mode)


def test_engine_log_mel_long_handle(L):
    enc = tiny_encoder()
    waves = [ragged_waves()[k] for k in (3, 6, 4)]
    h = enc.log_mel_long(enc.upload(waves), [len(w) for w in waves])
    want = run_logmel_long(L, waves, enc.geo.n_mels)
    for k in range(3):
        assert h.features(k).cpu().numpy().tobytes() == want[k].tobytes()
    h.release(1)
    more = [ragged_waves()[7], ragged_waves()[1]]                              # the first outgrows the buffer, the second fits the freed span
    assert enc.log_mel_long(enc.upload(more), [len(w) for w in more], into=h) is h and len(h) == 5
    want2 = run_logmel_long(L, more, enc.geo.n_mels)
    for k, w in ((0, want[0]), (2, want[2]), (3, want2[0]), (4, want2[1])):
        assert h.features(k).cpu().numpy().tobytes() == w.tobytes(), "a resident file survives admissions and growth"
    assert h.bases[4] == 0 or h.bases[4] < h.bases[3], "a released span is reused"
    with pytest.raises(ValueError, match="201"):
        enc.log_mel_long(enc.upload([noise(1, 200)]), [200])
    with pytest.raises(ValueError, match="not resident"):
        enc.forward_windows(h, [(1, 0, 10)])


@pytest.mark.parametrize("mode", ["f16x", "bf16"])
def test_forward_windows_window_zero_is_forward_and_replay_is_fresh(mode):
    enc = tiny_encoder(mode)
    thirty = noise(77, 480000)
    long = np.concatenate([noise(78, 300000), noise(79, 400123, 0.02)])
    ref = enc.forward(enc.upload([thirty]), [480000], slot=1)
    ref_states, ref_mel = ref.states.clone(), enc._plan([480000], 1)["mel"].clone()
    h = enc.log_mel_long(enc.upload([thirty, long]), [len(thirty), len(long)])
    hs = enc.forward_windows(h, [(0, 0, 3000)], slot=1)
    assert enc._plan_of(1, 1)["mel"].cpu().numpy().tobytes() == ref_mel.cpu().numpy().tobytes(), "window 0 of exactly 30 s is forward's log-mel"
    assert hs.states.cpu().numpy().tobytes() == ref_states.cpu().numpy().tobytes()
    F_long = len(long) // 160
    rows_a, rows_b = [(1, 0, 3000), (0, 1500, 1500)], [(1, 2999, F_long - 2999), (1, 1001, 3000)]
    first = enc.forward_windows(h, rows_a, slot=0).states.clone()              # records the (slot 0, B = 2) list
    tape = enc._plan_of(2, 0)["win"]["tape"]
    replay = enc.forward_windows(h, rows_b, slot=0).states.clone()             # replays it: only the row table changed
    assert enc._plan_of(2, 0)["win"]["tape"] is tape
    enc._cache.pop((0, 2))
    fresh = enc.forward_windows(h, rows_b, slot=0).states.clone()              # a fresh plan
    assert enc._plan_of(2, 0)["win"]["tape"] is not tape
    assert replay.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes() and not torch.equal(replay, first)
    again = enc.forward_windows(h, rows_a, slot=0).states
    assert again.cpu().numpy().tobytes() == first.cpu().numpy().tobytes()
    win = LR.window_of(h.features(1).cpu().numpy(), 2999, F_long - 2999)
    by_features = enc.forward_features(torch.from_numpy(np.stack([win, LR.window_of(h.features(1).cpu().numpy(), 1001, 3000)])).to(DEV), [480000] * 2, slot=0)
    assert by_features.states.cpu().numpy().tobytes() == replay.cpu().numpy().tobytes(), "a window is the slice, zero-padded"
    after = enc.forward(enc.upload([thirty]), [480000], slot=1)
    assert after.states.cpu().numpy().tobytes() == ref_states.cpu().numpy().tobytes(), "forward's own list is what it was"


# ---------------------------------------------------------------------------------------------------------------- the transcriber
EOS, START, TRANSLATE, TASK, NO_TS = 470, 471, 476, 477, 481
LANG_IDS = (472, 473, 474, 475)
TSB = NO_TS + 1
V_LONG = TSB + 1501                                                           # <|0.00|> .. <|30.00|>


def long_geo():
    from interspeech_ser_amd import config as Cfg
    import dataclasses
    return Cfg.with_decoder(dataclasses.replace(Cfg.TINY_WHISPER, name="tiny-whisper-long-d128h2"), 2, 2, 512, V_LONG, 64)


def long_spec(language=None):
    from interspeech_ser_amd import config as Cfg
    return Cfg.GenerationSpec(decoder_start_token_id=START, eos_token_id=EOS, pad_token_id=EOS,
                              suppress_tokens=tuple(range(30, 70)) + (START, TRANSLATE, TASK, 478, 479, 480) + LANG_IDS,
                              begin_suppress_tokens=(220, EOS), no_timestamps_token_id=NO_TS, lang_ids=LANG_IDS, task_id=TASK, max_length=24,
                              max_initial_timestamp_index=50, language=language)


@functools.lru_cache(maxsize=None)
def transcriber(mode="f16x"):
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperDecoder
    geo, spec = long_geo(), long_spec()
    dec = WhisperDecoder(geo, SR.fixture_state_dict(geo, 7, TSB, 1.0), DEV, mode, spec)
    return TR.WhisperTranscriber(tiny_encoder(mode), dec, spec)


@functools.lru_cache(maxsize=None)
def corpus():
    lengths = (700123, 16000 * 66 + 41, 481000, 100000, 480160 + 3)
    return tuple((f"f{k}.wav", np.concatenate([noise(300 + k, n // 2, 0.1), noise(400 + k, n - n // 2, 0.01 * (k + 1))])) for k, n in enumerate(lengths))


def engine_loop(tr, wave, language=None):
    """tests/whisper_long_ref.loop with every window decoded through the engine, one file at batch size 1"""
    enc, dec = tr.enc, tr.dec
    h = enc.log_mel_long(enc.upload([wave]), [len(wave)])
    state = dict(lang=language)

    def decode(k, seek, nf):
        hs = enc.forward_windows(h, [(0, seek, nf)], slot=0)
        res = dec.generate(hs.states[-1], 1, tr.spec, language=state["lang"], slot=0, timestamps=True, num_frames=[nf])
        assert not res.failed
        state["lang"] = int(res.languages[0])
        return res.lists[0]
    out = LR.loop(len(wave) // 160, decode, TSB)
    out["lang"] = state["lang"]
    return out


@pytest.mark.parametrize("mode", ["f16x", "bf16"])
def test_transcribe_long_equals_the_loop_alone_and_through_the_queue(mode):
    from interspeech_ser_amd import transcribe as TR
    tr = transcriber(mode)
    items = list(corpus())
    want = {name: engine_loop(tr, w) for name, w in items if TR.is_long(len(w))}
    assert len(want) == 4 and not any(e["stuck"] for e in want.values())
    for name, e in want.items():
        record(f"{mode} {name}: windows {e['windows']} language {e['lang']} tokens {len(e['sequence'])}")
    short = tr.transcribe([w for _, w in items if not TR.is_long(len(w))], timestamps=True)
    short_segments = list(tr.segments)
    runs = [(2, items), (16, items), (16, items[::-1])] + [(16, [it]) for it in items if TR.is_long(len(it[1]))]
    for batch, picked in runs:
        ids = tr.transcribe_long(iter(picked), batch=batch)
        assert tr.failed == []
        for k, (name, w) in enumerate(picked):
            if not TR.is_long(len(w)):
                assert ids[k] == short[0] and tr.segments[k] == short_segments[0]
                continue
            e = want[name]
            assert tr.sequences[k] == e["sequence"] and ids[k] == [t for t in e["sequence"] if t < TSB], (batch, name)
            assert tr.windows[k] == e["windows"] and tr.next_seek[k] == e["seek"] and tr.last_languages[k] == e["lang"]
            assert [(a, b, list(t)) for a, b, t in tr.segments[k]] == [(a, b, list(t)) for a, b, t in e["segments"]]
    assert any(len(e["windows"]) >= 3 for e in want.values())


def test_default_paths_after_a_long_form_run():
    tr = transcriber("f16x")
    waves = [w for _, w in corpus()][:4]
    before, before_ts = tr.transcribe(waves), tr.transcribe(waves, timestamps=True)
    segs, seeks = list(tr.segments), list(tr.next_seek)
    cut = [min(len(w), 480000) for w in waves]
    pl = tr.enc._plan(cut, 0)
    snap = lambda: C.string_at(C.addressof(pl["tape"].cmds), pl["tape"].n * C.sizeof(type(pl["tape"].cmds[0])))
    tape = snap()
    assert tr.transcribe_long(iter(corpus()), batch=4)[0] is not None
    assert tr.transcribe(waves) == before and tr.enc._plan(cut, 0) is pl and snap() == tape
    assert tr.transcribe(waves, timestamps=True) == before_ts and tr.segments == segs and tr.next_seek == seeks


def test_command_line_long_form(tmp_path, capsys):
    import wave as wavmod
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as TR
    geo, spec = long_geo(), long_spec()
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    lengths = (16000 * 33 + 5, 24000, 16000 * 61)
    for i, n in enumerate(lengths):
        with wavmod.open(str(wav_dir / f"f{i}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(np.clip(noise(70 + i, n, 0.1), -1, 1) * 32767.0).astype("<i2").tobytes())
    Cfg._REGISTRY["tiny-whisper-long"] = geo
    try:
        common = ["--ssl_type", "tiny-whisper-long", "--wav_dir", str(wav_dir), "--synthetic_weights", "--seed", "7", "--mode", "f16x"]
        before, before_json = tmp_path / "before.csv", tmp_path / "before.json"
        assert TR.run(common + ["--out_csv", str(before), "--segments_json", str(before_json)], spec=spec) == 0
        long_csv, long_json = tmp_path / "long.csv", tmp_path / "long.json"
        assert TR.run(common + ["--out_csv", str(long_csv), "--long_form", "--segments_json", str(long_json)], spec=spec) == 0
        only_csv = tmp_path / "only.csv"
        assert TR.run(common + ["--out_csv", str(only_csv), "--long_form"], spec=spec) == 0
        after, after_json = tmp_path / "after.csv", tmp_path / "after.json"
        assert TR.run(common + ["--out_csv", str(after), "--segments_json", str(after_json)], spec=spec) == 0
        tr, _ = TR.build(TR.parse_args(common + ["--out_csv", "x.csv"]), spec=spec, geo=geo)
        from interspeech_ser_amd.frontend import load_wav_16k
        loaded = [(f"f{i}.wav", load_wav_16k(str(wav_dir / f"f{i}.wav"))) for i in range(3)]
        ids = tr.transcribe_long(iter(loaded))
        for extra, flag in ((["--times_json", str(tmp_path / "t.json")], "--times_json"), (["--num_beams", "2"], "--num_beams")):
            capsys.readouterr()
            with pytest.raises(SystemExit):
                TR.run(common + ["--out_csv", str(tmp_path / "x.csv"), "--long_form"] + extra, spec=spec)
            err = capsys.readouterr().err
            assert "--long_form" in err and flag in err
        import dataclasses
        capsys.readouterr()
        assert TR.run(common + ["--out_csv", str(tmp_path / "x.csv"), "--long_form"], spec=dataclasses.replace(spec, num_beams=2)) == 0
        assert "--long_form with num_beams > 1 in generation_config.json" in capsys.readouterr().out and not (tmp_path / "x.csv").exists()
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-long")
    assert open(before, "rb").read() == open(after, "rb").read() and open(before_json, "rb").read() == open(after_json, "rb").read()
    assert open(long_csv, "rb").read() == open(only_csv, "rb").read()
    table, entries, short_entries = TR.read_table(str(long_csv)), json.load(open(long_json)), json.load(open(before_json))
    assert sorted(table) == sorted(entries) == ["f0.wav", "f1.wav", "f2.wav"]
    for k, name in enumerate(sorted(entries)):
        e = entries[name]
        assert sorted(e) == ["next_seek_s", "segments", "text", "windows"]
        assert e["text"] == " ".join(str(t) for t in ids[k]) and table[name] == (e["text"] or "nan")
        assert e["windows"] == len(tr.windows[k]) and e["next_seek_s"] == round(tr.next_seek[k] * 0.01, 2)
        assert [(a, b) for a, b, _ in e["segments"]] == [(round(a, 2), round(b, 2)) for a, b, _ in tr.segments[k]]
        if lengths[k] // 160 > 3000:
            assert e["windows"] >= 2 and e["next_seek_s"] >= round(lengths[k] // 160 * 0.01, 2)
        else:
            assert {x: e[x] for x in ("next_seek_s", "segments", "text")} == short_entries[name] and e["windows"] == 1


# ---------------------------------------------------------------------------------------------------------------- end to end against HF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = SR.P


@functools.lru_cache(maxsize=None)
def hf_fixture():
    return LR.load_fixture(GOLDEN)


@functools.lru_cache(maxsize=None)
def fixture_transcriber(mode):
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperDecoder, WhisperEncoder
    gold, geo, sd, spec, waves = hf_fixture()
    return TR.WhisperTranscriber(WhisperEncoder(geo, sd, DEV, mode), WhisperDecoder(geo, sd, DEV, mode, spec), spec)


def hf_expected(gold, i):
    """HF's record of file i: (windows [(seek, nf, advance)], sequence, segments [(start_s, end_s, ids)], final seek, language)"""
    seq = gold[f"f{i}_sequence"].tolist()
    segs, at = [], 0
    for (a, b), n in zip(gold[f"f{i}_seg_times"], gold[f"f{i}_seg_lens"]):
        segs.append((float(a), float(b), seq[at: at + int(n)]))
        at += int(n)
    assert at == len(seq)
    return [tuple(int(x) for x in w) for w in gold[f"f{i}_windows"]], seq, segs, int(gold[f"f{i}_seek"]), int(gold[f"f{i}_language"])


def device_windows(tr, wave, rows):
    """HF's windows of one file decoded one by one through the engine with the logits kept: [(DecodeResult, seek, nf)]"""
    enc, dec = tr.enc, tr.dec
    h = enc.log_mel_long(enc.upload([wave]), [len(wave)])
    out, lang = [], None
    for seek, nf, _ in rows:
        hs = enc.forward_windows(h, [(0, seek, nf)], slot=0)
        res = dec.generate(hs.states[-1], 1, tr.spec, language=lang, slot=0, timestamps=True, num_frames=[nf], keep_logits=True)
        assert not res.failed
        lang = int(res.languages[0])
        out.append((res, seek, nf))
    return out


@pytest.mark.parametrize("mode", ["f16x", "fp32x"])
def test_end_to_end_equals_hf(mode):
    """the device's logits are within g of HF's on the stored rows (the main file's decided rows: every one has margin and ts_gap >= 4 g,
    so no decision can differ), and sequences, seeks, nf, segments and texts equal HF's for every file, alone and through the queue"""
    gold, geo, sd, spec, waves = hf_fixture()
    tr = fixture_transcriber(mode)
    g = float(gold["g"])
    assert float(gold["min_margin"]) >= 4 * g
    windows, _, _, _, language = hf_expected(gold, 0)
    stored, at, worst = gold["f0_logits"].astype(np.float64), 0, 0.0
    for k, (res, seek, nf) in enumerate(device_windows(tr, waves[0], windows)):
        row = gold["f0_rows"][k]
        row = row[row >= 0]
        n = len(row) - P                                                       # decided positions P - 1 .. len(row) - 2
        assert res.sequences[0, : len(row)].tolist() == row.tolist() and (res.sequences[0, len(row):] == spec.pad_token_id).all(), (k, res.sequences[0])
        assert int(res.languages[0]) == language
        got = res.step_logits[:n, 0].cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(got - stored[at: at + n]).max()))
        at += n
    assert at == len(stored)
    record(f"end to end {mode}: max |device - HF| over {at} decided logit rows {worst:.3e}, g {g:.3e}, smallest margin / ts_gap {float(gold['min_margin']):.3e}")
    assert worst <= g, (worst, g)
    items = [(f"f{i}.wav", w) for i, w in enumerate(waves)]
    for batch, picked in [(16, [it]) for it in items] + [(2, items), (16, items), (16, items[::-1])]:
        ids = tr.transcribe_long(iter(picked), batch=batch)
        assert tr.failed == []
        for k, (name, _) in enumerate(picked):
            w, seq, segs, seek, lang = hf_expected(gold, int(name[1: -4]))
            assert tr.sequences[k] == seq and ids[k] == [t for t in seq if t < spec.timestamp_begin], (batch, name)
            assert tr.windows[k] == w and tr.next_seek[k] == seek and tr.last_languages[k] == lang
            assert [(a, b, list(t)) for a, b, t in tr.segments[k]] == segs
    w0 = hf_expected(gold, 0)[0]
    assert len(w0) >= 3 and any(adv != nf and adv % 3000 for _, nf, adv in w0) and any(adv == nf for _, nf, adv in w0) and w0[-1][1] < 3000


def test_end_to_end_bf16_is_the_rule_on_its_own_logits():
    """bf16 is not pinned to HF: over the device's own loop, the numpy rule fed the device's kept logits reproduces the device's tokens"""
    import whisper_dec_ref as R
    gold, geo, sd, spec, waves = hf_fixture()
    tr = fixture_transcriber("bf16")
    ids = tr.transcribe_long(iter([("f0.wav", waves[0])]))
    assert ids[0] is not None and len(tr.windows[0]) >= 2
    m = R.masks(spec, geo.decoder_vocab_size)
    checked = 0
    for res, seek, nf in device_windows(tr, waves[0], tr.windows[0]):
        logits = res.step_logits[:, 0].cpu().numpy()
        for s in range(logits.shape[0]):
            p = P - 1 + s
            if p + 1 >= res.sequences.shape[1]:
                break
            _, tok, _, _, _, _ = SR.rule(logits[s].astype(np.float64), m[1 if s == 0 else 0], res.sequences[0, P: p + 1], spec.timestamp_begin,
                                         spec.no_timestamps_token_id, spec.eos_token_id, spec.max_initial_timestamp_index)
            assert tok == int(res.sequences[0, p + 1]), (seek, p)
            checked += 1
            if tok == spec.eos_token_id:
                break
        segs, adv = SR.segments_of(res.lists[0], spec.timestamp_begin, nf, float(seek) * 0.02 / 2)
        assert (seek, nf, adv) in tr.windows[0]
    assert checked >= 3 * len(tr.windows[0])


def test_command_line_long_form_writes_hf_texts_and_segments(tmp_path, monkeypatch):
    """--long_form on the fixture's files (the loader and the model handed in: the fixture's waves are not 16-bit) writes HF's texts and
    segments"""
    from interspeech_ser_amd import frontend
    from interspeech_ser_amd import transcribe as TR
    gold, geo, sd, spec, waves = hf_fixture()
    tr = fixture_transcriber("f16x")
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    for i in range(len(waves)):
        (wav_dir / f"f{i}.wav").write_bytes(b"")
    monkeypatch.setattr(TR, "build", lambda args, spec=None, geo=None: (tr, None))
    monkeypatch.setattr(frontend, "load_wav_16k", lambda path, resample=False: waves[int(os.path.basename(path)[1: -4])])
    out_csv, out_json = tmp_path / "t.csv", tmp_path / "s.json"
    assert TR.run(["--wav_dir", str(wav_dir), "--out_csv", str(out_csv), "--long_form", "--segments_json", str(out_json)], spec=spec) == 0
    table, entries = TR.read_table(str(out_csv)), json.load(open(out_json))
    tsb = spec.timestamp_begin
    for i in range(len(waves)):
        w, seq, segs, seek, _ = hf_expected(gold, i)
        e = entries[f"f{i}.wav"]
        assert e["text"] == " ".join(str(t) for t in seq if t < tsb) == table[f"f{i}.wav"]
        assert e["windows"] == len(w) and e["next_seek_s"] == round(seek * 0.01, 2)
        assert e["segments"] == [[round(a, 2), round(b, 2), " ".join(str(t) for t in ids if t < tsb)] for a, b, ids in segs]
