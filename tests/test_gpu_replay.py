"""Replay against fresh eager forwards, every encoder family in every mode it accepts (-m gpu).

The drivers replay a recorded command list per forward (engine.Tape: one ser_run, per-batch sizes patched in); bench.py times a
hipGraph holding two utterance groups as parallel branches (_EncoderBase.capture_concurrent).  Each case here checks both, BIT FOR BIT,
against a reference that cannot share their state: a freshly built encoder, launched kernel by kernel (``use_tape = False``), running
the batch once -- the first forward over freshly allocated buffers.  A buffer that must start at zero (padding slots, halo rows,
block-scale words, the range-guard word) and is dirtied by an earlier forward or replay shows up as a difference; comparing against an
eager forward over the SAME buffers (what the older replay tests do) cannot see it.

Per case:
  * command list across shapes -- ragged batches that grow and shrink inside one arena (one recorded list), an utterance shorter than
    one 128-query attention block among them: each equals its own fresh reference;
  * concurrent graph -- two groups captured as parallel branches and replayed three times, the uploaded waveforms overwritten in
    place with a second batch of the same shape before the second replay and restored before the third: after each replay the states
    equal the fresh reference of what the inputs were then;
  * range guard -- after every forward / replay each slot's guard word (HiddenStates.take_range_bits) equals the fresh run's.
Text encoders have no command list and no concurrent path: their repeated forwards across (slot, B, T) plans, evicted and rebuilt
ones included, equal fresh references.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# engine.MODES / engine.POST_LN_MODES (kept literal so that collection does not import the package; test_mode_lists_are_the_engines pins them)
ALL_MODES = ("f16x", "f16mf", "f16m", "fp32x", "f16a", "f16q", "f16", "bf16")
POST_LN = ("f16x", "fp32x", "bf16")
# the stable-LN speech encoders at tiny width and six layers, so that "f16mf" has a real mixed form (qkv_m_from = 2)
STABLE = {"wavlm": dict(hidden=128, heads=2, ffn=256, pos_groups=2),          # head dim 64: the FP16M context-row path
          "wav2vec2": dict(hidden=960, heads=8, ffn=512, pos_groups=8),       # head dim 120
          "hubert": dict(hidden=320, heads=4, ffn=384, pos_groups=4)}         # head dim 80
POST_LN_SPEECH = ("TINY_WAVLM_BASE", "TINY_WAV2VEC2_BASE", "TINY_HUBERT_BASE", "TINY_DATA2VEC_AUDIO", "TINY_DATA2VEC_AUDIO_G48")
TEXT = ("TINY_ROBERTA", "TINY_DEBERTA", "TINY_DEBERTA_CONV")
# speech batches (samples): the first one sets every capacity of the arena (B, rows, longest utterance), the rest fit inside it;
# 700 samples = 1 frame, 8 000 = 24 frames, 41 000 = 127 frames: shorter than one 128-query block of ser_attention
SPEECH_BATCHES = ((61000, 700, 20000, 52000, 12000), (30000, 9000), (52000, 8000, 41000), (3000,), (41000, 61000, 700, 5000))
SPEECH_GROUPS = ((30000, 9000, 41000), (22000, 8000))
# Whisper: every utterance is one 30 s window (1 500 frames, 92 in the last 128-query block); plans are per (slot, B)
WHISPER_BATCHES = ((480000, 30000), (7000, 480000, 210000), (5000, 200000), (480000,), (480000, 2000))
WHISPER_GROUPS = ((480000, 61000), (9000, 480000, 240000))


def synth_wave(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    x = 0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


@pytest.fixture(scope="module")
def weights():
    """one synthetic state dict per geometry, shared by every mode of it"""
    from interspeech_ser_amd import config as C
    from interspeech_ser_amd.weights import synthetic_state_dict
    fam = {"wavlm": C.FAMILY_WAVLM, "wav2vec2": C.FAMILY_WAV2VEC2, "hubert": C.FAMILY_HUBERT}
    cache = {}

    def get(name):
        if name not in cache:
            if name in STABLE:
                geo = C.tiny_geometry(fam[name], layers=6, **STABLE[name])
            elif name == "whisper":
                geo = C.tiny_geometry(C.FAMILY_WHISPER, hidden=128, heads=2, ffn=256, layers=6)
            elif name == "whisper_wide":
                # Whisper-large's width (D = 1 280, 20 heads of 64) at three layers: its GEMM shapes pick the tiles of the real encoder
                # (the 3-product output projection on 256 x 256 tiles of 128-column waves), and "f16mf" keeps layer 0 out of FP16M
                geo = C.tiny_geometry(C.FAMILY_WHISPER, hidden=1280, heads=20, ffn=1280, layers=3)
            else:
                geo = getattr(C, name)
            cache[name] = (geo, synthetic_state_dict(geo, 17 + len(cache), fast=name == "whisper_wide"))
        return cache[name]
    return get


def _encoder(geo, sd, mode, tape=True):
    from interspeech_ser_amd.engine import build_encoder
    enc = build_encoder(geo, sd, DEV, mode)
    enc.use_tape = tape
    return enc


def _fresh(geo, sd, mode, waves):
    """the reference: a freshly built encoder, launched kernel by kernel, runs the batch once -> (states, range bits, frame offsets)"""
    enc = _encoder(geo, sd, mode, tape=False)
    hs = enc.forward(enc.upload(waves), [len(w) for w in waves])
    torch.cuda.synchronize()
    return hs.states.clone(), hs.take_range_bits(), list(hs.frame_offs)


def _same(hs, ref, what):
    states, bits, offs = ref
    assert hs.frame_offs == offs, what
    assert hs.states.shape == states.shape, what
    if not torch.equal(hs.states, states):
        d = (hs.states - states).abs()
        bad = torch.nonzero(d.flatten(1).amax(1)).flatten().tolist()
        raise AssertionError(f"{what}: states differ from the fresh eager forward in hidden states {bad} (max |diff| {float(d.max()):.3e}, "
                             f"max |ref| {float(states.abs().max()):.3e})")
    got_bits = hs.take_range_bits()
    assert got_bits == bits, (what, got_bits, bits)


def _tape_across_shapes(geo, sd, mode, batches):
    """item 2: one encoder, taped, over ragged batches; every batch equals its own fresh reference"""
    enc = _encoder(geo, sd, mode)
    tapes = []
    for k, lens in enumerate(batches):
        waves = [synth_wave(1000 * k + i, n) for i, n in enumerate(lens)]
        ref = _fresh(geo, sd, mode, waves)
        hs = enc.forward(enc.upload(waves), list(lens))
        torch.cuda.synchronize()
        _same(hs, ref, f"command list, batch {k} {lens}")
        tapes.append(enc.recorded_tape(lens, 0))
    return enc, tapes


def _graph(geo, sd, mode, spans, concurrent=True, second=None):
    """item 3: the groups captured (parallel branches, or ``capture``'s single branch for group 0), replayed three times; the uploaded
    waveforms are overwritten in place with a second batch of the same shape before replay 2 and restored before replay 3"""
    if not concurrent:
        spans = spans[:1]
    first = [[synth_wave(5000 + 100 * g + i, n) for i, n in enumerate(lens)] for g, lens in enumerate(spans)]
    if second is None:
        second = [[synth_wave(7000 + 100 * g + i, n) for i, n in enumerate(lens)] for g, lens in enumerate(spans)]
    else:
        second = second(first)
    refs = {}
    for v, sets in enumerate((first, second)):
        for g, waves in enumerate(sets):
            assert [len(w) for w in waves] == list(spans[g])
            refs[v, g] = _fresh(geo, sd, mode, waves)
    enc = _encoder(geo, sd, mode)
    devs = [enc.upload(waves, slot=g) for g, waves in enumerate(first)]
    torch.cuda.synchronize()
    if concurrent:
        graph, outs = enc.capture_concurrent([(d, list(lens)) for d, lens in zip(devs, spans)])
    else:
        graph, hs = enc.capture(devs[0], list(spans[0]))
        outs = [hs]
    torch.cuda.synchronize()
    for hs in outs:
        hs.take_range_bits()                              # what the warm-up forwards set
    for r, v in enumerate((0, 1, 0)):
        sets = (first, second)[v]
        for d, waves in zip(devs, sets):
            d.copy_(torch.from_numpy(np.concatenate(waves)))
        graph.replay()
        torch.cuda.synchronize()
        for g, hs in enumerate(outs):
            _same(hs, refs[v, g], f"{'concurrent' if concurrent else 'single-branch'} graph, replay {r + 1}, group {g}")
    return enc


def test_mode_lists_are_the_engines():
    from interspeech_ser_amd import engine
    assert set(ALL_MODES) == set(engine.MODES) and set(POST_LN) == set(engine.POST_LN_MODES)


# SER_F16M_OUT_M only reaches the layers whose packed projection multiplies in FP16M: the f16m / f16mf modes
STABLE_CASES = [(m, False) for m in ALL_MODES] + [("f16m", True), ("f16mf", True)]


@pytest.mark.parametrize("mode,out_m", STABLE_CASES, ids=[m + ("-f16m_out" if o else "") for m, o in STABLE_CASES])
@pytest.mark.parametrize("family", ["wavlm", "wav2vec2", "hubert", "whisper"])
def test_stable_ln_replay_equals_fresh_eager(weights, monkeypatch, family, mode, out_m):
    """Stable-LN speech encoders and Whisper, every mode; ``f16m_out``: SER_F16M_OUT_M=1 (FP16M context rows and output projection from
    qkv_m_from on, head dim 64 -- WavLM and Whisper here; the others must be unaffected by the switch)."""
    if out_m:
        monkeypatch.setenv("SER_F16M_OUT_M", "1")
    else:
        monkeypatch.delenv("SER_F16M_OUT_M", raising=False)
    geo, sd = weights(family)
    whisper = family == "whisper"
    enc, tapes = _tape_across_shapes(geo, sd, mode, WHISPER_BATCHES if whisper else SPEECH_BATCHES)
    if whisper:
        assert tapes[0] is tapes[4] and tapes[2] is tapes[0]          # B = 2 revisited: the same plan, the same recorded list
    else:
        assert min(geo.frames_for(n) for n in SPEECH_BATCHES[2]) < 128
        assert all(t is tapes[0] for t in tapes)                       # one arena, one recorded list: only the Sz fields moved
    layers = enc.layers
    if mode in ("f16m", "f16mf"):
        want = out_m and geo.head_dim == 64
        assert [lay["out_m"] for lay in layers] == [want and i >= enc.qkv_m_from for i in range(geo.num_layers)]
        assert enc.qkv_m_from == {"f16m": 0, "f16mf": 2}[mode]
    del enc
    _graph(geo, sd, mode, WHISPER_GROUPS if whisper else SPEECH_GROUPS)


@pytest.mark.parametrize("mode", ["f16m", "f16mf"])
@pytest.mark.parametrize("family", ["wavlm", "whisper"])
def test_single_branch_graph_with_f16m_context_rows(weights, monkeypatch, family, mode):
    """``capture``'s single-branch graph with SER_F16M_OUT_M=1: the step between the command list and two parallel branches."""
    monkeypatch.setenv("SER_F16M_OUT_M", "1")
    geo, sd = weights(family)
    _graph(geo, sd, mode, WHISPER_GROUPS if family == "whisper" else SPEECH_GROUPS, concurrent=False)


@pytest.mark.parametrize("mode", POST_LN)
@pytest.mark.parametrize("name", POST_LN_SPEECH)
def test_post_ln_speech_replay_equals_fresh_eager(weights, name, mode):
    """The *-base speech encoders (GroupNorm stem) and data2vec-audio, their three modes."""
    geo, sd = weights(name)
    _tape_across_shapes(geo, sd, mode, SPEECH_BATCHES)
    _graph(geo, sd, mode, SPEECH_GROUPS)


@pytest.mark.parametrize("mode", POST_LN)
@pytest.mark.parametrize("name", TEXT)
def test_text_plans_equal_fresh_eager(weights, name, mode):
    """RoBERTa / DeBERTa (with and without the ConvLayer): forwards over (slot, B, T) plans -- a repeated shape with new tokens, more
    shapes than the plan cache keeps (evicted plans rebuilt), a second slot -- each equal a fresh encoder's first forward."""
    geo, sd = weights(name)
    enc = _encoder(geo, sd, mode)
    g = torch.Generator().manual_seed(3)
    seq = [(2, 40, 0), (3, 17, 0), (1, 64, 0), (2, 40, 0), (4, 9, 0), (2, 33, 0), (3, 17, 1), (2, 40, 0), (3, 17, 0)]
    for k, (B, T, slot) in enumerate(seq):
        ids = torch.randint(4, geo.vocab_size, (B, T), generator=g)
        klen = torch.randint(1, T + 1, (B,), generator=g)
        klen[0] = T                                                    # one full-length sequence
        mask = (torch.arange(T)[None, :] < klen[:, None]).to(torch.int64)
        fresh = _encoder(geo, sd, mode)
        r = fresh.forward(ids, mask)
        torch.cuda.synchronize()
        ref = (r.states.clone(), r.take_range_bits(), list(r.frame_offs))
        del fresh, r
        hs = enc.forward(ids, mask, slot=slot)
        torch.cuda.synchronize()
        _same(hs, ref, f"plan {k} (slot {slot}, B {B}, T {T})")
        assert len(enc._cache) <= 4


@pytest.mark.parametrize("out_m", [False, True], ids=["default", "f16m_out"])
@pytest.mark.parametrize("name", ["whisper", "whisper_wide"])
def test_whisper_bench_shape_concurrent_graph(weights, monkeypatch, name, out_m):
    """bench.py's Whisper launch shapes: two groups of 8 x 30 s windows (T = 1 500, M = 12 000 rows per group) as parallel graph branches
    in "f16mf", with and without SER_F16M_OUT_M=1, at tiny width and at Whisper-large's width (three layers).  The second input of each
    group is the other group's batch.  Red before the fix of ser_gemm's row partials: at D = 1 280 with the FP16M
    context rows, every replay differed from the fresh forward from hidden state 1 on."""
    if out_m:
        monkeypatch.setenv("SER_F16M_OUT_M", "1")
    else:
        monkeypatch.delenv("SER_F16M_OUT_M", raising=False)
    geo, sd = weights(name)
    enc = _graph(geo, sd, "f16mf", ((480000,) * 8, (480000,) * 8), second=lambda first: first[::-1])
    assert [lay["out_m"] for lay in enc.layers] == [out_m and i >= enc.qkv_m_from for i in range(geo.num_layers)]
    assert enc.qkv_m_from == (geo.num_layers + 2) // 3 >= 1                 # a mixed form: FP16X layers first
