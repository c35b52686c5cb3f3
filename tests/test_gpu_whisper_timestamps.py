"""GPU: Whisper token timestamps (csrc/whisper_ts.hip, include/ser_hip.h "a33") against the numpy rule (tests/whisper_ts_ref.py) and HF's
recorded matrices and times (tests/golden/tiny_whisper_ts_d128h2.npz, tools/make_whisper_timestamps_golden.py).

Token-time equality is asserted only where it follows from the matrix gate: every fixture item's margin mu (the cost of the best path
with other jump times, minus the optimum) covers twice what a matrix within g = 1e-3 max(1, max|matrix|) of HF's and the fp32 cost table
can move a path's cost by (asserted on the CPU, tests/test_whisper_timestamps_host.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import whisper_dec_ref as R
import whisper_ts_ref as TS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = -777
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32), device=DEV)


# ---------------------------------------------------------------------------------------------------------------- the DTW kernel
def run_dtw(mats, max_rows=None, max_frames=None, pad=3):
    """ser_dtw_v over a batch of matrices (fp32 [N_b, M_b], shapes free); every output lies between canaries.  Returns per utterance
    (first frames, status, path text, path time) with the path in FORWARD order."""
    from interspeech_ser_amd._lib import DtwArgs, check, lib
    B = len(mats)
    rows, frames = [m.shape[0] for m in mats], [m.shape[1] for m in mats]
    R_, F_ = max_rows or max(1, max(rows)), max_frames or max(1, max(frames))
    ld_m, ld_t, pl = F_ + pad, R_ + pad, R_ + F_
    host = np.full((B, R_, ld_m), np.float32(3e38), dtype=np.float32)            # beyond a matrix: values that would wreck a path
    for b, m in enumerate(mats):
        host[b, : rows[b], : frames[b]] = m
    mat = torch.from_numpy(host).to(DEV)
    nb = int(lib.ser_dtw_work_bytes(B, R_, F_))
    assert nb == 8 * B * R_ * ((F_ + 31) // 32)
    work = torch.full((nb // 8 + 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    first = torch.full((B + 2, ld_t), CANARY, dtype=torch.int32, device=DEV)
    status = torch.full((B + 2,), CANARY, dtype=torch.int32, device=DEV)
    ptext = torch.full((B + 2, pl), CANARY, dtype=torch.int32, device=DEV)
    ptime = torch.full((B + 2, pl), CANARY, dtype=torch.int32, device=DEV)
    plen = torch.full((B + 2,), CANARY, dtype=torch.int32, device=DEV)
    n_rows, n_frames = dev_i32(rows), dev_i32(frames)
    a = DtwArgs()
    a.matrix, a.ld_m, a.n_rows, a.n_frames = mat.data_ptr(), ld_m, n_rows.data_ptr(), n_frames.data_ptr()
    a.work, a.work_bytes = work.data_ptr() + 8, nb
    a.first_frame, a.ld_t, a.status = first[1].data_ptr(), ld_t, status[1:].data_ptr()
    a.path_text, a.path_time, a.path_len = ptext[1].data_ptr(), ptime[1].data_ptr(), plen[1:].data_ptr()
    a.B, a.max_rows, a.max_frames = B, R_, F_
    check(lib.ser_dtw_v(C.byref(a), stream()), "ser_dtw")
    torch.cuda.synchronize()
    first, status, ptext, ptime, plen, work = (t.cpu().numpy() for t in (first, status, ptext, ptime, plen, work))
    assert (first[0] == CANARY).all() and (first[-1] == CANARY).all() and status[0] == CANARY and status[-1] == CANARY
    assert (ptext[[0, -1]] == CANARY).all() and (ptime[[0, -1]] == CANARY).all() and plen[0] == CANARY and plen[-1] == CANARY
    assert work[0] == 0x5A5A5A5A5A5A5A5A and work[-1] == 0x5A5A5A5A5A5A5A5A
    out = []
    for b in range(B):
        n = int(plen[1 + b])
        assert (first[1 + b, rows[b]:] == CANARY).all() and (ptext[1 + b, n:] == CANARY).all() and (ptime[1 + b, n:] == CANARY).all()
        out.append((first[1 + b, : rows[b]], int(status[1 + b]), ptext[1 + b, :n][::-1], ptime[1 + b, :n][::-1]))
    return out


def check_dtw(mats, **kw):
    for m, (first, status, text, time) in zip(mats, run_dtw(mats, **kw)):
        rt, ri, cost = TS.dtw_diag(m)
        assert np.array_equal(text, rt) and np.array_equal(time, ri), m.shape        # the path, cell for cell
        assert np.array_equal(first, TS.first_frames(rt, ri)), m.shape               # the times
        assert status == (0 if np.isfinite(cost[-1, -1]) else 1), m.shape


def test_dtw_small_shapes_equal_the_rule():
    """N and M at 1, 2, 63 / 64 / 65 (a wave of rows), M around the 32-frame back-pointer word and the 8-frame read-ahead, N > M, in one
    batch of mixed shapes: each utterance is its own block."""
    g = np.random.default_rng(5)
    shapes = [(n, m) for n in (1, 2, 63, 64, 65) for m in (1, 2, 63, 64, 65)]
    shapes += [(3, m) for m in (7, 8, 9, 15, 16, 17, 31, 32, 33)] + [(40, 5), (65, 2), (128, 33), (129, 31)]
    check_dtw([g.standard_normal(s).astype(np.float32) for s in shapes])


def test_dtw_band_boundaries_equal_the_rule():
    """one past every boundary of the backtrack's bands (SER_TS_BAND = 256 frames) and of the 64-bit words inside them"""
    from interspeech_ser_amd._lib import TS_BAND
    assert TS_BAND == 256
    g = np.random.default_rng(6)
    shapes = [(5, 255), (5, 256), (5, 257), (70, 288), (70, 289), (9, 511), (9, 512), (9, 513), (200, 300), (300, 200)]
    check_dtw([g.standard_normal(s).astype(np.float32) for s in shapes])


def test_dtw_ties_and_non_finite_follow_the_rule():
    """a constant matrix (every comparison a tie), matrices of three values, a NaN row (the n = 2 case: time 0), +-inf entries"""
    g = np.random.default_rng(7)
    mats = [np.full((6, 40), 0.5, np.float32), np.zeros((64, 65), np.float32), g.integers(-1, 2, (33, 70)).astype(np.float32),
            g.integers(0, 2, (65, 20)).astype(np.float32), np.full((1, 9), np.nan, np.float32)]
    bad = g.standard_normal((4, 12)).astype(np.float32)
    bad[2, 5], bad[1, 3] = np.inf, -np.inf
    mats.append(bad)
    nanm = g.standard_normal((3, 10)).astype(np.float32)
    nanm[1, 4] = np.nan
    mats.append(nanm)
    res = run_dtw(mats)
    for m, (first, status, text, time) in zip(mats, res):
        rt, ri, cost = TS.dtw_diag(m)
        assert np.array_equal(text, rt) and np.array_equal(time, ri)
        if rt.min() >= 0:                                                      # (a path through NaNs may leave the matrix: no times then)
            assert np.array_equal(first, TS.first_frames(rt, ri))
        assert status == (0 if np.isfinite(cost[-1, -1]) else 1)
    assert res[4][0].tolist() == [0] and res[4][1] == 1                           # the NaN row: time 0; the status is the caller's to ignore


def test_dtw_at_the_maxima_and_status_words():
    """444 x 1500 beside a small utterance, no rows, no frames, and counts outside the buffers: each utterance alone"""
    from interspeech_ser_amd._lib import DtwArgs, TS_BAD_SHAPE, TS_NO_FRAMES, check, lib
    g = np.random.default_rng(8)
    big, small = g.standard_normal((444, 1500)).astype(np.float32), g.standard_normal((4, 9)).astype(np.float32)
    check_dtw([big, small], max_rows=444, max_frames=1500, pad=0)
    # status words: the counts come from device tables, so they are set by hand here
    mat = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(small, (4, 4, 9)))).to(DEV)
    rows, frames = dev_i32([4, 0, 3, 5]), dev_i32([9, 9, 0, 9])
    first = torch.full((4, 4), CANARY, dtype=torch.int32, device=DEV)
    status = torch.full((4,), CANARY, dtype=torch.int32, device=DEV)
    work = torch.zeros(int(lib.ser_dtw_work_bytes(4, 4, 9)) // 8, dtype=torch.int64, device=DEV)
    a = DtwArgs()
    a.matrix, a.ld_m, a.n_rows, a.n_frames, a.work, a.work_bytes = mat.data_ptr(), 9, rows.data_ptr(), frames.data_ptr(), work.data_ptr(), work.numel() * 8
    a.first_frame, a.ld_t, a.status, a.B, a.max_rows, a.max_frames = first.data_ptr(), 4, status.data_ptr(), 4, 4, 9
    check(lib.ser_dtw_v(C.byref(a), stream()), "ser_dtw")
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, TS_NO_FRAMES, TS_BAD_SHAPE]
    rt, ri, _ = TS.dtw(small)
    assert first[0].cpu().tolist() == TS.first_frames(rt, ri).tolist() and (first[1:].cpu().numpy() == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------- the matrix stage
def run_matrix(ws, width=7, pad=2):
    """ser_ts_matrix_v over weights the test uploads (fp32 [A, R_b, F_b] per utterance); (matrices, status)."""
    from interspeech_ser_amd._lib import TsMatrixArgs, check, lib
    B, A = len(ws), ws[0].shape[0]
    rows, frames = [w.shape[1] for w in ws], [w.shape[2] for w in ws]
    R_, F_ = max(rows), max(frames)
    ld = F_ + pad
    host = np.full((B, A, R_, ld), np.float32(1e30), dtype=np.float32)
    for b, w in enumerate(ws):
        host[b, :, : rows[b], : frames[b]] = w
    wd = torch.from_numpy(host).to(DEV)
    stats = torch.zeros(B * A * F_ * 2, dtype=torch.float64, device=DEV)
    mat = torch.full((B + 2, R_, ld), float(CANARY), dtype=torch.float32, device=DEV)
    status = torch.full((B + 2,), CANARY, dtype=torch.int32, device=DEV)
    n_rows, n_frames = dev_i32(rows), dev_i32(frames)
    a = TsMatrixArgs()
    a.w, a.ld_w, a.n_rows, a.n_frames, a.stats = wd.data_ptr(), ld, n_rows.data_ptr(), n_frames.data_ptr(), stats.data_ptr()
    a.matrix, a.ld_m, a.status = mat[1].data_ptr(), ld, status[1:].data_ptr()
    a.B, a.n_align, a.max_rows, a.max_frames, a.width = B, A, R_, F_, width
    check(lib.ser_ts_matrix_v(C.byref(a), stream()), "ser_ts_matrix")
    torch.cuda.synchronize()
    mat, status = mat.cpu().numpy(), status.cpu().numpy()
    assert (mat[[0, -1]] == CANARY).all() and status[0] == CANARY and status[-1] == CANARY
    out = []
    for b in range(B):
        assert (mat[1 + b, rows[b]:] == CANARY).all() and (mat[1 + b, :, frames[b]:] == CANARY).all()
        out.append(mat[1 + b, : rows[b], : frames[b]])
    return out, status[1:-1]


def matrix_bound(w, m64):
    """The bound before the final rounding, from the operations used.  The device runs the rule's operations in the rule's order (sums in
    ascending row order, two passes, no contraction; IEEE float64 add, multiply, division and square root, which the device library rounds
    correctly), so the statistics and z-scores carry the SAME rounding as numpy's: the bound only has to cover a library whose division or
    sqrt is off by one unit in the last place.  One ulp of the mean moves z by eps |mean| / std, one ulp of std or of the division moves it by
    eps |z|; the median selects, the head mean adds A terms.  K = 4 of those units each."""
    eps = 2.0 ** -52
    w = w.astype(np.float64)
    mean, std = w.mean(1), w.std(1)
    amp = float((np.abs(mean) / std).max())
    return 4 * eps * (amp + 2 * float(np.abs(m64).max()) + w.shape[0]) * 4


@pytest.mark.parametrize("A", [1, 3])
def test_matrix_stage_equals_the_rule(A):
    """F in {1, 3, 4, 7, the 256-thread tile's edge}, rows 2 .. 9 in one batch; compared BEFORE the final rounding: the device's fp32 entry
    is the rounding of a float64 value within ``matrix_bound`` of the rule's."""
    g = np.random.default_rng(20 + A)
    shapes = [(2, 1), (3, 3), (5, 4), (4, 7), (9, 255), (6, 256), (7, 257), (8, 33)]
    ws = [(g.random((A, r, f)) / 1500).astype(np.float32) for r, f in shapes]
    mats, status = run_matrix(ws)
    assert (status == 0).all()
    for w, m in zip(ws, mats):
        m64 = TS.matrix64(w)
        tol = matrix_bound(w, m64)
        lo, hi = (m64 - tol).astype(np.float32), (m64 + tol).astype(np.float32)
        assert ((lo <= m) & (m <= hi)).all(), (w.shape, float(np.abs(m - m64).max()))
        exact = float((m == TS.matrix(w)).mean())
        print(f"TSMATRIX A={A} shape {w.shape[1:]}: {100 * exact:.1f}% of the entries equal the rule's fp32 bit for bit")


def test_matrix_stage_status_words():
    """a column whose std is 0 fails its utterance alone; one row is NaN by the rule and sets nothing; its batch mates are untouched"""
    from interspeech_ser_amd._lib import TS_NONFINITE
    g = np.random.default_rng(30)
    good = (g.random((2, 4, 12)) / 1500).astype(np.float32)
    flat = good.copy()
    flat[1, :, 7] = flat[1, 0, 7]                                              # head 1, frame 7: the same weight in all 4 rows (x + x + x + x and / 4 are exact: std = 0)
    one = good[:, :1].copy()
    nan = good.copy()
    nan[0, 2, 3] = np.nan
    mats, status = run_matrix([good, flat, one, nan, good])
    assert status.tolist() == [0, TS_NONFINITE, 0, TS_NONFINITE, 0]
    assert np.array_equal(mats[0].view(np.uint32), mats[4].view(np.uint32)) and np.isfinite(mats[0]).all()
    alone, _ = run_matrix([good])
    assert np.array_equal(alone[0].view(np.uint32), mats[0].view(np.uint32))
    assert np.isnan(mats[2]).all()


# ---------------------------------------------------------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def fx():
    gold, geo, sd, spec, enc = R.load_fixture(GOLDEN)
    ts = np.load(os.path.join(GOLDEN, "tiny_whisper_ts_d128h2.npz"))
    assert int(ts["decoder_seed"]) == int(gold["decoder_seed"]) and int(ts["enc_seed"]) == int(gold["enc_seed"])
    import dataclasses
    spec_ts = dataclasses.replace(spec, max_length=int(ts["max_length"]), alignment_heads=tuple((int(l), int(h)) for l, h in ts["alignment_heads"]))
    return dict(gold=gold, geo=geo, sd=sd, spec=spec, spec_ts=spec_ts, enc=enc, ts=ts)


@functools.lru_cache(maxsize=None)
def decoder(mode):
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = R.load_fixture(GOLDEN)
    return WhisperDecoder(geo, sd, DEV, mode, spec)


def enc_dev(enc, rows):
    return torch.from_numpy(np.ascontiguousarray(enc[rows])).to(DEV).reshape(-1, enc.shape[-1])


def item_matrix(res, b, n, F):
    return res.ts_matrix[b, : n - 1, :F].cpu().numpy()


def test_capture_leaves_decoding_untouched(fx):
    """generate(token_times=True): the same sequences and margins, bit for bit; the default plan's tape keeps its command count (11 per
    layer + 4) and the capture plan adds one launch per layer that holds an alignment head"""
    dec, spec = decoder("f16x"), fx["spec_ts"]
    lengths = [int(x) for x in fx["ts"]["lengths"]]
    plain = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec)
    timed = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True, lengths=lengths)
    again = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec)
    for r in (timed, again):
        assert np.array_equal(r.sequences, plain.sequences) and np.array_equal(r.margins.view(np.uint32), plain.margins.view(np.uint32))
        assert r.lists == plain.lists and not r.failed
    assert plain.token_times is None and plain.ts_status is None
    L = fx["geo"].decoder_layers
    default, capture = dec._plans[(0, 3)], dec._plans[(0, 3, spec.alignment_heads)]
    assert default["tape"].n == 11 * L + 4 and default["heads"] is None
    assert capture["tape"].n == default["tape"].n + len({l for l, _ in spec.alignment_heads})


def run_fixture(fx, mode):
    dec, spec, ts = decoder(mode), fx["spec_ts"], fx["ts"]
    lengths = [int(x) for x in ts["lengths"]]
    res = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True, lengths=lengths)
    assert not res.failed and (res.ts_status == 0).all()
    worst = []
    for b in range(3):
        n, F = int(ts["n_tokens"][b]), int(ts["frames"][b])
        ref = ts["matrix"][b, : n - 1, :F]
        worst.append(float(np.abs(item_matrix(res, b, n, F).astype(np.float64) - ref).max()) / float(ts["g"][b]))
    return res, worst


@pytest.mark.parametrize("mode", ["fp32x", "f16x"])
def test_token_times_equal_hf(fx, mode):
    """matrix within g of HF's float64 matrix, THEN token times equal to HF's for every item; alone == in the batch of 3, bit for bit; a
    second replay is identical"""
    dec, spec, ts = decoder(mode), fx["spec_ts"], fx["ts"]
    lengths = [int(x) for x in ts["lengths"]]
    res, worst = run_fixture(fx, mode)
    print(f"TSMATRIX {mode}: worst |device - HF| per item, in units of g: {[round(x, 4) for x in worst]}")
    assert max(worst) <= 1.0, worst
    mats = []
    for b in range(3):
        n, F = int(ts["n_tokens"][b]), int(ts["frames"][b])
        assert np.array_equal(res.sequences[b, : 4 + n], ts["sequences"][b, : 4 + n])
        assert np.array_equal(res.token_times[b], ts["token_timestamps"][b, 4: 4 + n]), (b, res.token_times[b])
        assert res.token_times[b].dtype == np.float32 and len(res.token_frames[b]) == n - 1
        mats.append(item_matrix(res, b, n, F))
    again = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True, lengths=lengths)
    for b in range(3):
        n, F = int(ts["n_tokens"][b]), int(ts["frames"][b])
        assert np.array_equal(item_matrix(again, b, n, F).view(np.uint32), mats[b].view(np.uint32))
        assert np.array_equal(again.token_frames[b], res.token_frames[b])
        one = dec.generate(enc_dev(fx["enc"], slice(b, b + 1)), 1, spec, token_times=True, lengths=lengths[b:b + 1])
        assert np.array_equal(item_matrix(one, 0, n, F).view(np.uint32), mats[b].view(np.uint32))
        assert np.array_equal(one.token_frames[0], res.token_frames[b]) and np.array_equal(one.token_times[0], res.token_times[b])


# worst |device - HF| of the fixture's matrices in bf16, in units of g, measured once on the MI355X (profiles/whisper_timestamps.txt,
# 2026-10-20): 11.84 / 12.48 / 13.24 g for the three items
BF16_MEASURED_G = 13.24


def test_token_times_bf16_measured(fx):
    """bf16 operands round every GEMM input to 8 bits: no gate from first principles and NO time equality in this mode.  The matrix
    error is measured and held to twice the value measured once on the MI355X."""
    res, worst = run_fixture(fx, "bf16")
    print(f"TSMATRIX bf16: worst |device - HF| per item, in units of g: {[round(x, 4) for x in worst]}")
    assert max(worst) <= 2 * BF16_MEASURED_G, (worst, BF16_MEASURED_G)


def test_edge_cases_and_failures(fx):
    """no frames fails the file alone (its batch mates keep their times); one generated token gives 0; two give the NaN row and 0;
    asking for times without alignment_heads raises the named error"""
    import dataclasses
    from interspeech_ser_amd._lib import TS_NO_FRAMES
    dec, spec, ts = decoder("f16x"), fx["spec_ts"], fx["ts"]
    lengths = [int(x) for x in ts["lengths"]]
    ref = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True, lengths=lengths)
    res = dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True, lengths=[lengths[0], 319, lengths[2]])
    assert res.ts_status.tolist() == [0, TS_NO_FRAMES, 0] and res.token_times[1] is None and not res.failed
    for b in (0, 2):
        assert np.array_equal(res.token_times[b], ref.token_times[b]) and np.array_equal(res.token_frames[b], ref.token_frames[b])
    for max_length, n in ((5, 1), (6, 2)):
        short = dec.generate(enc_dev(fx["enc"], slice(None)), 3, dataclasses.replace(spec, max_length=max_length), token_times=True, lengths=lengths)
        assert (short.ts_status == 0).all() and all(len(t) == n and (t == 0).all() for t in short.token_times)
    with pytest.raises(ValueError, match="alignment_heads"):
        dec.generate(enc_dev(fx["enc"], slice(None)), 3, fx["spec"], token_times=True, lengths=lengths)
    with pytest.raises(ValueError, match="lengths"):
        dec.generate(enc_dev(fx["enc"], slice(None)), 3, spec, token_times=True)


class _FakeEncoder:
    """The fixture's encoder states behind WhisperEncoder's interface: the transcriber's plumbing without an encoder forward."""

    def __init__(self, enc):
        self.enc, self.waves = enc, None

    def upload(self, waves, slot):
        self.waves = waves
        return None

    def forward(self, wav, lengths, slot=0):
        from types import SimpleNamespace
        rows = [int(w[0]) for w in self.waves]                                  # a wave's first sample names its fixture item
        return SimpleNamespace(states=[enc_dev(self.enc, rows)], take_range_bits=lambda: 0)


def test_transcriber_token_times_and_a_file_that_fails_alone(fx, capsys):
    from interspeech_ser_amd.transcribe import WhisperTranscriber
    ts, spec = fx["ts"], fx["spec_ts"]
    lengths = [int(x) for x in ts["lengths"]]
    waves = [np.full(lengths[b], float(b), dtype=np.float32) for b in range(3)] + [np.full(100, 1.0, dtype=np.float32)]
    tr = WhisperTranscriber(_FakeEncoder(fx["enc"]), decoder("f16x"), spec)
    ids = tr.transcribe(waves, ["a.wav", "b.wav", "c.wav", "short.wav"], token_times=True)
    out = capsys.readouterr().out
    assert "Failed to process short.wav: token times status 0x4" in out and tr.failed == ["short.wav"]
    times = tr.token_times
    assert times[3] is None and ids[3] == tr.transcribe(waves[3:])[0] and tr.failed == []      # no times; the ids do not depend on the flag
    capsys.readouterr()
    for b in range(3):
        n = int(ts["n_tokens"][b])
        row = ts["sequences"][b, 4: 4 + n].tolist()
        want = row[:-1] if row[-1] == spec.eos_token_id else row
        assert ids[b] == want
        assert times[b] == [float(t) for t in ts["token_timestamps"][b, 4: 4 + len(want)]]
    plain = tr.transcribe(waves[:3])
    assert plain == ids[:3] and tr.token_times == [None] * 3 and tr.failed == []
    with pytest.raises(ValueError, match="alignment_heads"):
        WhisperTranscriber(_FakeEncoder(fx["enc"]), decoder("f16x"), fx["spec"]).transcribe(waves[:1], token_times=True)


def test_command_line_writes_times_json_and_the_same_table(fx, tmp_path, capsys):
    """preprocessing/transcribe_whisper.py --times_json: the CSV is byte for byte the one without the flag; the JSON has an entry per file
    whose times exist (tokens only: no vocabulary files), none for the file without a frame"""
    import json
    import wave
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as T
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    sizes = {"a.wav": 4800, "b.wav": 11200, "c.wav": 200}
    rng = np.random.default_rng(4)
    for name, n in sizes.items():
        with wave.open(str(wav_dir / name), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(np.clip(0.1 * rng.standard_normal(n), -1, 1) * 32767.0).astype("<i2").tobytes())
    Cfg._REGISTRY["tiny-whisper-dec-times"] = fx["geo"]
    try:
        common = ["--ssl_type", "tiny-whisper-dec-times", "--wav_dir", str(wav_dir), "--synthetic_weights", "--seed", "7", "--mode", "f16x"]
        assert T.run(common + ["--out_csv", str(tmp_path / "plain.csv")], spec=fx["spec_ts"]) == 0
        assert T.run(common + ["--out_csv", str(tmp_path / "timed.csv"), "--times_json", str(tmp_path / "t.json")], spec=fx["spec_ts"]) == 0
        out = capsys.readouterr().out
        assert T.run(common + ["--out_csv", str(tmp_path / "none.csv"), "--times_json", str(tmp_path / "none.json")], spec=fx["spec"]) == 0
        assert "alignment_heads" in capsys.readouterr().out and not os.path.exists(tmp_path / "none.json")
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-dec-times")
    assert open(tmp_path / "plain.csv", "rb").read() == open(tmp_path / "timed.csv", "rb").read()
    table = T.read_table(str(tmp_path / "timed.csv"))
    times = json.loads(open(tmp_path / "t.json").read())
    assert sorted(table) == sorted(sizes) and sorted(times) == ["a.wav", "b.wav"] and "Failed to process c.wav: token times status 0x4" in out
    for name in ("a.wav", "b.wav"):
        e = times[name]
        assert e["text"] == table[name] and "words" not in e and [str(t[0]) for t in e["tokens"]] == table[name].split()
        F = (sizes[name] // 160) // 2
        starts = [t[1] for t in e["tokens"]]
        assert starts == sorted(starts) and starts[0] == 0.0 and max(starts) <= 0.02 * (F - 1) + 1e-9
        assert all(a[2] == b[1] for a, b in zip(e["tokens"], e["tokens"][1:])) and e["tokens"][-1][2] == e["tokens"][-1][1]
