"""GPU: Whisper segment timestamps (csrc/whisper_seg.hip, include/ser_hip.h "a36").

A. ser_dec_select_ts_v against the rule (tests/whisper_seg_ref.py) on scripted logits, no model: token, margin, finished, *pos and
   *unfinished exact, ts_gap within the float64 bound of ``gap_bound``; every branch of the rule, ties, L == M, forced and finished rows,
   the error bits, a row alone against the same row in a batch.  Every scripted row decides its sum rule by at least 1e-3 or by an exact
   tie (checked on the rule, on the CPU, before anything is launched).
B. The command line.
C. The engine on tests/golden/tiny_whisper_seg_d128h2.npz: HF's sequences, segments and seek advance in f16x and fp32x where four times the
   measured logit error stays below the fixture's smallest margin and ts_gap; bf16 against the rule on its own logits; the default path
   after a timestamps run.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import whisper_dec_ref as R
import whisper_seg_ref as SR
from interspeech_ser_amd._lib import DecSelectTsArgs                          # the feature's binding: the module needs it
from test_gpu_whisper_decoder import enc_dev, stream, synth_wave, teacher_forced_device

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAXPOS, P = 16, 3
MIN_GAP = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gap_bound(V, *magnitudes):
    """|device - numpy| of ts_gap = |L - M| from the same fp32 values, u = 2^-53: S = sum exp(x_v - m) has at most V terms in (0, 1], each
    exp within 1 ulp = 2 u relative, added in some order: S (1 + d), |d| <= (V + 1) u; log S moves by |d| absolutely plus its own ulp,
    2 u |log S|; L = m + log S and L - M add one rounding each, u times their magnitude.  One side: u ((V + 1) + 2 |log S| + |L| + |L - M|)
    <= u (V + 8) m with m the largest magnitude involved (>= 1).  Two sides: 2^-52 (V + 8) m."""
    return 2.0 ** -52 * (V + 8) * max(1.0, *[float(abs(x)) for x in magnitudes])


class Layout:
    """A token layout in a real checkpoint's order: text < eos < no_timestamps < timestamps."""

    def __init__(self, V, ts_begin):
        self.V, self.tsb, self.no_ts, self.eos, self.K = V, ts_begin, ts_begin - 1, ts_begin - 2, V - ts_begin
        self.ld = (V + 7) // 8 * 8 + (8 if V % 8 == 0 else 0)                  # a padded pitch whatever V is
        assert self.eos >= 3 and self.K >= 4

    def ts(self, k):
        return self.tsb + k


LAYOUTS = {"V9": Layout(9, 5), "V522": Layout(522, 482), "V51866": Layout(51866, 50365)}


def run_select_ts(lay, logits, ids, *, pos, forced=None, phase=None, finished=None, mask=None, max_initial=-1, pad=0, begin_index=P, mutate=None):
    """One launch.  logits fp32 [B, V] (host; the padded columns are filled with NaN: a kernel that read one would fail the batch),
    ids [B, <= MAXPOS] the rows so far.  Returns dict of the state afterwards (host)."""
    from interspeech_ser_amd import _lib
    B, V = logits.shape[0], lay.V
    z = np.full((B, lay.ld), np.nan, dtype=np.float32)
    z[:, :V] = logits
    lg = torch.from_numpy(z).to(DEV)
    mk = torch.zeros((3, V), dtype=torch.float32, device=DEV) if mask is None else torch.from_numpy(mask.astype(np.float32)).to(DEV)
    ph = torch.zeros(MAXPOS, dtype=torch.int32, device=DEV) if phase is None else torch.tensor(phase, dtype=torch.int32, device=DEV)
    fo = torch.full((MAXPOS,), -1, dtype=torch.int32, device=DEV) if forced is None else torch.tensor(forced, dtype=torch.int32, device=DEV)
    host_ids = np.full((B + 2, MAXPOS), -9, dtype=np.int32)
    for b, row in enumerate(ids):
        host_ids[b + 1, : len(row)] = row
    idt = torch.from_numpy(host_ids).to(DEV)
    fin = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    fin[B] = -9
    if finished is not None:
        fin[:B] = torch.tensor(finished, dtype=torch.int32)
    margin = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float32, device=DEV)
    gap = torch.full((B + 2, MAXPOS), -9.0, dtype=torch.float64, device=DEV)
    word = torch.tensor([pos, -9, 0, 0, 0, -9], dtype=torch.int32, device=DEV)            # pos, unfinished, work[2], err, canary
    x = DecSelectTsArgs()
    a = x.base
    a.logits, a.ldl, a.mask, a.ldm, a.phase, a.forced = lg.data_ptr(), lay.ld, mk.data_ptr(), V, ph.data_ptr(), fo.data_ptr()
    a.ids, a.ld_ids, a.finished = idt.data_ptr() + MAXPOS * 4, MAXPOS, fin.data_ptr()
    a.margin, a.ld_margin = margin.data_ptr() + MAXPOS * 4, MAXPOS
    a.pos, a.unfinished, a.work, a.err = word.data_ptr(), word.data_ptr() + 4, word.data_ptr() + 8, word.data_ptr() + 16
    a.B, a.V, a.eos, a.pad, a.max_pos = B, V, lay.eos, pad, MAXPOS
    x.ts_gap, x.ld_gap = gap.data_ptr() + MAXPOS * 8, MAXPOS
    x.ts_begin, x.no_ts, x.begin_index, x.max_initial = lay.tsb, lay.no_ts, begin_index, max_initial
    if mutate is not None:
        mutate(x)
        return _lib.lib.ser_dec_select_ts_v(C.byref(x), stream())
    _lib.check(_lib.lib.ser_dec_select_ts_v(C.byref(x), stream()), "ser_dec_select_ts_v")
    torch.cuda.synchronize()
    ids_h, mg, gp, w, f = idt.cpu().numpy(), margin.cpu().numpy(), gap.cpu().numpy(), word.cpu().numpy(), fin.cpu().numpy()
    assert (ids_h[0] == -9).all() and (ids_h[B + 1] == -9).all() and (mg[0] == -9).all() and (mg[B + 1] == -9).all() and f[B] == -9 and w[5] == -9
    assert (gp[0] == -9).all() and (gp[B + 1] == -9).all()
    written = np.zeros_like(ids_h, dtype=bool)
    if 0 <= pos < MAXPOS - 1:
        written[1: B + 1, pos + 1] = True
    assert np.array_equal(ids_h[~written], host_ids[~written]), "ids changed outside column pos + 1"
    other = np.ones_like(gp[1: B + 1], dtype=bool)
    if 0 <= pos < MAXPOS - 1:
        other[:, pos] = False
    assert (gp[1: B + 1][other] == -9).all() and (mg[1: B + 1][other] == -9).all(), "margin / ts_gap changed outside column pos"
    assert w[2] == 0 and w[3] == 0, "the ticket words must be left zero"
    col = min(max(pos, 0), MAXPOS - 1)
    return dict(token=ids_h[1: B + 1, min(pos + 1, MAXPOS - 1)], margin=mg[1: B + 1, col], gap=gp[1: B + 1, col], finished=f[:B], pos=int(w[0]),
                unfinished=int(w[1]), err=int(w[4]) & 0xffffffff)


def expect(lay, logits, ids, pos, mask_row, max_initial=None, exact_tie=()):
    """the rule per row on the fp32 logits: (tokens, fp32 margins, gaps, fired), after checking that every row decides by MIN_GAP (or is
    listed in ``exact_tie``: L == M by construction)"""
    toks, margins, gaps, fired = [], [], [], []
    for b, row in enumerate(ids):
        x, tok, _, gp, fr, _ = SR.rule(logits[b].astype(np.float64), mask_row, row[P: pos + 1], lay.tsb, lay.no_ts, lay.eos, max_initial)
        assert gp >= MIN_GAP or (b in exact_tie and gp == 0.0), f"row {b} decides its sum rule by {gp:.3e}: script it again"
        top = np.sort(x)[-2:].astype(np.float32)
        with np.errstate(invalid="ignore"):
            margins.append(np.float32(top[1] - top[0]))
        toks.append(tok)
        gaps.append(gp)
        fired.append(fr)
    return np.array(toks), np.array(margins, dtype=np.float32), np.array(gaps), fired


def check(lay, r, want, logits, rows=None):
    toks, margins, gaps, _ = want
    rows = range(len(toks)) if rows is None else rows
    for b in rows:
        assert r["token"][b] == toks[b], (b, r["token"][b], toks[b])
        assert r["margin"][b] == margins[b] or (np.isnan(r["margin"][b]) and np.isnan(margins[b])), (b, r["margin"][b], margins[b])
        if np.isinf(gaps[b]):
            assert np.isinf(r["gap"][b]) and r["gap"][b] > 0, (b, r["gap"][b])
        else:
            assert abs(r["gap"][b] - gaps[b]) <= gap_bound(lay.V, np.abs(logits[b][np.isfinite(logits[b])]).max(), gaps[b], np.log(lay.V)), (b, r["gap"][b], gaps[b])


def steady_script(lay, seed=0):
    """Rows at n = 5 generated tokens (pos = P + 4), one per branch of steps 2, 3 and 5; returns (logits [B, V] fp32, id rows, names, the
    rows whose L == M by construction)."""
    g = np.random.default_rng(seed)
    V, K, ts = lay.V, lay.K, lay.ts
    t0, t1, t2 = 0, 1, 2
    prompt = [lay.eos + 1 if lay.eos + 1 < lay.no_ts else 0, 0, 0]
    rows, zs, names = [], [], []

    def add(name, gen, edit=None, base=None):
        z = (2.0 * g.standard_normal(V)).astype(np.float32) if base is None else np.full(V, base, dtype=np.float32)
        if edit is not None:
            edit(z)
        rows.append(prompt + gen)
        zs.append(z)
        names.append(name)

    def put(**kw):
        def edit(z):
            for k, v in kw.items():
                z[int(k[1:])] = v
        return edit

    add("text-text", [ts(0), t0, t1, t0, t1], put(**{f"c{t2}": 50.0}))                               # t2 is the token the callers' static mask suppresses
    add("text-timestamp", [ts(0), t0, t1, t0, ts(1)], put(**{f"c{t1}": 30.0}))                       # text would win: only a timestamp or eos may follow
    add("text-timestamp-eos", [ts(0), t0, t1, t0, ts(1)], put(**{f"c{t1}": 30.0, f"c{lay.eos}": 25.0}))
    add("timestamp-timestamp", [ts(0), t0, t1, ts(1), ts(1)], put(**{f"c{ts(3)}": 30.0}))            # a timestamp would win: text has to follow
    add("timestamp-text", [ts(0), t0, ts(1), ts(1), t0])
    add("bound-removes-winner", [ts(0), t0, ts(2), ts(2), t1], put(**{f"c{ts(1)}": 30.0}))
    add("not-monotone", [ts(3), t0, ts(1), ts(1), t0], put(**{f"c{ts(2)}": 30.0}))                   # the LAST timestamp bounds, not the largest
    live = K - 1                                                                                  # gen [ts0, text ...]: ts(1) .. ts(K - 1) are live
    def flat_ts(best_text):
        def edit(z):
            z[lay.tsb:] = 0.2
            z[t1] = best_text
        return edit
    add("sum-fires", [ts(0), t0, t1, t0, t1], flat_ts(np.float32(0.2 + np.log(live) - 0.25)), base=-40.0)
    add("sum-silent", [ts(0), t0, t1, t0, t1], flat_ts(np.float32(0.2 + np.log(live) + 0.25)), base=-40.0)
    add("text-tie", [ts(0), t0, t1, t0, t1], put(**{f"c{t0}": 30.0, f"c{t1}": 30.0}))
    def one_live(z):
        z[ts(K - 1)] = 3.0
        z[t1] = 3.0
    add("L-equals-M", [ts(0), t0, ts(K - 2), ts(K - 2), t1], one_live, base=-40.0)                 # one live timestamp equal to the best text
    add("id-past-vocabulary", [ts(0), t0, t1, V + 3, t0], put(**{f"c{ts(K - 1)}": 30.0}))            # a teacher-forced id >= V: the bound stops at V
    return np.stack(zs), rows, names, (names.index("L-equals-M"),)


@pytest.mark.parametrize("name", ["V9", "V522"])
def test_select_ts_equals_the_rule_on_every_branch(name):
    lay = LAYOUTS[name]
    V = lay.V
    mask = np.zeros((3, V))
    mask[0, 2] = mask[1, 2] = -np.inf                                         # a suppressed text token, everywhere
    mask[1, lay.ts(0)] = -np.inf                                              # begin-suppress: <|0.00|> itself (row 1 is the first generated position)
    mask[2] = -np.inf
    mask[2, [0, 1]] = 0.0                                                     # the language set
    phase = [2] + [0] * (P - 2) + [1] + [0] * (MAXPOS - P)
    # n >= 2: every branch of steps 2, 3 and 5, a finished row among them
    z, rows, names, ties = steady_script(lay)
    pos = P + 4
    want = expect(lay, z, rows, pos, mask[0], exact_tie=ties)
    fired = dict(zip(names, want[3]))
    assert fired["sum-fires"] and not fired["sum-silent"] and not fired["L-equals-M"] and not fired["timestamp-timestamp"]
    tok = dict(zip(names, want[0]))
    assert tok["text-timestamp"] >= lay.tsb and tok["text-timestamp-eos"] == lay.eos and tok["timestamp-timestamp"] < lay.eos
    assert tok["not-monotone"] == lay.ts(2) and tok["bound-removes-winner"] != lay.ts(1) and tok["text-tie"] == 0 and tok["L-equals-M"] == 1
    fin = [0] * len(rows)
    fin[4] = 1
    r = run_select_ts(lay, z, rows, pos=pos, mask=mask, phase=phase, finished=fin, pad=7 if V > 9 else 1)
    check(lay, r, want, z, rows=[b for b in range(len(rows)) if b != 4])
    assert r["token"][4] == (7 if V > 9 else 1) and np.isinf(r["margin"][4]) and np.isinf(r["gap"][4]), "a finished row emits pad and decides nothing"
    done = [1 if b == 4 or want[0][b] == lay.eos else 0 for b in range(len(rows))]
    assert r["finished"].tolist() == done and done[names.index("text-timestamp-eos")] == 1
    assert r["pos"] == pos + 1 and r["unfinished"] == len(rows) - sum(done) and r["err"] == 0
    assert tok["id-past-vocabulary"] < lay.tsb and np.isinf(r["gap"][names.index("id-past-vocabulary")]), "bound > V: no timestamp column is left"
    assert r["margin"][names.index("text-tie")] == 0.0 and r["margin"][names.index("L-equals-M")] == 0.0 and r["gap"][names.index("L-equals-M")] == 0.0
    # n == 0: text masked; with max_initial the raw winner behind it loses; the begin-suppress row of the static mask comes first
    g = np.random.default_rng(5)
    z0 = (2.0 * g.standard_normal((3, V))).astype(np.float32)
    z0[:, 1] = 40.0                                                           # a text token would win everywhere
    z0[1, lay.ts(3)] = 30.0
    z0[2, lay.ts(0)] = 30.0                                                   # begin-suppressed
    rows0 = [[0, 0, 0]] * 3
    for mi in (None, 2, lay.K - 1, lay.K + 10):                               # the last two: ts_begin + max_initial + 1 >= V, nothing to cut
        want0 = expect(lay, z0, rows0, P - 1, mask[1], max_initial=mi)
        assert (want0[0] >= lay.tsb).all() and want0[0][2] != lay.ts(0) and (mi != 2) == (want0[0][1] == lay.ts(3))
        r0 = run_select_ts(lay, z0, rows0, pos=P - 1, mask=mask, phase=phase, max_initial=-1 if mi is None else mi)
        check(lay, r0, want0, z0)
        assert r0["err"] == 0 and r0["pos"] == P and np.isinf(r0["gap"]).all(), "n == 0 has no live text column: nothing to compare"
    # n == 1: a first timestamp is followed by text (pen_ts holds for n < 2); a teacher-forced first text token binds nothing
    z1 = (2.0 * g.standard_normal((2, V))).astype(np.float32)
    z1[0, lay.ts(2)] = 30.0
    rows1 = [[0, 0, 0, lay.ts(0)], [0, 0, 0, 1]]
    want1 = expect(lay, z1, rows1, P, mask[0])
    assert want1[0][0] < lay.tsb
    check(lay, run_select_ts(lay, z1, rows1, pos=P, mask=mask, phase=phase), want1, z1)
    # a forced position reads no logits; a prompt step (n < 0) is ser_dec_select_v's: the language set, no rule, no gap
    nan = np.full((2, V), np.nan, dtype=np.float32)
    forced = [-1] * MAXPOS
    forced[1] = lay.eos - 1
    f = run_select_ts(lay, nan, [[0, 0], [0, 0]], pos=1, mask=mask, phase=phase, forced=forced)
    assert f["token"].tolist() == [lay.eos - 1] * 2 and f["err"] == 0 and f["pos"] == 2 and np.isinf(f["margin"]).all() and np.isinf(f["gap"]).all()
    zl = (2.0 * g.standard_normal((2, V))).astype(np.float32)
    zl[0, lay.no_ts], zl[1, 0], zl[1, lay.ts(1)] = 50.0, 1.0, 60.0
    zl[0, 1], zl[0, 0] = 5.0, 4.0
    lang = run_select_ts(lay, zl, [[0], [0]], pos=0, mask=mask, phase=phase)
    assert lang["token"].tolist() == [1, 0 if zl[1, 0] > zl[1, 1] else 1] and lang["err"] == 0 and np.isinf(lang["gap"]).all()
    assert lang["margin"][0] == np.float32(1.0)


def test_select_ts_large_vocabulary_one_launch():
    """V = 51 866, ts_begin = 50 365 (large-v3), B = 3: the sum rule over 1 500 live timestamp columns fires and stays silent, and
    [text, timestamp] leaves eos and the timestamps"""
    lay = LAYOUTS["V51866"]
    z, rows, names, ties = steady_script(lay, seed=3)
    pick = [names.index(n) for n in ("sum-fires", "sum-silent", "text-timestamp")]
    z, rows = z[pick], [rows[b] for b in pick]
    g = np.random.default_rng(9)
    z[0, lay.tsb:] += (0.5 * g.standard_normal(lay.K)).astype(np.float32)       # not flat: the sum is not a multiple of one term
    z[0, 1] = np.float32(SR.logsumexp(z[0, lay.ts(1):].astype(np.float64)) - 0.25)
    pos = P + 4
    want = expect(lay, z, rows, pos, np.zeros(lay.V))
    assert want[3][:2] == [True, False] and want[0][2] >= lay.tsb
    r = run_select_ts(lay, z, rows, pos=pos)
    check(lay, r, want, z)
    assert r["err"] == 0 and r["pos"] == pos + 1 and r["unfinished"] == 3 and r["finished"].tolist() == [0, 0, 0]


def test_select_ts_errors():
    lay = LAYOUTS["V522"]
    z, rows, names, ties = steady_script(lay, seed=1)
    pos = P + 4
    assert run_select_ts(lay, z, rows, pos=pos)["err"] == 0
    bad = z.copy()
    bad[0, 100] = np.nan                                                      # a live NaN wins and fails the batch
    e = run_select_ts(lay, bad, rows, pos=pos)
    assert e["err"] & 1 and e["token"][0] == 100
    hidden = z.copy()
    hidden[names.index("timestamp-timestamp"), lay.ts(5)] = np.nan            # a NaN in a column the rule masks fails the batch as well
    assert run_select_ts(lay, hidden, rows, pos=pos)["err"] & 1
    mask = np.zeros((3, lay.V))
    mask[0, : lay.tsb] = -np.inf                                              # no text token is left: [timestamp, timestamp] has no live column
    dead = run_select_ts(lay, z, rows, pos=pos, mask=mask)
    assert dead["err"] & 1
    fin = [0] * len(rows)
    fin[0] = 1
    assert run_select_ts(lay, bad, rows, pos=pos, finished=fin)["err"] == 0, "a finished row's logits decide nothing"
    full = [row + [0] * (MAXPOS - len(row)) for row in rows]
    end = run_select_ts(lay, z, full, pos=MAXPOS - 1)
    assert end["err"] & 4 and end["pos"] == MAXPOS - 1, "the position left the buffer: nothing written, not advanced"


def test_select_ts_alone_equals_batched_bit_for_bit():
    lay = LAYOUTS["V522"]
    z, rows, names, ties = steady_script(lay, seed=2)
    z, rows = z[5:10], rows[5:10]
    pos = P + 4
    both = run_select_ts(lay, z, rows, pos=pos)
    for b in range(5):
        one = run_select_ts(lay, z[b: b + 1], rows[b: b + 1], pos=pos)
        assert one["token"][0] == both["token"][b]
        assert one["margin"][:1].tobytes() == both["margin"][b: b + 1].tobytes() and one["gap"][:1].tobytes() == both["gap"][b: b + 1].tobytes()


def test_select_ts_refuses_bad_arguments():
    lay = LAYOUTS["V9"]
    z = np.zeros((1, 9), dtype=np.float32)
    for what in (lambda x: setattr(x, "ts_begin", 0), lambda x: setattr(x, "ts_begin", 9), lambda x: setattr(x, "no_ts", 9),
                 lambda x: setattr(x, "begin_index", 0), lambda x: setattr(x, "begin_index", MAXPOS), lambda x: setattr(x, "max_initial", -2),
                 lambda x: setattr(x, "ts_gap", 0), lambda x: setattr(x, "ld_gap", MAXPOS - 2), lambda x: setattr(x.base, "V", 1)):
        assert run_select_ts(lay, z, [[0, 0, 0]], pos=2, mutate=what) != 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the command line
@functools.lru_cache(maxsize=None)
def fixture():
    return SR.load_fixture(GOLDEN)


def test_command_line_segments_json(tmp_path, capsys):
    """--segments_json on synthetic weights with two short wavs: the schema, the CSV rows of the same run, both refusals, and a run without
    the flag that writes what it wrote before any timestamps run"""
    import wave
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as TR
    gold, geo, sd, spec, _ = fixture()
    wav_dir = tmp_path / "Audios"
    wav_dir.mkdir()
    for i, s in enumerate((0.4, 1.5)):
        with wave.open(str(wav_dir / f"f{i}.wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(np.round(synth_wave(70 + i, int(16000 * s)) * 32767.0).astype("<i2").tobytes())
    Cfg._REGISTRY["tiny-whisper-dec-segments"] = geo
    try:
        common = ["--ssl_type", "tiny-whisper-dec-segments", "--wav_dir", str(wav_dir), "--synthetic_weights", "--seed", "7", "--mode", "f16x"]
        before = tmp_path / "before.csv"
        assert TR.run(common + ["--out_csv", str(before)], spec=spec) == 0
        seg_csv, seg_json = tmp_path / "seg.csv", tmp_path / "seg.json"
        assert TR.run(common + ["--out_csv", str(seg_csv), "--segments_json", str(seg_json)], spec=spec) == 0
        after = tmp_path / "after.csv"
        assert TR.run(common + ["--out_csv", str(after)], spec=spec) == 0
        for extra, flag in ((["--times_json", str(tmp_path / "t.json")], "--times_json"), (["--num_beams", "2"], "--num_beams")):
            capsys.readouterr()
            with pytest.raises(SystemExit):
                TR.run(common + ["--out_csv", str(tmp_path / "x.csv"), "--segments_json", str(seg_json)] + extra, spec=spec)
            err = capsys.readouterr().err
            assert "--segments_json" in err and flag in err
    finally:
        Cfg._REGISTRY.pop("tiny-whisper-dec-segments")
    assert open(before, "rb").read() == open(after, "rb").read()
    table = TR.read_table(str(seg_csv))
    entries = json.load(open(seg_json))
    assert sorted(table) == sorted(entries) == ["f0.wav", "f1.wav"]
    for name, e in entries.items():
        assert sorted(e) == ["next_seek_s", "segments", "text"] and isinstance(e["next_seek_s"], float) and 0.0 <= e["next_seek_s"] <= 30.0
        assert table[name] == (e["text"] or "nan") and all(w.isdigit() and int(w) < spec.timestamp_begin for w in e["text"].split())
        assert len(e["segments"]) >= 1
        for a, b, text in e["segments"]:
            assert isinstance(a, float) and isinstance(b, float) and 0.0 <= a <= b <= 30.0 and isinstance(text, str)
            assert all(w.isdigit() and int(w) < spec.timestamp_begin for w in text.split())


# ---------------------------------------------------------------------------------------------------------------- the engine
# E = worst |device - HF| over the fixture's decided logit rows through the teacher-forced path (profiles/whisper_segments.txt)
@functools.lru_cache(maxsize=None)
def seg_decoder(mode):
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = fixture()
    return WhisperDecoder(geo, sd, DEV, mode, spec)


@functools.lru_cache(maxsize=None)
def measured_E(mode):
    gold, geo, sd, spec, enc = fixture()
    dec = seg_decoder(mode)
    seq, keep = gold["sequences"], gold["decided"]
    ref = np.zeros(keep.shape + (geo.decoder_vocab_size,))
    ref[keep] = gold["logits"].astype(np.float64)
    worst = 0.0
    for b in range(seq.shape[0]):
        n = int(np.nonzero(keep[b])[0].max()) + 2                             # up to the token its last decided row emits
        got = teacher_forced_device(dec, enc[b], seq[b, :n], spec)
        worst = max(worst, float(np.abs(got[keep[b, :n]] - ref[b][keep[b]]).max()))
    return worst


def hf_expected(gold, spec, lengths):
    """per utterance (ids up to and excluding eos, segments, next_seek) of HF's recorded sequences"""
    from interspeech_ser_amd.transcribe import window_frames
    out = []
    for b, row in enumerate(gold["sequences"]):
        gen = row[P:].tolist()
        body = gen[: gen.index(spec.eos_token_id)] if spec.eos_token_id in gen else gen
        out.append((body,) + SR.segments_of(body, spec.timestamp_begin, window_frames(lengths[b])))
    return out


LENGTHS = [480000, 200000, 16000 * 3]


@pytest.mark.parametrize("mode", ["f16x", "fp32x"])
def test_engine_equals_hf_where_the_margins_allow(mode):
    """4 E < the fixture's smallest margin and smallest ts_gap: no decision of the device can differ from HF's, so sequences, segments and
    next_seek equal HF's for every item, alone and batched"""
    gold, geo, sd, spec, enc = fixture()
    E = measured_E(mode)
    margin, gap, g = float(gold["min_margin"]), float(gold["min_gap"]), float(gold["g"])
    print(f"SEGHF {mode}: E {E:.3e}, g {g:.3e}, min margin {margin:.3e}, min ts_gap {gap:.3e}, 4 E / min {4 * E / min(margin, gap):.4f}")
    assert 4 * E < min(margin, gap), (E, margin, gap)
    dec = seg_decoder(mode)
    want = hf_expected(gold, spec, LENGTHS)
    B = len(want)
    runs = [(dec.generate(enc_dev(enc, slice(None)), B, timestamps=True, lengths=LENGTHS), list(range(B)))]
    runs += [(dec.generate(enc_dev(enc, slice(b, b + 1)), 1, timestamps=True, lengths=LENGTHS[b: b + 1]), [b]) for b in range(B)]
    for res, which in runs:
        assert not res.failed and res.segments is not None
        for i, b in enumerate(which):
            body, segs, seek = want[b]
            n = res.sequences.shape[1]
            assert res.sequences[i].tolist() == gold["sequences"][b, :n].tolist() and (gold["sequences"][b, n:] == spec.pad_token_id).all()
            assert int(res.languages[i]) == int(gold["languages"][b])
            assert res.lists[i] == body and res.segments[i] == segs and int(res.next_seek[i]) == seek
            dec_pos = np.nonzero(gold["decided"][b])[0]
            assert np.isfinite(res.margins[i, dec_pos]).all() and (res.margins[i, dec_pos] >= margin - 2 * E).all()
            gaps = res.ts_gaps[i, dec_pos]
            assert (gaps[np.isfinite(gaps)] >= gap - 2 * E - 1e-9).all() and np.isinf(res.ts_gaps[i, : P - 1]).all()
    assert any(len(s) >= 2 for _, s, _ in want) and len({k for _, _, k in want}) >= 2, "closed segments and different seek advances"


def test_engine_bf16_is_the_rule_on_its_own_logits():
    """bf16 is not pinned to HF: the numpy rule, fed the device's own kept logits, reproduces the device's tokens, margins and gaps"""
    gold, geo, sd, spec, enc = fixture()
    dec = seg_decoder("bf16")
    B, V = enc.shape[0], geo.decoder_vocab_size
    res = dec.generate(enc_dev(enc, slice(None)), B, timestamps=True, keep_logits=True)
    assert not res.failed and res.step_logits is not None and res.step_logits.shape[1:] == (B, V)
    logits = res.step_logits.cpu().numpy()
    m = R.masks(spec, V)
    checked = 0
    for b in range(B):
        for s in range(logits.shape[0]):
            p = P - 1 + s
            if p + 1 >= res.sequences.shape[1]:
                break
            x, tok, _, gp, _, _ = SR.rule(logits[s, b].astype(np.float64), m[1 if s == 0 else 0], res.sequences[b, P: p + 1], spec.timestamp_begin,
                                          spec.no_timestamps_token_id, spec.eos_token_id, spec.max_initial_timestamp_index)
            assert gp > gap_bound(V, np.abs(logits[s, b]).max(), np.log(V)) * 4, "the device's own sum rule was decided by rounding"
            assert tok == int(res.sequences[b, p + 1]), (b, p)
            top = np.sort(x)[-2:].astype(np.float32)
            assert res.margins[b, p] == np.float32(top[1] - top[0])
            if np.isfinite(gp):
                assert abs(res.ts_gaps[b, p] - gp) <= gap_bound(V, np.abs(logits[s, b]).max(), gp, np.log(V))
            else:
                assert np.isinf(res.ts_gaps[b, p])
            checked += 1
            if tok == spec.eos_token_id:
                break
    assert checked >= 3 * B
    print(f"SEGBF16: {checked} steps reproduced; rows {[l for l in res.lists]}")


def test_default_path_after_a_timestamps_run_and_refusals():
    """the default plan of the existing decoder fixture: its command list and its ids are what they were, after a timestamps run on the same
    decoder and slot"""
    from interspeech_ser_amd.engine import WhisperDecoder
    gold, geo, sd, spec, enc = R.load_fixture(GOLDEN)
    dec = WhisperDecoder(geo, sd, DEV, "f16x", spec)                         # its own: the plan cache of a shared decoder may drop a plan
    first = dec.generate(enc_dev(enc, slice(None)), 3)
    pl = dec._plan(3, 0)
    snap = lambda: C.string_at(C.addressof(pl["tape"].cmds), pl["tape"].n * C.sizeof(type(pl["tape"].cmds[0])))
    tape = snap()
    ts = dec.generate(enc_dev(enc, slice(None)), 3, timestamps=True)
    assert ts.segments is not None and len(ts.segments) == 3 and ts.sequences[:, :3].tolist() == [[spec.decoder_start_token_id, int(l), spec.task_id] for l in ts.languages]
    assert (ts.sequences[:, 3] >= spec.timestamp_begin).all(), "the first generated token of a timestamps run is a timestamp"
    res = dec.generate(enc_dev(enc, slice(None)), 3)
    assert dec._plan(3, 0) is pl and snap() == tape
    assert np.array_equal(res.sequences, gold["a_sequences"]) and np.array_equal(res.sequences, first.sequences)
    assert res.margins.tobytes() == first.margins.tobytes() and res.segments is None and res.ts_gaps is None
    with pytest.raises(ValueError, match="timestamps=True with token_times"):
        dec.generate(enc_dev(enc, slice(None)), 3, timestamps=True, token_times=True, lengths=[16000] * 3)
    with pytest.raises(ValueError, match="timestamps=True with num_beams"):
        dec.generate(enc_dev(enc, slice(None)), 3, timestamps=True, num_beams=2)


def test_transcriber_segments_and_per_file_retry(capsys):
    """waveforms to segments through WhisperTranscriber: the batch equals the per-file runs, and a file that sets the error bit fails alone
    through batchloop, as on the greedy path"""
    from interspeech_ser_amd import config as Cfg
    from interspeech_ser_amd import transcribe as TR
    from interspeech_ser_amd.engine import WhisperEncoder
    from interspeech_ser_amd.weights import synthetic_state_dict
    gold, geo, sd, spec, _ = fixture()
    enc = WhisperEncoder(geo, synthetic_state_dict(Cfg.TINY_WHISPER, 14), DEV, "f16x")
    waves = [synth_wave(3000, 16000), synth_wave(3013, 100000)]
    tr = TR.WhisperTranscriber(enc, seg_decoder("f16x"), spec)
    both = tr.transcribe(waves, timestamps=True)
    segs, seeks = list(tr.segments), list(tr.next_seek)
    assert all(ids is not None and all(t < spec.timestamp_begin for t in ids) for ids in both) and all(s for s in segs)
    assert all(0 <= k <= TR.window_frames(len(w)) for k, w in zip(seeks, waves))
    for i, w in enumerate(waves):
        assert tr.transcribe([w], timestamps=True) == [both[i]] and tr.segments == [segs[i]] and tr.next_seek == [seeks[i]]
    bad = waves[0][:15000]
    forward = enc.forward

    def poisoned(wav, lengths, **kw):
        hs = forward(wav, lengths, **kw)
        for i, n in enumerate(lengths):
            if n == len(bad):
                hs.states[-1].view(len(lengths), -1, geo.hidden)[i, 7, 3] = float("nan")
        return hs
    enc.forward = poisoned
    try:
        assert tr.transcribe([bad, waves[1]], ["bad.wav", "good.wav"], timestamps=True) == [None, both[1]] and tr.failed == ["bad.wav"]
        assert tr.segments == [None, segs[1]] and tr.next_seek == [None, seeks[1]]
    finally:
        enc.forward = forward
    assert "Failed to process bad.wav: decoder error word" in capsys.readouterr().out
