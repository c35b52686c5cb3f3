"""GPU: the O(B) tables of every plan and every head (-m gpu).

A forward over a new ragged batch puts a few integer tables on the device (sample offsets, frame offsets per level, halo / tap base
rows) and builds the O(rows) row tables from them with ser_ragged_index.  Per waveform encoder, ``_plan`` runs over a grow / shrink /
repeat sequence of batches on two interleaved slots, lengths at the family's minimum among them; after each plan every table the plan
exposes equals what numpy computes here from the lengths and the geometry functions, the other slot's tables are untouched, and a
repeated plan is the same dict over the same addresses.  The heads run two forwards of different B on one slot, the offsets uploaded by
the head itself, bit-equal to a freshly built head's.  Only plan keys and public arguments are read.
"""
import numpy as np
import pytest
import torch

import fusion3_ref as R3
import fusion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t, n=None):
    a = t.detach().cpu().numpy()
    return a if n is None else a[:n]


def _cum(v):
    return np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))])


def _ragged(row_offs, base, step, mult, div):
    """ser_ragged_index in numpy: out[m] = (base[b] + step (m - row_offs[b])) mult / div, b the utterance that owns row m"""
    row_offs, base = np.asarray(row_offs, dtype=np.int64), np.asarray(base, dtype=np.int64)
    m = np.arange(row_offs[-1], dtype=np.int64)
    b = np.searchsorted(row_offs[1:], m, side="right")
    return ((base[b] + step * (m - row_offs[b])) * mult // div).astype(np.int32)


def _halo(offs, half, width, taps=None):
    """the zero-halo'd layout: starts[b] = half (b + 1) + offs[b]; (row map, tap offsets per entry of taps (default: half))"""
    offs = np.asarray(offs, dtype=np.int64)
    starts = half * (np.arange(len(offs) - 1) + 1) + offs[:-1]
    return _ragged(offs, starts, 1, 1, 1), [_ragged(offs, starts - t, 1, width, 8) for t in (taps or (half,))], starts


def _common(pl, lengths, offs, Tmax):
    """the keys every arena plan has: {name: (got, want)}"""
    B, M = len(lengths), int(offs[-1])
    assert pl["lengths"] == tuple(lengths) and pl["frame_offs_host"] == [int(v) for v in offs]
    assert (int(pl["B"]), int(pl["M"]), int(pl["Tmax"])) == (B, M, Tmax)
    assert (pl["sizes"]["B"], pl["sizes"]["M"], pl["sizes"]["Tmax"]) == (B, M, Tmax)
    assert pl["sample_offs"].dtype == torch.int64 and pl["frame_offs"].dtype == torch.int32
    return {"sample_offs": (_np(pl["sample_offs"], B + 1), _cum(lengths)), "frame_offs": (_np(pl["frame_offs"], B + 1), offs)}


def _speech_tables(enc, pl, lengths):
    geo = enc.geo
    nl, C0, D, half = len(geo.conv_dim), geo.conv_dim[0], geo.hidden, geo.pos_conv_kernel // 2
    chains = [geo.frame_chain(n) for n in lengths]
    offs = [_cum([c[i] for c in chains]) for i in range(nl)]
    t = _common(pl, lengths, offs[-1], max(c[-1] for c in chains))
    assert [int(r) for r in pl["rows"]] == [int(o[-1]) for o in offs]
    assert all(pl["sizes"][f"rows{i}"] == int(o[-1]) for i, o in enumerate(offs))
    t["frame_offs0"] = (_np(pl["frame_offs0"], len(lengths) + 1), offs[0])
    for i in range(1, nl):
        t[f"conv_rowoff{i}"] = (_np(pl["conv_rowoff"][i - 1], offs[i][-1]), _ragged(offs[i], offs[i - 1][:-1], geo.conv_stride[i], C0, 8))
    rowmap, (pos,), _ = _halo(offs[-1], half, D)
    t["halo_rowmap"], t["pos_rowoff"] = (_np(pl["halo_rowmap"], len(rowmap)), rowmap), (_np(pl["pos_rowoff"], len(pos)), pos)
    return t


def _whisper_tables(enc, pl, lengths):
    B, T2 = len(lengths), enc.geo.max_source_positions
    offs = np.arange(B + 1) * T2
    assert pl["lengths"] == tuple(lengths) and pl["frame_offs_host"] == offs.tolist() and (int(pl["B"]), int(pl["M"])) == (B, B * T2)
    return {"sample_offs": (_np(pl["sample_offs"], B + 1), _cum(lengths)), "frame_offs": (_np(pl["frame_offs"], B + 1), offs)}


def _prosody_tables(enc, pl, lengths):
    from interspeech_ser_amd.frontend import prosody_frames
    T = [prosody_frames(n) for n in lengths]
    offs = _cum(T)
    t = _common(pl, lengths, offs, max(T))
    rowmap, (fc1,), _ = _halo(offs, enc.spec.kernel // 2, enc.spec.hidden)
    t["halo_rowmap"], t["fc1_rowoff"] = (_np(pl["halo_rowmap"], len(rowmap)), rowmap), (_np(pl["fc1_rowoff"], len(fc1)), fc1)
    return t


def _codec_tables(enc, pl, lengths):
    from interspeech_ser_amd import prosody as P
    sp, B = enc.spec, len(lengths)
    t = {"prosody " + k: v for k, v in _prosody_tables(enc.prosody, pl["ppl"], lengths).items()}
    lens = np.array([sp.level_lengths(n) for n in lengths], dtype=np.int64)
    offs = [_cum(lens[:, l]) for l in range(lens.shape[1])]
    assert pl["lengths"] == tuple(lengths) and int(pl["M"]) == int(offs[-1][-1]) == int(pl["ppl"]["M"])
    for l, lv in enumerate(pl["lv"]):
        assert (pl["sizes"][f"M{l}"], pl["sizes"][f"R{l}"]) == (int(offs[l][-1]), int(lens[:, l].max())) == (int(pl["Ms"][l]), int(pl["Rs"][l]))
        assert lv["offs"].dtype == torch.int32 and lv["offs64"].dtype == torch.int64
        t[f"lv{l} offs"], t[f"lv{l} offs64"] = (_np(lv["offs"], B + 1), offs[l]), (_np(lv["offs64"], B + 1), offs[l])
        if "rowmap" not in lv:
            continue
        C, n = sp.channels[l], int(offs[l][-1])
        last = l == len(sp.strides)
        rowmap, taps, starts = _halo(offs[l], P.WIDE_HALO, C, taps=(1,) if last else (3, 9, 27))
        t[f"lv{l} rowmap"] = (_np(lv["rowmap"], n), rowmap)
        if last:
            t[f"lv{l} rowoff_k3"] = (_np(lv["rowoff_k3"], n), taps[0])
        else:
            for j in range(3):
                t[f"lv{l} rowoff{j}"] = (_np(lv["rowoff"][j], n), taps[j])
            t[f"lv{l} down_rowoff"] = (_np(lv["down_rowoff"], offs[l + 1][-1]),
                                       _ragged(offs[l + 1], starts - enc.levels[l]["pad"], sp.strides[l], C, 8))
    ts = sp.timbre
    rowmap, (fc1,), _ = _halo(offs[-1], ts.kernel // 2, ts.hidden)
    t["halo_rowmap"], t["fc1_rowoff"] = (_np(pl["halo_rowmap"], len(rowmap)), rowmap), (_np(pl["fc1_rowoff"], len(fc1)), fc1)
    return t


def _w2vbert_tables(enc, pl, lengths):
    from interspeech_ser_amd.frontend import w2vbert_mel_frames
    Fr = [w2vbert_mel_frames(n) for n in lengths]
    T = [f // enc.geo.fbank_stride for f in Fr]
    t = _common(pl, lengths, _cum(T), max(T))
    assert int(pl["Fmax"]) == pl["sizes"]["Fmax"] == max(Fr) and int(pl["MH"]) == pl["sizes"]["MH"] == sum(T) * enc.geo.heads
    t["mel_offs"] = (_np(pl["mel_offs"], len(lengths) + 1), _cum(Fr))
    return t


def _speech(name):
    def build():
        from interspeech_ser_amd import config as C
        from interspeech_ser_amd.engine import build_encoder
        from interspeech_ser_amd.weights import synthetic_state_dict
        geo = getattr(C, name)
        return build_encoder(geo, synthetic_state_dict(geo, 5), DEV, "f16x")
    return build


def _prosody():
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.engine import ProsodyEncoder
    return ProsodyEncoder(P.synthetic_state_dict(seed=11), DEV, "f16x")


def _codec():
    from interspeech_ser_amd import prosody as P
    from interspeech_ser_amd.engine import SpeakerProsodyEncoder
    dec = P.synthetic_state_dict(seed=11)
    dec.update(P.synthetic_timbre_state_dict(seed=13))
    return SpeakerProsodyEncoder(dec, P.synthetic_codec_state_dict(), DEV, "f16x")


# per slot: B = 2; B = 3 with longer utterances (the arena grows); B = 1 (it shrinks); the B = 2 lengths again.  400 samples is the conv
# stack's and the prosody streams' minimum, 560 w2v-BERT's; Whisper takes any length up to its 30 s window
CONV_SEQ = (((400, 3000), (2000, 401)), ((5000, 400, 9000), (8000, 7000, 799)), ((1200,), (400,)), ((400, 3000), (2000, 401)))
W2V_SEQ = (((560, 3000), (2000, 719)), ((5000, 560, 9000), (8000, 7000, 880)), ((1200,), (560,)), ((560, 3000), (2000, 719)))
WHISPER_SEQ = (((1, 3000), (480000, 400)), ((5000, 400, 480000), (8000, 7000, 799)), ((1200,), (480000,)), ((1, 3000), (480000, 400)))
HOSTS = {"wavlm-ln-stem": (_speech("TINY_WAVLM"), _speech_tables, CONV_SEQ),
         "wavlm-base-gn-stem": (_speech("TINY_WAVLM_BASE"), _speech_tables, CONV_SEQ),
         "data2vec-audio": (_speech("TINY_DATA2VEC_AUDIO"), _speech_tables, CONV_SEQ),
         "whisper": (_speech("TINY_WHISPER"), _whisper_tables, WHISPER_SEQ),
         "prosody": (_prosody, _prosody_tables, CONV_SEQ),
         "speaker-prosody": (_codec, _codec_tables, CONV_SEQ),
         "w2v-bert": (_speech("TINY_W2V_BERT"), _w2vbert_tables, W2V_SEQ)}


def _check(tables, what):
    for name, (got, want) in tables.items():
        assert got.shape == np.shape(want) and np.array_equal(got, want), f"{what}: table {name}"


def _tensors(pl, out=None, path="pl"):
    """every tensor reachable from the plan keys the tables are read through: {path: tensor}"""
    out = {} if out is None else out
    keys = ("sample_offs", "frame_offs", "frame_offs0", "mel_offs", "halo_rowmap", "pos_rowoff", "fc1_rowoff", "conv_rowoff", "lv", "ppl",
            "offs", "offs64", "rowmap", "rowoff", "down_rowoff", "rowoff_k3")
    for k in keys:
        v = pl.get(k)
        if torch.is_tensor(v):
            out[f"{path}.{k}"] = v
        elif isinstance(v, dict):
            _tensors(v, out, f"{path}.{k}")
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                _tensors({k: e} if torch.is_tensor(e) else e, out, f"{path}.{k}[{i}]")
    return out


@pytest.mark.parametrize("host", list(HOSTS))
def test_plan_tables_over_grow_shrink_repeat_on_two_slots(built_library, host):
    build, tables, seq = HOSTS[host]
    enc = build()
    first_ptrs, owners = {}, []                                # per owning buffer set: the addresses of its first plan
    for step, per_slot in enumerate(seq):
        plans = []
        for slot, lengths in enumerate(per_slot):
            pl = enc._plan(list(lengths), slot)
            torch.cuda.synchronize()
            what = f"{host}, step {step}, slot {slot}, lengths {lengths}"
            _check(tables(enc, pl, lengths), what)
            plans.append((pl, lengths, what))
            if slot == 1:                                      # slot 0's tables as they were before slot 1 planned
                _check(tables(enc, *plans[0][:2]), plans[0][2] + " after slot 1's plan")
            # the hit path: the same dict, over the addresses of the first plan laid out in this buffer set
            ptrs = {k: t.data_ptr() for k, t in _tensors(pl).items()}
            again = enc._plan(list(lengths), slot)
            assert again is pl and {k: t.data_ptr() for k, t in _tensors(again).items()} == ptrs, what
            owner = enc._arenas[slot] if hasattr(enc, "_arenas") else pl
            owners.append(owner)                               # kept alive: an id is not re-used
            assert first_ptrs.setdefault(id(owner), ptrs) == ptrs, what + ": a table moved inside one arena"
    if hasattr(enc, "_arenas"):
        assert len({id(o) for o in owners}) == 4               # per slot: the first arena and the one grown for B = 3, re-used after


# --------------------------------------------------------------------------------------------------------------------- heads
def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _states(geo, offs, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((geo.num_layers + 1, offs[-1], geo.hidden), generator=g).to(DEV)


@pytest.fixture(scope="module")
def wavlm(built_library):
    return _speech("TINY_WAVLM")()


HEAD_OFFS = ([0, 7, 40, 41], [0, 130, 133, 134, 150, 163])     # B = 3, then B = 5 with more rows: the head's buffers grow


@pytest.mark.parametrize("kind", ["pool", "classifier"])
def test_encoder_heads_upload_their_offsets(wavlm, kind):
    """PoolHead / ClassifierHead on hidden states that come without offsets on the device: two forwards of different B on one slot."""
    from interspeech_ser_amd.baseline import synthetic_head_state_dicts
    from interspeech_ser_amd.config import ClassifierSpec
    from interspeech_ser_amd.engine import ClassifierHead, HiddenStates, PoolHead
    geo = wavlm.geo
    D, L1 = geo.hidden, geo.num_layers + 1

    def make():
        if kind == "pool":
            return PoolHead(wavlm, *synthetic_head_state_dicts(D, 96, 8, seed=5))
        g = torch.Generator().manual_seed(9)
        sd = {"projector.weight": torch.randn((32, D), generator=g) * 0.1, "projector.bias": torch.randn(32, generator=g) * 0.1,
              "classifier.weight": torch.randn((4, 32), generator=g) * 0.1, "classifier.bias": torch.randn(4, generator=g) * 0.1,
              "layer_weights": torch.randn(L1, generator=g)}
        return ClassifierHead(wavlm, sd, ClassifierSpec(True, 32, 4, ("a", "b", "c", "d")))
    head = make()
    for k, offs in enumerate(HEAD_OFFS + HEAD_OFFS[:1]):
        hs = HiddenStates(_states(geo, offs, 20 + k), offs)
        assert hs.frame_offs_dev is None
        got = _bits(head.forward(hs))
        want = _bits(make().forward(hs))
        assert got.shape[0] == len(offs) - 1 and np.array_equal(got, want), (kind, k)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _offs(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _scattered(xs, starts, rows):
    """the utterances' rows at ``starts`` inside one [rows, D] device matrix (NaN elsewhere): what a RowSource reads"""
    t = torch.full((rows, xs[0].shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    for x, s in zip(xs, starts):
        t[s:s + len(x)] = _dev(x)
    return t


def test_fusion_head_two_batches_and_a_row_source(built_library):
    from interspeech_ser_amd.engine import FusionHead, RowSource
    cases = []
    for seed, (l1, l2, starts) in enumerate((((1, 37, 12), (5, 16, 9), (40, 0, 20)), ((9, 3, 20, 2, 41), (4, 8, 3, 30, 6), (10, 60, 0, 20, 70)))):
        sd, xs1, _ = R.seeded_case(128, 64, l1, 3 + seed, h=64)
        xs2 = [np.random.default_rng(40 + 10 * seed + i).standard_normal((t, 64)).astype(np.float32) for i, t in enumerate(l2)]
        cases.append((sd, _dev(np.concatenate(xs1)), _offs(l1), RowSource(_scattered(xs2, starts, 110), starts), _dev(np.concatenate(xs2)), _offs(l2)))
    sd = cases[0][0]
    head = FusionHead(sd, 128, 64, DEV, "f16x")
    for k in (0, 1, 0):
        _, x1, o1, src2, x2, o2 = cases[k]
        got = _bits(head.forward(x1, o1, src2, o2))
        assert head.status() == (0, 0)
        fresh = FusionHead(sd, 128, 64, DEV, "f16x")
        assert np.array_equal(got, _bits(fresh.forward(x1, o1, src2, o2))), k
        assert np.array_equal(got, _bits(fresh.forward(x1, o1, x2, o2))), k     # and to the rows handed in as a tensor


def test_trimodal_head_two_batches(built_library):
    from interspeech_ser_amd.engine import TrimodalHead
    dims = (64, 128, 64)
    cases = [R3.seeded_case(dims, lengths, 4 + k, h=64) for k, lengths in
             enumerate((((1, 37, 12), (5, 16, 9), (7, 2, 33)), ((9, 3, 20, 2), (4, 8, 3, 30), (6, 6, 1, 12))))]
    sd = cases[0][0]
    head = TrimodalHead(sd, *dims, DEV, "f16x")
    for k in (0, 1, 0):
        args = []
        for xs in cases[k][1:]:
            args += [_dev(np.concatenate(xs)), _offs([len(x) for x in xs])]
        got = _bits(head.forward(*args))
        assert head.status() == (0, 0)
        assert np.array_equal(got, _bits(TrimodalHead(sd, *dims, DEV, "f16x").forward(*args))), k
