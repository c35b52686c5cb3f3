"""GPU: ser_select_rows_v (csrc/rowops.hip), the device heads' ragged gather, against bit patterns.

Every expectation is exact: the fp32 output is the selected source value (or numpy's float32 (((a + b) + c) + d) / 4), the operand planes
are what ser_pack_rows_flagged stores for the same fp32 rows handed to it contiguously and the host's restated split, and every byte a
launch must not touch holds its planted garbage afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, FP32X, FP16X = 1, 2, 4
GARBAGE = -3                                  # int16 0xfffd: a NaN in bf16 and in fp16
F16_MAX = 65504.0
SRC_ROWS = 200
SRC_OFFS = (90, 0, 40, 7)                     # not ascending


def _counts():
    from interspeech_ser_amd import _lib
    R = _lib.SELECT_ROWS_TILE
    return (1, 5, R + 1, 33)                  # a single row, inside one tile, one row into a second tile, the longest (max_rows = 33)


def stream():
    return torch.cuda.current_stream().cuda_stream


def n_planes(mode):
    return 2 if mode in (FP32X, FP16X) else 1


def _sources(D, ld, seed, n=4):
    """n fp32 [SRC_ROWS, D] matrices at row pitch ld on the device (NaN in the padding columns) and their host copies"""
    rng = np.random.default_rng(seed)
    host = [(rng.standard_normal((SRC_ROWS, D)) * (1.0 + k)).astype(np.float32) for k in range(n)]
    dev = []
    for h in host:
        t = torch.full((SRC_ROWS, ld), float("nan"), dtype=torch.float32, device=DEV)
        t[:, :D] = torch.from_numpy(h).to(DEV)
        dev.append(t)
    return host, dev


def _offs(counts):
    return [0] + [int(v) for v in np.cumsum(counts)]


def _gathered(host, counts, src_offs=SRC_OFFS):
    return np.concatenate([host[s:s + c] for s, c in zip(src_offs, counts)])


def select(srcs, ld, src_offs, counts, D, mode, want_act=True, want_f32=True, flag=None, spare=3, pad=8):
    """one launch into garbage-filled buffers of `spare` extra rows and `pad` extra columns -> (planes int16 [P, M + spare, D + pad] or None,
    fp32 [M + spare, D + pad] or None), on the host"""
    from interspeech_ser_amd import _lib
    offs = _offs(counts)
    M, B = offs[-1], len(counts)
    so = torch.tensor(src_offs, dtype=torch.int32, device=DEV)
    do = torch.tensor(offs, dtype=torch.int32, device=DEV)
    act = torch.full((n_planes(mode), M + spare, D + pad), GARBAGE, dtype=torch.int16, device=DEV) if want_act else None
    f32 = torch.full((M + spare, D + pad), float("nan"), dtype=torch.float32, device=DEV) if want_f32 else None
    a = _lib.SelectRowsArgs()
    for k, s in enumerate(srcs):
        a.src[k] = s.data_ptr()
    a.ld_src, a.src_offs, a.dst_offs = ld, so.data_ptr(), do.data_ptr()
    if act is not None:
        a.out_act, a.ldo_act, a.out_plane_stride = act.data_ptr(), D + pad, (M + spare) * (D + pad)
    if f32 is not None:
        a.out_f32, a.ldo_f32 = f32.data_ptr(), D + pad
    a.range_flag = None if flag is None else flag.data_ptr()
    a.n_src, a.B, a.D, a.max_rows, a.mode = len(srcs), B, D, max(counts), mode
    _lib.check(_lib.lib.ser_select_rows_v(C.byref(a), stream()), "ser_select_rows_v")
    torch.cuda.synchronize()
    return (None if act is None else act.cpu().numpy()), (None if f32 is None else f32.cpu().numpy())


def packed_planes(x: np.ndarray, mode: int) -> np.ndarray:
    """what ser_pack_rows_flagged stores for the contiguous fp32 rows x: int16 [P, M, D]"""
    from interspeech_ser_amd import _lib
    M, D = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.full((n_planes(mode), M, D), GARBAGE, dtype=torch.int16, device=DEV)
    _lib.check(_lib.lib.ser_pack_rows_flagged(xd.data_ptr(), D, 1, M, D, 0, out.data_ptr(), D, M * D, mode, None, stream()), "ser_pack_rows_flagged")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def host_split_f16(x: np.ndarray) -> np.ndarray:
    """hi = fp16(x), lo = fp16(x - hi) (values inside the fp16 range)"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    hi = t.half()
    lo = (t - hi.float()).half()
    return torch.stack([hi.view(torch.int16), lo.view(torch.int16)]).numpy()


SHAPES = [(64, 64), (128, 136)]               # (D, row pitch of the sources)


@pytest.mark.parametrize("D,ld", SHAPES, ids=["D64", "D128-pitch136"])
@pytest.mark.parametrize("n_src", [1, 4])
def test_fp32_output_is_the_selected_value(built_library, D, ld, n_src):
    counts = _counts()
    host, dev = _sources(D, ld, 11)
    _, f32 = select(dev[:n_src], ld, SRC_OFFS, counts, D, BF16, want_act=False)
    M = sum(counts)
    if n_src == 1:
        want = _gathered(host[0], counts)
    else:
        a, b, c, d = (_gathered(h, counts) for h in host)
        want = (((a + b) + c) + d) / np.float32(4)
        assert want.dtype == np.float32
    assert np.array_equal(f32[:M, :D].view(np.uint32), want.view(np.uint32))
    assert np.isnan(f32[M:]).all() and np.isnan(f32[:, D:]).all()          # rows dst_offs[B] .. and the pitch columns: untouched


@pytest.mark.parametrize("D,ld", SHAPES, ids=["D64", "D128-pitch136"])
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X], ids=["bf16", "fp32x", "f16x"])
@pytest.mark.parametrize("n_src", [1, 4])
def test_operand_planes_equal_pack_rows(built_library, D, ld, mode, n_src):
    counts = _counts()
    host, dev = _sources(D, ld, 12)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    act, f32 = select(dev[:n_src], ld, SRC_OFFS, counts, D, mode, flag=flag)
    M = sum(counts)
    rows = np.ascontiguousarray(f32[:M, :D])
    assert np.array_equal(act[:, :M, :D], packed_planes(rows, mode))
    if mode == FP16X:
        assert np.array_equal(act[:, :M, :D], host_split_f16(rows))
    assert (act[:, M:] == GARBAGE).all() and (act[:, :, D:] == GARBAGE).all()   # every plane byte outside [M, D]
    assert np.isnan(f32[M:]).all() and np.isnan(f32[:, D:]).all()
    assert int(flag.item()) == 0
    only_act, none = select(dev[:n_src], ld, SRC_OFFS, counts, D, mode, want_f32=False)
    assert none is None and np.array_equal(only_act, act)                  # the fp32 output is optional; NULL range word


def test_range_word_sees_selected_rows_only(built_library):
    D, counts = 64, _counts()
    M = sum(counts)
    host, dev = _sources(D, D, 13, n=1)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    # directly behind utterance 0's single row (source row 91) and behind utterance 2's rows (its second tile's second row): never read
    dev[0][SRC_OFFS[0] + counts[0], 5] = 7.0e4
    dev[0][SRC_OFFS[2] + counts[2], 17] = 7.0e4
    dev[0][199, 0] = float("nan")
    act, _ = select(dev, D, SRC_OFFS, counts, D, FP16X, flag=flag)
    assert int(flag.item()) == 0
    clean, _ = select([torch.from_numpy(host[0]).to(DEV)], D, SRC_OFFS, counts, D, FP16X)
    assert np.array_equal(act, clean)
    dev[0][SRC_OFFS[2] + counts[2] - 1, 9] = 7.0e4                         # the last selected row of utterance 2 (its second tile)
    select(dev, D, SRC_OFFS, counts, D, FP16X, flag=flag)
    assert int(flag.item()) & 1
    flag.zero_()
    select(dev, D, SRC_OFFS, counts, D, BF16, flag=flag)                   # bf16 planes have fp32's range: no report
    assert int(flag.item()) == 0
    act, f32 = select(dev, D, SRC_OFFS, counts, D, FP16X, flag=None)       # NULL word: runs, stores the same rows
    assert f32[_offs(counts)[2] + counts[2] - 1, 9] == np.float32(7.0e4) and act.shape[1] == M + 3


@pytest.mark.parametrize("n_src", [1, 4])
def test_an_utterance_alone_equals_its_batched_rows(built_library, n_src):
    D, ld, counts = 128, 136, _counts()
    offs = _offs(counts)
    host, dev = _sources(D, ld, 14)
    act, f32 = select(dev[:n_src], ld, SRC_OFFS, counts, D, FP16X)
    for b, c in enumerate(counts):
        a1, f1 = select(dev[:n_src], ld, SRC_OFFS[b:b + 1], (c,), D, FP16X)
        assert np.array_equal(a1[:, :c, :D], act[:, offs[b]:offs[b + 1], :D]), b
        assert np.array_equal(f1[:c, :D].view(np.uint32), f32[offs[b]:offs[b + 1], :D].view(np.uint32)), b
