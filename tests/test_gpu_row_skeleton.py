"""-m gpu: the wave-per-row skeleton (csrc/row_common.h) at the widths where its chunk loop can go wrong, through the three entry points
that sit on every part of it: ser_layernorm_v (load, statistics, LayerNorm tail), ser_pos_ln_v (both forms: the in-place second pass and
the tail) and ser_row_center_v (its own chunk loop, the FP16M arm inside it).

A lane owns 4 consecutive columns of every 256-column chunk, so D = 4 is one lane of one chunk, 252 stops at the last lane of a chunk,
256 is a whole chunk, 260 one lane into the next, 2044 / 2048 the partial and the full eighth chunk.  One row is a block with three
idle waves; six rows are a full block of four waves and a half-empty one.  All pitches are wider than D and every output starts as
planted garbage: a column past D or a row past the last one that changes is a store out of the row.

Bounds.  fp32 outputs: 2e-5 absolute against float64 (the bound of test_layernorm and the text row kernels up to D = 2048).  Operand
planes: the host split of the kernel's own fp32 values, bit for bit.  Where no fp32 output exists the rules of the kernel's own test
hold: test_pos_ln_intermediate_form's error relative to max(1, max |ref|) -- 4e-3 bf16, 2e-5 two-plane, and for the single fp16 plane
(which that test does not run) half an ulp of 11 significand bits, 2^-11, on top of the 2e-5 --, and for ser_row_center the planes are
exact, x - shift[row] being one fp32 subtraction of two numbers the test holds.  The inputs are O(1) rows with a moderate mean: what is
pinned here is the indexing, not the conditioning (test_gpu_data2vec.py has the rows with a large mean)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import f16m_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, FP32X, FP16, FP16X, FP16M = 1, 2, 3, 4, 6
MODES = [BF16, FP32X, FP16, FP16X]
WIDTHS = [4, 252, 256, 260, 2044, 2048]
ROWS = [1, 6]
EXTRA = 2                                     # spare rows behind the last one
GARBAGE = -3                                  # int16 0xfffd: a NaN in bf16 and in fp16
F16_MAX = 65504.0


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def n_planes(mode):
    return 2 if mode in (FP32X, FP16X) else 1


def host_split(y: torch.Tensor, mode: int) -> torch.Tensor:
    """fp32 CPU tensor -> int16 [P, *y.shape]: the planes a kernel must store for the fp32 values y (RNE; fp16 planes saturate at 65504)"""
    if mode in (FP16, FP16X):
        hi = y.clamp(-F16_MAX, F16_MAX).half()
        lo = (y - hi.float()).clamp(-F16_MAX, F16_MAX).half()
    else:
        hi = y.to(torch.bfloat16)
        lo = (y - hi.float()).to(torch.bfloat16)
    return torch.stack([p.view(torch.int16) for p in [hi, lo][:n_planes(mode)]])


def planes_value(a: torch.Tensor, mode: int) -> torch.Tensor:
    """int16 [P, R, D] planes -> the float64 value they hold"""
    dt = torch.float16 if mode in (FP16, FP16X) else torch.bfloat16
    return a.view(dt).double().sum(0)


def garbage_planes(P, rows, ld):
    return torch.full((P, rows, ld), GARBAGE, dtype=torch.int16, device=DEV)


def garbage_f32(rows, ld):
    return torch.full((rows, ld), float("nan"), device=DEV)


def pitched(x: torch.Tensor, ld: int) -> torch.Tensor:
    """x [R, D] -> device [R, ld], NaN in the pitch columns: a load past D poisons its row"""
    out = torch.full((x.shape[0], ld), float("nan"))
    out[:, : x.shape[1]] = x
    return out.to(DEV)


def inputs(rows, D, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=gen) * 3 + 0.5
    res = torch.randn(rows, D, generator=gen) * 2 + 1.0
    g, b = 1.0 + 0.3 * torch.randn(D, generator=gen), 0.2 * torch.randn(D, generator=gen)
    return x, res, g, b


def only_garbage_outside(a: torch.Tensor, rows, D, written_rows=None) -> bool:
    """int16 planes [P, R, ld]: everything but [written rows, :D] still holds the planted pattern"""
    keep = torch.ones(a.shape[1:], dtype=torch.bool)
    keep[torch.arange(rows) if written_rows is None else written_rows.long(), :D] = False
    return bool((a[:, keep] == GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------------------ ser_layernorm_v
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_layernorm_widths(L, mode, D):
    """LayerNorm (with and without GELU), 1 and 6 rows: fp32 within 2e-5 of float64, planes the host split of it, nothing stored past D
    or past the last row; with only one of the two outputs asked for the other holds the same bytes."""
    P, ldx, ldof, ldoa = n_planes(mode), D + 4, D + 8, D + 12
    for rows in ROWS:
        x, _, g, b = inputs(rows, D, 100 * D + rows)
        xd, gd, bd = pitched(x, ldx), g.to(DEV), b.to(DEV)
        for gelu in (0, 1):
            ref = F.layer_norm(x.double(), (D,), g.double(), b.double(), 1e-5)
            ref = F.gelu(ref) if gelu else ref

            def launch(want_f32=True, want_act=True):
                of = garbage_f32(rows + EXTRA, ldof) if want_f32 else None
                oa = garbage_planes(P, rows + EXTRA, ldoa) if want_act else None
                flag = torch.zeros(1, dtype=torch.int32, device=DEV)
                a = L.LayerNormArgs()
                a.x, a.ldx, a.g, a.b, a.eps, a.gelu = xd.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), 1e-5, gelu
                a.out_f32, a.ldo_f32 = (of.data_ptr(), ldof) if want_f32 else (None, 0)
                a.out_act, a.ldo_act, a.out_plane_stride = (oa.data_ptr(), ldoa, (rows + EXTRA) * ldoa) if want_act else (None, 0, 0)
                a.mode, a.rows, a.D, a.range_flag = mode, rows, D, flag.data_ptr()
                L.check(L.lib.ser_layernorm_v(C.byref(a), stream()), "ser_layernorm_v")
                torch.cuda.synchronize()
                assert int(flag.item()) == 0
                return (None if of is None else of.cpu()), (None if oa is None else oa.cpu())

            f, a = launch()
            err = (f[:rows, :D].double() - ref).abs().max().item()
            print(f"ser_layernorm mode {mode} D {D} rows {rows} gelu {gelu}: fp32 error {err:.2e}")
            assert err < 2e-5
            assert bool(f[rows:].isnan().all()) and bool(f[:, D:].isnan().all())
            assert torch.equal(a[:, :rows, :D], host_split(f[:rows, :D], mode))
            assert only_garbage_outside(a, rows, D)
            f2, _ = launch(want_act=False)
            assert torch.equal(f2.view(torch.int32), f.view(torch.int32))
            _, a2 = launch(want_f32=False)
            assert torch.equal(a2, a)


# --------------------------------------------------------------------------------------------------------------------------- ser_pos_ln_v
def run_pos_ln(L, mode, rows, D, xd, ldx, oa, ldoa, *, rowmap=None, res=None, ldr=0, g=None, b=None, of=None, ldof=0):
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    last = res is not None
    a = L.PosLnArgs()
    a.x, a.ldx = xd.data_ptr(), ldx
    a.out_act, a.ldo_act, a.out_plane_stride = (None, 0, 0) if oa is None else (oa.data_ptr(), ldoa, oa.shape[1] * ldoa)
    a.out_rowmap = None if rowmap is None else rowmap.data_ptr()
    a.residual, a.ldr = (res.data_ptr(), ldr) if last else (None, 0)
    a.g, a.b = (g.data_ptr(), b.data_ptr()) if last else (None, None)
    a.out_f32, a.ldo_f32 = (of.data_ptr(), ldof) if last else (None, 0)
    a.eps_pos, a.eps, a.last, a.mode, a.rows, a.D = 1e-5, 1e-5, int(last), mode, rows, D
    a.range_flag = flag.data_ptr()
    L.check(L.lib.ser_pos_ln_v(C.byref(a), stream()), "ser_pos_ln_v")
    torch.cuda.synchronize()
    assert int(flag.item()) == 0


INTERMEDIATE_BOUND = {BF16: 4e-3, FP32X: 2e-5, FP16: 2.0 ** -11 + 2e-5, FP16X: 2e-5}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_pos_ln_intermediate_widths(L, mode, D):
    """gelu(LN(x)) to the planes only: one row at row m, six rows scattered through a row map to every second row; the rows between them,
    the spare rows and the pitch columns keep the planted pattern."""
    P, ldx, ldoa = n_planes(mode), D + 4, D + 12
    for rows in ROWS:
        x, _, _, _ = inputs(rows, D, 200 * D + rows)
        ref = F.gelu(F.layer_norm(x.double(), (D,), eps=1e-5))
        rowmap = None if rows == 1 else (2 * torch.arange(rows, dtype=torch.int32) + 1)
        out_rows = rows + EXTRA if rowmap is None else 2 * rows + EXTRA
        oa = garbage_planes(P, out_rows, ldoa)
        run_pos_ln(L, mode, rows, D, pitched(x, ldx), ldx, oa, ldoa, rowmap=None if rowmap is None else rowmap.to(DEV))
        a = oa.cpu()
        written = torch.arange(rows) if rowmap is None else rowmap
        err = float((planes_value(a[:, written.long(), :D], mode) - ref).abs().max() / max(1.0, float(ref.abs().max())))
        print(f"ser_pos_ln intermediate mode {mode} D {D} rows {rows}: plane error {err:.2e}")
        assert err < INTERMEDIATE_BOUND[mode]
        assert only_garbage_outside(a, rows, D, written)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_pos_ln_last_widths(L, mode, D):
    """LN(gelu(LN(x)) + residual) * g + b: fp32 within 2e-5 of float64, planes the host split of it; without out_act the same fp32 bytes."""
    P, ldx, ldr, ldof, ldoa = n_planes(mode), D + 4, D + 16, D + 8, D + 12
    for rows in ROWS:
        x, res, g, b = inputs(rows, D, 300 * D + rows)
        t = F.gelu(F.layer_norm(x.double(), (D,), eps=1e-5)) + res.double()
        ref = F.layer_norm(t, (D,), g.double(), b.double(), 1e-5)
        xd, rd, gd, bd = pitched(x, ldx), pitched(res, ldr), g.to(DEV), b.to(DEV)
        of, oa = garbage_f32(rows + EXTRA, ldof), garbage_planes(P, rows + EXTRA, ldoa)
        run_pos_ln(L, mode, rows, D, xd, ldx, oa, ldoa, res=rd, ldr=ldr, g=gd, b=bd, of=of, ldof=ldof)
        f, a = of.cpu(), oa.cpu()
        err = (f[:rows, :D].double() - ref).abs().max().item()
        print(f"ser_pos_ln last mode {mode} D {D} rows {rows}: fp32 error {err:.2e}")
        assert err < 2e-5
        assert bool(f[rows:].isnan().all()) and bool(f[:, D:].isnan().all())
        assert torch.equal(a[:, :rows, :D], host_split(f[:rows, :D], mode))
        assert only_garbage_outside(a, rows, D)
        of2 = garbage_f32(rows + EXTRA, ldof)
        run_pos_ln(L, mode, rows, D, xd, ldx, None, 0, res=rd, ldr=ldr, g=gd, b=bd, of=of2, ldof=ldof)
        assert torch.equal(of2.cpu().view(torch.int32), f.view(torch.int32))


# ----------------------------------------------------------------------------------------------------------------------- ser_row_center_v
STAT_GROUPS = 4


def run_row_center(L, mode, rows, D, xd, ldx, oa, ldoa, osc=None):
    """-> (shift [rows + EXTRA], stats [rows + EXTRA, STAT_GROUPS, 2]) on the CPU, both planted with NaN"""
    st = torch.full((rows + EXTRA, STAT_GROUPS, 2), float("nan"), device=DEV)
    sh = torch.full((rows + EXTRA,), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = L.RowCenterArgs()
    a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = xd.data_ptr(), ldx, oa.data_ptr(), ldoa, oa.shape[1] * ldoa
    a.stats, a.shift, a.stat_groups, a.mode, a.rows, a.D = st.data_ptr(), sh.data_ptr(), STAT_GROUPS, mode, rows, D
    if osc is not None:
        a.out_scale, a.out_scale_ld = osc.data_ptr(), osc.shape[1]
    a.range_flag = flag.data_ptr()
    L.check(L.lib.ser_row_center_v(C.byref(a), stream()), "ser_row_center_v")
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return sh.cpu(), st.cpu()


def check_shift_and_stats(x, rows, D, sh, st):
    """shift = the row mean (1e-5: test_row_center_f16m's bound); stats = [sum d, sum d^2, 0 ...] of d = x - shift as the kernel's fp32
    values.  A lane adds at most 32 terms and the butterfly 6 more levels, so either sum carries at most 39 roundings of 2^-24 relative to
    its sum of magnitudes: 2.4e-6, bound 1e-5.  -> d (fp32)"""
    assert bool(sh[rows:].isnan().all()) and bool(st[rows:].isnan().all())
    assert float((sh[:rows].double() - x.double().mean(1)).abs().max()) < 1e-5
    d = x - sh[:rows, None]                               # one fp32 subtraction, as in the kernel
    d64 = d.double()
    assert bool(((st[:rows, 0, 0].double() - d64.sum(1)).abs() <= 1e-5 * d64.abs().sum(1)).all())
    assert bool(((st[:rows, 0, 1].double() - d64.pow(2).sum(1)).abs() <= 1e-5 * d64.pow(2).sum(1)).all())
    assert bool((st[:rows, 1:].contiguous().view(torch.int32) == 0).all())
    return d


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_row_center_widths(L, mode, D):
    """The centred operand copy: planes = the host split of x - shift[row], bit for bit; shift and the row partials as stated above."""
    P, ldx, ldoa = n_planes(mode), D + 4, D + 12
    for rows in ROWS:
        x = inputs(rows, D, 400 * D + rows)[0] * (2.0 / 3.0) + 5.0
        oa = garbage_planes(P, rows + EXTRA, ldoa)
        sh, st = run_row_center(L, mode, rows, D, pitched(x, ldx), ldx, oa, ldoa)
        d = check_shift_and_stats(x, rows, D, sh, st)
        a = oa.cpu()
        assert torch.equal(a[:, :rows, :D], host_split(d, mode))
        assert only_garbage_outside(a, rows, D)


@pytest.mark.parametrize("D", [64, 320, 2048])
def test_row_center_f16m_widths(L, D):
    """FP16M (whole 64-column tiles): hi plane, e4m3 bytes and scale words = tests/f16m_ref.py's packing of x - shift[row], bit for bit;
    the pitch tile of every row, the spare rows and the scale words of the spare rows keep the planted pattern."""
    ldx, ldoa = D + 4, D + 64
    for rows in ROWS:
        x = inputs(rows, D, 500 * D + rows)[0] * (2.0 / 3.0) + 5.0
        oa = garbage_planes(2, rows + EXTRA, ldoa)
        osc = torch.full((D // 64, rows + EXTRA), GARBAGE, dtype=torch.int32, device=DEV)
        sh, st = run_row_center(L, FP16M, rows, D, pitched(x, ldx), ldx, oa, ldoa, osc)
        d = check_shift_and_stats(x, rows, D, sh, st)
        ref = R.pack(d, False)
        a, s = oa.cpu(), osc.cpu()
        assert torch.equal(a[0, :rows, :D], ref["hi"].view(torch.int16))
        x8 = a[1].contiguous().view(torch.uint8).reshape(rows + EXTRA, 2 * ldoa)       # plane 1 as bytes: 2 D of them per row
        assert torch.equal(x8[:rows, : 2 * D], ref["x8"])
        assert torch.equal(s[:, :rows], ref["scales"].view(torch.int32))
        assert only_garbage_outside(a, rows, D)
        assert bool((s[:, rows:] == GARBAGE).all())
