"""Kernel-level parity tests: every libserhip entry point against a plain fp32/fp64
PyTorch-CPU statement of the same op, called through the C ABI (ctypes).  -m gpu."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def mode_tol(mode, bf16, fp32x):
    """bound per numerics mode: fp16 operands (mode 3) round 8x finer than bf16; gate at 1/2.5 of the bf16 bound.  fp16 hi + lo (mode 4)
    keeps 22 significand bits against fp32x's 16: it takes fp32x's bound."""
    return {1: bf16, 2: fp32x, 3: max(bf16 / 2.5, fp32x), 4: fp32x}[mode]


def act_dtype(mode):
    return torch.float16 if mode in (3, 4) else torch.bfloat16


def to_act(x, mode):
    """fp32 CPU [rows, cols] -> device operand planes the way ser_split_bf16 does (host restatement):
    mode 1 = one bf16 plane, 2 = bf16 hi + lo, 3 = one fp16 plane."""
    if mode == 3:
        return x.to(torch.float16)[None].contiguous().to(DEV)
    hi = x.to(torch.bfloat16)
    if mode == 1:
        return hi[None].contiguous().to(DEV)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous().to(DEV)


def act_value(t):
    """operand planes [P, ...] -> the value they hold, summed in float64 (an fp16 hi + lo pair need not add exactly in fp32)"""
    return t.double().sum(0)


def run_gemm(L, A_act, W_act, M, N, K, mode, **kw):
    g = L.GemmArgs()
    g.A = A_act.data_ptr() + kw.get("a_byte_offset", 0)
    g.a_plane_stride = A_act.shape[1] * A_act.shape[2]
    g.a_rowoff = kw["a_rowoff"].data_ptr() if kw.get("a_rowoff") is not None else None
    g.lda = kw.get("lda", A_act.shape[2])
    g.kc, g.ldj = kw.get("kc", 0), kw.get("ldj", 0)
    g.W = W_act.data_ptr()
    g.w_plane_stride = W_act.shape[1] * W_act.shape[2]
    g.M, g.N, g.K = M, N, K
    g.groups = kw.get("groups", 1)
    g.a_group_stride, g.w_group_stride, g.c_group_stride = kw.get("ags", 0), kw.get("wgs", 0), kw.get("cgs", 0)
    g.mode = mode
    bias = kw.get("bias")
    g.bias = bias.data_ptr() if bias is not None else None
    g.act = kw.get("act", 0)
    res = kw.get("residual")
    g.residual = res.data_ptr() if res is not None else None
    g.ldr = kw.get("ldr", 0)
    g.res_row_mod = kw.get("res_row_mod", 0)
    ncols = kw.get("out_cols", N * g.groups)
    out_f32 = torch.full((kw.get("out_rows", M), ncols), float("nan"), device=DEV) if kw.get("want_f32", True) else None
    if kw.get("in_place"):                                   # the encoder layers' residual GEMMs write the state they read
        out_f32 = res
    g.out_f32 = out_f32.data_ptr() if out_f32 is not None else None
    g.ldo_f32 = ncols
    planes = 2 if mode == 2 else 1
    out_act = None
    if kw.get("want_act", False):
        out_act = torch.zeros((planes, kw.get("out_act_rows", M), ncols), dtype=act_dtype(mode), device=DEV)
        g.out_act = out_act.data_ptr()
        g.ldo_act = ncols
        g.out_plane_stride = out_act.shape[1] * ncols
    rm = kw.get("out_rowmap")
    g.out_rowmap = rm.data_ptr() if rm is not None else None
    if kw.get("ln") is not None:
        g.ln_gamma, g.ln_beta, g.ln_eps = kw["ln"][0].data_ptr(), kw["ln"][1].data_ptr(), 1e-5
    if kw.get("ln_stats") is not None:
        g.ln_stats_in, g.ln_groups, g.ln_colsum = kw["ln_stats"].data_ptr(), kw["ln_groups"], kw["ln_colsum"].data_ptr()
        g.ln_eps = 1e-5
    if kw.get("stat_out") is not None:
        g.stat_out, g.stat_groups = kw["stat_out"].data_ptr(), kw["stat_out"].shape[1]
    g.tile_cfg = kw.get("tile_cfg", 0)
    if kw.get("shift_out") is not None:
        si = kw.get("shift_in")
        g.shift_in = si.data_ptr() if si is not None else None
        g.shift_out, g.shift_const = kw["shift_out"].data_ptr(), kw.get("shift_const", 0.0)
    if kw.get("out_mode"):
        g.out_mode = kw["out_mode"]
        out_act = torch.zeros((1, kw.get("out_act_rows", M), ncols), dtype=act_dtype(kw["out_mode"]), device=DEV)
        g.out_act, g.ldo_act, g.out_plane_stride = out_act.data_ptr(), ncols, out_act.shape[1] * ncols
    if kw.get("mean_out") is not None:
        ls = kw.get("ln_shift")
        g.ln_shift = ls.data_ptr() if ls is not None else None
        g.mean_out = kw["mean_out"].data_ptr()
    L.check(L.lib.ser_gemm(C.byref(g), stream()), "ser_gemm")
    torch.cuda.synchronize()
    return out_f32, out_act


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 200, 192), (77, 8, 64), (515, 392, 1024)])
def test_gemm_integer_exact(L, mode, M, N, K):
    """Small-integer operands are exact in bf16 and fp32: any layout / swizzle / permutation slip
    shows up as a wrong integer.  W is asymmetric on purpose."""
    g = torch.Generator().manual_seed(M * 7 + N)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3).float()
    ref = A.double() @ W.double().T
    out, _ = run_gemm(L, to_act(A, mode), to_act(W, mode), M, N, K, mode)
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cfg", [1, 2, 3])
@pytest.mark.parametrize("M,N,K", [(700, 520, 256), (257, 264, 64), (1030, 128, 640), (300, 136, 128), (140, 256, 192), (129, 8, 320)])
def test_gemm_every_tile_config_integer_exact(L, mode, cfg, M, N, K):
    """128x128 / 256x128 / 256x256 block tiles (2- and 3-stage rings; K = 64..640 covers every ring fill / drain
    length) forced through tile_cfg -- in modes 1 (BF16) and 3 (FP16), which honour it.  Mode 2 (FP32X) ignores tile_cfg, as FP16X does
    (include/ser_hip.h): its three cfg cases run the automatically chosen two-plane tile three times (128x128x64 at these sizes, 128x64x32
    at N = 8).  The two-plane 256x128x32 and 256x256x32 tiles are reached by size, in tests/test_gpu_f16q.py."""
    g = torch.Generator().manual_seed(M + N + cfg)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    ref = A.double() @ W.double().T + bias.double()
    out, _ = run_gemm(L, to_act(A, mode), to_act(W, mode), M, N, K, mode, bias=bias.to(DEV), tile_cfg=cfg)
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("cfg", [1, 2, 3])
def test_gemm_many_tiles_per_cu_integer_exact(L, cfg):
    """Grids of several tiles per CU (3 768 / 1 896 / 948 tiles of 128x128 / 256x128 / 256x256), ragged edges, bias + residual: exact
    integers.  tools/gemm_persist_ab.sh runs this file once more under SER_GEMM_PERSIST=1, where these launches take the persistent
    tile-loop form of the kernel (round 3 experiment) and must give the same integers."""
    M, N, K = 20011, 3000, 192
    g = torch.Generator().manual_seed(cfg)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    res = torch.randint(-9, 10, (M, N), generator=g).float()
    ref = A.double() @ W.double().T + bias.double() + res.double()
    out, _ = run_gemm(L, to_act(A, 1), to_act(W, 1), M, N, K, 1, bias=bias.to(DEV), residual=res.to(DEV), ldr=N, tile_cfg=cfg)
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.parametrize("M,N,K,mod", [(1000, 1024, 1024, 0), (515, 392, 512, 0), (700, 264, 576, 0), (300, 256, 448, 0), (600, 384, 640, 100)])
def test_gemm_residual_in_place_integer_exact(L, M, N, K, mod):
    """The encoder layers' residual GEMMs write the fp32 state they read (engine.py `_gemm(ctx, out, residual=h, out_f32=h)`): exact integers
    against fp64 with the residual IN PLACE on the 128x128 and 256x128 tiles, ragged M / N edges, 7 - 16 K tiles, and a row-periodic residual.
    (Round 5 tried requesting the residual tile during the K loop on these shapes -- slower, DEADENDS.md -- and this is the test it had to pass.)"""
    g = torch.Generator().manual_seed(M + K)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    res = torch.randint(-9, 10, (mod or M, N), generator=g).float()
    ref = A.double() @ W.double().T + bias.double() + (res.double().repeat(M // mod, 1) if mod else res.double())
    for cfg in (1, 2):
        out, _ = run_gemm(L, to_act(A, 1), to_act(W, 1), M, N, K, 1, bias=bias.to(DEV), residual=res.clone().to(DEV), ldr=N, tile_cfg=cfg,
                          in_place=(mod == 0), res_row_mod=mod)
        assert torch.equal(out.cpu().double(), ref), cfg


def test_gemm_fp32x_large_grid_tile_integer_exact(L):
    """FP32X launches with >= 100 tiles of 256 x 128 take the 256x128 / BK = 32 / 3-stage ping-pong tile (gemm.hip, ser_gemm): ragged M
    and N edges, K = 64..320 (ring fill and drain at 2..10 K tiles), integer operands so that one misplaced fragment shows."""
    for M, N, K in ((2561, 1288, 192), (2700, 1536, 64), (3000, 1160, 320)):
        assert ((M + 255) // 256) * ((N + 127) // 128) >= 100
        g = torch.Generator().manual_seed(M + N)
        A = torch.randint(-3, 4, (M, K), generator=g).float()
        W = torch.randint(-3, 4, (N, K), generator=g).float() + (torch.arange(N)[:, None] % 3).float()
        bias = torch.randint(-4, 5, (N,), generator=g).float()
        ref = A.double() @ W.double().T + bias.double()
        out, _ = run_gemm(L, to_act(A, 2), to_act(W, 2), M, N, K, 2, bias=bias.to(DEV))
        assert torch.equal(out.cpu().double(), ref), (M, N, K)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("M,N,K,bias", [(300, 512, 192, True), (1000, 512, 1536, False), (77, 64, 128, True),
                                        (13001, 512, 128, True), (25999, 512, 64, False)])
def test_gemm_layernorm_gelu_epilogue(L, mode, M, N, K, bias):
    """Conv-stack epilogue: act(LayerNorm_row(acc + bias)) over the full (<= 512 wide) row.  The row counts pick all
    three row-complete tiles in bf16 mode (32 x 512 below 12 800 rows, 64 x 512 below 25 600, 128 x 512 above)."""
    g = torch.Generator().manual_seed(N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) if bias else None
    lw, lb = torch.randn(N, generator=g), torch.randn(N, generator=g)
    Aa, Wa = to_act(A, mode), to_act(W, mode)
    pre = act_value(Aa).cpu().double() @ act_value(Wa).cpu().double().T
    if bias:
        pre = pre + b.double()
    ref = torch.nn.functional.gelu(torch.nn.functional.layer_norm(pre, (N,), lw.double(), lb.double(), 1e-5))
    out, oact = run_gemm(L, Aa, Wa, M, N, K, mode, bias=b.to(DEV) if bias else None, act=1,
                         ln=(lw.to(DEV), lb.to(DEV)), want_act=True)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < 2e-4, err
    err_act = (act_value(oact).cpu().double() - ref).abs().max().item()
    assert err_act < mode_tol(mode, 4e-2, 3e-4), err_act


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cfg", [1, 3])
def test_gemm_row_stats_and_deferred_layernorm(L, mode, cfg):
    """Producer GEMM writes x (fp32 + act) and per-64-column (sum, sum^2) partials; the consumer GEMM
    applies LayerNorm(x) W^T + b as rstd*(x W'^T - mu*colsum(W')) + (beta W^T + b) from the RAW x."""
    M, D, N2 = 333, 320, 200
    g = torch.Generator().manual_seed(77 + cfg)
    A0 = torch.randn(M, 128, generator=g)
    W0 = torch.randn(D, 128, generator=g) / math.sqrt(128)
    res = torch.randn(M, D, generator=g) * 2 + 0.7                       # non-zero row mean on purpose
    G = (D + 63) // 64
    G += G & 1
    stat = torch.zeros(M, G, 2, device=DEV)
    x_f32, x_act = run_gemm(L, to_act(A0, mode), to_act(W0, mode), M, D, 128, mode, residual=res.to(DEV), ldr=D,
                            want_act=True, stat_out=stat, tile_cfg=cfg)
    x = x_f32.cpu().double()
    st = stat.cpu().double().sum(1)
    assert (st[:, 0] - x.sum(1)).abs().max() < 1e-3 and (st[:, 1] - (x * x).sum(1)).abs().max() < 2e-2
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    W = torch.randn(N2, D, generator=g) / math.sqrt(D)
    b = torch.randn(N2, generator=g)
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (D,), gamma.double(), beta.double(), 1e-5),
                                     W.double(), b.double())
    Wp = to_act((W.double() * gamma.double()[None, :]).float(), mode)
    colsum = act_value(Wp).double().sum(1).float().contiguous()
    t = (W.double() @ beta.double() + b.double()).float().to(DEV)
    out, _ = run_gemm(L, x_act, Wp, M, N2, D, mode, bias=t, ln_stats=stat, ln_groups=G, ln_colsum=colsum, tile_cfg=cfg)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < mode_tol(mode, 3e-2, 5e-5), err


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("cfg", [1, 2])
def test_shifted_operand_chain_large_row_mean(L, mode, cfg):
    """Rows whose mean is ~50 standard deviations (an offset living in the residual stream): ser_row_center gives the
    first centred copy, a producer GEMM (residual + bias with a uniform offset) carries the shift forward from the
    residual's row partials, and the consumer's deferred LayerNorm -- which never sees the shift, LayerNorm being
    shift invariant -- matches fp64.  Unshifted, bf16(x) alone would be off by 50 * 2^-9 = 10 % of a standard deviation."""
    M, D, N2 = 300, 320, 136
    g = torch.Generator().manual_seed(5 + cfg)
    x0 = torch.randn(M, D, generator=g) + 50.0 + torch.randn(M, 1, generator=g) * 20
    planes = 2 if mode == 2 else 1
    x0_act = torch.zeros((planes, M, D), dtype=act_dtype(mode), device=DEV)
    st0 = torch.full((M, 2, 2), float("nan"), device=DEV)
    sh0 = torch.zeros(M, device=DEV)
    L.check(L.lib.ser_row_center(x0.to(DEV).data_ptr(), D, x0_act.data_ptr(), D, M * D, st0.data_ptr(), 2, sh0.data_ptr(),
                                 mode, M, D, stream()), "ser_row_center")
    torch.cuda.synchronize()
    mean0 = x0.double().mean(1)
    assert (sh0.cpu().double() - mean0).abs().max() < 1e-4
    cen = x0.double() - sh0.cpu().double()[:, None]
    assert (act_value(x0_act).cpu().double() - cen).abs().max() < mode_tol(mode, 2e-2, 2e-4)
    assert (st0.cpu().double()[:, 0, 1] - (cen * cen).sum(1)).abs().max() < 1e-2 and float(st0[:, 1].abs().max()) == 0.0
    # producer: x1 = x0 + A W^T + b, b carries a uniform +3
    A0 = torch.randn(M, 128, generator=g)
    W0 = torch.randn(D, 128, generator=g) / math.sqrt(128)
    b0 = torch.randn(D, generator=g) * 0.1 + 3.0
    G = (D + 63) // 64
    G += G & 1
    stat = torch.zeros(M, G, 2, device=DEV)
    sh1 = torch.zeros(M, device=DEV)
    x1_f32, x1_act = run_gemm(L, to_act(A0, mode), to_act(W0, mode), M, D, 128, mode, bias=b0.to(DEV), residual=x0.to(DEV), ldr=D,
                              want_act=True, stat_out=stat, tile_cfg=cfg, shift_in=sh0, shift_out=sh1,
                              shift_const=float(b0.double().mean()))
    x1 = x1_f32.cpu().double()
    c1 = sh1.cpu().double()
    assert (c1 - (mean0 + b0.double().mean())).abs().max() < 1e-3               # shift = mean(residual row) + mean(bias)
    assert (x1.mean(1) - c1).abs().max() < 1.0                                    # ... which tracks the true row mean
    assert (act_value(x1_act).cpu().double() - (x1 - c1[:, None])).abs().max() < mode_tol(mode, 3e-2, 3e-4)
    ssum = stat.cpu().double().sum(1)
    assert (ssum[:, 0] - (x1 - c1[:, None]).sum(1)).abs().max() < 1e-2
    # consumer: LayerNorm(x1) W^T + b from the shifted copy and its partials
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    W = torch.randn(N2, D, generator=g) / math.sqrt(D)
    b = torch.randn(N2, generator=g)
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(x1, (D,), gamma.double(), beta.double(), 1e-5),
                                     W.double(), b.double())
    Wp = to_act((W.double() * gamma.double()[None, :]).float(), mode)
    colsum = act_value(Wp).double().sum(1).float().contiguous()
    t = (W.double() @ beta.double() + b.double()).float().to(DEV)
    m1 = torch.full((M,), float("nan"), device=DEV)
    out, _ = run_gemm(L, x1_act, Wp, M, N2, D, mode, bias=t, ln_stats=stat, ln_groups=G, ln_colsum=colsum, tile_cfg=cfg,
                      ln_shift=sh1, mean_out=m1)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err
    assert (m1.cpu().double() - x1.mean(1)).abs().max() < 1e-3                  # the consumer reports the absolute row mean


def test_gemm_fp32x_in_fp16_out(L):
    """The stem -> layers boundary of the "f16" numerics mode: a 3-product FP32X GEMM whose operand copy is written as one
    fp16 plane (ser_gemm_args.out_mode); the copy is the fp16 rounding of the fp32 result, and other conversions are refused."""
    M, N, K = 300, 200, 192
    g = torch.Generator().manual_seed(8)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    out, oact = run_gemm(L, to_act(A, 2), to_act(W, 2), M, N, K, 2, out_mode=3)
    ref = A.double() @ W.double().T
    assert (out.cpu().double() - ref).abs().max() < 2e-4
    assert oact.dtype == torch.float16 and torch.equal(oact[0].cpu(), out.cpu().to(torch.float16))
    ga = L.GemmArgs()
    a1, w1 = to_act(A, 1), to_act(W, 1)
    ga.A, ga.W, ga.M, ga.N, ga.K, ga.groups, ga.mode, ga.out_mode, ga.lda = a1.data_ptr(), w1.data_ptr(), M, N, K, 1, 1, 3, K
    ga.out_f32, ga.ldo_f32 = out.data_ptr(), N
    assert L.lib.ser_gemm(C.byref(ga), stream()) < 0 and b"out_mode" in L.lib.ser_last_error()


@pytest.mark.parametrize("mode,tol", [(1, 2e-2), (2, 2e-5)])
def test_gemm_epilogue_and_precision(L, mode, tol):
    M, N, K = 391, 264, 512
    g = torch.Generator().manual_seed(3)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    ref = torch.nn.functional.gelu(A.double() @ W.double().T + bias.double()) + res.double()
    out, oact = run_gemm(L, to_act(A, mode), to_act(W, mode), M, N, K, mode, bias=bias.to(DEV), act=1,
                         residual=res.to(DEV), ldr=N, want_act=True)
    err = (out.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < tol, err
    # the act output is the same value, re-split
    err_act = (act_value(oact).cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err_act < mode_tol(mode, 1e-2, 5e-5), err_act


def test_gemm_fp32x_beats_bf16(L):
    M, N, K = 256, 256, 2048
    g = torch.Generator().manual_seed(5)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ref = A.double() @ W.double().T
    e = {}
    for mode in (1, 2):
        out, _ = run_gemm(L, to_act(A, mode), to_act(W, mode), M, N, K, mode)
        e[mode] = ((out.cpu().double() - ref).abs().max() / ref.abs().max()).item()
    assert e[2] < 2e-5 and e[2] * 50 < e[1], e


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_gemm_conv_rowmap(L, mode):
    """Strided Conv1d (k=3, stride 2) over channels-last rows of two packed utterances."""
    Cin, Cout, k, s = 64, 72, 3, 2
    T_in = [41, 30]
    g = torch.Generator().manual_seed(9)
    x = torch.randint(-2, 3, (sum(T_in), Cin), generator=g).float()
    w = torch.randint(-2, 3, (Cout, Cin, k), generator=g).float()
    T_out = [(t - k) // s + 1 for t in T_in]
    offs_in = np.concatenate([[0], np.cumsum(T_in)])
    ro = np.concatenate([(offs_in[b] + s * np.arange(T_out[b])) * Cin // 8 for b in range(2)])
    ref = []
    for b in range(2):
        xb = x[offs_in[b]:offs_in[b + 1]].T[None]
        ref.append(torch.nn.functional.conv1d(xb, w, stride=s)[0].T)
    ref = torch.cat(ref)
    W2 = w.permute(0, 2, 1).reshape(Cout, k * Cin)
    out, _ = run_gemm(L, to_act(x, mode), to_act(W2, mode), sum(T_out), Cout, k * Cin, mode,
                      a_rowoff=torch.tensor(ro, dtype=torch.int32, device=DEV))
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("Cg", [64, 80, 120])
def test_gemm_grouped_posconv(L, mode, Cg):
    """Grouped conv (k=128, pad 64, drop last frame) through the kc/ldj map with channel padding
    to 64 and a zero-halo'd input, + GELU + residual."""
    G, k = 2, 128
    D = G * Cg
    kc = ((Cg + 63) // 64) * 64
    T = [37, 20]
    half = k // 2
    g = torch.Generator().manual_seed(Cg)
    x = torch.randn(sum(T), D, generator=g)
    x = x.to(torch.bfloat16).float() if mode == 1 else x
    w = torch.randn(D, Cg, k, generator=g) / math.sqrt(Cg * k)
    w = w.to(torch.bfloat16).float() if mode == 1 else w
    bias = torch.randn(D, generator=g)
    offs = np.concatenate([[0], np.cumsum(T)])
    starts = [half * (b + 1) + offs[b] for b in range(2)]
    halo_rows = sum(T) + half * 3
    xh = torch.zeros(halo_rows + 1, D)
    for b in range(2):
        xh[starts[b]:starts[b] + T[b]] = x[offs[b]:offs[b + 1]]
    ro = np.concatenate([(starts[b] - half + np.arange(T[b])) * D // 8 for b in range(2)])
    wp = torch.zeros(G, Cg, k, kc)
    wp[..., :Cg] = w.view(G, Cg, Cg, k).permute(0, 1, 3, 2)
    ref = []
    for b in range(2):
        xb = x[offs[b]:offs[b + 1]].T[None].double()
        y = torch.nn.functional.conv1d(xb, w.double(), bias.double(), padding=half, groups=G)[:, :, :-1]
        ref.append(torch.nn.functional.gelu(y)[0].T + x[offs[b]:offs[b + 1]].double())
    ref = torch.cat(ref)
    out, _ = run_gemm(L, to_act(xh, mode), to_act(wp.reshape(G * Cg, k * kc), mode), sum(T), Cg, k * kc, mode,
                      a_rowoff=torch.tensor(ro, dtype=torch.int32, device=DEV), kc=kc, ldj=D, groups=G, ags=Cg,
                      wgs=Cg * k * kc, cgs=Cg, bias=bias.to(DEV), act=1, residual=x.to(DEV), ldr=D)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 2e-3, 3e-5), err


def test_gemm_rowmap_and_rowmod(L):
    M, N, K, mod = 90, 64, 64, 30
    g = torch.Generator().manual_seed(2)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    pos = torch.randint(-5, 6, (mod, N), generator=g).float()
    rowmap = torch.tensor(np.arange(M) * 2 + 1, dtype=torch.int32, device=DEV)
    out, oact = run_gemm(L, to_act(A, 1), to_act(W, 1), M, N, K, 1, residual=pos.to(DEV), ldr=N, res_row_mod=mod,
                         want_act=True, out_act_rows=2 * M + 1, out_rowmap=rowmap)
    ref = A @ W.T + pos.repeat(M // mod, 1)
    assert torch.equal(out.cpu(), ref)
    got = act_value(oact).cpu().float()
    assert torch.equal(got[1::2][:M], ref.to(torch.bfloat16).float())
    assert torch.count_nonzero(got[0::2]) == 0


def test_gemm_rejects_bad_shapes(L):
    g = L.GemmArgs()
    assert L.lib.ser_gemm(C.byref(g), None) < 0
    assert b"null" in L.lib.ser_last_error()


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("D,gelu", [(512, True), (1024, False), (1920, False), (64, True), (1536, False)])
def test_layernorm(L, mode, D, gelu):
    """ser_layernorm in every mode it writes (3 = one fp16 plane, 4 = fp16 hi + lo: the post-LN layers of the text and *-base speech
    encoders in f16x).  The planes are written from the same fp32 y as `of`, so they must be the host split of `of` bit for bit."""
    rows = 37
    g = torch.Generator().manual_seed(D)
    x = torch.randn(rows, D, generator=g) * 3 + 0.5
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-5)
    if gelu:
        ref = torch.nn.functional.gelu(ref)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    of = torch.empty(rows, D, device=DEV)
    planes = 2 if mode in (2, 4) else 1
    oa = torch.empty(planes, rows, D, dtype=act_dtype(mode), device=DEV)
    L.check(L.lib.ser_layernorm(xd.data_ptr(), D, wd.data_ptr(), bd.data_ptr(), 1e-5, int(gelu), of.data_ptr(), D,
                                oa.data_ptr(), D, rows * D, mode, rows, D, stream()))
    torch.cuda.synchronize()
    assert (of.cpu().double() - ref).abs().max().item() < 2e-5
    assert (act_value(oa).cpu().double() - ref).abs().max().item() < mode_tol(mode, 4e-2, 1e-4)
    f = of.cpu()
    hi = f.clamp(-65504.0, 65504.0).half() if mode in (3, 4) else f.to(torch.bfloat16)
    assert torch.equal(oa[0].cpu().view(torch.int16), hi.view(torch.int16))
    if planes == 2:
        d = f - hi.float()
        lo = d.clamp(-65504.0, 65504.0).half() if mode == 4 else d.to(torch.bfloat16)
        assert torch.equal(oa[1].cpu().view(torch.int16), lo.view(torch.int16))


def test_wave_norm(L):
    lens = [16000, 401, 23457]
    g = np.random.default_rng(0)
    waves = [(0.1 * g.standard_normal(n) + 0.03).astype(np.float32) for n in lens]
    packed = torch.from_numpy(np.concatenate(waves)).to(DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    out = torch.empty_like(packed)
    L.check(L.lib.ser_wave_norm(packed.data_ptr(), offs.data_ptr(), len(lens), out.data_ptr(), stream()))
    got = out.cpu().numpy()
    o = 0
    for w in waves:
        ref = (w - w.mean()) / np.sqrt(w.var() + 1e-7)          # HF zero_mean_unit_var_norm
        assert np.abs(got[o:o + len(w)] - ref).max() < 2e-5
        o += len(w)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Cc,bias", [(64, True), (512, False)])
def test_conv0_ln_gelu(L, mode, Cc, bias):
    lens = [2000, 1205]
    k, s = 10, 5
    g = torch.Generator().manual_seed(Cc)
    x = [torch.randn(n, generator=g) for n in lens]
    w = torch.randn(Cc, 1, k, generator=g) * 0.5
    bvec = torch.randn(Cc, generator=g) if bias else None
    lw, lb = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    T = [(n - k) // s + 1 for n in lens]
    ref = []
    for xb in x:
        y = torch.nn.functional.conv1d(xb[None, None].double(), w.double(), None if bvec is None else bvec.double(), stride=s)
        y = torch.nn.functional.layer_norm(y[0].T, (Cc,), lw.double(), lb.double(), 1e-5)
        ref.append(torch.nn.functional.gelu(y))
    ref = torch.cat(ref)
    packed = torch.cat(x).to(DEV)
    soffs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    foffs = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=DEV)
    planes = 2 if mode == 2 else 1
    out = torch.empty(planes, sum(T), Cc, dtype=torch.bfloat16, device=DEV)
    wd = w.reshape(Cc, k).contiguous().to(DEV)
    bd = bvec.to(DEV) if bias else None
    lwd, lbd = lw.to(DEV), lb.to(DEV)
    L.check(L.lib.ser_conv0_ln_gelu(packed.data_ptr(), soffs.data_ptr(), foffs.data_ptr(), 2, wd.data_ptr(),
                                    bd.data_ptr() if bias else None, lwd.data_ptr(), lbd.data_ptr(), out.data_ptr(),
                                    sum(T) * Cc, mode, Cc, k, s, sum(T), stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 4e-2, 2e-4), err


@pytest.mark.parametrize("mode", [1, 2])
def test_wave_frames_feeds_matrix_core_conv0(L, mode):
    """ser_wave_frames (normalise + framing) -> ser_gemm(K=64, LayerNorm+GELU epilogue) == Conv1d(1,C,10,5) -> LN -> GELU
    of the HF-normalised waveform, for a ragged pair."""
    lens, k, s, Cc = [3000, 1207], 10, 5, 512
    rng = np.random.default_rng(1)
    waves = [(0.1 * rng.standard_normal(n) + 0.02).astype(np.float32) for n in lens]
    T = [(n - k) // s + 1 for n in lens]
    rows = sum(T)
    packed = torch.from_numpy(np.concatenate(waves)).to(DEV)
    soffs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    foffs = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=DEV)
    planes = 2 if mode == 2 else 1
    frames = torch.empty(planes, rows, 64, dtype=torch.bfloat16, device=DEV)
    work = torch.empty(L.lib.ser_workspace_bytes(L.WS_WAVE_FRAMES, 2, 0, 0, 0, mode), dtype=torch.uint8, device=DEV)
    L.check(L.lib.ser_wave_frames(packed.data_ptr(), soffs.data_ptr(), foffs.data_ptr(), 2, k, s, frames.data_ptr(),
                                  rows * 64, mode, work.data_ptr(), rows, stream()))
    torch.cuda.synchronize()
    fv = act_value(frames).cpu()
    o = 0
    for b, w in enumerate(waves):
        xn = (w - w.mean()) / np.sqrt(w.var() + 1e-7)                      # HF zero_mean_unit_var_norm
        ref = np.stack([xn[s * t: s * t + k] for t in range(T[b])])
        assert np.abs(fv[o:o + T[b], :k].numpy() - ref).max() < mode_tol(mode, 2e-2, 3e-5)
        assert torch.count_nonzero(fv[o:o + T[b], k:]) == 0
        o += T[b]
    g = torch.Generator().manual_seed(0)
    w = torch.randn(Cc, 1, k, generator=g) * 0.5
    lw, lb = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    wp = torch.zeros(Cc, 64)
    wp[:, :k] = w[:, 0]
    Wa = to_act(wp, mode)
    pre = fv.double() @ act_value(Wa).cpu().double().T
    ref = torch.nn.functional.gelu(torch.nn.functional.layer_norm(pre, (Cc,), lw.double(), lb.double(), 1e-5))
    _, oact = run_gemm(L, frames, Wa, rows, Cc, 64, mode, act=1, ln=(lw.to(DEV), lb.to(DEV)), want_act=True, want_f32=False)
    err = (act_value(oact).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 4e-2, 3e-4), err


def test_bias_table_bit_exact(L, golden_dir):
    """Bucket function against the committed HF table for rel in [-1500, 1500] (integer gate)."""
    gold = np.load(os.path.join(golden_dir, "integer_tables.npz"))
    T, H, NB = 1501, 4, 320
    emb = (torch.arange(NB)[:, None] * 10 + torch.arange(H)[None, :]).float()      # value encodes (bucket, head)
    table = torch.empty(H, 2 * T - 1, device=DEV)
    embd = emb.to(DEV)
    L.check(L.lib.ser_wavlm_bias_table(embd.data_ptr(), table.data_ptr(), T, H, NB, 800, stream()))
    got = table.cpu()
    buckets = torch.from_numpy(gold["buckets"].astype(np.int64))                     # rel = -1500..1500
    for h in range(H):
        assert torch.equal(got[h], buckets.float() * 10 + h)


@pytest.mark.parametrize("mode", [1, 2])
def test_wavlm_gate(L, mode):
    rows, H, dh = 53, 4, 64
    g = torch.Generator().manual_seed(1)
    x = torch.randn(rows, H * dh, generator=g)
    w8, b8, cst = torch.randn(8, dh, generator=g) * 0.3, torch.randn(8, generator=g) * 0.3, torch.randn(H, generator=g)
    xa = to_act(x, mode)
    xv = act_value(xa).cpu().double()
    p = torch.nn.functional.linear(xv.view(rows, H, dh), w8.double(), b8.double()).view(rows, H, 2, 4).sum(-1)
    a, b = torch.sigmoid(p).unbind(-1)
    ref = a * (b * cst.double()[None, :] - 1.0) + 2.0
    gate = torch.empty(rows, H, device=DEV)
    w8d, b8d, cd = w8.to(DEV), b8.to(DEV), cst.to(DEV)
    L.check(L.lib.ser_wavlm_gate(xa.data_ptr(), H * dh, rows * H * dh, mode, w8d.data_ptr(), b8d.data_ptr(),
                                 cd.data_ptr(), gate.data_ptr(), rows, H, dh, stream()))
    assert (gate.cpu().double() - ref).abs().max().item() < 1e-5


def attention_reference(q, k, v, scale, table=None, gate=None):
    """fp64 statement of softmax(q k^T scale + gate*bias) v for one utterance, [H, T, dh] inputs."""
    T = q.shape[1]
    s = torch.matmul(q, k.transpose(1, 2)) * scale
    if table is not None:
        idx = (torch.arange(T)[None, :] - torch.arange(T)[:, None]) + (table.shape[1] - 1) // 2
        s = s + gate.T[:, :, None] * table[:, idx]
    return torch.matmul(torch.softmax(s, dim=-1), v)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dh,H,bias", [(64, 2, True), (64, 3, False), (80, 2, False), (120, 2, False), (128, 1, False), (80, 2, True), (120, 2, True)])
def test_attention(L, mode, dh, H, bias):
    Ts = [70, 129, 5, 200]
    D = H * dh
    M = sum(Ts)
    g = torch.Generator().manual_seed(dh + H)
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    Tmax = max(Ts)
    table = gate = None
    if bias:
        table = torch.randn(H, 2 * Tmax - 1, generator=g)
        gate = torch.rand(M, H, generator=g) * 2
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        tb = gt = None
        if bias:
            c = Tmax - 1
            tb = table[:, c - (T - 1): c + T].double()
            gt = gate[offs[b]:offs[b + 1]].double()
        o = attention_reference(q, k, v, dh ** -0.5, tb, gt)
        ref[offs[b]:offs[b + 1]] = o.permute(1, 0, 2).reshape(T, D)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td = table.to(DEV) if bias else None
    gd = gate.to(DEV) if bias else None
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax,
                                td.data_ptr() if bias else None, Tmax if bias else 0, gd.data_ptr() if bias else None,
                                out.data_ptr(), D, M * D, H, dh, dh ** -0.5, mode, 0, None, None, None, 0, stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("mode", [1, 2])
def test_attention_long_utterance_bias_window(L, mode):
    """A 22 s utterance (1100 frames, 9 query tiles) next to a short one: the bias window of a block (T + 192 distances) no longer
    fits one staging pass of 256 threads x 4 slots, so the further passes of the copy loop run, and every query tile has its own
    window start / alignment shift (jmin).  Same reference as test_attention."""
    Ts, H, dh = [1100, 37], 2, 64
    D, M, Tmax = H * dh, sum(Ts), max(Ts)
    g = torch.Generator().manual_seed(1100)
    qkv = torch.randn(M, 3 * D, generator=g)
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    table = torch.randn(H, 2 * Tmax - 1, generator=g)
    gate = torch.rand(M, H, generator=g) * 2
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        c = Tmax - 1
        o = attention_reference(q, k, v, dh ** -0.5, table[:, c - (T - 1): c + T].double(), gate[offs[b]:offs[b + 1]].double())
        ref[offs[b]:offs[b + 1]] = o.permute(1, 0, 2).reshape(T, D)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td, gd = table.to(DEV), gate.to(DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax,
                                td.data_ptr(), Tmax, gd.data_ptr(), out.data_ptr(), D, M * D, H, dh, dh ** -0.5, mode, 0,
                                None, None, None, 0, stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_attention_unbounded_utterance_reads_the_table_from_global_memory(L, mode):
    """The reference has no utterance-length limit (preprocess_speech.py:47-50).  An utterance whose relative-position window no
    longer fits the 160 KiB of LDS (8 200 frames = 164 s here; the LDS form stops at ~5 900-7 900 depending on the mode) takes the
    kernel form that reads the [H, 2T-1] table from global memory; a short utterance in the same ragged batch shares the launch.
    q pre-scaled (the host always does), fused gate columns.  Reference in fp64, queries in chunks."""
    Ts, H, dh = [8200, 150], 1, 64
    D, M, Tmax = H * dh, sum(Ts), max(Ts)
    g = torch.Generator().manual_seed(8200)
    ld = 3 * D + 8
    qkv = torch.randn(M, ld, generator=g)
    c = dh ** -0.5 * 1.4426950408889634
    pre = qkv.clone()
    pre[:, :D] *= c
    qa = to_act(pre, mode)
    qv = act_value(qa).cpu().double()
    table = torch.randn(H, 2 * Tmax - 1, generator=g)
    cst = torch.randn(H, generator=g) + 1.0
    pg = qv[:, 3 * D: 3 * D + 2 * H].view(M, H, 2)
    gate = torch.sigmoid(pg[..., 0]) * (torch.sigmoid(pg[..., 1]) * cst.double()[None, :] - 1.0) + 2.0
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        sl = slice(offs[b], offs[b + 1])
        q, k, v = qv[sl, :D] / c, qv[sl, D:2 * D], qv[sl, 2 * D:3 * D]
        tb = table[0, Tmax - 1 - (T - 1): Tmax - 1 + T].double()
        for q0 in range(0, T, 1024):
            q1 = min(T, q0 + 1024)
            idx = (torch.arange(T)[None, :] - torch.arange(q0, q1)[:, None]) + (T - 1)
            sc = (q[q0:q1] @ k.T) * dh ** -0.5 + gate[sl][q0:q1, 0:1] * tb[idx]
            ref[offs[b] + q0: offs[b] + q1] = torch.softmax(sc, dim=-1) @ v
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td, cd = table.to(DEV), cst.to(DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), ld, M * ld, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax, td.data_ptr(), Tmax,
                                None, out.data_ptr(), D, M * D, H, dh, -1.0, mode, 3 * D, cd.data_ptr(), None, None, 0, stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_attention_fused_gate_columns(L, mode):
    """WavLM gate from its two pre-activation columns per head inside the packed projection matrix."""
    Ts, H, dh = [90, 200], 2, 64
    D, M = H * dh, sum(Ts)
    g = torch.Generator().manual_seed(5)
    ld = 3 * D + 2 * H + 4                                      # +4: pitch stays a multiple of 8
    qkv = torch.randn(M, ld, generator=g)
    qkv[:, : 2 * D] *= 1.5
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    Tmax = max(Ts)
    table = torch.randn(H, 2 * Tmax - 1, generator=g)
    cst = torch.randn(H, generator=g) + 1.0
    pre = qv[:, 3 * D: 3 * D + 2 * H].view(M, H, 2)
    a, bsg = torch.sigmoid(pre[..., 0]), torch.sigmoid(pre[..., 1])
    gate = a * (bsg * cst.double()[None, :] - 1.0) + 2.0
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        c = Tmax - 1
        o = attention_reference(q, k, v, dh ** -0.5, table[:, c - (T - 1): c + T].double(), gate[offs[b]:offs[b + 1]])
        ref[offs[b]:offs[b + 1]] = o.permute(1, 0, 2).reshape(T, D)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td, cd = table.to(DEV), cst.to(DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), ld, M * ld, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax, td.data_ptr(), Tmax,
                                None, out.data_ptr(), D, M * D, H, dh, dh ** -0.5, mode, 3 * D, cd.data_ptr(), None, None, 0, stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dh,H", [(64, 2), (64, 16), (32, 3)])
def test_attention_gate_from_operand_copy(L, mode, dh, H, pre):
    """ser_attention_v with gate_x: the WavLM gate's two pre-activations per (row, head) are computed INSIDE the kernel from the layer
    input's operand copy, (relative mean, rstd) per row and the LayerNorm-folded weights (HF modeling_wavlm.py:167-180 on
    LayerNorm1(x)) -- against an fp64 statement of LayerNorm -> Linear(dh, 8) -> sums of four -> sigmoids."""
    Ts = [90, 200, 37]
    D, M, Tmax = H * dh, sum(Ts), 200
    g = torch.Generator().manual_seed(dh + H)
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    if pre:                                            # what the encoders launch: q pre-scaled by the projection epilogue
        qkv[:, :D] *= dh ** -0.5 * 1.4426950408889634
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    if pre:
        qv[:, :D] /= dh ** -0.5 * 1.4426950408889634
    x = torch.randn(M, D, generator=g) * 2.0 + torch.randn(M, 1, generator=g)          # layer input; rows with their own offsets
    xa = to_act(x, mode)
    xv = act_value(xa).cpu().double()                                                   # what the kernel reads
    gam, bet = torch.rand(D, generator=g).double() + 0.5, torch.randn(D, generator=g).double() * 0.2
    w8, b8 = torch.randn(8, dh, generator=g).double() * 0.3, torch.randn(8, generator=g).double() * 0.2
    cst = torch.randn(H, generator=g) + 1.0
    table = torch.randn(H, 2 * Tmax - 1, generator=g)
    mu, var = xv.mean(1, keepdim=True), xv.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    ln = ((xv - mu) * rstd * gam + bet).view(M, H, dh)
    pre8 = ln @ w8.T + b8                                                               # [M, H, 8]
    a, bsg = torch.sigmoid(pre8[..., :4].sum(-1)), torch.sigmoid(pre8[..., 4:].sum(-1))
    gate = a * (bsg * cst.double()[None, :] - 1.0) + 2.0
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    for b, T in enumerate(Ts):
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        c = Tmax - 1
        o = attention_reference(q, k, v, dh ** -0.5, table[:, c - (T - 1): c + T].double(), gate[offs[b]:offs[b + 1]])
        ref[offs[b]:offs[b + 1]] = o.permute(1, 0, 2).reshape(T, D)
    # host side of the fold (engine._layer_weights): operand planes [planes][H][2][dh], column sums of exactly those planes
    wab = torch.stack([w8[:4].sum(0), w8[4:].sum(0)], 0)                                # [2, dh]
    gwa = to_act((gam.view(H, 1, dh) * wab[None]).reshape(2 * H, dh).float(), mode)
    gwv = act_value(gwa).cpu().double().view(H, 2, dh)
    # the kernel multiplies the ROUNDED weights: the reference gate above is the exact one, so allow for that rounding below
    cb = torch.cat([gwv.sum(2), (bet.view(H, 1, dh) * wab[None]).sum(2) + torch.stack([b8[:4].sum(), b8[4:].sum()])[None]], 1)
    cbd = cb.float().contiguous().to(DEV)
    std = torch.cat([mu, rstd], 1).float().contiguous().to(DEV)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td, cd = table.to(DEV), cst.to(DEV)
    a_ = L.AttentionArgs()
    a_.qkv, a_.ld, a_.plane_stride, a_.q_col, a_.k_col, a_.v_col, a_.B = qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, len(Ts)
    a_.frame_offs, a_.table, a_.max_frames, a_.table_T = foffs.data_ptr(), td.data_ptr(), Tmax, Tmax
    a_.out, a_.ldo, a_.out_plane_stride, a_.H, a_.dh, a_.scale, a_.mode = out.data_ptr(), D, M * D, H, dh, (-1.0 if pre else dh ** -0.5), mode
    a_.gru_const = cd.data_ptr()
    a_.gate_x, a_.gate_x_ld, a_.gate_x_plane_stride, a_.gate_x_planes = xa.data_ptr(), D, M * D, planes
    a_.gate_stat, a_.gate_w, a_.gate_cb, a_.gate_w_plane_stride = std.data_ptr(), gwa.data_ptr(), cbd.data_ptr(), 2 * H * dh
    L.check(L.lib.ser_attention_v(C.byref(a_), stream()), "ser_attention_v")
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err
    a_.gate_w = None                                                                    # incomplete gate_x arguments are refused
    assert L.lib.ser_attention_v(C.byref(a_), stream()) != 0


def test_gemm_reports_row_statistics_for_the_gate(L):
    """ser_gemm_args.lnstat_out: the consumer of a deferred LayerNorm writes (mean relative to the rows' shift, rstd) per row --
    the numbers ser_attention's in-kernel gate applies to the same operand copy."""
    M, N, K = 300, 128, 256
    g = torch.Generator().manual_seed(3)
    shift = torch.randn(M, generator=g) * 3.0
    xc = torch.randn(M, K, generator=g) * 1.5 + 0.3                                      # rows as stored: x - shift
    W = torch.randn(N, K, generator=g) / K ** 0.5
    groups = K // 64
    part = torch.stack([xc.view(M, groups, 64).sum(-1), (xc.view(M, groups, 64) ** 2).sum(-1)], -1).contiguous()   # [M, groups, 2]
    Aa, Wa = to_act(xc, 1), to_act(W, 1)
    ga = L.GemmArgs()
    out = torch.empty(M, N, device=DEV)
    lnst = torch.zeros(M, 2, device=DEV)
    mean_abs = torch.zeros(M, device=DEV)
    pd, sd_, cs = part.to(DEV), shift.to(DEV), act_value(Wa).sum(1).float().contiguous()
    ga.A, ga.lda, ga.W, ga.M, ga.N, ga.K, ga.groups, ga.mode = Aa.data_ptr(), K, Wa.data_ptr(), M, N, K, 1, 1
    ga.out_f32, ga.ldo_f32 = out.data_ptr(), N
    ga.ln_stats_in, ga.ln_groups, ga.ln_colsum, ga.ln_eps = pd.data_ptr(), groups, cs.data_ptr(), 1e-5
    ga.ln_shift, ga.mean_out, ga.lnstat_out = sd_.data_ptr(), mean_abs.data_ptr(), lnst.data_ptr()
    L.check(L.lib.ser_gemm(C.byref(ga), stream()), "ser_gemm")
    torch.cuda.synchronize()
    mu = xc.double().mean(1)
    rstd = 1.0 / torch.sqrt(xc.double().var(1, unbiased=False) + 1e-5)
    assert (lnst[:, 0].cpu().double() - mu).abs().max() < 1e-5
    assert ((lnst[:, 1].cpu().double() - rstd) / rstd).abs().max() < 1e-5
    assert (mean_abs.cpu().double() - (mu + shift.double())).abs().max() < 1e-5


def _prescaled_case(L, mode, dh, bias, Ts, ramp=0.0, H=2, pre_scaled=True, check=None):
    D, M = H * dh, sum(Ts)
    g = torch.Generator().manual_seed(dh)
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    if ramp:                                                   # scores that climb with the key position, and one late spike per utterance
        u = torch.ones(dh) / dh ** 0.5
        pos = torch.cat([torch.arange(T) / max(T - 1, 1) for T in Ts])
        for h in range(H):
            qkv[:, h * dh:(h + 1) * dh] += 3.0 * u
            qkv[:, D + h * dh: D + (h + 1) * dh] += (ramp * pos)[:, None] * u
        o0 = 0
        for T in Ts:
            if T > 40:
                qkv[o0 + T - 20, D: D + dh] += qkv[o0 + 7, :dh] * 6.0    # head 0: key T-20 lines up with query 7
            o0 += T
    pre = qkv.clone()
    if pre_scaled:
        pre[:, :D] *= dh ** -0.5 * 1.4426950408889634
    qa = to_act(pre, mode)
    qv = act_value(qa).cpu().double()
    if pre_scaled:
        qv[:, :D] /= dh ** -0.5 * 1.4426950408889634           # reference sees the un-scaled (already rounded) q
    Tmax = max(Ts)
    table = torch.randn(H, 2 * Tmax - 1, generator=g) if bias else None
    gate = torch.rand(M, H, generator=g) * 2 if bias else None
    offs = np.concatenate([[0], np.cumsum(Ts)])
    ref = torch.empty(M, D, dtype=torch.float64)
    which = range(len(Ts)) if check is None else check         # utterances compared with the fp64 statement (all by default)
    for b, T in enumerate(Ts):
        if b not in which:
            continue
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        c = Tmax - 1
        o = attention_reference(q, k, v, dh ** -0.5, table[:, c - (T - 1): c + T].double() if bias else None,
                                gate[offs[b]:offs[b + 1]].double() if bias else None)
        ref[offs[b]:offs[b + 1]] = o.permute(1, 0, 2).reshape(T, D)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td = table.to(DEV) if bias else None
    gd = gate.to(DEV) if bias else None
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax,
                                td.data_ptr() if bias else None, Tmax if bias else 0, gd.data_ptr() if bias else None,
                                out.data_ptr(), D, M * D, H, dh, -1.0 if pre_scaled else dh ** -0.5, mode, 0, None, None, None, 0, stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all())
    got = act_value(out).cpu().double()
    return max((got[offs[b]:offs[b + 1]] - ref[offs[b]:offs[b + 1]]).abs().max().item() for b in which)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("dh,bias", [(64, True), (64, False), (120, False)])
def test_attention_prescaled_q(L, mode, dh, bias):
    """scale <= 0: q arrives multiplied by dh^-0.5*log2(e) (projection epilogue); scores are exp2 exponents and,
    with a bias table, the MFMA accumulators start at gate*bias."""
    err = _prescaled_case(L, mode, dh, bias, [150, 64, 333])
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("dh,bias", [(64, True), (64, False), (80, False), (128, False), (80, True), (120, True)])
def test_attention_stale_running_maximum(L, mode, dh, bias):
    """Pre-scaled launches with a bias table keep a STALE row maximum in the accumulators' start value and only raise it when a tile
    exceeds it by 2^8 (csrc/attention.hip, LAZY); the others track the exact maximum.  Scores that climb ~50 exp2-units across 11 key
    tiles plus a late spike drive the raise / rescale branch every other tile; utterances of 1 and 65 frames cover a first tile that is
    (almost) all padding.  (fp32x bound: one-hot rows over |v| ~ 4 with logits of +-100 -- 1.5e-4 on either form.)"""
    err = _prescaled_case(L, mode, dh, bias, [700, 65, 1, 130], ramp=100.0)
    assert err < mode_tol(mode, 3e-2, 3e-4), err


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("Ts", [[499, 1, 31, 33, 64, 65, 128, 257, 512], [500, 499, 448, 449, 3], [150]])
def test_attention_tile_and_query_block_edges(L, mode, bias, Ts):
    """Ragged batches whose lengths sit on every key-tile / query-block edge (1, 31 | 33, 64 | 65, 448 | 449, 512), a climbing score ramp
    with a late spike so that the stale running maximum is raised in later tiles, with and without the WavLM bias table, head dim 64,
    single-plane modes, pre-scaled q.  (Written for the K/V-resident experiment of round 4, whose source is gone: DEADENDS.md; these shapes
    run the tiled kernel, which is what this test pins.  The gate_x form and H = 16 are test_attention_gate_from_operand_copy[pre].)"""
    err = _prescaled_case(L, mode, 64, bias, Ts, ramp=60.0)
    assert err < mode_tol(mode, 3e-2, 3e-4), err


@pytest.mark.parametrize("mode", [1, 3])
def test_attention_full_batch_launch_shape(L, mode):
    """The launch shape of BASELINE configs[1]: 16 utterances x 16 heads x up to 499 frames = 1 024 blocks -> the high-occupancy arm (OCC: one K/V
    buffer, four blocks per CU) WITH the WavLM bias table + gate[].  (OCC without a table: test_attention_high_occupancy_arm_without_table.)"""
    H, dh = 16, 64
    Ts = [499, 499, 149, 333, 250, 499, 64, 401, 499, 200, 450, 499, 97, 499, 310, 499]
    D, M, Tmax = H * dh, sum(Ts), 499
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(M, 3 * D, generator=g)
    qkv[:, : 2 * D] *= 1.5
    qkv[:, :D] *= dh ** -0.5 * 1.4426950408889634
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    qv[:, :D] /= dh ** -0.5 * 1.4426950408889634
    table = torch.randn(H, 2 * Tmax - 1, generator=g)
    gate = torch.rand(M, H, generator=g) * 2
    offs = np.concatenate([[0], np.cumsum(Ts)])
    out = torch.zeros(1, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.tensor(offs, dtype=torch.int32, device=DEV)
    td, gd = table.to(DEV), gate.to(DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), len(Ts), Tmax, td.data_ptr(), Tmax,
                                gd.data_ptr(), out.data_ptr(), D, M * D, H, dh, -1.0, mode, 0, None, None, None, 0, stream()))
    torch.cuda.synchronize()
    got = act_value(out).cpu().double()
    worst = 0.0
    for b in (0, 2, 6, 12, 15):                                 # full-length, short and one-tile utterances; every head
        T = Ts[b]
        blk = qv[offs[b]:offs[b + 1]]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        c = Tmax - 1
        o = attention_reference(q, k, v, dh ** -0.5, table[:, c - (T - 1): c + T].double(), gate[offs[b]:offs[b + 1]].double())
        worst = max(worst, (got[offs[b]:offs[b + 1]] - o.permute(1, 0, 2).reshape(T, D)).abs().max().item())
    assert bool(torch.isfinite(got).all())
    assert worst < mode_tol(mode, 3e-2, 3e-4), worst


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("pre_scaled", [True, False])
def test_attention_high_occupancy_arm_without_table(L, mode, pre_scaled):
    """the OCC arm (single-plane, head dim 64, 513 .. 1 024 blocks) was covered with a bias table only.  Without one it runs for
    wav2vec2-large / HuBERT-large at 16 x 10 s and for Whisper tail batches; here 16 utterances x 16 heads, ragged up to 499 frames = 1 024
    blocks, pre-scaled q (scores are exp2 exponents) and plain q with scale = dh^-0.5, bf16 and fp16, against the fp64 statement."""
    Ts = [499, 499, 149, 333, 250, 499, 64, 401, 499, 200, 450, 499, 97, 499, 310, 499]
    err = _prescaled_case(L, mode, 64, False, Ts, H=16, pre_scaled=pre_scaled, check=(0, 2, 6, 12, 15))
    assert err < mode_tol(mode, 3e-2, 3e-4), err


@pytest.mark.parametrize("mode", [1, 3])
def test_attention_high_occupancy_arm_with_table_and_plain_q(L, mode):
    """The OCC arm with the bias table + gate[] and scale = dh^-0.5 (q not pre-scaled): the one combination of the arm's four that
    neither test_attention_full_batch_launch_shape (table, pre-scaled) nor the test above (no table) launches.  Same 1 024-block shape."""
    Ts = [499, 499, 149, 333, 250, 499, 64, 401, 499, 200, 450, 499, 97, 499, 310, 499]
    err = _prescaled_case(L, mode, 64, True, Ts, H=16, pre_scaled=False, check=(0, 2, 6, 12, 15))
    assert err < mode_tol(mode, 3e-2, 3e-4), err


def test_gemm_column_scale(L):
    M, N, K = 130, 96, 64
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-3, 4, (N, K), generator=g).float()
    gargs = dict(bias=torch.ones(N).to(DEV))
    ref = (A @ W.T + 1.0)
    ref[:, :32] *= 0.5
    g2 = L.GemmArgs()
    out = torch.empty(M, N, device=DEV)
    Aa, Wa, b = to_act(A, 1), to_act(W, 1), torch.ones(N, device=DEV)
    g2.A, g2.lda, g2.W, g2.M, g2.N, g2.K, g2.groups, g2.mode = Aa.data_ptr(), K, Wa.data_ptr(), M, N, K, 1, 1
    g2.bias, g2.out_f32, g2.ldo_f32, g2.col_scale, g2.col_scale_end = b.data_ptr(), out.data_ptr(), N, 0.5, 32
    L.check(L.lib.ser_gemm(C.byref(g2), stream()))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("mode", [1, 2])
def test_attention_key_lengths(L, mode):
    """Text encoders: every sequence keeps all T query rows, keys >= key_lens[b] are padding."""
    T, B, H, dh = 80, 3, 2, 64
    D, M = H * dh, B * T
    klens = [80, 37, 5]
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(M, 3 * D, generator=g)
    qa = to_act(qkv, mode)
    qv = act_value(qa).cpu().double()
    ref = torch.empty(M, D, dtype=torch.float64)
    for b in range(B):
        blk = qv[b * T:(b + 1) * T]
        q, k, v = (blk[:, i * D:(i + 1) * D].view(T, H, dh).permute(1, 0, 2) for i in range(3))
        s = torch.matmul(q, k.transpose(1, 2)) * dh ** -0.5
        s[:, :, klens[b]:] = float("-inf")
        ref[b * T:(b + 1) * T] = torch.matmul(torch.softmax(s, -1), v).permute(1, 0, 2).reshape(T, D)
    planes = 2 if mode == 2 else 1
    out = torch.zeros(planes, M, D, dtype=act_dtype(mode), device=DEV)
    foffs = torch.arange(0, M + 1, T, dtype=torch.int32, device=DEV)
    kl = torch.tensor(klens, dtype=torch.int32, device=DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), B, T, None, 0, None,
                                out.data_ptr(), D, M * D, H, dh, dh ** -0.5, mode, 0, None, kl.data_ptr(), None, 0, stream()))
    torch.cuda.synchronize()
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 1e-4), err


@pytest.mark.parametrize("mode", [1, 2])
def test_embed_ln(L, mode):
    B, T, D, V, pad = 3, 20, 128, 50, 1
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(2, V, (B, T), generator=g)
    ids[1, 12:] = pad
    ids[2, 3:] = pad
    w, pe, te = torch.randn(V, D, generator=g), torch.randn(T + 2, D, generator=g), torch.randn(D, generator=g)
    lw, lb = torch.randn(D, generator=g), torch.randn(D, generator=g)
    m = (ids != pad).long()
    pos = torch.cumsum(m, 1) * m + pad
    ref = torch.nn.functional.layer_norm((w[ids] + pe[pos] + te).double(), (D,), lw.double(), lb.double(), 1e-5).view(B * T, D)
    idd = ids.to(torch.int32).to(DEV)
    of = torch.empty(B * T, D, device=DEV)
    planes = 2 if mode == 2 else 1
    oa = torch.empty(planes, B * T, D, dtype=torch.bfloat16, device=DEV)
    wd, ped, ted, lwd, lbd = (t.to(DEV) for t in (w, pe, te, lw, lb))
    L.check(L.lib.ser_embed_ln(idd.data_ptr(), wd.data_ptr(), ped.data_ptr(), ted.data_ptr(), lwd.data_ptr(), lbd.data_ptr(),
                               1e-5, of.data_ptr(), oa.data_ptr(), B * T * D, mode, B, T, D, pad, stream()))
    torch.cuda.synchronize()
    assert (of.cpu().double() - ref).abs().max().item() < 2e-5
    assert (act_value(oa).cpu().double() - ref).abs().max().item() < mode_tol(mode, 4e-2, 1e-4)


def test_attention_online_softmax_rescale(L):
    """A key in a late tile dominates: forces the running-max rescale branch (one spike per head)."""
    T, H, dh = 300, 1, 64
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(T, 3 * dh, generator=g) * 0.5
    qkv[250, dh:2 * dh] = qkv[10, :dh] * 30           # key 250 aligned with query 10
    qa = to_act(qkv, 2)
    qv = act_value(qa).cpu().double()
    q, k, v = (qv[:, i * dh:(i + 1) * dh].view(T, 1, dh).permute(1, 0, 2) for i in range(3))
    ref = attention_reference(q, k, v, dh ** -0.5)[0]
    out = torch.zeros(2, T, dh, dtype=torch.bfloat16, device=DEV)
    foffs = torch.tensor([0, T], dtype=torch.int32, device=DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * dh, T * 3 * dh, 0, dh, 2 * dh, foffs.data_ptr(), 1, T, None, 0, None,
                                out.data_ptr(), dh, T * dh, H, dh, dh ** -0.5, 2, 0, None, None, None, 0, stream()))
    torch.cuda.synchronize()
    assert (act_value(out).cpu().double() - ref).abs().max().item() < 1e-4


def test_mean4_and_split(L):
    n = 1000
    g = torch.Generator().manual_seed(4)
    s = [torch.randn(n, generator=g) for _ in range(4)]
    d = [t.to(DEV) for t in s]
    out = torch.empty(n, device=DEV)
    L.check(L.lib.ser_mean4(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out.data_ptr(), n, stream()))
    assert torch.equal(out.cpu(), torch.stack(s).mean(0)) or (out.cpu() - torch.stack(s).mean(0)).abs().max() < 1e-7
    x = torch.randn(777, generator=g)
    xo = torch.empty(2, 777, dtype=torch.bfloat16, device=DEV)
    xd = x.to(DEV)
    L.check(L.lib.ser_split_bf16(xd.data_ptr(), xo.data_ptr(), 777, 2, 777, stream()))
    ref = to_act(x[None], 2)[:, 0]
    assert torch.equal(xo.cpu(), ref.cpu())


def test_logmel_whisper(L, golden_dir):
    from interspeech_ser_amd.frontend import whisper_mel_filters
    from oracle import ssl_oracle as O
    lens = [16000, 100000, 500000]
    rng = np.random.default_rng(3)
    waves = [np.clip(0.1 * rng.standard_normal(n) + 0.2 * np.sin(2 * np.pi * 220 * np.arange(n) / 16000), -1, 1).astype(np.float32)
             for n in lens]
    packed = torch.from_numpy(np.concatenate(waves)).to(DEV)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    mel = torch.from_numpy(whisper_mel_filters(128)).to(DEV)
    B = len(lens)
    out = torch.empty(B, 128, 3000, device=DEV)
    ws = L.lib.ser_workspace_bytes(L.WS_LOGMEL, B, 0, 0, 0, 1)
    work = torch.empty(ws, dtype=torch.uint8, device=DEV)
    L.check(L.lib.ser_logmel_init(work.data_ptr(), B, stream()), "ser_logmel_init")          # twiddle table: once per work buffer
    L.check(L.lib.ser_logmel_whisper(packed.data_ptr(), offs.data_ptr(), B, mel.data_ptr(), 128, out.data_ptr(),
                                     work.data_ptr(), stream()))
    got = out.cpu().numpy()
    for b, w in enumerate(waves):
        ref = O.whisper_log_mel(w, 128)
        assert np.abs(got[b] - ref).max() < 1e-3, np.abs(got[b] - ref).max()


@pytest.mark.parametrize("step,mult,div", [(2, 512, 8), (1, 1, 1), (1, 1024, 8), (5, 64, 8)])
def test_ragged_index_tables_match_numpy(L, step, mult, div):
    """ser_ragged_index == the host-side table it replaces (implicit-conv row offsets, halo map)."""
    rng = np.random.default_rng(step * 7 + mult)
    counts = rng.integers(1, 700, size=37)
    counts[5] = 1
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    base = (rng.integers(0, 100000, size=37)).astype(np.int64)
    want = np.concatenate([(base[b] + step * np.arange(counts[b], dtype=np.int64)) * mult // div for b in range(37)]).astype(np.int32)
    d_offs, d_base = torch.from_numpy(offs).to(DEV), torch.from_numpy(base).to(DEV)
    out = torch.full((int(offs[-1]) + 3,), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib.ser_ragged_index(d_offs.data_ptr(), d_base.data_ptr(), 37, step, mult, div, out.data_ptr(), int(offs[-1]),
                                   torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    assert np.array_equal(got[:-3], want) and (got[-3:] == -7).all()


def test_gemm_deep_k_dispatch_is_exact(L):
    """Auto dispatch of a deep-K, narrow-N launch (the FC2 shape class -> 256x128 tiles): integer-exact like every
    forced configuration."""
    M, N, K = 777, 384, 2048
    g = torch.Generator().manual_seed(5)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    out, _ = run_gemm(L, to_act(A, 1), to_act(W, 1), M, N, K, 1, bias=bias.to(DEV))
    assert torch.equal(out.cpu().double(), A.double() @ W.double().T + bias.double())


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("T", [80, 200])
def test_deberta_dense_bias_attention(L, mode, T):
    """DeBERTa's disentangled attention on the matrix cores: ser_deberta_bias (dense c2p + p2c bias per (sequence, head))
    + ser_attention(bias2d) against an fp64 statement of softmax((Qc Kc^T + c2p + p2c) / sqrt(3 dh)) V with HF's both-token
    mask (a padded query row = the uniform average of all T value rows), and -- at T <= 128 -- against the
    one-thread-per-query kernel ser_deberta_attention it replaces on the encoder path.  T = 200 has no counterpart there."""
    B, H, dh, Nr = 3, 2, 64, 40
    D, M = H * dh, B * T
    g = torch.Generator().manual_seed(T + mode)
    qkv = torch.randn(M, 3 * D, generator=g)
    lens = [T, max(1, T // 3), 5][:B]
    c2p = torch.randn(M, H * Nr, generator=g) * 0.5
    p2c = torch.randn(M, H * Nr, generator=g) * 0.5
    ci = torch.randint(0, Nr, (2 * T - 1,), generator=g, dtype=torch.int32)
    pi = torch.randint(0, Nr, (2 * T - 1,), generator=g, dtype=torch.int32)
    scale = 1.0 / math.sqrt(3.0 * dh)
    s2 = scale * 1.4426950408889634
    qa_raw = to_act(qkv, mode)
    qv = act_value(qa_raw).cpu().double()
    ref = torch.empty(M, D, dtype=torch.float64)
    idx = torch.arange(T)
    for b in range(B):
        n = lens[b]
        blk = qv[b * T:(b + 1) * T]
        for h in range(H):
            q, k, v = (blk[:, i * D + h * dh: i * D + (h + 1) * dh] for i in range(3))
            cq = c2p[b * T:(b + 1) * T, h * Nr:(h + 1) * Nr].double()
            pk = p2c[b * T:(b + 1) * T, h * Nr:(h + 1) * Nr].double()
            s = q @ k.T
            s = s + torch.gather(cq, 1, ci[(idx[:, None] - idx[None, :]) + T - 1].long())                       # c2p[q][ci[q-k]]
            s = s + torch.gather(pk, 1, pi[(idx[:, None] - idx[None, :]) + T - 1].long()).T                     # p2c[k][pi[k-q]]
            s = s * scale
            real = (idx[:, None] < n) & (idx[None, :] < n)
            s = torch.where(real, s, torch.full_like(s, torch.finfo(torch.float32).min))
            ref[b * T:(b + 1) * T, h * dh:(h + 1) * dh] = torch.softmax(s, dim=-1) @ v
    planes = 2 if mode == 2 else 1
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    cid, pid = ci.to(DEV), pi.to(DEV)
    c2p_d, p2c_d, c2p_s = c2p.to(DEV), p2c.to(DEV), (c2p * s2).to(DEV)            # keep the device copies alive across the launches
    if T <= 128:
        out_old = torch.zeros(planes, M, D, dtype=torch.bfloat16, device=DEV)
        L.check(L.lib.ser_deberta_attention(qa_raw.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, c2p_d.data_ptr(), p2c_d.data_ptr(),
                                            H * Nr, Nr, cid.data_ptr(), pid.data_ptr(), kl.data_ptr(), out_old.data_ptr(), D, M * D,
                                            B, T, H, dh, mode, stream()), "ser_deberta_attention")
        torch.cuda.synchronize()
        assert (act_value(out_old).cpu().double() - ref).abs().max() < mode_tol(mode, 3e-2, 1e-4)
    # new path: q pre-scaled (as the QKV GEMM's col_scale does), c2p from that q
    qkv_s = qv.clone().float()
    qkv_s[:, :D] *= s2
    qa = to_act(qkv_s, mode)
    ld = (T + 63) // 64 * 64
    bias = torch.full((B, H, T, ld), float("nan"), device=DEV)
    L.check(L.lib.ser_deberta_bias(c2p_s.data_ptr(), p2c_d.data_ptr(), H * Nr, Nr, cid.data_ptr(), pid.data_ptr(),
                                   kl.data_ptr(), bias.data_ptr(), ld, B, T, H, s2, stream()), "ser_deberta_bias")
    out = torch.zeros(planes, M, D, dtype=torch.bfloat16, device=DEV)
    foffs = torch.arange(0, M + 1, T, dtype=torch.int32, device=DEV)
    L.check(L.lib.ser_attention(qa.data_ptr(), 3 * D, M * 3 * D, 0, D, 2 * D, foffs.data_ptr(), B, T, None, 0, None,
                                out.data_ptr(), D, M * D, H, dh, -1.0, mode, 0, None, kl.data_ptr(), bias.data_ptr(), ld, stream()),
            "ser_attention")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(bias).all())
    err = (act_value(out).cpu().double() - ref).abs().max().item()
    assert err < mode_tol(mode, 3e-2, 2e-4), err


@pytest.mark.parametrize("Cn", [80, 128, 36])                 # Whisper's mel counts, and a channel count that is a multiple of 4 but not of 8
@pytest.mark.parametrize("mode", [1, 2, 4])                   # bf16, bf16 hi + lo (fp32x), fp16 hi + lo (fp16x)
def test_pack_act_channels_last_against_numpy(L, mode, Cn):
    """ser_pack_act_v (OP_PACK_ACT, the first command of Whisper's list): [B, C, T] fp32 -> channels-last operand rows, utterance b at rows
    b (T + 2 halo) .., its halo rows written as zeros by the kernel itself (planted garbage before the launch), columns C .. ldo and
    rows past the last utterance untouched; the planes bit for bit those of numpy's transpose rounded to nearest even, and the range
    guard's bits (fp16 planes only) those of the largest |x|.  Modes it does not write are refused with the buffer untouched."""
    B, T, halo, EXTRA = 3, 3000, 1, 5
    ldo, Tp = Cn + 4, T + 2 * halo
    g = torch.Generator().manual_seed(Cn + mode)
    x = torch.randn(B, Cn, T, generator=g) * torch.logspace(-4, 1, T)[None, None, :]
    x[1, Cn - 1, T - 1] = 4.0e4                                          # past half of fp16's range: guard bit 1
    planes, dt = (1, torch.bfloat16) if mode == 1 else ((2, torch.bfloat16) if mode == 2 else (2, torch.float16))
    xt = x.permute(0, 2, 1)                                              # [B, T, C]
    hi = xt.to(dt)
    lo = (xt - hi.float()).to(dt)
    want = torch.zeros(planes, B, Tp, Cn, dtype=dt)
    want[0, :, halo:halo + T] = hi
    if planes == 2:
        want[1, :, halo:halo + T] = lo
    xd = x.to(DEV).contiguous()
    R_ = B * Tp + EXTRA
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch(m):
        out = torch.full((planes, R_, ldo), -3, dtype=torch.int16, device=DEV)      # planted: garbage halo rows, pitch tail, spare rows
        a = L.PackActArgs()
        a.x, a.out, a.ldo, a.out_plane_stride = xd.data_ptr(), out.data_ptr(), ldo, R_ * ldo
        a.B, a.C, a.T, a.halo, a.mode, a.range_flag = B, Cn, T, halo, m, flag.data_ptr()
        rc = L.lib.ser_pack_act_v(C.byref(a), stream())
        torch.cuda.synchronize()
        return rc, out.cpu()

    rc, out = launch(mode)
    assert rc == 0, L.lib.ser_last_error()
    got = out[:, :B * Tp, :Cn].reshape(planes, B, Tp, Cn)
    assert torch.equal(got, want.view(torch.int16))                    # bit patterns: a -0.0 for +0.0 is a difference too
    assert bool((out[:, :, Cn:] == -3).all()) and bool((out[:, B * Tp:] == -3).all())
    assert int(flag.item()) == (2 if dt == torch.float16 else 0)
    x[1, Cn - 1, T - 1] = 7.0e4                                          # beyond fp16's range: both bits (saturated in the fp16 plane)
    xd.copy_(x.to(DEV))
    flag.zero_()
    rc, out = launch(mode)
    assert rc == 0 and int(flag.item()) == (3 if dt == torch.float16 else 0)
    for bad in (3, 5, 6):                                                # FP16, FP16Q, FP16M: not written by this kernel
        flag.zero_()
        rc, out = launch(bad)
        assert rc < 0 and f"ser_pack_act: mode {bad} ".encode() in L.lib.ser_last_error()
        assert bool((out == -3).all()) and int(flag.item()) == 0


@pytest.mark.parametrize("mode", [2, 4])                       # the 3-product modes: bf16 hi + lo (fp32x), fp16 hi + lo (fp16x)
def test_gemm_stat_out_writes_every_slot_it_covers(L, mode):
    """Row partials (stat_out) of the 3-product 256x256 tile, whose waves cover 128 columns each -- what the output projection of Whisper-large
    runs on at M = 12 000, N = 1 280: every 64-column slot of the N columns is written (the wave's partials in the first of its two slots, a
    zero in the second) and the slots add up to the row sums of the values written.  Each slot starts as a planted NaN; the slots past the
    N columns keep it.  A slot the launch left alone handed the consumer's LayerNorm whatever an earlier launch had put there: with the
    FP16M context rows (SER_F16M_OUT_M=1) the FP16M output projections of the later layers fill it, and from the second forward on the
    first layers' LayerNorm read it (Whisper-large-v3, "f16mf": 0.57 from the oracle)."""
    M, N, K, G = 12000, 1280, 128, 22                              # 235 tiles of 256 x 256: the tile the launcher picks; 2 padding slots
    g = torch.Generator().manual_seed(90 + mode)
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    res = torch.randn(M, N, generator=g) + 0.5

    def planes(x):
        if mode == 2:
            return to_act(x, 2)
        h = x.half()
        return torch.stack([h, (x - h.float()).half()]).contiguous().to(DEV)
    stat = torch.full((M, G, 2), float("nan"), device=DEV)
    out, _ = run_gemm(L, planes(A), planes(W), M, N, K, mode, residual=res.to(DEV), ldr=N, stat_out=stat)
    st = stat.cpu().double()
    assert not bool(st[:, :N // 64].isnan().any())                 # every slot of the N columns written ...
    assert bool(st[:, N // 64:].isnan().all())                     # ... none past them
    x = out.cpu().double()
    s = st[:, :N // 64].sum(1)
    assert float(((s[:, 0] - x.sum(1)).abs() / x.abs().sum(1)).max()) < 1e-5
    assert float(((s[:, 1] - (x * x).sum(1)).abs() / (x * x).sum(1)).max()) < 1e-5
