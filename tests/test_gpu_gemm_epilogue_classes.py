"""ser_gemm's epilogue classes (csrc/launch_plan.h: gemm_pick_epi) against its GENERIC epilogue, bit for bit.  -m gpu.

A launch that fits the LN_ACT class (packed projection, FC1) or the RESID class (output projection, FC2) runs a kernel compiled without the
epilogue features the class never has.  Every such launch is repeated on the same data with one INERT extra feature that the class does not
admit, so that the plan sends it to the GENERIC kernel:
    LN_ACT -> an out_f32 buffer with f32_col_begin >= N (no column is stored; the buffer must come back untouched),
    RESID  -> col_scale = 1.0 over all columns.
Every output buffer of the two launches must be torch.equal: operand copy (FP16M: both planes and the block scales), fp32 output, row
partials, shift_out, mean_out, lnstat_out, range_flag.  That the two launches took different kernels is asked of the plan itself:
``launch_plan_check --epi`` (plain g++ build of the same launch_plan.h) prints the class of each argument set.

Shapes, per hot tile BM x BN (tile_cfg 1, 2, 3): M = BM + 16 (two row tiles, the second ragged), N = BN + 64 (a ragged last column tile)
or N = 3 BN with col_scale_end = BN (tiles wholly inside / outside the scaled columns), col_scale_end = 72 (a tile the boundary cuts:
the per-lane test), K = 64 (one K tile) and K = 192 (more tiles than ring stages); bf16, fp16 and FP16M operands (FP16M also with the
FP16X operand copy).
"""
import ctypes as C
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interspeech_ser_amd", "csrc")
BF16, FP16, FP16X, FP16M = 1, 3, 4, 6
GELU = 1
TILES = {1: (128, 128), 2: (256, 128), 3: (256, 256)}
# the members of ser_gemm_args that launch_plan_check reads (launch_plan_check.cc: GEMM_FIELDS), pointers as 0 / 1
PLAN_PTRS = ("A", "a_rowoff", "W", "residual", "out_f32", "out_act", "ln_gamma", "ln_beta", "ln_stats_in", "ln_colsum", "stat_out", "shift_out",
             "mean_out", "lnstat_out", "a_scale", "w_scale", "out_scale", "gn_scale", "gn_shift", "gn_row_offs")
PLAN_INTS = ("lda", "kc", "M", "N", "K", "groups", "c_group_stride", "mode", "act", "ldr", "ldo_f32", "ldo_act", "tile_cfg", "ln_groups",
             "stat_groups", "f32_col_begin", "col_scale_end", "out_mode", "a_scale_ld", "w_scale_ld", "gn_B", "gn_ld")


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


@pytest.fixture(scope="module")
def plan_check():
    subprocess.check_call(["make", "-C", CSRC, "plan_check"], stdout=subprocess.DEVNULL)
    return os.path.join(CSRC, "build", "plan_check", "launch_plan_check")


def stream():
    return torch.cuda.current_stream().cuda_stream


def plan_line(g):
    f = [f"{n}={1 if getattr(g, n) else 0}" for n in PLAN_PTRS] + [f"{n}={int(getattr(g, n))}" for n in PLAN_INTS]
    return "gemm " + " ".join(f)


def classes_of(plan_check, lines):
    r = subprocess.run([plan_check, "--epi"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return [dict(kv.split("=") for kv in o.split() if "=" in kv)["epi"] if " err " not in o else o for o in out], [o.split()[1] for o in out]


class Operands:
    """A [M, K] and W [N, K] in `mode`'s operand format, and what every case of one (mode, tile, K) shares."""

    def __init__(self, L, mode, M, N, K, seed):
        g = torch.Generator().manual_seed(seed)
        self.mode, self.M, self.N, self.K = mode, M, N, K
        a = torch.randn(M, K, generator=g) + 0.25
        w = torch.randn(N, K, generator=g) / K ** 0.5
        self.a_scale = self.w_scale = None
        if mode == FP16M:
            self.A, self.a_scale = self.pack(L, a, False)
            self.W, self.w_scale = self.pack(L, w, True)
        else:
            dt = torch.bfloat16 if mode == BF16 else torch.float16
            self.A, self.W = a.to(dt)[None].contiguous().to(DEV), w.to(dt)[None].contiguous().to(DEV)
        self.bias = torch.randn(N, generator=g).to(DEV)
        self.colsum = torch.randn(N, generator=g).to(DEV)
        stats = torch.zeros(M, 2, 2)
        stats[:, 0, 0], stats[:, 0, 1] = a.sum(1), (a * a).sum(1)            # (sum, sum of squares) of the rows: a plausible mean / rstd
        self.stats = stats.to(DEV)
        self.ln_shift = torch.randn(M, generator=g).to(DEV)
        self.residual = (torch.randn(M, N, generator=g) * 2 + 0.7).to(DEV)
        self.shift_in = torch.randn(M, generator=g).to(DEV)

    @staticmethod
    def pack(L, x, weight):
        rows, cols = x.shape
        xd = x.to(DEV).contiguous()
        out = torch.zeros((2, rows, cols), dtype=torch.float16, device=DEV)
        sc = torch.zeros((cols // 64, rows), dtype=torch.int32, device=DEV)
        L.check(L.lib.ser_pack_f16m(xd.data_ptr(), cols, rows, cols, out.data_ptr(), cols, rows * cols, sc.data_ptr(), rows, int(weight),
                                    None, stream()), "ser_pack_f16m")
        return out, sc


def launch(L, op, cfg, lines, *, ln=False, act=0, col_scale=0.0, col_scale_end=0, residual=False, in_place=False, res_row_mod=0,
           want_f32=False, f32_col_begin=0, want_act=False, stats=False, shift=False, out_mode=0):
    """One ser_gemm launch on `op`; returns its output buffers by name.  Appends the launch's plan_check line to `lines`."""
    M, N, K, mode = op.M, op.N, op.K, op.mode
    keep = []                                                   # buffers the argument struct points to
    g = L.GemmArgs()
    g.A, g.a_plane_stride, g.lda = op.A.data_ptr(), M * K, K
    g.W, g.w_plane_stride = op.W.data_ptr(), N * K
    g.M, g.N, g.K, g.groups, g.mode, g.tile_cfg, g.act = M, N, K, 1, mode, cfg, act
    g.c_group_stride = N
    g.bias = op.bias.data_ptr()
    if mode == FP16M:
        g.a_scale, g.a_scale_ld, g.w_scale, g.w_scale_ld = op.a_scale.data_ptr(), M, op.w_scale.data_ptr(), N
    out = {}
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    g.range_flag = flag.data_ptr()
    out["range_flag"] = flag
    if ln:
        g.ln_stats_in, g.ln_groups, g.ln_colsum, g.ln_eps = op.stats.data_ptr(), 2, op.colsum.data_ptr(), 1e-5
        out["mean_out"] = torch.full((M,), -7.0, device=DEV)
        out["lnstat_out"] = torch.full((M, 2), -7.0, device=DEV)
        g.ln_shift, g.mean_out, g.lnstat_out = op.ln_shift.data_ptr(), out["mean_out"].data_ptr(), out["lnstat_out"].data_ptr()
    g.col_scale, g.col_scale_end = col_scale, col_scale_end
    if residual:
        res = op.residual.clone()
        keep.append(res)
        g.residual, g.ldr, g.res_row_mod = res.data_ptr(), N, res_row_mod
        if in_place:                                            # the encoder layers' residual GEMMs write the state they read
            out["out_f32"] = res
    if want_f32 and "out_f32" not in out:
        out["out_f32"] = torch.full((M, N), -7.0, device=DEV)
    if "out_f32" in out:
        g.out_f32, g.ldo_f32, g.f32_col_begin = out["out_f32"].data_ptr(), N, f32_col_begin
    if want_act:
        planes = 2 if mode == FP16M or out_mode == FP16X else 1
        g.out_mode = out_mode
        out["out_act"] = torch.zeros((planes, M, N), dtype=torch.bfloat16 if mode == BF16 else torch.float16, device=DEV)
        g.out_act, g.ldo_act, g.out_plane_stride = out["out_act"].data_ptr(), N, M * N
        if mode == FP16M and not out_mode:
            out["out_scale"] = torch.zeros((N // 64, M), dtype=torch.int32, device=DEV)
            g.out_scale, g.out_scale_ld = out["out_scale"].data_ptr(), M
    if stats:
        G = (N + 63) // 64
        G += G & 1
        out["stat_out"] = torch.full((M, G, 2), -7.0, device=DEV)
        g.stat_out, g.stat_groups = out["stat_out"].data_ptr(), G
    if shift:
        out["shift_out"] = torch.full((M,), -7.0, device=DEV)
        g.shift_in, g.shift_out, g.shift_const = op.shift_in.data_ptr(), out["shift_out"].data_ptr(), 0.375
    lines.append(plan_line(g))
    L.check(L.lib.ser_gemm(C.byref(g), stream()), "ser_gemm")
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)      # (an FP16M cross-term plane read as fp16 holds NaN patterns)


def same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs between the class kernel and GENERIC"


@pytest.mark.parametrize("cfg", [1, 2, 3])
@pytest.mark.parametrize("mode", [BF16, FP16, FP16M])
def test_class_kernels_match_generic_bit_for_bit(L, plan_check, mode, cfg):
    BM, BN = TILES[cfg]
    M = BM + 16
    lines, want, names = [], [], []

    def pair(op, cls, what, **kw):
        got = launch(L, op, cfg, lines, **kw)
        if cls == "LN_ACT":      # inert: an fp32 output that receives no column
            ref = launch(L, op, cfg, lines, want_f32=True, f32_col_begin=(op.N + 7) // 8 * 8, **kw)
            f32 = ref.pop("out_f32")
            assert torch.equal(f32, torch.full_like(f32, -7.0)), f"{what}: the inert fp32 buffer was written"
        else:                    # inert: every column scaled by 1.0
            ref = launch(L, op, cfg, lines, col_scale=1.0, col_scale_end=op.N, **kw)
        wrote = got["out_f32"] if cls == "RESID" else got["out_act"][0]
        assert float(wrote.float().abs().max()) > 0.1, what                  # (the launch wrote something)
        same(got, ref, what)
        want.extend([cls, "GENERIC"])
        names.extend([what, what + " (forced generic)"])

    for K in (64, 192):
        op = Operands(L, mode, M, BN + 64, K, seed=100 * cfg + K + mode)
        pair(op, "LN_ACT", f"FC1 form K={K}", ln=True, act=GELU, want_act=True)
        pair(op, "LN_ACT", f"no GELU, no scale K={K}", ln=True, want_act=True)
        pair(op, "LN_ACT", f"scale boundary inside a tile K={K}", ln=True, want_act=True, col_scale=0.18, col_scale_end=72)
        pair(op, "LN_ACT", f"GELU and scale K={K}", ln=True, act=GELU, want_act=True, col_scale=0.18, col_scale_end=BN)
        pair(op, "RESID", f"producer form K={K}", residual=True, in_place=True, want_act=True, stats=True, shift=True)
        pair(op, "RESID", f"unshifted copy K={K}", residual=True, want_f32=True, want_act=True, stats=True)
        pair(op, "RESID", f"fp32 only, row-mod residual K={K}", residual=True, want_f32=True, res_row_mod=M - 3)
        op3 = Operands(L, mode, M, 3 * BN, K, seed=100 * cfg + K + mode + 1)
        pair(op3, "LN_ACT", f"packed projection form K={K}", ln=True, want_act=True, col_scale=0.18, col_scale_end=BN)
        if mode == FP16M:       # the converting pair of "f16m" / "f16mf": fp16 hi + lo planes out of FP16M operands
            pair(op3, "LN_ACT", f"packed projection form, FP16X copy K={K}", ln=True, want_act=True, col_scale=0.18, col_scale_end=BN, out_mode=FP16X)
            pair(op, "RESID", f"producer form, FP16X copy K={K}", residual=True, in_place=True, want_act=True, stats=True, shift=True, out_mode=FP16X)
    got, tiles = classes_of(plan_check, lines)
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert set(tiles) == {f"{BM}x{BN}"}, set(tiles)
