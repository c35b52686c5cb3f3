"""fp16 range guard, kernel by kernel (-m gpu).  Every producer that rounds values to an fp16 operand plane (the FP16 / FP16X / FP16M formats)
ORs into a device word (ser_hip.h, ser_gemm_args.range_flag): bit 1 if a stored value exceeds 65504 / 2 in magnitude, bits 0 and 1 if one
exceeds 65504 or is a NaN / Inf.  The drivers fail a batch's files on that word, so a wrong bit either writes clipped features silently or
discards good ones.  Each test plants one value, runs the launch through the C ABI with a zeroed word and compares the word with the bits a
plain float64 restatement of the values the launch STORES demands; values the launch computes but never stores (tail columns of the last
column tile, padding beyond the row) must not count.  The same launch with range_flag = NULL must store the same bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import f16m_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP16, FP16X, FP16M = 3, 4, 6
F16_MAX = 65504.0
HALF, OVER = 0.75 * F16_MAX, 1.5 * F16_MAX        # planted magnitudes, clear of both thresholds
PLANTS = ["small", "half", "over", "nan", "inf", "masked"]


@pytest.fixture(scope="module")
def L():
    from interspeech_ser_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def expected_bits(stored: torch.Tensor) -> int:
    """the guard's contract on the float64 values a launch stores into an fp16 plane"""
    v = stored.double()
    if not bool(torch.isfinite(v).all()):
        return 3
    amax = float(v.abs().max()) if v.numel() else 0.0
    return 3 if amax > F16_MAX else (2 if amax > 0.5 * F16_MAX else 0)


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def planted(kind: str) -> float:
    return {"half": HALF, "over": OVER, "nan": float("nan"), "inf": float("inf")}[kind]


def run_flagged(launch):
    """launch(flag_ptr) -> tuple of output tensors; runs it with a zeroed word and with NULL, returns (bits, outputs of the flagged run)"""
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = launch(flag.data_ptr())
    torch.cuda.synchronize()
    bits = int(flag.item())
    plain = launch(None)
    torch.cuda.synchronize()
    for a, b in zip(got, plain):
        assert same_bytes(a, b), "range_flag changed what the launch stores"
    return bits, got


# ------------------------------------------------------------------------------------------------------------------------------- ser_gemm
def planes(x: torch.Tensor, mode: int):
    """fp32 CPU [R, C] -> (device planes [P, R, C] fp16, scales or None): FP16 one plane, FP16X hi + lo, FP16M tests/f16m_ref.pack"""
    if mode == FP16M:
        raise AssertionError("use pack_m")
    hi = x.to(torch.float16)
    if mode == FP16:
        return hi[None].contiguous().to(DEV)
    lo = (x - hi.float()).to(torch.float16)
    return torch.stack([hi, lo]).contiguous().to(DEV)


def pack_m(L, x: torch.Tensor, weight: bool):
    rows, cols = x.shape
    xd = x.to(DEV).contiguous()
    out = torch.zeros((2, rows, cols), dtype=torch.float16, device=DEV)
    sc = torch.zeros((cols // 64, rows), dtype=torch.int32, device=DEV)
    L.check(L.lib.ser_pack_f16m(xd.data_ptr(), cols, rows, cols, out.data_ptr(), cols, rows * cols, sc.data_ptr(), rows, int(weight),
                                None, stream()), "ser_pack_f16m")
    torch.cuda.synchronize()
    return out, sc


def gelu(x):
    return torch.nn.functional.gelu(x)


def gemm_case(L, *, mode, out_mode, path, cfg, M, N, K, plant):
    """One ser_gemm launch whose stored out_act values the host knows in float64.  Operands are small integers (exact in every format);
    columns 0..3 of A are 1.  Plants:  a stored column c0 gets a large / NaN / Inf value through the path's additive term (bias, LayerNorm
    beta, GroupNorm shift);  "masked": W row N - 1 = 30000 on those 4 columns, and its bias cancels that, so stored column N - 1 is small
    while the tail columns past N (the clamped row N - 1, bias 0) hold 120 000.  Deferred LayerNorm: rows with mean ~40 and W row N - 1
    constant 30, so column N - 1 is rstd * (x . w - mu * colsum) = 0 while a tail column, rstd * x . w, is ~9e4."""
    om = out_mode or mode
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K + cfg + mode)
    A = torch.randint(-2, 3, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()
    bias = torch.randint(-3, 4, (N,), generator=g).float()
    A[:, :4] = 1.0
    W[:, :4] = 0.0
    c0 = 8
    if path == "deferred":
        A = 40.0 + torch.randint(-1, 2, (M, K), generator=g).float()
    if plant == "masked":
        if path == "deferred":
            W[N - 1] = 30.0
            bias[N - 1] = 0.0
        else:
            W[N - 1, :4] = 30000.0
            W[N - 1, 4:] = 0.0
            bias[N - 1] = -120000.0
    kw = {}
    Ad = Wd = As = Ws = None
    if mode == FP16M:
        Ad, As = pack_m(L, A, False)
        Wd, Ws = pack_m(L, W, True)
    else:
        Ad, Wd = planes(A, mode), planes(W, mode)
    acc = A.double() @ W.double().T
    ln_g = ln_b = None
    if path == "ln":
        ln_g = 1.0 + torch.randint(0, 3, (N,), generator=g).float()
        ln_b = torch.randint(-3, 4, (N,), generator=g).float()
        if plant in ("half", "over", "inf"):
            ln_b[c0] = planted(plant)
        elif plant == "nan":
            ln_g[c0] = float("nan")
        x = acc + bias.double()
        ref = torch.nn.functional.layer_norm(x, (N,), ln_g.double(), ln_b.double(), 1e-5)
        ref = gelu(ref)
        kw["act"] = 1
    else:
        if plant in ("half", "over", "nan", "inf"):
            bias[c0] = planted(plant)
        x = acc + bias.double()
        if path == "deferred":
            mu = A.double().mean(1, keepdim=True)
            rs = 1.0 / torch.sqrt(A.double().var(1, unbiased=False, keepdim=True) + 1e-5)
            colsum = W.double().sum(1)
            x = rs * (acc - mu * colsum[None, :]) + bias.double()[None, :]
            G = 2
            st = torch.zeros(M, G, 2)
            st[:, 0, 0] = A.double().sum(1).float()
            st[:, 0, 1] = (A.double() ** 2).sum(1).float()
            kw["ln_stats"], kw["ln_groups"], kw["ln_colsum"] = st.to(DEV), G, colsum.float().to(DEV)
        if path == "gn":
            # two utterances of the batch; the planted shift sits in the second one only
            offs = [0, M // 3, M]
            gsc = 1.0 + torch.randint(0, 2, (2, N), generator=g).float()
            gsh = torch.randint(-2, 3, (2, N), generator=g).float()
            if plant in ("half", "over", "nan", "inf"):
                bias[c0] = 1.0
                gsh[1, c0] = planted(plant)
                x = acc + bias.double()
            u = torch.zeros(M, dtype=torch.long)
            u[offs[1]:] = 1
            x = x * gsc.double()[u] + gsh.double()[u]
            kw["gn"] = (gsc.to(DEV), gsh.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV))
        if path == "colscale":
            x = x.clone()
            x[:, :64] *= 0.5
            kw["col_scale"] = (0.5, 64)
        ref = x
        if path == "plain":
            ref = gelu(x)
            res = torch.randint(-3, 4, (M, N), generator=g).float()
            ref = ref + res.double()
            kw["act"], kw["residual"] = 1, res.to(DEV)
    rowmap = None
    if path == "rowmap":
        rowmap = torch.randperm(M, generator=g).to(torch.int32)
    stored = ref[:M, :N]
    bd = bias.to(DEV)
    lnd = (ln_g.to(DEV), ln_b.to(DEV)) if path == "ln" else None

    def launch(flag):
        a = L.GemmArgs()
        a.A, a.a_plane_stride, a.lda = Ad.data_ptr(), Ad.shape[1] * Ad.shape[2], K
        a.W, a.w_plane_stride = Wd.data_ptr(), Wd.shape[1] * Wd.shape[2]
        a.M, a.N, a.K, a.groups, a.mode, a.tile_cfg = M, N, K, 1, mode, cfg
        if mode == FP16M:
            a.a_scale, a.a_scale_ld, a.w_scale, a.w_scale_ld = As.data_ptr(), M, Ws.data_ptr(), N
        if path == "ln":
            a.ln_gamma, a.ln_beta, a.ln_eps = lnd[0].data_ptr(), lnd[1].data_ptr(), 1e-5
        a.bias = bd.data_ptr()
        a.act = kw.get("act", 0)
        if "residual" in kw:
            a.residual, a.ldr = kw["residual"].data_ptr(), N
        if "ln_stats" in kw:
            a.ln_stats_in, a.ln_groups, a.ln_colsum, a.ln_eps = kw["ln_stats"].data_ptr(), kw["ln_groups"], kw["ln_colsum"].data_ptr(), 1e-5
        if "gn" in kw:
            gs, gh, go = kw["gn"]
            a.gn_scale, a.gn_shift, a.gn_row_offs, a.gn_B, a.gn_ld = gs.data_ptr(), gh.data_ptr(), go.data_ptr(), 2, N
        if "col_scale" in kw:
            a.col_scale, a.col_scale_end = kw["col_scale"]
        out = torch.full((M, N), float("nan"), device=DEV)
        a.out_f32, a.ldo_f32 = out.data_ptr(), N
        oa = torch.zeros((2 if om in (FP16X, FP16M) else 1, M, N), dtype=torch.float16, device=DEV)
        a.out_act, a.ldo_act, a.out_plane_stride, a.out_mode = oa.data_ptr(), N, M * N, out_mode
        osc = torch.zeros((N // 64 if om == FP16M else 1, M), dtype=torch.int32, device=DEV)
        if om == FP16M:
            a.out_scale, a.out_scale_ld = osc.data_ptr(), M
        rm = None
        if rowmap is not None:
            rm = rowmap.to(DEV)
            a.out_rowmap = rm.data_ptr()
        a.range_flag = flag
        L.check(L.lib.ser_gemm(C.byref(a), stream()), "ser_gemm")
        torch.cuda.synchronize()
        return out, oa, osc

    bits, (out, oa, osc) = run_flagged(launch)
    return bits, expected_bits(stored), stored, out, oa, osc, rowmap


GEMM_CASES = [
    # (mode, out_mode, path, cfg, M, N, K)
    (FP16, 0, "plain", 1, 300, 200, 64),
    (FP16, 0, "plain", 2, 300, 392, 128),
    (FP16, 0, "plain", 3, 515, 200, 64),
    (FP16, FP16X, "plain", 1, 300, 392, 64),
    (FP16X, 0, "plain", 0, 300, 200, 64),
    (FP16X, 0, "plain", 0, 130, 40, 64),           # N <= 64: the 128x64 tile
    (FP16X, FP16, "plain", 0, 300, 200, 64),
    (FP16X, FP16M, "plain", 0, 300, 192, 64),      # FP16M out: N % 64 == 0, 64 tail columns on the 128-wide tile
    (FP16M, 0, "plain", 1, 300, 192, 128),
    (FP16M, 0, "plain", 2, 300, 192, 128),
    (FP16M, 0, "plain", 3, 515, 320, 64),
    (FP16M, FP16X, "plain", 3, 300, 200, 64),
    (FP16, 0, "ln", 0, 300, 200, 64),
    (FP16X, 0, "ln", 0, 100, 392, 64),
    (FP16, 0, "deferred", 1, 300, 200, 64),
    (FP16, 0, "deferred", 3, 300, 392, 64),
    (FP16X, 0, "deferred", 0, 300, 200, 64),
    (FP16M, 0, "deferred", 2, 300, 192, 64),
    (FP16, 0, "gn", 2, 300, 200, 64),
    (FP16X, 0, "gn", 0, 300, 200, 64),
    (FP16, 0, "colscale", 1, 300, 200, 64),
    (FP16X, 0, "rowmap", 0, 300, 200, 64),
    (FP16M, 0, "rowmap", 1, 300, 192, 64),
]


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("mode,out_mode,path,cfg,M,N,K", GEMM_CASES)
def test_gemm_range_flag(L, mode, out_mode, path, cfg, M, N, K, plant):
    bits, want, stored, out, oa, osc, rowmap = gemm_case(L, mode=mode, out_mode=out_mode, path=path, cfg=cfg, M=M, N=N, K=K, plant=plant)
    assert bits == want, (bits, want, float(stored.abs().max()))
    if plant == "masked":
        assert want == 0
    if plant not in ("small", "masked"):
        return
    # finite cases: the fp32 output is the float64 statement, and the operand copy is exactly that output rounded to the copy's format
    f = out.cpu()
    assert float((f.double() - stored).abs().max()) <= 1e-3 * max(1.0, float(stored.abs().max()))
    act = oa.cpu()
    if rowmap is not None:
        act = act[:, rowmap.long()]
    om = out_mode or mode
    if om == FP16M:
        # ... block scales included: columns past N never enter a stored block's scale (N % 64 == 0: a block is stored whole or not at all)
        ref = R.pack(f, False)
        assert torch.equal(act[0].view(torch.int16), ref["hi"].view(torch.int16))
        assert torch.equal(act[1].contiguous().view(torch.uint8).reshape(M, 2 * N), ref["x8"])
        assert torch.equal(osc.cpu() if rowmap is None else osc.cpu()[:, rowmap.long()], ref["scales"])
    else:
        hi = f.half()
        assert torch.equal(act[0].view(torch.int16), hi.view(torch.int16))
        if om == FP16X:
            assert torch.equal(act[1].view(torch.int16), (f - hi.float()).half().view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("mode", [FP16, FP16X])
@pytest.mark.parametrize("D,gelu_on", [(200, False), (200, True), (1032, True)])
def test_layernorm_range_flag(L, mode, D, gelu_on, plant):
    """ser_layernorm_v: D not a multiple of the 256 columns a wave covers per step; "masked" = a huge value in the row pitch past D"""
    rows, ldx = 37, D + 8
    g = torch.Generator().manual_seed(D + mode)
    x = torch.randn(rows, ldx, generator=g)
    w, b = 1.0 + torch.rand(D, generator=g), torch.randn(D, generator=g)
    r, c = 5, 17
    if plant in ("half", "over", "inf"):
        b[c] = planted(plant)
    elif plant == "nan":
        x[r, c] = float("nan")
    elif plant == "masked":
        x[:, D:] = 3.0e5
    ref = torch.nn.functional.layer_norm(x[:, :D].double(), (D,), w.double(), b.double(), 1e-5)
    if gelu_on:
        ref = gelu(ref)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)

    def launch(flag):
        oa = torch.zeros((2 if mode == FP16X else 1, rows, D), dtype=torch.float16, device=DEV)
        a = L.LayerNormArgs()
        a.x, a.ldx, a.g, a.b, a.eps, a.gelu = xd.data_ptr(), ldx, wd.data_ptr(), bd.data_ptr(), 1e-5, int(gelu_on)
        a.out_act, a.ldo_act, a.out_plane_stride, a.mode, a.rows, a.D = oa.data_ptr(), D, rows * D, mode, rows, D
        a.range_flag = flag
        L.check(L.lib.ser_layernorm_v(C.byref(a), stream()), "ser_layernorm_v")
        return (oa,)

    bits, _ = run_flagged(launch)
    assert bits == expected_bits(ref), (bits, expected_bits(ref))


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("mode", [FP16X, FP16M])
def test_row_center_range_flag(L, mode, plant):
    """ser_row_center_v stores x - mean(x) per row; "masked" = a huge value in the row pitch past D"""
    rows, D, ldx = 21, 192, 200
    g = torch.Generator().manual_seed(mode)
    x = torch.randint(-4, 5, (rows, ldx), generator=g).float() + 3.0
    if plant in ("half", "over", "nan", "inf"):
        x[4, 70] = planted(plant)
    elif plant == "masked":
        x[:, D:] = 3.0e5
    xc = x[:, :D].double()
    ref = xc - xc.mean(1, keepdim=True)
    xd = x.to(DEV)

    def launch(flag):
        oa = torch.zeros((2, rows, D), dtype=torch.float16, device=DEV)
        st = torch.zeros((rows, 4, 2), device=DEV)
        sh = torch.zeros(rows, device=DEV)
        osc = torch.zeros((D // 64, rows), dtype=torch.int32, device=DEV)
        a = L.RowCenterArgs()
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = xd.data_ptr(), ldx, oa.data_ptr(), D, rows * D
        a.stats, a.shift, a.stat_groups, a.mode, a.rows, a.D = st.data_ptr(), sh.data_ptr(), 4, mode, rows, D
        if mode == FP16M:
            a.out_scale, a.out_scale_ld = osc.data_ptr(), rows
        a.range_flag = flag
        L.check(L.lib.ser_row_center_v(C.byref(a), stream()), "ser_row_center_v")
        return (oa, osc) if mode == FP16M else (oa,)

    bits, _ = run_flagged(launch)
    assert bits == expected_bits(ref), (bits, expected_bits(ref))


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("no_norm", [0, 1])
def test_wave_frames_range_flag(L, no_norm, plant):
    """ser_wave_frames_v (FP16X frames of a ragged pair, k = 10, stride 5): the planted sample sits in the second utterance; "masked" =
    a huge sample past the last frame of the first one (3003 samples: frames cover 0..2999), which no frame stores."""
    lens, k, s = [3003, 1207], 10, 5
    rng = np.random.default_rng(7)
    waves = [(0.1 * rng.standard_normal(n) + 0.02).astype(np.float32) for n in lens]
    if plant in ("half", "over", "nan", "inf"):
        waves[1][600] = planted(plant)
    elif plant == "masked":
        waves[0][3001] = 3.0e5
    T = [(n - k) // s + 1 for n in lens]
    rows = sum(T)
    frames_ref = []
    for b, w in enumerate(waves):
        wd_ = w.astype(np.float64)
        if not no_norm:
            with np.errstate(invalid="ignore"):
                wd_ = (wd_ - wd_.mean()) / np.sqrt(wd_.var() + 1e-7)
        frames_ref.append(np.stack([wd_[s * t: s * t + k] for t in range(T[b])]))
    ref = torch.from_numpy(np.concatenate(frames_ref))
    packed = torch.from_numpy(np.concatenate(waves)).to(DEV)
    soffs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=DEV)
    foffs = torch.tensor(np.concatenate([[0], np.cumsum(T)]), dtype=torch.int32, device=DEV)
    work = torch.empty(L.lib.ser_workspace_bytes(L.WS_WAVE_FRAMES, 2, 0, 0, 0, FP16X), dtype=torch.uint8, device=DEV)

    def launch(flag):
        fr = torch.zeros((2, rows, 64), dtype=torch.float16, device=DEV)
        a = L.WaveFramesArgs()
        a.wav, a.sample_offs, a.frame_offs, a.B, a.k, a.stride, a.mode = packed.data_ptr(), soffs.data_ptr(), foffs.data_ptr(), 2, k, s, FP16X
        a.out, a.out_plane_stride, a.work, a.total_rows, a.no_norm = fr.data_ptr(), rows * 64, work.data_ptr(), rows, no_norm
        a.range_flag = flag
        L.check(L.lib.ser_wave_frames_v(C.byref(a), stream()), "ser_wave_frames_v")
        return (fr,)

    bits, _ = run_flagged(launch)
    assert bits == expected_bits(ref), (bits, expected_bits(ref))
    if plant == "masked" and not no_norm:
        assert bits == 0


@pytest.mark.parametrize("plant", ["small", "half", "over", "nan", "inf"])
@pytest.mark.parametrize("halo", [0, 64])
def test_pack_act_range_flag(L, halo, plant):
    """ser_pack_act_v (FP16X, [B, C, T] -> channels-last rows with zero halo rows): every input element is stored, so it has no masked
    case; the halo rows are written as zeros and must not disturb the word."""
    B, Cc, T = 2, 72, 50
    g = torch.Generator().manual_seed(halo)
    x = torch.randn(B, Cc, T, generator=g)
    if plant != "small":
        x[1, 9, T - 1] = planted(plant)
    xd = x.to(DEV)
    Tp = T + 2 * halo

    def launch(flag):
        o = torch.zeros((2, B * Tp, Cc), dtype=torch.float16, device=DEV)
        a = L.PackActArgs()
        a.x, a.out, a.ldo, a.out_plane_stride = xd.data_ptr(), o.data_ptr(), Cc, B * Tp * Cc
        a.B, a.C, a.T, a.halo, a.mode = B, Cc, T, halo, FP16X
        a.range_flag = flag
        L.check(L.lib.ser_pack_act_v(C.byref(a), stream()), "ser_pack_act_v")
        return (o,)

    bits, _ = run_flagged(launch)
    assert bits == expected_bits(x)


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("rows,cols", [(9, 192), (70, 576)])
def test_pack_f16m_range_flag(L, weight, rows, cols, plant):
    """ser_pack_f16m, activation and weight roles, cols not a multiple of the 512 columns a wave covers per step; "masked" = a huge value
    in the row pitch past cols.  Finite cases: the planes still equal the host restatement bit for bit."""
    ldx = cols + 4
    g = torch.Generator().manual_seed(rows + cols)
    x = torch.randn(rows, ldx, generator=g) * 3.0
    if plant in ("half", "over", "nan", "inf"):
        x[rows - 1, cols - 3] = planted(plant)
    elif plant == "masked":
        x[:, cols:] = 3.0e5
    xd = x.to(DEV)

    def launch(flag):
        out = torch.zeros((2, rows, cols), dtype=torch.float16, device=DEV)
        sc = torch.zeros((cols // 64, rows), dtype=torch.int32, device=DEV)
        L.check(L.lib.ser_pack_f16m(xd.data_ptr(), ldx, rows, cols, out.data_ptr(), cols, rows * cols, sc.data_ptr(), rows, int(weight),
                                    flag, stream()), "ser_pack_f16m")
        return out, sc

    bits, (out, sc) = run_flagged(launch)
    stored = x[:, :cols]
    assert bits == expected_bits(stored), (bits, expected_bits(stored))
    if plant in ("small", "half", "masked"):
        ref = R.pack(stored.contiguous(), weight)
        assert torch.equal(out[0].cpu().view(torch.int16), ref["hi"].view(torch.int16))
        assert torch.equal(sc.cpu(), ref["scales"])


# ---------------------------------------------------------------------------------------------------------- text embeddings / ConvLayer
def text_ids(B, T, V, pad, gen):
    ids = torch.randint(pad + 1, V, (B, T), generator=gen)
    ids[1, T // 2:] = pad
    ids[0, 5:8] = pad
    return ids


@pytest.mark.parametrize("plant", PLANTS)
def test_embed_ln_range_flag(L, plant):
    """ser_embed_ln_flagged (FP16X, the text drivers' default): word + position + token type -> LayerNorm, planted through the LayerNorm bias or
    a NaN in a word embedding row; "masked" = a huge value in the position-embedding rows no token reaches (row 0 below the pad id's,
    and the row past T + pad id)."""
    B, T, D, V, pad = 3, 70, 200, 40, 1
    gen = torch.Generator().manual_seed(11)
    ids = text_ids(B, T, V, pad, gen)
    w, pe, te = torch.randn(V, D, generator=gen), torch.randn(T + pad + 2, D, generator=gen), torch.randn(D, generator=gen)
    g, b = 1.0 + torch.rand(D, generator=gen), torch.randn(D, generator=gen)
    c = 17
    if plant in ("half", "over", "inf"):
        b[c] = planted(plant)
    elif plant == "nan":
        w[int(ids[2, 3]), c] = float("nan")
    elif plant == "masked":
        pe[0, c] = pe[T + pad + 1, c + 1] = 3.0e5
    m = (ids != pad).long()
    pos = torch.cumsum(m, 1) * m + pad
    ref = torch.nn.functional.layer_norm((w[ids] + pe[pos] + te).double(), (D,), g.double(), b.double(), 1e-5)
    idd = ids.to(torch.int32).to(DEV)
    wd, ped, ted, gd, bd = (t.to(DEV) for t in (w, pe, te, g, b))

    def launch(flag):
        of = torch.zeros((B * T, D), device=DEV)
        oa = torch.zeros((2, B * T, D), dtype=torch.float16, device=DEV)
        L.check(L.lib.ser_embed_ln_flagged(idd.data_ptr(), wd.data_ptr(), ped.data_ptr(), ted.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                           1e-5, of.data_ptr(), oa.data_ptr(), B * T * D, FP16X, B, T, D, pad, flag, stream()),
                "ser_embed_ln_flagged")
        return of, oa

    bits, _ = run_flagged(launch)
    assert bits == expected_bits(ref), (bits, expected_bits(ref))
    if plant == "masked":
        assert bits == 0


@pytest.mark.parametrize("plant", PLANTS)
def test_embed_ln_masked_range_flag(L, plant):
    """ser_embed_ln_masked_flagged (FP16X): padded rows (t >= key_lens[b]) store zeros; "masked" = a NaN and 3e5 in the embedding row of the pad
    token, which only padded positions read."""
    B, T, D, V, pad = 3, 70, 200, 40, 0
    lens = [70, 1, 33]
    gen = torch.Generator().manual_seed(12)
    ids = torch.randint(1, V, (B, T), generator=gen)
    for bi, n in enumerate(lens):
        ids[bi, n:] = pad
    w = torch.randn(V, D, generator=gen)
    g, b = 1.0 + torch.rand(D, generator=gen), torch.randn(D, generator=gen)
    c = 9
    if plant in ("half", "over", "inf"):
        b[c] = planted(plant)
    elif plant == "nan":
        w[int(ids[2, 4]), c] = float("nan")
    elif plant == "masked":
        w[pad, c], w[pad, c + 1] = float("nan"), 3.0e5
    real = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    ref = torch.nn.functional.layer_norm(w[ids].double(), (D,), g.double(), b.double(), 1e-7).view(B * T, D)
    stored = ref[real]                                     # padded rows store zeros
    idd, kl = ids.to(torch.int32).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    wd, gd, bd = (t.to(DEV) for t in (w, g, b))

    def launch(flag):
        of = torch.zeros((B * T, D), device=DEV)
        oa = torch.zeros((2, B * T, D), dtype=torch.float16, device=DEV)
        L.check(L.lib.ser_embed_ln_masked_flagged(idd.data_ptr(), wd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-7, kl.data_ptr(),
                                                  of.data_ptr(), oa.data_ptr(), B * T * D, FP16X, B, T, D, flag, stream()),
                "ser_embed_ln_masked_flagged")
        return of, oa

    bits, (of, oa) = run_flagged(launch)
    assert bits == expected_bits(stored), (bits, expected_bits(stored))
    if plant == "masked":
        assert bits == 0
        assert bool((oa.cpu()[:, ~real] == 0).all())


@pytest.mark.parametrize("plant", PLANTS)
@pytest.mark.parametrize("halo", [0, 1])
def test_pack_rows_range_flag(L, halo, plant):
    """ser_pack_rows_flagged (FP16X, the ConvLayer's halo'd copy of hidden_states[0]): every value of the D columns is stored; "masked" = a huge
    value in x's pitch columns past D, which the copy never reads."""
    B, T, D = 3, 37, 200
    ldx, ldo = D + 8, D + 4
    gen = torch.Generator().manual_seed(13 + halo)
    x = torch.randn(B * T, ldx, generator=gen)
    if plant in ("half", "over", "nan", "inf"):
        x[B * T - 1, D - 3] = planted(plant)
    elif plant == "masked":
        x[:, D:] = 3.0e5
    xd = x.to(DEV)
    R_ = B * (T + 2 * halo)

    def launch(flag):
        o = torch.zeros((2, R_, ldo), dtype=torch.float16, device=DEV)
        L.check(L.lib.ser_pack_rows_flagged(xd.data_ptr(), ldx, B, T, D, halo, o.data_ptr(), ldo, R_ * ldo, FP16X, flag, stream()),
                "ser_pack_rows_flagged")
        return (o,)

    bits, _ = run_flagged(launch)
    stored = x[:, :D]
    assert bits == expected_bits(stored), (bits, expected_bits(stored))
    if plant == "masked":
        assert bits == 0
