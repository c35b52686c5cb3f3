"""Text-side row kernels against float64 and against bit patterns (-m gpu): ser_embed_ln (RoBERTa), ser_embed_ln_masked (DeBERTa),
ser_pack_rows and ser_zero_padded_rows (DeBERTa's ConvLayer), in every operand format they write -- 1 = bf16, 2 = bf16 hi + lo (fp32x),
4 = fp16 hi + lo (f16x, the text drivers' default).

Each kernel writes its fp32 output and its operand planes from the same fp32 value, so the planes need no tolerance: they are the host
split of the kernel's own fp32 output, bit for bit (compared as int16 patterns, so a -0.0 for a +0.0 is a difference too).  The fp32
output is compared with a float64 statement of the op.  Output buffers hold planted garbage before each launch, and every byte a launch
must not touch (spare rows, pitch columns past D, halo rows) is checked to still hold it; a refused launch leaves every buffer as it was."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, FP32X, FP16, FP16X, FP16Q, FP16M = 1, 2, 3, 4, 5, 6
REFUSED_MODES = (FP16, FP16Q, FP16M)         # formats these kernels do not write
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
    if mode == FP16X:
        hi = y.clamp(-F16_MAX, F16_MAX).half()
        lo = (y - hi.float()).clamp(-F16_MAX, F16_MAX).half()
    else:
        hi = y.to(torch.bfloat16)
        lo = (y - hi.float()).to(torch.bfloat16)
    planes = [hi, lo][:n_planes(mode)]
    return torch.stack([p.view(torch.int16) for p in planes])


def garbage_planes(P, rows, cols):
    return torch.full((P, rows, cols), GARBAGE, dtype=torch.int16, device=DEV)


def garbage_f32(rows, cols):
    return torch.full((rows, cols), float("nan"), device=DEV)


def f32_bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int32)


def ln64(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float) -> torch.Tensor:
    return torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), eps)


# ------------------------------------------------------------------------------------------------------------------------------ launchers
# (the forms without the range-guard word; tests/test_gpu_range_guard.py pins the word through the *_flagged forms, and shows that a NULL
# word stores the same bytes)
def embed_ln(L, ids, w, pe, te, g, b, eps, of, oa, plane, mode, B, T, D, pad):
    return L.lib.ser_embed_ln(ids.data_ptr(), w.data_ptr(), pe.data_ptr(), te.data_ptr(), g.data_ptr(), b.data_ptr(), eps,
                              None if of is None else of.data_ptr(), None if oa is None else oa.data_ptr(), plane, mode, B, T, D, pad,
                              stream())


def embed_ln_masked(L, ids, w, g, b, eps, kl, of, oa, plane, mode, B, T, D):
    return L.lib.ser_embed_ln_masked(ids.data_ptr(), w.data_ptr(), g.data_ptr(), b.data_ptr(), eps, kl.data_ptr(),
                                     None if of is None else of.data_ptr(), None if oa is None else oa.data_ptr(), plane, mode, B, T, D,
                                     stream())


def pack_rows(L, x, ldx, B, T, D, halo, out, ldo, plane, mode):
    return L.lib.ser_pack_rows(x.data_ptr(), ldx, B, T, D, halo, out.data_ptr(), ldo, plane, mode, stream())


def zero_padded_rows(L, x, ldx, act, lda, plane, mode, kl, B, T, D):
    return L.lib.ser_zero_padded_rows(None if x is None else x.data_ptr(), ldx, None if act is None else act.data_ptr(), lda, plane, mode,
                                      kl.data_ptr(), B, T, D, stream())


# ------------------------------------------------------------------------------------------------------------------------- ser_embed_ln
def roberta_ids(B, T, V, pad, gen):
    """ids [B, T] with pad tokens at the end of some sequences and inside one; never the pad id among the real tokens"""
    ids = torch.randint(pad + 1, V, (B, T), generator=gen)
    if B > 1:
        ids[1, T // 2 + 1:] = pad
    ids[0, T // 3: T // 3 + 3] = pad                 # pads in the middle of a sequence: they keep position pad_id, the count resumes after
    ids[B - 1, T - 1] = pad
    return ids


EMBED_SHAPES = [(3, 7, 128), (2, 13, 1028), (1, 512, 1024), (3, 67, 2048)]       # B*T = 21, 26, 512, 201; T = 512 and T > 64


@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("B,T,D", EMBED_SHAPES)
def test_embed_ln_against_float64(L, mode, B, T, D):
    """RoBERTa embeddings word[id] + position[cumsum(id != pad) * (id != pad) + pad] + token_type[0] -> LayerNorm (HF's
    create_position_ids_from_input_ids): fp32 output within 2e-5 of float64, planes the host split of it, spare rows untouched; with
    out_f32 or out_act NULL the other output holds the same bytes."""
    V, pad, EXTRA, eps = 97, 1, 3, 1e-5
    gen = torch.Generator().manual_seed(B * 1000 + T + D + mode)
    ids = roberta_ids(B, T, V, pad, gen)
    w = torch.randn(V, D, generator=gen)
    pe = torch.randn(T + pad + 1, D, generator=gen)       # exactly the rows HF's position ids reach
    te = torch.randn(D, generator=gen) * 0.5
    g, b = 1.0 + 0.2 * torch.randn(D, generator=gen), 0.2 * torch.randn(D, generator=gen)
    m = (ids != pad).long()
    pos = torch.cumsum(m, 1) * m + pad
    ref = ln64(w[ids] + pe[pos] + te, g, b, eps).view(B * T, D)
    rows, P = B * T, n_planes(mode)
    idd = ids.to(torch.int32).to(DEV)
    wd, ped, ted, gd, bd = (t.to(DEV) for t in (w, pe, te, g, b))
    plane = (rows + EXTRA) * D

    def launch(want_f32=True, want_act=True, m_=mode, D_=D):
        of = garbage_f32(rows + EXTRA, D) if want_f32 else None
        oa = garbage_planes(P, rows + EXTRA, D) if want_act else None
        rc = embed_ln(L, idd, wd, ped, ted, gd, bd, eps, of, oa, plane, m_, B, T, D_, pad)
        torch.cuda.synchronize()
        return rc, of, oa

    rc, of, oa = launch()
    assert rc == 0, L.lib.ser_last_error()
    f = of.cpu()
    assert (f[:rows].double() - ref).abs().max().item() < 2e-5
    assert bool(f[rows:].isnan().all())
    a = oa.cpu()
    assert torch.equal(a[:, :rows], host_split(f[:rows], mode))
    assert bool((a[:, rows:] == GARBAGE).all())
    rc, of2, _ = launch(want_act=False)
    assert rc == 0 and torch.equal(f32_bits(of2), f32_bits(of))
    rc, _, oa2 = launch(want_f32=False)
    assert rc == 0 and torch.equal(oa2.cpu(), a)
    for m_, D_ in [(bad, D) for bad in REFUSED_MODES] + [(mode, D - 2)]:
        rc, of3, oa3 = launch(m_=m_, D_=D_)
        assert rc < 0 and b"ser_embed_ln" in L.lib.ser_last_error()
        assert bool(of3.isnan().all()) and bool((oa3 == GARBAGE).all())


def test_embed_ln_refuses_rows_wider_than_2048(L):
    """D > 2048 does not fit the kernel's eight 256-column steps: refused before any launch, buffers untouched (all sized for D = 2052)."""
    B, T, D, V, pad = 1, 5, 2052, 8, 1
    ids = torch.full((B, T), 2, dtype=torch.int32, device=DEV)
    w, pe = torch.zeros(V, D, device=DEV), torch.zeros(T + 2, D, device=DEV)
    te, g, b = torch.zeros(D, device=DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    for mode in (BF16, FP32X, FP16X):
        of, oa = garbage_f32(B * T, D), garbage_planes(2, B * T, D)
        rc = embed_ln(L, ids, w, pe, te, g, b, 1e-5, of, oa, B * T * D, mode, B, T, D, pad)
        torch.cuda.synchronize()
        assert rc < 0 and b"ser_embed_ln" in L.lib.ser_last_error()
        assert bool(of.isnan().all()) and bool((oa == GARBAGE).all())
        kl = torch.full((B,), T, dtype=torch.int32, device=DEV)
        rc = embed_ln_masked(L, ids, w, g, b, 1e-7, kl, of, oa, B * T * D, mode, B, T, D)
        torch.cuda.synchronize()
        assert rc < 0 and b"ser_embed_ln_masked" in L.lib.ser_last_error()
        assert bool(of.isnan().all()) and bool((oa == GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------------ ser_embed_ln_masked
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("D", [128, 1024, 1536, 2048])
def test_embed_ln_masked_against_float64(L, mode, D):
    """DeBERTa-v3 embeddings: LayerNorm(word[id]) on real rows (t < key_lens[b]), +0.0 on padded rows in fp32 and in every plane, the
    lo plane included.  The pad token's embedding row holds a NaN: padded rows read it and must leak it into nothing."""
    B, T, V, pad, EXTRA, eps = 4, 37, 61, 0, 2, 1e-7
    lens = [1, T, 20, 36]                                # one real token, no padding, two mixed
    gen = torch.Generator().manual_seed(D + mode)
    ids = torch.randint(1, V, (B, T), generator=gen)
    for bi, n in enumerate(lens):
        ids[bi, n:] = pad
    w = torch.randn(V, D, generator=gen) * 0.7 + 0.1
    w[pad, D // 2] = float("nan")
    g, b = 1.0 + 0.2 * torch.randn(D, generator=gen), 0.2 * torch.randn(D, generator=gen)
    ref = ln64(w[ids], g, b, eps).view(B * T, D)
    real = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    rows, P = B * T, n_planes(mode)
    idd, kl = ids.to(torch.int32).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    wd, gd, bd = (t.to(DEV) for t in (w, g, b))
    plane = (rows + EXTRA) * D

    def launch(want_f32=True, want_act=True, m_=mode, D_=D):
        of = garbage_f32(rows + EXTRA, D) if want_f32 else None
        oa = garbage_planes(P, rows + EXTRA, D) if want_act else None
        rc = embed_ln_masked(L, idd, wd, gd, bd, eps, kl, of, oa, plane, m_, B, T, D_)
        torch.cuda.synchronize()
        return rc, of, oa

    rc, of, oa = launch()
    assert rc == 0, L.lib.ser_last_error()
    f = of.cpu()
    assert (f[:rows][real].double() - ref[real]).abs().max().item() < 2e-5
    assert bool((f32_bits(f[:rows][~real]) == 0).all())
    assert bool(f[rows:].isnan().all())
    a = oa.cpu()
    assert torch.equal(a[:, :rows], host_split(f[:rows], mode))
    assert bool((a[:, :rows][:, ~real] == 0).all())
    assert bool((a[:, rows:] == GARBAGE).all())
    rc, of2, _ = launch(want_act=False)
    assert rc == 0 and torch.equal(f32_bits(of2), f32_bits(of))
    rc, _, oa2 = launch(want_f32=False)
    assert rc == 0 and torch.equal(oa2.cpu(), a)
    for m_, D_ in [(bad, D) for bad in REFUSED_MODES] + [(mode, D - 2)]:
        rc, of3, oa3 = launch(m_=m_, D_=D_)
        assert rc < 0 and b"ser_embed_ln_masked" in L.lib.ser_last_error()
        assert bool(of3.isnan().all()) and bool((oa3 == GARBAGE).all())


# ------------------------------------------------------------------------------------------------------------------------ ser_pack_rows
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("halo", [0, 1, 2])
def test_pack_rows_layout_and_bits(L, mode, halo):
    """Row b*T + t of x lands at row b*(T + 2 halo) + halo + t of every plane, bit for bit the host split of x (values past fp16's range
    saturate the fp16 planes, as the split states); the halo rows (the caller's zeros), the pitch columns past D and the spare rows after
    the last sequence keep what they held."""
    B, T, D, EXTRA = 3, 37, 1536, 3
    ldx, ldo = D + 8, D + 12
    Tp = T + 2 * halo
    R_ = B * Tp + EXTRA
    gen = torch.Generator().manual_seed(halo * 10 + mode)
    x = torch.randn(B * T, ldx, generator=gen) * torch.logspace(-5, 2, D + 8)[None, :]
    x[4, 7], x[50, D - 1], x[B * T - 1, 0] = 7.0e4, -2.0e5, 4.0e4
    x[:, D:] = float("nan")                             # pitch columns of x: never read into a plane
    xd = x.to(DEV)
    P = n_planes(mode)
    want = host_split(x[:, :D], mode)
    rows = torch.tensor([bi * Tp + halo + t for bi in range(B) for t in range(T)])

    def launch(m_=mode, ldx_=ldx, D_=D):
        out = garbage_planes(P, R_, ldo)
        rc = pack_rows(L, xd, ldx_, B, T, D_, halo, out, ldo, R_ * ldo, m_)
        torch.cuda.synchronize()
        return rc, out.cpu()

    rc, out = launch()
    assert rc == 0, L.lib.ser_last_error()
    assert torch.equal(out[:, rows, :D], want)
    untouched = torch.ones(R_, dtype=torch.bool)
    untouched[rows] = False
    assert bool((out[:, untouched] == GARBAGE).all())              # halo rows and spare rows
    assert bool((out[:, :, D:] == GARBAGE).all())                  # pitch columns
    for m_, ldx_, D_ in [(bad, ldx, D) for bad in REFUSED_MODES] + [(mode, ldx - 2, D), (mode, ldx, D - 2)]:
        rc, out = launch(m_, ldx_, D_)
        assert rc < 0 and b"ser_pack_rows" in L.lib.ser_last_error()
        assert bool((out == GARBAGE).all())


# ----------------------------------------------------------------------------------------------------------------- ser_zero_padded_rows
@pytest.mark.parametrize("mode", [BF16, FP32X, FP16X])
@pytest.mark.parametrize("which", ["f32", "act", "both"])
def test_zero_padded_rows(L, mode, which):
    """Rows t >= key_lens[b] of the fp32 matrix and / or its planes become +0.0 (every plane, the lo plane included); real rows and the
    pitch columns past D keep their planted pattern bit for bit."""
    B, T, D = 4, 37, 1536
    lens = [1, T, 20, 36]
    ldx, lda = D + 4, D + 8
    gen = torch.Generator().manual_seed(mode * 3 + len(which))
    x0 = torch.randn(B * T, ldx, generator=gen) * 100.0
    P = n_planes(mode)
    a0 = torch.randint(-32768, 32768, (P, B * T, lda), generator=gen, dtype=torch.int32).to(torch.int16)
    a0[a0 == 0] = 1                                                 # a zero in the pattern would hide a missed store
    x0[x0 == 0] = 1.0
    kl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    pad = ~(torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    use_x, use_a = which in ("f32", "both"), which in ("act", "both")

    def launch(m_=mode, ldx_=ldx, lda_=lda, D_=D):
        xd, ad = x0.to(DEV), a0.to(DEV)
        rc = zero_padded_rows(L, xd if use_x else None, ldx_, ad if use_a else None, lda_, B * T * lda, m_, kl, B, T, D_)
        torch.cuda.synchronize()
        return rc, xd.cpu(), ad.cpu()

    rc, x, a = launch()
    assert rc == 0, L.lib.ser_last_error()
    if use_x:
        assert torch.equal(f32_bits(x[~pad]), f32_bits(x0[~pad]))
        assert bool((f32_bits(x[pad][:, :D]) == 0).all())
        assert torch.equal(f32_bits(x[:, D:]), f32_bits(x0[:, D:]))
    else:
        assert torch.equal(f32_bits(x), f32_bits(x0))
    if use_a:
        assert torch.equal(a[:, ~pad], a0[:, ~pad])
        assert bool((a[:, pad][:, :, :D] == 0).all())
        assert torch.equal(a[:, :, D:], a0[:, :, D:])
    else:
        assert torch.equal(a, a0)
    bad_args = [(bad, ldx, lda, D) for bad in REFUSED_MODES] + [(mode, ldx, lda, D - 2)]
    bad_args += [(mode, ldx - 2, lda, D)] if use_x else []
    bad_args += [(mode, ldx, lda - 2, D)] if use_a else []
    for m_, ldx_, lda_, D_ in bad_args:
        rc, x, a = launch(m_, ldx_, lda_, D_)
        assert rc < 0 and b"ser_zero_padded_rows" in L.lib.ser_last_error()
        assert torch.equal(f32_bits(x), f32_bits(x0)) and torch.equal(a, a0)
