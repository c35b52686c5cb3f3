"""The launch plans of ser_gemm and ser_attention_v (csrc/launch_plan.h), pinned on the host -- no GPU.

A wrong tile still computes the right numbers: a slip in a selection threshold shows only as a slower step.  So the plan functions are
plain host code, ``make -C interspeech_ser_amd/csrc plan_check`` builds them with g++ into a program that prints one plan per input
line, and this test compares what it prints for the case list below with ``tests/golden/launch_plans.txt``.

The golden file was NOT written by this program.  It was recorded once from the commit before launch_plan.h existed: that commit's
host sections of gemm.hip and attention.hip, compiled with ``launch_mode`` / ``launch_attention`` replaced by stubs that print their
template arguments, grid and LDS bytes, fed the same case list.  A change of a selection rule has to change the golden line by hand,
with the measurement that justifies it.

Cases: the GEMM shapes of one forward of every shipped geometry at its benchmark batch (from the geometry: conv stack, projection,
positional conv, packed projection, output projection, FC1, FC2; Whisper's stem and decoder step; the text encoders) in every mode and
legal conversion, then every threshold of gemm_pick_tile one tile / one row below, at and above, ``tile_cfg`` 0..3 per mode family,
activation / LayerNorm epilogue on and off, groups 1 and 16, N around 64, and every (mode, out_mode) pair on a dense, a narrow and a
LayerNorm tile.  Attention: every head dim x mode x scale sign x bias kind, the block counts around the high-occupancy window, and bias
windows around the 40 KiB and 160 KiB limits.
"""
import os
import subprocess

import pytest

from interspeech_ser_amd import config as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "interspeech_ser_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")

BF16, FP32X, FP16, FP16X, FP16Q, FP16M = 1, 2, 3, 4, 5, 6
GEMM_MODES = (BF16, FP32X, FP16, FP16X, FP16M)
CONVERSIONS = {BF16: (), FP32X: (FP16,), FP16: (FP16X,), FP16X: (FP16, FP16M), FP16M: (FP16X,)}


def gemm(M, N, K, mode, out_mode=0, *, groups=1, act=0, ln=0, tile_cfg=0, conv=0, **more):
    """One ser_gemm case whose arguments pass every check that does not depend on what the case is about."""
    up64 = (N + 63) // 64 * 64
    f = dict(A=1, W=1, M=M, N=N, K=K, lda=K, groups=groups, c_group_stride=N, mode=mode, out_mode=out_mode, act=act, tile_cfg=tile_cfg,
             out_f32=1, ldo_f32=up64, out_act=1, ldo_act=up64, out_scale=1)
    if ln:
        f.update(ln_gamma=1, ln_beta=1)
    if conv:                                     # implicit-conv row map: K-chunks of 64
        f.update(a_rowoff=1, kc=64)
    if mode == FP16M:
        f.update(a_scale=1, w_scale=1, a_scale_ld=M, w_scale_ld=N)
    f.update(more)
    return "gemm " + " ".join(f"{k}={v}" for k, v in f.items())


def gemm_all_modes(M, N, K, **kw):
    out = []
    for mode in GEMM_MODES:
        if mode == FP16M and (kw.get("ln") or kw.get("conv") or kw.get("groups", 1) != 1) and not kw.get("refusals"):
            continue                             # refused with -23 whatever the shape: pinned once per reason in gemm_cases
        kw.pop("refusals", None)
        out.append(gemm(M, N, K, mode, **kw))
        if not kw.get("ln"):                     # (no conversion with the LayerNorm epilogue: -21, pinned in gemm_cases' pair block)
            out.extend(gemm(M, N, K, mode, om, **kw) for om in CONVERSIONS[mode])
    return out


def speech_forward(geo, utts, seconds):
    chain = geo.frame_chain(int(seconds * 16000))
    ln = 1 if geo.feat_extract_norm == "layer" else 0
    out = gemm_all_modes(utts * chain[0], geo.conv_dim[0], 64, act=1, ln=ln)
    cin = geo.conv_dim[0]
    for t, c, k in list(zip(chain, geo.conv_dim, geo.conv_kernel))[1:]:
        out += gemm_all_modes(utts * t, c, cin * k, act=1, ln=ln, conv=1)
        cin = c
    M, D, F = utts * chain[-1], geo.hidden, geo.ffn
    cg = D // geo.pos_conv_groups
    out += gemm_all_modes(M, D, cin)
    out += gemm_all_modes(M, cg, (cg + 63) // 64 * 64 * geo.pos_conv_kernel, groups=geo.pos_conv_groups, act=1, conv=1)
    return out + layer_gemms(M, D, F)


def layer_gemms(M, D, F, qkv_cols=None):
    out = gemm_all_modes(M, qkv_cols or 3 * D, D)              # packed projection
    out += gemm_all_modes(M, D, D, residual=1, ldr=D)          # output projection
    out += gemm_all_modes(M, F, D, act=1)                      # FC1
    out += gemm_all_modes(M, D, F, residual=1, ldr=D)          # FC2
    return out


def whisper_forward(geo, utts):
    D, F, S = geo.hidden, geo.ffn, geo.max_source_positions
    out = gemm_all_modes(utts * 2 * S, D, geo.n_mels * 3, act=1, conv=1)
    out += gemm_all_modes(utts * S, D, D * 3, act=1, conv=1, residual=1, ldr=D)
    out += layer_gemms(utts * S, D, F)
    # one decoder step: M = utts rows; the cross keys | values of the whole batch; the vocabulary projection
    out += layer_gemms(utts, D, geo.decoder_ffn_dim)
    out += gemm_all_modes(utts, D, D)
    out += gemm_all_modes(utts * S, 2 * D, D)
    out += gemm_all_modes(utts, (geo.decoder_vocab_size + 63) // 64 * 64, D)
    return out


def text_forward(geo, texts, tokens):
    M, D, F = texts * tokens, geo.hidden, geo.ffn
    out = layer_gemms(M, D, F)
    if geo.family == C.FAMILY_DEBERTA:           # content x position terms: one group per head and side
        out += gemm_all_modes(M, 2 * geo.position_buckets, geo.head_dim, groups=2 * geo.heads)
    return out


def threshold_rows(threshold, col_tiles, groups):
    """Row counts that put ceil(M / 256) * col_tiles * groups one 256-row tile below the threshold, one row into the tile that reaches
    it, at the end of that tile and one row past it."""
    r = -(-threshold // (col_tiles * groups))
    return [m for m in ((r - 1) * 256, (r - 1) * 256 + 1, r * 256, r * 256 + 1) if m > 0]


def gemm_cases():
    out = []
    for geo, utts, seconds in ((C.WAVLM_LARGE, 16, 10.0), (C.HUBERT_XLARGE, 16, 10.0), (C.XLSR_2B, 8, 10.0),
                               (C.WAVLM_BASE, 16, 10.0), (C.DATA2VEC_AUDIO_BASE, 16, 10.0)):
        out += speech_forward(geo, utts, seconds)
    out += layer_gemms(16 * C.WAVLM_LARGE.frames_for(160000), 1024, 4096, qkv_cols=3 * 1024 + 64)     # the gate's pre-activations ride along
    out += whisper_forward(C.WHISPER_LARGE_V3, 16)
    out += text_forward(C.ROBERTA_LARGE, 16, 80)
    out += text_forward(C.DEBERTA_V3_LARGE, 16, 80)
    # the LayerNorm tiles' row thresholds 200 * 128 and 200 * 64
    for M in (12800 - 64, 12799, 12800, 12801, 12800 + 64, 25600 - 128, 25599, 25600, 25601, 25600 + 128):
        for N in (256, 512):
            out += gemm_all_modes(M, N, 64, act=1, ln=1)
    # tile-count thresholds: 150 (t256_min, x32_sq_min) and 100 (x32_256_min, FP16M) over 256- and 128-column tiles
    for threshold in (100, 150):
        for colw in (128, 256):
            for N in (colw, 1024):
                for groups in (1, 16):
                    for M in threshold_rows(threshold, -(-N // colw), groups):
                        for mode in GEMM_MODES:
                            if mode != FP16M or groups == 1:
                                out.append(gemm(M, N, 256, mode, groups=groups))
                        if threshold == 150 and colw == 256:
                            out += [gemm(M, N, 256, mode, groups=groups, act=1) for mode in (FP32X, FP16X)]
    # the two-plane square tile: from 150 tiles, and only while the last round of 256 blocks is >= 85 % full
    for tiles in (149, 150, 151, 217, 218, 256, 257, 434, 435, 436, 512, 513):
        for mode in (FP32X, FP16X, BF16, FP16M):
            out += [gemm(256 * tiles, 256, 64, mode, act=act) for act in (0, 1)]
    # N around 64 (the 128x64 tiles), groups 1 and 16
    for N in (8, 64, 72, 128, 256):
        for groups in (1, 16):
            for M in ((512, 40000) if groups == 1 else (512,)):
                out += gemm_all_modes(M, N, 128, groups=groups, refusals=(M == 512))
    # deep K, narrow N
    for K in (1984, 2048):
        for N in (120, 128):
            for M in (511, 512):
                for groups in (1, 16):
                    out += [gemm(M, N, K, mode, groups=groups) for mode in GEMM_MODES]
    # tile_cfg per mode family, with and without the LayerNorm epilogue and an activation
    for M, N, K in ((512, 256, 64), (40000, 512, 64), (512, 64, 64), (40000, 4096, 1024)):
        for tile_cfg in ((0, 1, 2, 3, 4, -1) if N == 256 else (0, 1, 2, 3)):
            for mode in GEMM_MODES:
                out.append(gemm(M, N, K, mode, tile_cfg=tile_cfg))
                if tile_cfg in (0, 3):
                    out.append(gemm(M, N, K, mode, tile_cfg=tile_cfg, act=1))
                if N <= 512 and mode != FP16M:
                    out.append(gemm(M, N, K, mode, tile_cfg=tile_cfg, ln=1))
    # every (mode, out_mode), legal or not, on a dense tile, a narrow one and a LayerNorm tile
    for mode in range(0, 8):
        for om in (range(0, 8) if 1 <= mode <= 6 else (0,)):
            out.append(gemm(1024, 256, 64, mode, om))
            out.append(gemm(1024, 64, 64, mode, om))
            out.append(gemm(1024, 512, 64, mode, om, ln=1))
    # a few refused argument sets
    out += [gemm(512, 256, 96, BF16), gemm(512, 252, 64, BF16), gemm(512, 256, 64, BF16, groups=0), gemm(512, 256, 64, BF16, out_f32=0, out_act=0),
            gemm(512, 1024, 64, BF16, ln=1), gemm(512, 256, 64, FP16M, a_scale=0), gemm(512, 256, 64, FP16X, FP16M, out_scale=0),
            gemm(512, 256, 64, BF16, stat_out=1, stat_groups=3), gemm(512, 256, 64, BF16, mean_out=1), gemm(512, 512, 64, FP16M, ln=1),
            gemm(512, 256, 64, FP16M, conv=1)]
    return out


def attn(B, H, dh, max_frames, mode, scale, bias="none", **more):
    f = dict(qkv=1, frame_offs=1, out=1, ld=3 * H * dh, ldo=H * dh, k_col=H * dh, v_col=2 * H * dh, B=B, H=H, dh=dh, max_frames=max_frames,
             mode=mode, scale=scale)
    if bias == "gate":
        f.update(table=1, table_T=max_frames, gate=1)
    elif bias == "gru":
        f.update(table=1, table_T=max_frames, gru_const=1, gate_col=0)
    elif bias == "bias2d":
        f.update(bias2d=1, bias2d_ld=(max_frames + 63) // 64 * 64, key_lens=1)
    f.update(more)
    return "attn " + " ".join(f"{k}={v}" for k, v in f.items())


def attn_cases():
    out = []
    modes = (BF16, FP32X, FP16, FP16X, FP16Q)
    for dh in (8, 64, 72, 80, 96, 104, 120, 128):
        for mode in modes:
            for scale in (-1.0, 0.125):
                for bias in ("none", "gate", "gru", "bias2d"):
                    if bias != "bias2d" or scale <= 0 or dh == 64:          # (bias2d without a pre-scaled q: -11 at every width)
                        out.append(attn(16, 16, dh, 499, mode, scale, bias))
    # blocks = roundup(H * B, 8) * ceil(max_frames / 128) around the high-occupancy window (512, 1024]
    for B in (512, 513, 1024, 1025):
        for mode in modes:
            for bias in ("none", "gate"):
                out += [attn(B, 1, 64, 100, mode, -1.0, bias), attn(B, 1, 64, 100, mode, 0.125, bias)]
        out += [attn(B, 1, 64, 100, BF16, -1.0, "bias2d"), attn(B, 1, 80, 100, BF16, -1.0), attn(B, 1, 128, 100, FP16, -1.0)]
    # shipped shapes: 16 x 10 s and 8 x 10 s WavLM-large, HuBERT-xlarge (dh 80), Whisper (20 heads x 1500 frames), the text encoders
    for mode in modes:
        out += [attn(16, 16, 64, 499, mode, -1.0, "gru", gate_x=1, gate_stat=1, gate_w=1, gate_cb=1, gate_x_ld=1024,
                     gate_x_planes=2 if mode in (FP32X, FP16X, FP16Q) else 1),
                attn(8, 16, 64, 499, mode, -1.0, "gru"), attn(16, 16, 80, 499, mode, -1.0), attn(8, 16, 120, 499, mode, -1.0),
                attn(16, 20, 64, 1500, mode, -1.0), attn(16, 20, 64, 1500, mode, 0.125), attn(16, 16, 64, 80, mode, -1.0, key_lens=1),
                attn(16, 12, 64, 499, mode, -1.0, "gate")]
    out += [attn(16, 16, 64, 499, FP16X, -1.0, "gru", out_mode=FP16M, out_scale=1, out_scale_ld=8000),
            attn(16, 16, 64, 499, FP16, -1.0, "gru", out_mode=FP16M, out_scale=1, out_scale_ld=8000)]
    # bias window around 40 KiB (the high-occupancy form gives way; 8 x 8 heads x 10 query tiles = 640 blocks) ...
    for max_frames in range(1224, 1234):
        out += [attn(8, 8, 64, max_frames, mode, -1.0, "gate") for mode in (BF16, FP16, FP32X)]
    # ... and around 160 KiB (the table moves to global memory, or the launch is refused): one-plane, FP16Q's three planes, two-plane
    for lo, ms in ((7872, (BF16, FP16)), (6848, (FP16Q,)), (5824, (FP32X, FP16X))):
        for max_frames in range(lo + 6, lo + 14):
            for mode in ms:
                out.append(attn(1, 16, 64, max_frames, mode, -1.0, "gate"))
                out.append(attn(1, 16, 64, max_frames, mode, 0.125, "gate"))
                out.append(attn(1, 16, 128, max_frames, mode, -1.0, "gate"))
    # one long utterance: 16 heads x 63 query tiles = 1 008 blocks, 133 KiB of bias window
    out += [attn(1, 16, 64, 8000, mode, -1.0, "gate") for mode in modes]
    out += [attn(1, 16, 64, 8000, BF16, -1.0), attn(1, 16, 64, 20000, FP32X, 0.125, "gate")]
    return out


def cases():
    return list(dict.fromkeys(gemm_cases() + attn_cases()))          # shapes that several geometries share, once


@pytest.fixture(scope="module")
def plan_check():
    subprocess.check_call(["make", "-C", CSRC, "plan_check"], stdout=subprocess.DEVNULL)
    path = os.path.join(CSRC, "build", "plan_check", "launch_plan_check")
    assert os.path.isfile(path)
    return path


def test_launch_plans_match_the_recorded_ones(plan_check):
    lines = cases()
    r = subprocess.run([plan_check], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(lines) == len(want)
    wrong = [(c, g, w) for c, g, w in zip(lines, got, want) if g != w]
    assert not wrong, "\n".join(f"{c}\n  plan     {g}\n  recorded {w}" for c, g, w in wrong[:10]) + f"\n({len(wrong)} of {len(lines)} differ)"


def test_the_case_list_reaches_every_tile_conversion_and_attention_form():
    """The recorded plans name all twelve tiles, all ten (mode, out_mode) pairs, every attention head width with every form flag both
    ways, and the refusals -8, -13, -21 and -22: a pruned case list would not pin them."""
    with open(GOLDEN) as f:
        want = [l.split() for l in f.read().splitlines()]
    g = [l for l in want if l[0] == "gemm" and l[1] != "err"]
    assert len({l[1] for l in g}) == 12 and len({l[2] for l in g}) == 10
    assert {l[2] for l in want if l[1] == "err"} >= {"-8", "-13", "-21", "-22"}
    a = [l for l in want if l[0] == "attn" and l[1] != "err"]
    assert {l[1] for l in a} == {"64", "96", "128"} and {l[2] for l in a} == {"1", "2", "3", "4", "5"}
    for i, flag in enumerate("PTBGO"):
        assert {l[3][i] for l in a} == {flag, "-"}, flag
    assert {l[4] for l in a} == {"nbuf=1", "nbuf=2"}
