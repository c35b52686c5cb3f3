#!/usr/bin/env python
"""A/B of two builds of libserhip on the row kernels of csrc/rowops.hip and csrc/deberta.hip: bit-equal results and per-kernel time.

    python tools/rowops_ab.py PARENT.so BRANCH.so [--pairs 3] [--no-times] [--out rowops_ab.txt]

PARENT.so is the library of the parent commit (built from a `git worktree` of it), BRANCH.so the one under test.  Every measurement runs
in a fresh child process with SER_HIP_LIB set to one of the two, so the two libraries never share a process.

  results  every entry point that launches a row kernel, over a fixed seeded case list: every mode it accepts, both output selections, the
           fp16 range-guard word.  The child prints one SHA-256 per output buffer; the two lists must be identical, line for line.
  times    the skeleton's kernels at the shapes the encoders launch for 16 x 10 s (7 984 rows; the text embeddings at 16 x 80 tokens):
           device events around 200 launches after 20 warm-up launches, parent and branch children alternating, `--pairs` of them.  A
           kernel passes if its branch median is no slower than the parent median by more than the spread (max - min) of the parent runs.

Exit status 1 if a hash differs or a kernel is slower beyond the spread."""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, FP32X, FP16, FP16X, FP16M = 1, 2, 3, 4, 6
NAME = {BF16: "bf16", FP32X: "fp32x", FP16: "f16", FP16X: "f16x", FP16M: "f16m"}
WIDTHS, ROWS = [4, 252, 256, 260, 2044, 2048], [1, 6]          # tests/test_gpu_row_skeleton.py
M_STEP = 7984                                                  # encoder rows of 16 x 10 s
GARBAGE = -3


# ================================================================================================================= child: one library
class Child:
    def __init__(self):
        import torch
        sys.path.insert(0, ROOT)
        from interspeech_ser_amd import _lib
        self.t, self.L, self.dev = torch, _lib, "cuda:0"
        self.lines = []

    # ---- buffers
    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    def gen(self, seed):
        return self.t.Generator().manual_seed(seed)

    def planes(self, mode, rows, ld):
        P = 2 if mode in (FP32X, FP16X, FP16M) else 1
        return self.t.full((P, rows, ld), GARBAGE, dtype=self.t.int16, device=self.dev)

    def f32(self, rows, ld):
        return self.t.full((rows, ld), float("nan"), device=self.dev)

    def flag(self):
        return self.t.zeros(1, dtype=self.t.int32, device=self.dev)

    def emit(self, case, **bufs):
        self.t.cuda.synchronize()
        for name, b in bufs.items():
            if b is not None:
                h = hashlib.sha256(b.detach().cpu().contiguous().view(self.t.uint8).numpy().tobytes()).hexdigest()
                self.lines.append(f"{case} {name} {h}")

    def check(self, rc, what):
        self.L.check(rc, what)

    # ---- launchers (return the buffers they wrote; `outs` = "both" | "f32" | "act")
    def layernorm(self, mode, rows, D, gelu, outs, x, g, b, pad=True):
        t, L = self.t, self.L
        ldx, ldof, ldoa = (D + 4, D + 8, D + 12) if pad else (D, D, D)
        xd = t.full((rows, ldx), float("nan"), device=self.dev)
        xd[:, :D] = x.to(self.dev)
        of = self.f32(rows + 2, ldof) if outs != "act" else None
        oa = self.planes(mode, rows + 2, ldoa) if outs != "f32" else None
        fl, gd, bd = self.flag(), g.to(self.dev), b.to(self.dev)
        a = L.LayerNormArgs()
        a.x, a.ldx, a.g, a.b, a.eps, a.gelu = xd.data_ptr(), ldx, gd.data_ptr(), bd.data_ptr(), 1e-5, gelu
        if of is not None:
            a.out_f32, a.ldo_f32 = of.data_ptr(), ldof
        if oa is not None:
            a.out_act, a.ldo_act, a.out_plane_stride = oa.data_ptr(), ldoa, (rows + 2) * ldoa
        a.mode, a.rows, a.D, a.range_flag = mode, rows, D, fl.data_ptr()
        keep = (xd, gd, bd, of, oa, fl)
        return a, keep, dict(f32=of, act=oa, flag=fl)

    def pos_ln(self, mode, rows, D, last, x, res, g, b, pad=True, want_act=True):
        t, L = self.t, self.L
        ldx, ldr, ldof, ldoa = (D + 4, D + 16, D + 8, D + 12) if pad else (D, D, D, D)
        xd = t.full((rows, ldx), float("nan"), device=self.dev)
        xd[:, :D] = x.to(self.dev)
        rd = t.full((rows, ldr), float("nan"), device=self.dev)
        rd[:, :D] = res.to(self.dev)
        gd, bd, fl = g.to(self.dev), b.to(self.dev), self.flag()
        rowmap = None if last else (2 * t.arange(rows, dtype=t.int32) + 1).to(self.dev)
        out_rows = rows + 2 if last else 2 * rows + 2
        oa = self.planes(mode, out_rows, ldoa) if want_act else None
        of = self.f32(rows + 2, ldof) if last else None
        a = L.PosLnArgs()
        a.x, a.ldx = xd.data_ptr(), ldx
        if oa is not None:
            a.out_act, a.ldo_act, a.out_plane_stride = oa.data_ptr(), ldoa, out_rows * ldoa
        if last:
            a.residual, a.ldr, a.g, a.b, a.out_f32, a.ldo_f32 = rd.data_ptr(), ldr, gd.data_ptr(), bd.data_ptr(), of.data_ptr(), ldof
        else:
            a.out_rowmap = rowmap.data_ptr()
        a.eps_pos, a.eps, a.last, a.mode, a.rows, a.D, a.range_flag = 1e-5, 1e-5, int(last), mode, rows, D, fl.data_ptr()
        keep = (xd, rd, gd, bd, rowmap, oa, of, fl)
        return a, keep, dict(f32=of, act=oa, flag=fl)

    def row_center(self, mode, rows, D, x, pad=True):
        t, L = self.t, self.L
        m = mode == FP16M
        ldx, ldoa = (D + 4, D + (64 if m else 12)) if pad else (D, D)
        xd = t.full((rows, ldx), float("nan"), device=self.dev)
        xd[:, :D] = x.to(self.dev)
        oa = self.planes(mode, rows + 2, ldoa)
        st, sh, fl = self.f32(rows + 2, 8), self.f32(1, rows + 2), self.flag()
        osc = t.full((max(D // 64, 1), rows + 2), GARBAGE, dtype=t.int32, device=self.dev) if m else None
        a = L.RowCenterArgs()
        a.x, a.ldx, a.out_act, a.ldo_act, a.out_plane_stride = xd.data_ptr(), ldx, oa.data_ptr(), ldoa, (rows + 2) * ldoa
        a.stats, a.shift, a.stat_groups, a.mode, a.rows, a.D = st.data_ptr(), sh.data_ptr(), 4, mode, rows, D
        if m:
            a.out_scale, a.out_scale_ld = osc.data_ptr(), rows + 2
        a.range_flag = fl.data_ptr()
        keep = (xd, oa, st, sh, fl, osc)
        return a, keep, dict(act=oa, stats=st, shift=sh, scales=osc, flag=fl)

    def embed(self, masked, mode, B, T, D, outs, seed):
        """-> (launch(), buffers): ser_embed_ln_flagged (RoBERTa) or ser_embed_ln_masked_flagged (DeBERTa)"""
        t, L = self.t, self.L
        gen = self.gen(seed)
        V, pad, rows = 97, 1, B * T
        ids = t.randint(pad + 1, V, (B, T), generator=gen)
        lens = [max(1, T - 3 * i) for i in range(B)]
        for i, n in enumerate(lens):
            ids[i, n:] = pad
        w, pe, te = t.randn(V, D, generator=gen), t.randn(T + pad + 1, D, generator=gen), t.randn(D, generator=gen) * 0.5
        g, b = 1.0 + 0.2 * t.randn(D, generator=gen), 0.2 * t.randn(D, generator=gen)
        b[D // 2] = 40000.0                                       # half of fp16's range: the guard word gets bit 1
        idd, kl = ids.to(t.int32).to(self.dev), t.tensor(lens, dtype=t.int32, device=self.dev)
        wd, ped, ted, gd, bd = (v.to(self.dev) for v in (w, pe, te, g, b))
        of = self.f32(rows + 2, D) if outs != "act" else None
        oa = self.planes(mode, rows + 2, D) if outs != "f32" else None
        fl = self.flag()
        ofp, oap, plane = (None if of is None else of.data_ptr()), (None if oa is None else oa.data_ptr()), (rows + 2) * D
        keep = (idd, kl, wd, ped, ted, gd, bd, of, oa, fl)
        if masked:
            def launch():
                return L.lib.ser_embed_ln_masked_flagged(idd.data_ptr(), wd.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1e-7, kl.data_ptr(), ofp,
                                                         oap, plane, mode, B, T, D, fl.data_ptr(), self.stream())
        else:
            def launch():
                return L.lib.ser_embed_ln_flagged(idd.data_ptr(), wd.data_ptr(), ped.data_ptr(), ted.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                                                  1e-5, ofp, oap, plane, mode, B, T, D, pad, fl.data_ptr(), self.stream())
        return launch, keep, dict(f32=of, act=oa, flag=fl)

    def ln_inputs(self, rows, D, seed, plant=False):
        t, gen = self.t, self.gen(seed)
        x = t.randn(rows, D, generator=gen) * 3 + 0.5
        res = t.randn(rows, D, generator=gen) * 2 + 1.0
        g, b = 1.0 + 0.3 * t.randn(D, generator=gen), 0.2 * t.randn(D, generator=gen)
        if plant:
            b[D // 2] = 40000.0
        return x, res, g, b

    # ---- the case list
    def results(self):
        t, L, lib = self.t, self.L, self.L.lib
        s = self.stream
        shapes = [(r, D) for D in WIDTHS for r in ROWS]
        # ser_layernorm_v
        for mode in (BF16, FP32X, FP16, FP16X):
            for rows, D, plant in [(r, D, False) for r, D in shapes] + [(M_STEP, 512, True), (M_STEP, 1024, True)]:
                x, _, g, b = self.ln_inputs(rows, D, 100 * D + rows, plant)
                for gelu in (0, 1):
                    for outs in ("both", "f32", "act"):
                        if rows == M_STEP and outs != "both":
                            continue
                        a, keep, bufs = self.layernorm(mode, rows, D, gelu, outs, x, g, b)
                        self.check(lib.ser_layernorm_v(C.byref(a), s()), "ser_layernorm_v")
                        self.emit(f"layernorm {NAME[mode]} rows={rows} D={D} gelu={gelu} outs={outs}", **bufs)
        # the positional form of the same entry point
        x, _, g, b = self.ln_inputs(37, 1536, 5)
        xd, gd, bd = x.to(self.dev), g.to(self.dev), b.to(self.dev)
        of, oa = self.f32(37, 1536), self.planes(FP16X, 37, 1536)
        self.check(lib.ser_layernorm(xd.data_ptr(), 1536, gd.data_ptr(), bd.data_ptr(), 1e-5, 1, of.data_ptr(), 1536, oa.data_ptr(), 1536,
                                     37 * 1536, FP16X, 37, 1536, s()), "ser_layernorm")
        self.emit("layernorm positional f16x rows=37 D=1536", f32=of, act=oa)
        # ser_pos_ln_v
        for mode in (BF16, FP32X, FP16, FP16X):
            for rows, D, plant in [(r, D, False) for r, D in shapes] + [(M_STEP, 768, True)]:
                x, res, g, b = self.ln_inputs(rows, D, 200 * D + rows, plant)
                for last, want_act in ((False, True), (True, True), (True, False)):
                    a, keep, bufs = self.pos_ln(mode, rows, D, last, x, res, g, b, want_act=want_act)
                    self.check(lib.ser_pos_ln_v(C.byref(a), s()), "ser_pos_ln_v")
                    self.emit(f"pos_ln {NAME[mode]} rows={rows} D={D} last={int(last)} act={int(want_act)}", **bufs)
        # ser_row_center_v
        for mode in (BF16, FP32X, FP16, FP16X, FP16M):
            sh = [(r, D) for D in (64, 320, 2048) for r in ROWS] if mode == FP16M else shapes
            for rows, D in sh + [(M_STEP, 1024)]:
                x = self.ln_inputs(rows, D, 400 * D + rows)[0] * (2.0 / 3.0) + 5.0
                if rows == M_STEP:
                    x[5, 7], x[11, 900] = 40000.0, float("nan")   # the guard word: half range in one row, a NaN in another
                a, keep, bufs = self.row_center(mode, rows, D, x)
                self.check(lib.ser_row_center_v(C.byref(a), s()), "ser_row_center_v")
                self.emit(f"row_center {NAME[mode]} rows={rows} D={D}", **bufs)
        x = self.ln_inputs(77, 320, 9)[0]
        xd, oa, st, shf = x.to(self.dev), self.planes(FP16X, 77, 320), self.f32(77, 4), self.f32(1, 77)
        self.check(lib.ser_row_center(xd.data_ptr(), 320, oa.data_ptr(), 320, 77 * 320, st.data_ptr(), 2, shf.data_ptr(), FP16X, 77, 320, s()),
                   "ser_row_center")
        self.emit("row_center positional f16x rows=77 D=320", act=oa, stats=st, shift=shf)
        # ser_embed_ln_flagged / ser_embed_ln_masked_flagged
        for masked in (False, True):
            for mode in (BF16, FP32X, FP16X):
                for B, T, D in [(3, 7, 128), (2, 13, 1028), (3, 67, 2048), (16, 80, 1024)]:
                    for outs in ("both", "f32", "act"):
                        launch, keep, bufs = self.embed(masked, mode, B, T, D, outs, B * 1000 + T + D)
                        self.check(launch(), "ser_embed_ln")
                        self.emit(f"embed_ln{'_masked' if masked else ''} {NAME[mode]} B={B} T={T} D={D} outs={outs}", **bufs)
        # ser_pack_rows_flagged / ser_zero_padded_rows (DeBERTa's ConvLayer support)
        for mode in (BF16, FP32X, FP16X):
            for B, T, D, halo in [(3, 37, 1536, 1), (16, 80, 1024, 1), (2, 5, 4, 0)]:
                gen = self.gen(B + T + D)
                x = t.randn(B * T, D + 8, generator=gen) * 100.0
                x[1, 3] = 7.0e4
                xd, out, fl = x.to(self.dev), self.planes(mode, B * (T + 2 * halo) + 3, D + 12), self.flag()
                self.check(lib.ser_pack_rows_flagged(xd.data_ptr(), D + 8, B, T, D, halo, out.data_ptr(), D + 12, out.shape[1] * (D + 12), mode,
                                                     fl.data_ptr(), s()), "ser_pack_rows_flagged")
                self.emit(f"pack_rows {NAME[mode]} B={B} T={T} D={D} halo={halo}", act=out, flag=fl)
                kl = t.tensor([max(1, T - 2 * i) for i in range(B)], dtype=t.int32, device=self.dev)
                for which in ("both", "f32", "act"):
                    xz = x.to(self.dev) if which != "act" else None
                    az = t.randint(1, 30000, (out.shape[0], B * T, D + 12), generator=gen, dtype=t.int32).to(t.int16).to(self.dev) \
                        if which != "f32" else None
                    self.check(lib.ser_zero_padded_rows(None if xz is None else xz.data_ptr(), D + 8, None if az is None else az.data_ptr(),
                                                        D + 12, B * T * (D + 12), mode, kl.data_ptr(), B, T, D, s()), "ser_zero_padded_rows")
                    self.emit(f"zero_padded_rows {NAME[mode]} B={B} T={T} D={D} outs={which}", f32=xz, act=az)
        # ser_wave_frames_v, ser_conv0_ln_gelu, ser_pack_act_v, ser_wavlm_gate, ser_select_rows_v: their mode dispatch
        lens, k, st_ = [2000, 1205, 16000], 10, 5
        gen = self.gen(3)
        wav = t.cat([0.1 * t.randn(n, generator=gen) + 0.03 for n in lens])
        wav[100] = 9.0e4
        T_ = [(n - k) // st_ + 1 for n in lens]
        rows = sum(T_)
        wd = wav.to(self.dev)
        soffs = t.tensor([0] + list(itertools.accumulate(lens)), dtype=t.int64, device=self.dev)
        foffs = t.tensor([0] + list(itertools.accumulate(T_)), dtype=t.int32, device=self.dev)
        for mode in (BF16, FP32X, FP16X):
            for no_norm in (0, 1):
                out, fl = self.planes(mode, rows + 2, 64), self.flag()
                work = t.zeros(lib.ser_workspace_bytes(L.WS_WAVE_FRAMES, len(lens), 0, 0, 0, mode), dtype=t.uint8, device=self.dev)
                a = L.WaveFramesArgs()
                a.wav, a.sample_offs, a.frame_offs = wd.data_ptr(), soffs.data_ptr(), foffs.data_ptr()
                a.B, a.k, a.stride, a.mode, a.total_rows, a.no_norm = len(lens), k, st_, mode, rows, no_norm
                a.out, a.out_plane_stride, a.work, a.range_flag = out.data_ptr(), (rows + 2) * 64, work.data_ptr(), fl.data_ptr()
                self.check(lib.ser_wave_frames_v(C.byref(a), s()), "ser_wave_frames_v")
                self.emit(f"wave_frames {NAME[mode]} no_norm={no_norm}", act=out, flag=fl)
        xn = (t.randn(sum(lens), generator=gen)).to(self.dev)
        for mode in (BF16, FP32X):
            for Cc, kk in [(64, 10), (128, 10), (256, 3), (512, 10), (512, 16)]:
                Tk = [(n - kk) // st_ + 1 for n in lens]
                fo = t.tensor([0] + list(itertools.accumulate(Tk)), dtype=t.int32, device=self.dev)
                w = (t.randn(Cc, kk, generator=gen) * 0.5).to(self.dev)
                bv, lg, lb = (t.randn(Cc, generator=gen).to(self.dev) for _ in range(3))
                out = self.planes(mode, sum(Tk) + 2, Cc)
                self.check(lib.ser_conv0_ln_gelu(xn.data_ptr(), soffs.data_ptr(), fo.data_ptr(), len(lens), w.data_ptr(), bv.data_ptr(),
                                                 lg.data_ptr(), lb.data_ptr(), out.data_ptr(), (sum(Tk) + 2) * Cc, mode, Cc, kk, st_, sum(Tk),
                                                 s()), "ser_conv0_ln_gelu")
                self.emit(f"conv0_ln_gelu {NAME[mode]} C={Cc} k={kk}", act=out)
        for mode in (BF16, FP32X, FP16X):
            B, Cc, Tt, halo = 3, 64, 50, 2
            x = t.randn(B, Cc, Tt, generator=gen) * 50.0
            x[1, 2, 3] = 5.0e4
            xd, out, fl = x.to(self.dev), self.planes(mode, B * (Tt + 2 * halo) + 2, Cc + 4), self.flag()
            a = L.PackActArgs()
            a.x, a.out, a.ldo, a.out_plane_stride = xd.data_ptr(), out.data_ptr(), Cc + 4, out.shape[1] * (Cc + 4)
            a.B, a.C, a.T, a.halo, a.mode, a.range_flag = B, Cc, Tt, halo, mode, fl.data_ptr()
            self.check(lib.ser_pack_act_v(C.byref(a), s()), "ser_pack_act_v")
            self.emit(f"pack_act {NAME[mode]}", act=out, flag=fl)
        for mode in (BF16, FP32X, FP16):                           # any mode but fp32x reads one bf16 plane
            for rows_, H, dh in [(53, 4, 64), (M_STEP, 16, 64)]:
                x = t.randn(2, rows_, H * dh, generator=gen).to(t.bfloat16).to(self.dev)
                w8, b8 = (t.randn(8, dh, generator=gen) * 0.3).to(self.dev), (t.randn(8, generator=gen) * 0.3).to(self.dev)
                cst = t.randn(H, generator=gen).to(self.dev)
                gate = self.f32(rows_ + 2, H)
                self.check(lib.ser_wavlm_gate(x.data_ptr(), H * dh, rows_ * H * dh, mode, w8.data_ptr(), b8.data_ptr(), cst.data_ptr(),
                                              gate.data_ptr(), rows_, H, dh, s()), "ser_wavlm_gate")
                self.emit(f"wavlm_gate mode={mode} rows={rows_} H={H}", f32=gate)
        for mode in (BF16, FP32X, FP16X):
            for n_src in (1, 4):
                D, counts, src_offs, ld = 260, [5, 1, 40], [2, 60, 90], 264
                srcs = [(t.randn(140, ld, generator=gen) * 30.0).to(self.dev) for _ in range(n_src)]
                M = sum(counts)
                do = t.tensor([0, 5, 6, 46], dtype=t.int32, device=self.dev)
                so = t.tensor(src_offs, dtype=t.int32, device=self.dev)
                oa, of, fl = self.planes(mode, M + 3, D + 8), self.f32(M + 3, D + 8), self.flag()
                a = L.SelectRowsArgs()
                for i, sr in enumerate(srcs):
                    a.src[i] = sr.data_ptr()
                a.ld_src, a.src_offs, a.dst_offs = ld, so.data_ptr(), do.data_ptr()
                a.out_act, a.ldo_act, a.out_plane_stride, a.out_f32, a.ldo_f32 = oa.data_ptr(), D + 8, (M + 3) * (D + 8), of.data_ptr(), D + 8
                a.range_flag, a.n_src, a.B, a.D, a.max_rows, a.mode = fl.data_ptr(), n_src, 3, D, max(counts), mode
                self.check(lib.ser_select_rows_v(C.byref(a), s()), "ser_select_rows_v")
                self.emit(f"select_rows {NAME[mode]} n_src={n_src}", act=oa, f32=of, flag=fl)
        return self.lines

    # ---- timing
    def time_launch(self, launch, what, launches=200, warmup=20):
        t = self.t
        for _ in range(warmup):
            self.check(launch(), what)
        t.cuda.synchronize()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        t.cuda.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / launches            # us per launch

    def times(self):
        lib, s, out = self.L.lib, self.stream(), {}
        for D, mode in [(512, BF16), (512, FP16X), (1024, BF16), (1024, FP16X)]:
            x, _, g, b = self.ln_inputs(M_STEP, D, D)
            a, keep, _ = self.layernorm(mode, M_STEP, D, 0, "both", x, g, b, pad=False)
            out[f"layernorm D={D} {NAME[mode]}"] = self.time_launch(lambda: lib.ser_layernorm_v(C.byref(a), s), "ser_layernorm_v")
        for mode in (BF16, FP16X, FP16M):
            x = self.ln_inputs(M_STEP, 1024, 7)[0]
            a, keep, _ = self.row_center(mode, M_STEP, 1024, x, pad=False)
            out[f"row_center D=1024 {NAME[mode]}"] = self.time_launch(lambda: lib.ser_row_center_v(C.byref(a), s), "ser_row_center_v")
        for mode in (BF16, FP16X):
            for last in (False, True):
                x, res, g, b = self.ln_inputs(M_STEP, 768, 8)
                a, keep, _ = self.pos_ln(mode, M_STEP, 768, last, x, res, g, b, pad=False)
                out[f"pos_ln D=768 last={int(last)} {NAME[mode]}"] = self.time_launch(lambda: lib.ser_pos_ln_v(C.byref(a), s), "ser_pos_ln_v")
        for masked in (False, True):
            for mode in (BF16, FP16X):
                launch, keep, _ = self.embed(masked, mode, 16, 80, 1024, "both", 9)
                out[f"embed_ln{'_masked' if masked else ''} 16x80 D=1024 {NAME[mode]}"] = self.time_launch(launch, "ser_embed_ln")
        return out


# ====================================================================================================================== parent: the A/B
def run_child(lib_path, what):
    env = dict(os.environ, SER_HIP_LIB=os.path.abspath(lib_path))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child ({what}, {lib_path}) ended with status {p.returncode}")
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent", nargs="?")
    ap.add_argument("branch", nargs="?")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--no-times", action="store_true")
    ap.add_argument("--out", default="", help="also write the report to this file")
    ap.add_argument("--child", choices=("results", "times"))
    args = ap.parse_args()
    if args.child:
        c = Child()
        print(json.dumps({"lib": c.L.LIB_PATH, "data": c.results() if args.child == "results" else c.times()}))
        return 0
    if not args.parent or not args.branch:
        ap.error("two library paths: PARENT.so BRANCH.so")
    log = open(args.out, "w") if args.out else None

    def say(line=""):
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()

    bad = 0
    rp, rb = run_child(args.parent, "results"), run_child(args.branch, "results")
    assert rp["lib"] == os.path.abspath(args.parent) and rb["lib"] == os.path.abspath(args.branch)
    hp, hb = rp["data"], rb["data"]
    say(f"== results: parent {args.parent}, branch {args.branch}")
    for ln in hb:
        say("  " + ln)
    diff = [(p, b) for p, b in zip(hp, hb) if p != b]
    bad += len(diff) + abs(len(hp) - len(hb))
    for p, b in diff:
        say(f"  DIFFERENT  parent: {p}\n             branch: {b}")
    digest = hashlib.sha256("\n".join(hb).encode()).hexdigest()
    say(f"{len(hb)} buffers hashed per library (SHA-256 of the branch list {digest}); {len(diff)} differ, "
        f"list lengths {len(hp)} / {len(hb)}: {'IDENTICAL' if hp == hb else 'NOT IDENTICAL'}")
    if not args.no_times:
        tp, tb = [], []
        for _ in range(args.pairs):
            tp.append(run_child(args.parent, "times")["data"])
            tb.append(run_child(args.branch, "times")["data"])
        say(f"\n== times: us per launch over 200 launches after 20 warm-up launches, {args.pairs} alternating pairs of child processes")
        say(f"  {'kernel':44s} {'parent runs':>27s} {'median':>8s} {'spread':>7s}   {'branch runs':>27s} {'median':>8s}   verdict")
        for k in tp[0]:
            p, b = [r[k] for r in tp], [r[k] for r in tb]
            mp, mb, spread = statistics.median(p), statistics.median(b), max(p) - min(p)
            slower = mb > mp + spread
            bad += slower
            verdict = "SLOWER beyond the spread" if slower else ("faster beyond the spread" if mb < mp - spread else "within the spread")
            runs_p, runs_b = " ".join(f"{v:8.2f}" for v in p), " ".join(f"{v:8.2f}" for v in b)
            say(f"  {k:44s} {runs_p:>27s} {mp:8.2f} {spread:7.2f}   {runs_b:>27s} {mb:8.2f}   {verdict}")
    say(f"\n{'FAIL' if bad else 'PASS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
