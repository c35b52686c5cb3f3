"""ser_gemm on the four encoder-layer launches of WavLM-large at 16 x 10 s (M = 7 984) IN THE FORM THE LAYERS LAUNCH THEM, one launch at a
time (tools/, GPU):     [SER_HIP_LIB=<another build>] python tools/gemm_epilogue_bench.py [M]
  qkv: deferred LayerNorm, q columns scaled, operand copy              (epilogue class LN_ACT)
  out: residual, fp32 state, shifted operand copy + row partials       (RESID)
  fc1: deferred LayerNorm, GELU, operand copy                          (LN_ACT)
  fc2: as out                                                          (RESID)
in bf16 and FP16M operands.  tools/gemm_f16m_bench.py times the same shapes without these epilogue features (which is the GENERIC class);
this one is the A/B of the epilogue classes between two builds of the library (profiles/epilogue_classes.txt)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from interspeech_ser_amd import _lib as L                     # noqa: E402

DEV = "cuda:0"
M = int(sys.argv[1]) if len(sys.argv) > 1 else 7984
SHAPES = [("qkv", 3072, 1024, "ln"), ("out", 1024, 1024, "res"), ("fc1", 4096, 1024, "ln"), ("fc2", 1024, 4096, "res")]
MODES = [("bf16", 1), ("f16m", 6)]


def operand(rows, cols, mode, weight, st):
    x = torch.randn(rows, cols, device=DEV) * (0.03 if weight else 1.0)
    if mode == 6:
        t = torch.zeros((2, rows, cols), dtype=torch.float16, device=DEV)
        s = torch.zeros((cols // 64, rows), dtype=torch.int32, device=DEV)
        L.check(L.lib.ser_pack_f16m(x.data_ptr(), cols, rows, cols, t.data_ptr(), cols, rows * cols, s.data_ptr(), rows, int(weight), None, st), "pack")
        return x, t, s
    t = torch.zeros((1, rows, cols), dtype=torch.bfloat16, device=DEV)
    L.check(L.lib.ser_split_bf16(x.data_ptr(), t.data_ptr(), rows * cols, mode, rows * cols, st), "split")
    return x, t, None


def main():
    st = torch.cuda.current_stream().cuda_stream
    print(f"M = {M}; microseconds per launch (median of 5 x 20 launches), library {os.environ.get('SER_HIP_LIB', '(in tree)')}")
    for name, N, K, form in SHAPES:
        row = []
        for mname, mode in MODES:
            x, A, As = operand(M, K, mode, False, st)
            _, W, Ws = operand(N, K, mode, True, st)
            planes = 2 if mode == 6 else 1
            oa = torch.zeros((planes, M, N), dtype=torch.bfloat16 if mode == 1 else torch.float16, device=DEV)
            osc = torch.zeros((N // 64, M), dtype=torch.int32, device=DEV)
            bias, colsum = torch.randn(N, device=DEV) * 0.1, torch.randn(N, device=DEV) * 0.1
            G = (N + 63) // 64
            keep = [bias, colsum]
            g = L.GemmArgs()
            g.A, g.a_plane_stride, g.lda = A.data_ptr(), M * K, K
            g.W, g.w_plane_stride = W.data_ptr(), N * K
            g.M, g.N, g.K, g.groups, g.mode, g.c_group_stride = M, N, K, 1, mode, N
            g.bias = bias.data_ptr()
            g.out_act, g.ldo_act, g.out_plane_stride = oa.data_ptr(), N, M * N
            if mode == 6:
                g.a_scale, g.a_scale_ld, g.w_scale, g.w_scale_ld = As.data_ptr(), M, Ws.data_ptr(), N
                g.out_scale, g.out_scale_ld = osc.data_ptr(), M
            if form == "ln":
                stats = torch.zeros(M, 2, 2, device=DEV)
                stats[:, 0, 0], stats[:, 0, 1] = x.sum(1), (x * x).sum(1)
                shift, mean = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
                keep += [stats, shift, mean]
                g.ln_stats_in, g.ln_groups, g.ln_colsum, g.ln_eps = stats.data_ptr(), 2, colsum.data_ptr(), 1e-5
                g.ln_shift, g.mean_out = shift.data_ptr(), mean.data_ptr()
                if name == "qkv":
                    g.col_scale, g.col_scale_end = 0.18, 1024
                else:
                    g.act = L.ACT_GELU
            else:
                res, state = torch.randn(M, N, device=DEV), torch.zeros(M, N, device=DEV)
                part = torch.zeros(M, G + (G & 1), 2, device=DEV)
                s_in, s_out = torch.zeros(M, device=DEV), torch.zeros(M, device=DEV)
                keep += [res, state, part, s_in, s_out]
                g.residual, g.ldr, g.out_f32, g.ldo_f32 = res.data_ptr(), N, state.data_ptr(), N
                g.stat_out, g.stat_groups = part.data_ptr(), G + (G & 1)
                g.shift_in, g.shift_out, g.shift_const = s_in.data_ptr(), s_out.data_ptr(), 0.0
            ts = []
            for rep in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    L.check(L.lib.ser_gemm(C.byref(g), st), "ser_gemm")
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1000 / 20)
            t = sorted(ts[1:])[2]
            row.append(f"{mname} {t:7.1f} us ({2.0 * M * N * K / t / 1e6:6.0f} TF/s)")
        print(f"  {name:4s} N={N:5d} K={K:5d}: " + "   ".join(row))


if __name__ == "__main__":
    main()
