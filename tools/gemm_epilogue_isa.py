#!/usr/bin/env python3
"""Static instruction table of ser_gemm's kernels from hipcc's assembly (no GPU).

    cd interspeech_ser_amd/csrc && hipcc <the Makefile's CXXFLAGS> -save-temps -c gemm.hip -o /tmp/gemm.o
    python tools/gemm_epilogue_isa.py gemm-hip-amdgcn-amd-amdhsa-gfx950.s [more.s ...]

Per kernel: template arguments, VGPRs, scratch bytes, instructions from the first to the last v_mfma (the K loop), and for the
instructions behind the last v_mfma (the epilogue) the VALU count, v_cndmask, s_*_saveexec, branches, 64-bit address operations and the
kernel's code bytes.  Used for profiles/epilogue_classes.txt."""
import re
import subprocess
import sys

ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_u32", "v_addc_co_u32", "v_lshlrev_b64")


def kernels(path):
    name, body, meta = None, [], {}
    with open(path) as f:
        for line in f:
            s = line.strip()
            m = re.match(r"^(_Z\w*ser_gemm_kernel\w*):", s)
            if m and name is None:
                name, body, meta = m.group(1), [], {}
                continue
            if name is None:
                continue
            if s.startswith(".amdhsa_next_free_vgpr"):
                meta["vgpr"] = int(s.split()[1])
            elif s.startswith(".amdhsa_accum_offset"):
                meta["accum"] = int(s.split()[1])
            elif s.startswith(".amdhsa_private_segment_fixed_size"):
                meta["scratch"] = int(s.split()[1])
            elif s.startswith("; codeLenInByte"):           # "Kernel info" follows the kernel descriptor
                meta["bytes"] = int(s.split("=")[1])
                yield name, body, meta
                name = None
            elif s and not s.startswith((".", ";")) and not s.endswith(":") and "vgpr" not in meta:
                body.append(s.split()[0])


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r".*ser_gemm_kernel<(.*)>\(.*", r"\1", o) for o in out]


def main():
    rows = []
    for path in sys.argv[1:]:
        rows += list(kernels(path))
    print("WM,WN,TM,TN,BK,ST,MODE,LNEPI,OM,EPI | vgpr scratch | kloop | epilogue: valu cndmask saveexec branch addr64 | code bytes")
    for (name, body, meta), targs in zip(rows, demangle([r[0] for r in rows])):
        mf = [i for i, op in enumerate(body) if op.startswith("v_mfma")]
        epi = body[mf[-1] + 1:]
        valu = sum(op.startswith("v_") for op in epi)
        print(f"{targs:44s} | {meta.get('vgpr', -1):3d} {meta.get('scratch', -1):4d} | {mf[-1] - mf[0] + 1:5d} | {valu:5d} "
              f"{sum(op.startswith('v_cndmask') for op in epi):4d} {sum('saveexec' in op for op in epi):4d} "
              f"{sum(op.startswith('s_cbranch') for op in epi):4d} {sum(op.startswith(ADDR64) for op in epi):4d} | {meta.get('bytes', -1)}")


if __name__ == "__main__":
    main()
