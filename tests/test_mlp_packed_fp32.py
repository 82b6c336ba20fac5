"""csrc/mlp_fused_h.hip is built without packed FP32 (csrc/Makefile NOPK_SRCS) for the block
MLP's sake: its GELU and scale folds run beside the MFMAs, where the packed forms cost more
than the scalar ones they replace (profiles/r11_mlp_io).  The inner-skip
kernels live in a unit of their own, csrc/skip_h.hip, which is not in NOPK_SRCS and so keeps
packed FP32, because they measured slower without.  Both halves are one Makefile word
each and silent if lost, so this checks the built library: no v_pk_{add,mul,fma}_f32 in
any mlp_fused_h_kernel, some in skip_hp_kernel and skip_h_kernel.  CPU only: disassembles
the fat binary's gfx950 code objects."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd", "msfno_amd",
                   "libmsfno.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def packed_ops():
    """{mangled kernel symbol: number of packed-FP32 instructions} of the block-MLP
    (mlp_fused_h.hip) and inner-skip (skip_h.hip) kernels in libmsfno.so"""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    import isa_audit as A
    counts = {}
    with tempfile.TemporaryDirectory() as td:
        cos = []
        for i, (triple, elf) in enumerate(A.code_objects(LIB)):
            if "gfx950" not in triple:
                continue
            f = os.path.join(td, f"co{i}.elf")
            with open(f, "wb") as fh:
                fh.write(elf)
            cos.append(f)
        cos += A.compressed_gfx950(LIB, td)
        assert cos, "no gfx950 code object in libmsfno.so"
        for co in cos:
            out = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", co], capture_output=True,
                                 text=True, check=True).stdout
            sym = None
            for line in out.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    sym = m.group(1)
                    if re.search(r"mlp_fused_h_kernel|skip_hp?_kernel", sym):
                        counts.setdefault(sym, 0)
                elif sym in counts and A.ANY.search(line):
                    counts[sym] += 1
    return counts


def test_block_mlp_kernels_hold_no_packed_fp32(packed_ops):
    mlp = {k: v for k, v in packed_ops.items() if "mlp_fused_h_kernel" in k}
    assert len(mlp) >= 2, f"mlp_fused_h_kernel instantiations found: {sorted(mlp)}"
    assert not any(mlp.values()), mlp


def test_inner_skip_kernels_keep_packed_fp32(packed_ops):
    for name in ("skip_hp_kernel", "skip_h_kernel"):
        got = {k: v for k, v in packed_ops.items() if name in k}
        assert got and all(got.values()), (name, got)
