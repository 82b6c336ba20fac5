"""The kernels bench.py looks up by their full demangled names (its STAGE_KERNEL_*
dicts; profiles/ and DESIGN.md §4 use the same names) exist in the built library.

Retiring a kernel variant means not instantiating it, never changing a kernel's
template parameter list: that would rename every instantiation and silently
empty the per-stage rows of the roofline.  CPU only: lists the function symbols of
the fat binary's gfx950 code objects."""
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import REPO

sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import bench  # noqa: E402

LIB = os.path.join(REPO, "modulated-spherical-fourier-neural-operator_amd", "msfno_amd",
                   "libmsfno.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

# (dict, stages): every stage of the x3h and linear tables; of the x6 table the stages
# whose names the default build has always carried
TABLES = [
    ("STAGE_KERNEL_X3H", sorted(bench.STAGE_KERNEL_X3H)),
    ("STAGE_KERNEL_LINEAR", sorted(bench.STAGE_KERNEL_LINEAR)),
    ("STAGE_KERNEL_X6", ["mlp_fc1", "mlp_fc2", "mlp_fused"]),
]


@pytest.fixture(scope="module")
def kernel_symbols():
    """Demangled function symbols of every gfx950 code object in libmsfno.so."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    import isa_audit as A
    lines = []
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
            out = subprocess.run([OBJDUMP, "-t", "-C", co], capture_output=True, text=True,
                                 check=True).stdout
            lines += [ln for ln in out.splitlines() if " F " in ln and ".text" in ln]
    assert lines, "no function symbol in the gfx950 code objects"
    return lines


@pytest.mark.parametrize("table,stage", [(t, s) for t, stages in TABLES for s in stages])
def test_bench_stage_kernel_is_in_the_library(kernel_symbols, table, stage):
    names = getattr(bench, table)[stage]
    names = (names,) if isinstance(names, str) else names
    assert any(n in ln for n in names for ln in kernel_symbols), (
        f"bench.{table}[{stage!r}]: none of {names} is a kernel of libmsfno.so")
