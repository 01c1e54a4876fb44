"""The paged recentre kernel's registers (CPU test: needs hipcc's llvm-readelf, no GPU; the pattern of
tests/test_recentre_budget.py).  DESIGN §5 has the measurement behind the bound on the scalar
registers.

page_recentre_kernel<0>, the instantiation of the defaults, is held to 80 SGPRs (an attribute on the
kernel) and to 64 VGPRs, no scratch, no LDS: with 100 SGPRs, what the compiler takes when left alone, a
fleet at rest cost 0.0076 ms against the plain call's 0.0068 ms, and 0.0070 ms once held to 80.
Scalars parked in the lanes of a vector register are counted as SGPR spills and are wanted here; VGPR spills and scratch are not.  page_recentre_kernel<1> carries recentre_move's 32 KiB of LDS,
which holds it to five workgroups a CU whatever its registers."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most SGPRs, most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam20page_recentre_kernelILi0EEEvNS_8PageArgsE": (80, 64, 0),
    "_ZN5lslam20page_recentre_kernelILi1EEEvNS_8PageArgsE": (104, 72, 32768),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("page_budget"))
    so = os.path.join(tmp, "lib.so")
    shutil.copy(build.build(verbose=False), so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=tmp,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = [f for f in os.listdir(tmp) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], text=True)
    return re.split(r"\n\s+- \.", text)


@pytest.mark.parametrize("symbol", sorted(KERNELS))
def test_registers(notes, symbol):
    max_sgpr, max_vgpr, lds = KERNELS[symbol]
    mine = [b for b in notes if re.search(r"\.name:\s+%s\s" % re.escape(symbol), b)]
    assert len(mine) == 1, "%s is missing from the code object" % symbol
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.?(\w+):\s+(\d+)\s*\n", mine[0])}
    print(symbol, {n: k[n] for n in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "group_segment_fixed_size", "kernarg_segment_size")})
    assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["sgpr_count"] <= max_sgpr and k["vgpr_count"] <= max_vgpr and k["group_segment_fixed_size"] == lds, k
    assert k["kernarg_segment_size"] == 120, k
