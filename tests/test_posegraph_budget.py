"""The pose-graph kernel's registers and its place (CPU test: needs hipcc's llvm-readelf, no GPU; the pattern of
tests/test_gridpoints_budget.py).

posegraph_kernel<0>: one 256-thread workgroup a graph, everything in dynamic LDS: static LDS is exactly 0 (the
workgroup OR is an LDS word of the dynamic block, not a library reduction with static LDS of its own), no
scratch, and no spill of either kind.  Built at 153 VGPRs and 99 SGPRs: an edge's terms are 43 doubles, and the
kernel keeps its pointers and sizes in vector registers because cos and sin's constants fill the scalar ones.
The ceilings (158 and 104) leave the compiler a few registers and stay at three waves a SIMD (170 VGPRs), which is what
the LDS of a 24-node graph allows anyway.  The kernel's arguments are 152 bytes."""
import os
import re
import shutil
import subprocess

import pytest

from lidar_slam_amd import posegraph  # noqa: F401  (the feature under test)

LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOL = "_ZN5lslam16posegraph_kernelILi0EEEvNS_13PoseGraphArgsE"
MAX_SGPR, MAX_VGPR = 104, 158

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("posegraph_budget"))
    so = os.path.join(tmp, "lib.so")
    shutil.copy(build.build(verbose=False), so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=tmp,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = [f for f in os.listdir(tmp) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], text=True)
    return re.split(r"\n\s+- \.", text)


def test_registers(notes):
    mine = [b for b in notes if re.search(r"\.name:\s+%s\s" % re.escape(SYMBOL), b)]
    assert len(mine) == 1, "%s is missing from the code object" % SYMBOL
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.?(\w+):\s+(\d+)\s*\n", mine[0])}
    print({n: k[n] for n in ("sgpr_count", "vgpr_count", "sgpr_spill_count", "group_segment_fixed_size", "kernarg_segment_size")})
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["sgpr_count"] <= MAX_SGPR and k["vgpr_count"] <= MAX_VGPR and k["group_segment_fixed_size"] == 0, k
    assert k["kernarg_segment_size"] == 152, k


def test_the_kernel_stands_directly_ahead_of_the_gridpoints_kernels(notes):
    """One instantiation, directly ahead of the four gridpoints kernels, which tests/test_gridpoints_budget.py
    holds to the places -11..-8: every kernel before it keeps its place against the others."""
    names = [m.group(1) for b in notes for m in [re.search(r"\.name:\s+(\S+)\s", b)] if m and ".symbol" in b]
    mine = [i for i, n in enumerate(names) if "posegraph_kernel" in n]
    assert mine == [len(names) - 12], (mine, names[-13:])
    assert all("gridpoints_kernel" in n for n in names[-11:-7]), names[-11:-7]
