"""The closure gate's kernel: its registers and its place (CPU test: needs hipcc's llvm-readelf, no GPU; the pattern
of tests/test_posegraph_budget.py).

posegate_kernel<0>: one 256-thread workgroup a graph, everything in dynamic LDS: static LDS is exactly 0, no
scratch, and no spill of either kind.  Built at 126 VGPRs and 84 SGPRs (BUILT_VGPR, BUILT_SGPR); the
ceilings (131 and 89) are those plus five, the margin tests/test_posegraph_budget.py gives, and stay at three waves a SIMD
(170 VGPRs), which is what the LDS of a 24-node graph allows anyway.  The kernel's arguments are 192 bytes: the
batch (144), the params (40) and the candidates of a block."""
import os
import re
import shutil
import subprocess

import pytest

from lidar_slam_amd import _lib

LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOL = "_ZN5lslam15posegate_kernelILi0EEEvNS_12PoseGateArgsE"
BUILT_SGPR, BUILT_VGPR = 84, 126
MAX_SGPR, MAX_VGPR = BUILT_SGPR + 5, BUILT_VGPR + 5

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    assert "lslam_pose_graph_gate" in _lib.EXPORTS  # (the feature under test)
    tmp = str(tmp_path_factory.mktemp("posegate_budget"))
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
    assert k["kernarg_segment_size"] == 192, k


def test_the_kernel_stands_directly_ahead_of_the_pose_graph_kernel(notes):
    """One instantiation at the place -13, directly ahead of posegraph_kernel<0>, which tests/test_posegraph_budget.py
    holds to the place -12: every kernel before it keeps its place against the others."""
    names = [m.group(1) for b in notes for m in [re.search(r"\.name:\s+(\S+)\s", b)] if m and ".symbol" in b]
    mine = [i for i, n in enumerate(names) if "posegate_kernel" in n]
    assert mine == [len(names) - 13], (mine, names[-14:])
    assert "posegraph_kernel" in names[-12], names[-13:]
