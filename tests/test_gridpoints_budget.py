"""The map-as-revolution kernels' registers (CPU test: needs hipcc's llvm-readelf, no GPU; the pattern of
tests/test_gridmerge_budget.py).

gridpoints_kernel<CELLS, WRITE>: one wave a workgroup, so there is no cross-wave prefix and the design
holds no LDS at all: static LDS is exactly 0 in every instantiation, and no scratch.  The count pass keeps a
unit's occupancy mask, the range mask and two counters: built at 16 and 15 VGPRs, 40 and 38 SGPRs.  The write
pass adds the ordinals and a point: built at 22 VGPRs, 60 and 57 SGPRs.  The ceilings leave the compiler a
few registers and keep every instantiation far inside eight waves a SIMD (64 VGPRs).  The kernel's arguments
are 112 bytes."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most SGPRs, most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam17gridpoints_kernelILi8ELb0EEEvNS_14GridPointsArgsE": (48, 24, 0),
    "_ZN5lslam17gridpoints_kernelILi8ELb1EEEvNS_14GridPointsArgsE": (64, 32, 0),
    "_ZN5lslam17gridpoints_kernelILi1ELb0EEEvNS_14GridPointsArgsE": (48, 24, 0),
    "_ZN5lslam17gridpoints_kernelILi1ELb1EEEvNS_14GridPointsArgsE": (64, 32, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("gridpoints_budget"))
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
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["sgpr_count"] <= max_sgpr and k["vgpr_count"] <= max_vgpr and k["group_segment_fixed_size"] == lds, k
    assert k["kernarg_segment_size"] == 112, k


def test_the_kernels_stand_directly_ahead_of_the_merge_kernels(notes):
    """The four instantiations stand together, directly ahead of the merge's four kernels, which
    tests/test_gridmerge_budget.py holds to the places -7..-4: every kernel before them keeps its place."""
    names = [m.group(1) for b in notes for m in [re.search(r"\.name:\s+(\S+)\s", b)] if m and ".symbol" in b]
    assert len(names) > 24
    mine = [i for i, n in enumerate(names) if "gridpoints_kernel" in n]
    assert mine == list(range(len(names) - 11, len(names) - 7)), (mine, names[-12:])
    assert all("gridmerge_kernel" in n for n in names[-7:-3]), names[-7:-3]
