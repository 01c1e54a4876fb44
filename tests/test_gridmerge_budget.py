"""The map merge kernels' registers (CPU test: needs hipcc's llvm-readelf, no GPU; the pattern of
tests/test_page_budget.py).

gridmerge_kernel<CELLS, APPLY>: no LDS and no scratch in any instantiation; the direct gather keeps
nothing between cells.  The statistics pass with 8 cells a thread holds 8 gathers and 7 counters: at most
64 VGPRs, so eight waves a SIMD stay possible; the compiler parks some scalars in the lanes of a vector
register there (counted as SGPR spills, and harmless: they are not scratch); VGPR spills and scratch are
not allowed.  The merge pass is half of that.  The kernel's arguments are 136 bytes."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most SGPRs, most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam16gridmerge_kernelILi8ELb0EEEvNS_9MergeArgsE": (106, 64, 0),
    "_ZN5lslam16gridmerge_kernelILi8ELb1EEEvNS_9MergeArgsE": (72, 48, 0),
    "_ZN5lslam16gridmerge_kernelILi1ELb0EEEvNS_9MergeArgsE": (106, 48, 0),
    "_ZN5lslam16gridmerge_kernelILi1ELb1EEEvNS_9MergeArgsE": (72, 32, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("gridmerge_budget"))
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
    assert k["kernarg_segment_size"] == 136, k


def test_the_merge_kernels_stand_ahead_of_the_relocalisation_priors(notes):
    """The four instantiations stand together, directly ahead of the relocalisation priors' three kernels, which
    tests/test_relocprior_budget.py holds to the code object's end: every kernel before them keeps its place."""
    names = [m.group(1) for b in notes for m in [re.search(r"\.name:\s+(\S+)\s", b)] if m and ".symbol" in b]
    assert len(names) > 20
    mine = [i for i, n in enumerate(names) if "gridmerge_kernel" in n]
    assert mine == list(range(len(names) - 7, len(names) - 3)), (mine, names[-8:])
    assert all("relocprior" in n for n in names[-3:]), names[-3:]
