"""The three kernels of relocalisation with priors keep what they hold in registers: no spills, no scratch
(CPU test: needs hipcc's llvm-readelf, no GPU).  DESIGN §4.4 quotes the counts.

relocprior_search_kernel is reloc_search_kernel<0> over the live spans: 32 sums, 8 planes and 8 windows per
thread, and the span's admissible bits; its LDS is dynamic (the bitmap, the staged points, the bits, the
task list).  relocprior_admit_kernel holds a robot's bits in 8 KiB of static LDS (2048 dwords: Wc <= 256
rows of at most 8 spans) and a 4-byte counter; relocprior_select_kernel is one thread per robot."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs: the count DESIGN quotes, rounded up to the next allocation step of 8; static LDS bytes)
KERNELS = {
    "_ZN5lslam23relocprior_admit_kernelILi0EEEvNS_14RelocPriorArgsE": (48, 8196),
    "_ZN5lslam24relocprior_search_kernelILi0EEEvNS_14RelocPriorArgsE": (96, 0),
    "_ZN5lslam24relocprior_select_kernelILi0EEEvNS_14RelocPriorArgsE": (40, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("relocprior_budget"))
    so = os.path.join(tmp, "lib.so")
    shutil.copy(build.build(verbose=False), so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=tmp,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = [f for f in os.listdir(tmp) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, co[0])], text=True)
    # one YAML map per kernel, keys in alphabetical order: .group_segment_fixed_size precedes .name, the rest follow
    return re.split(r"\n\s+- \.", text)


@pytest.mark.parametrize("symbol", sorted(KERNELS))
def test_kernel_has_no_spills_and_no_scratch(notes, symbol):
    max_vgpr, lds = KERNELS[symbol]
    mine = [b for b in notes if re.search(r"\.name:\s+%s\s" % re.escape(symbol), b)]
    assert len(mine) == 1, "%s is missing from the code object" % symbol
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.?(\w+):\s+(\d+)\s*\n", mine[0])}
    print(symbol, {n: k[n] for n in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= max_vgpr and k["group_segment_fixed_size"] == lds, k


def test_the_new_kernels_stand_behind_every_other(notes):
    """The rule at the include of lslam_launch_map.h: a new kernel takes the code object's end, so that no
    kernel moves against another."""
    names = [m.group(1) for b in notes for m in [re.search(r"\.name:\s+(\S+)\s", b)] if m]
    assert len(names) > len(KERNELS) and set(names[-len(KERNELS):]) == set(KERNELS), names[-5:]
