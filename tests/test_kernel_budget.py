"""The matcher, match-fusion and relocalisation kernels keep what they hold in registers: no spills, no
scratch (CPU test: needs hipcc's llvm-readelf, no GPU).  DESIGN §4.4 quotes the counts.

The two search kernels of the correlative matcher (lslam_corr.h's loop) run at the edge of the scalar
registers, 106 of them in the scan matcher's loop, so a spill is what a change to the shared code would
show first; two 512-thread workgroups per CU, which their LDS sizes assume, leave a wave 128 VGPRs.
The match-fusion kernel holds ten 64-bit sums and the 3x3 matrices of thread 0; the relocalisation
search holds 32 sums, 8 planes and 8 windows per thread.  The search kernels' LDS is dynamic."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam19match_search_kernelENS_9MatchArgsE": (128, 0),
    "_ZN5lslam17match_pick_kernelENS_9MatchArgsE": (128, 32),
    "_ZN5lslam22mapmatch_search_kernelENS_12MapMatchArgsE": (128, 0),
    "_ZN5lslam20mapmatch_pick_kernelENS_12MapMatchArgsE": (128, 32),
    "_ZN5lslam19mapfuse_pick_kernelILi0EEEvNS_11MapFuseArgsE": (128, 352),
    "_ZN5lslam19reloc_search_kernelILi0EEEvNS_9RelocArgsE": (128, 0),
    "_ZN5lslam19reloc_search_kernelILi1EEEvNS_9RelocArgsE": (128, 0),
    "_ZN5lslam17reloc_peak_kernelENS_9RelocArgsE": (128, 32),
    "_ZN5lslam17reloc_topk_kernelENS_9RelocArgsE": (128, 32),
    "_ZN5lslam19reloc_select_kernelENS_9RelocArgsE": (128, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("kernel_budget"))
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
