"""The grid recentre kernel keeps a band in registers: no spills, no scratch (CPU test: needs hipcc's
llvm-readelf, no GPU; the pattern of tests/test_raycast_budget.py).  DESIGN §4.4 quotes the counts.

recentre_kernel<0>, launched when grid_w and quantum are multiples of 8, holds eight 16-byte groups
per thread (32 VGPRs of data, 62 in all) and no LDS; recentre_kernel<1> adds the lane-per-cell path
and parks its band in 32 KiB of static LDS (68 VGPRs).  At no more than 64 VGPRs a SIMD holds eight
waves of recentre_kernel<0>, a CU eight of its 256-thread workgroups: 256 KiB in flight per CU.
recentre_kernel<1> is held to 72 (seven waves per SIMD); its LDS allows five workgroups per CU."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam15recentre_kernelILi0EEEvNS_12RecentreArgsE": (64, 0),
    "_ZN5lslam15recentre_kernelILi1EEEvNS_12RecentreArgsE": (72, 32768),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("recentre_budget"))
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


def test_a_band_is_what_a_workgroup_holds():
    """The arithmetic of lslam_recentre.h: 256 threads x 8 groups x 16 bytes = one band of 16384 cells."""
    import recentre_ref as rr
    assert 256 * 8 * 16 == rr.BAND_CELLS * 2 == 32768
    for w in (16, 64, 512, 2048):
        assert rr.band_rows(w) * (w // 8) <= 256 * 8
