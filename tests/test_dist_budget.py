"""The distance-field kernels keep what they hold in registers: no spills, no scratch (CPU test: needs
hipcc's llvm-readelf, no GPU; the pattern of tests/test_raycast_budget.py).  DESIGN §4.4 quotes the counts.

dist_kernel is launched with 512 threads and, at the defaults, 47,120 B of LDS (16 B of counters, the
32 KiB bitmap of a 512-cell map, eight waves' rows of d2 and g and their column masks): at least two workgroups to a CU, 16
waves, four per SIMD, which leaves a wave 128 VGPRs.  Its LDS is dynamic; fieldscore_kernel has none."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam11dist_kernelILi8EEEvNS_8DistArgsE": (128, 0),
    "_ZN5lslam11dist_kernelILi1EEEvNS_8DistArgsE": (128, 0),
    "_ZN5lslam17fieldscore_kernelENS_14FieldScoreArgsE": (128, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("dist_budget"))
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


def lds_bytes(W, band, d_max):
    """The arithmetic of lslam_dist.h: dist_blocks and dist_lds_bytes."""
    hal = min(d_max, W) - 1
    nblk = (min(W, band + 2 * hal) + 31) >> 5
    return 16 + ((4 * W * nblk + 15) & ~15) + 8 * (((W + 15) & ~15) * 3 + 256)


def test_lds_sizes():
    assert lds_bytes(512, 512, 64) == 47120 and 3 * 47120 <= 160 * 1024   # the defaults, one band per robot
    assert lds_bytes(512, 32, 64) == 24592                                # 16 bands per robot: 160 rows of bitmap
    assert lds_bytes(2048, 144, 40) <= 160 * 1024                         # the largest map at d_max 40
    # what the header documents as the limit: grid_w 1757 holds every d_max, 2048 up to 205
    assert lds_bytes(1757, 8, 255) <= 160 * 1024 < lds_bytes(1758, 8, 255)
    assert lds_bytes(2048, 8, 205) <= 160 * 1024 < lds_bytes(2048, 8, 206)
