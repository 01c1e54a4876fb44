"""The field-alignment kernel keeps what it holds in registers: no spills, no scratch (CPU test: needs
hipcc's llvm-readelf, no GPU; the pattern of tests/test_dist_budget.py).  DESIGN §4.4 quotes the counts.

fieldalign_kernel runs one wave per robot, four to a 256-thread workgroup, with no LDS at all: the ten
64-bit sums are reduced by the wave's butterfly and every lane makes the same step.  It is designed for
four waves per SIMD (4096 robots are four waves on each of the chip's 1024 SIMDs), which leaves a wave
128 VGPRs."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam17fieldalign_kernelENS_14FieldAlignArgsE": (128, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("fieldalign_budget"))
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
