"""The field-fusion kernel keeps its matrices in registers: no spills, no scratch, no LDS (CPU test: needs
hipcc's llvm-readelf, no GPU; the pattern of tests/test_fieldalign_budget.py).  DESIGN §4.4 quotes the
counts.

fieldfuse_kernel runs one thread per robot, 64 to a workgroup: steps 5-11 of lslam_field_fuse as
straight-line FP64 code (lslam_fieldfuse_core.h), a dozen 3 x 3 matrices live at once.  Written with
branches around the failed inverses it kept info and info_f in 144 bytes of scratch; with selects it
compiles to 120 VGPRs, 58 SGPRs and none.  The cap is that compiled figure: a fleet of 4096 is 64 waves
on a chip of 1024 SIMDs, so occupancy is not what the cap protects; a growth would mean that a matrix
has left the registers."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# kernel -> (most VGPRs, static LDS bytes)
KERNELS = {
    "_ZN5lslam16fieldfuse_kernelILi0EEEvNS_13FieldFuseArgsE": (120, 0),
}

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from lidar_slam_amd import build
    tmp = str(tmp_path_factory.mktemp("fieldfuse_budget"))
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
