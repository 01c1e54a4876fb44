"""The match-fusion kernel keeps its ten 64-bit sums and the 3x3 matrices of thread 0 in registers:
no spills, no scratch (CPU test: needs hipcc's llvm-readelf, no GPU).  DESIGN §4.4 quotes the counts."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOL = "_ZN5lslam19mapfuse_pick_kernelILi0EEEvNS_11MapFuseArgsE"

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-readelf")), reason="needs llvm-readelf")


def test_mapfuse_pick_kernel_has_no_spills_and_no_scratch(tmp_path):
    from lidar_slam_amd import build
    so = str(tmp_path / "lib.so")
    shutil.copy(build.build(verbose=False), so)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], cwd=str(tmp_path),
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    co = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert co, "no gfx950 code object in the library"
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / co[0])], text=True)
    # one YAML map per kernel, keys in alphabetical order: .group_segment_fixed_size precedes .name, the rest follow
    blocks = re.split(r"\n\s+- \.", text)
    mine = [b for b in blocks if re.search(r"\.name:\s+%s\s" % re.escape(SYMBOL), b)]
    assert len(mine) == 1, "mapfuse_pick_kernel is missing from the code object"
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.?(\w+):\s+(\d+)\s*\n", mine[0])}
    print({n: k[n] for n in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 128 and k["group_segment_fixed_size"] == 352, k
