"""The plain C++ of the map merge (lidar_slam_amd/csrc/lslam_gridmerge_plan.h), compiled with g++ on the
CPU: the text the kernels compile.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

The program is the kernels' two passes over heap arrays of exactly the grids' sizes: for every slice of
the pair's tiles, every cell of every tile gathers its source cell through merge_src_cell, is classed
with merge_near_occupied and merged with merge_value, as gridmerge_kernel does it.  An index outside
either array is an error there (the sanitizer's, and the program's own count).  It also counts how often
each destination cell is visited: the tiles of all slices must cover the map once.  Its dst, stats and
flags must equal tests/gridmerge_ref.py's, so the NumPy form and the kernels' C++ are held to each other
without a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gridmerge_ref as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_gridmerge_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv: W Sw want occ_min fill dry l_min l_max min_support max_permille cell, then 8 doubles (c s tx ty oxd oyd oxs oys);
// stdin: Sw*Sw source values, W*W destination values
int main(int argc, char **argv) {
    if (argc != 20) return 2;
    const int W = std::atoi(argv[1]), Sw = std::atoi(argv[2]), want = std::atoi(argv[3]), occ_min = std::atoi(argv[4]);
    const int fill = std::atoi(argv[5]), dry = std::atoi(argv[6]), l_min = std::atoi(argv[7]), l_max = std::atoi(argv[8]);
    const int min_support = std::atoi(argv[9]), max_permille = std::atoi(argv[10]);
    MergeXform t;
    t.cell = std::atof(argv[11]);
    t.inv = 1.0 / t.cell;
    t.c = std::atof(argv[12]), t.s = std::atof(argv[13]), t.tx = std::atof(argv[14]), t.ty = std::atof(argv[15]);
    t.oxd = std::atof(argv[16]), t.oyd = std::atof(argv[17]), t.oxs = std::atof(argv[18]), t.oys = std::atof(argv[19]);
    t.src_w = Sw;
    std::vector<int16_t> S((size_t)Sw * Sw), L((size_t)W * W);
    for (auto &v : S) { int x; if (std::scanf("%d", &x) != 1) return 3; v = (int16_t)x; }
    for (auto &v : L) { int x; if (std::scanf("%d", &x) != 1) return 3; v = (int16_t)x; }
    std::vector<int> seen((size_t)W * W);
    long bad = 0;
    int st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int flags = 0;
    if (!merge_xform_finite(t)) {
        flags = 16;
    } else {
        const int nt = merge_tiles(W), per = merge_slice_tiles(nt, want), ns = merge_slices(nt, per);
        if (per < 1 || (long)ns * per < nt || (ns - 1) * per >= nt) bad++;
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                flags = merge_gates(st[MERGE_SUPP], st[MERGE_CONTRA], min_support, max_permille);
                if (flags || dry) break;
                flags = 1;
            }
            for (int slice = 0; slice < ns; slice++) {
                const int t0 = slice * per, t1 = t0 + per < nt ? t0 + per : nt;
                for (int ti = t0; ti < t1; ti++) {
                    const MergeTile q = merge_tile(W, ti);
                    if (q.x0 < 0 || q.x0 >= q.x1 || q.x1 > W || q.y0 < 0 || q.y0 >= q.y1 || q.y1 > W) { bad++; continue; }
                    for (int Y = q.y0; Y < q.y1; Y++)
                        for (int X = q.x0; X < q.x1; X++) {
                            const int sc = merge_src_cell(t, merge_world(t.oxd, X, t.cell), merge_world(t.oyd, Y, t.cell));
                            if (sc >= Sw * Sw) { bad++; continue; }
                            const int v = sc >= 0 ? (int)S[(size_t)sc] : 0, l = (int)L[(size_t)Y * W + X];
                            if (pass == 0) {
                                seen[(size_t)Y * W + X]++;
                                st[MERGE_ON] += sc >= 0;
                                st[MERGE_NZ] += v != 0;
                                if (v >= occ_min) {
                                    if (merge_near_occupied(L.data(), W, X, Y, occ_min)) st[MERGE_SUPP]++;
                                    else if (l < 0) st[MERGE_CONTRA]++;
                                    else st[MERGE_NEW]++;
                                }
                                const bool both = v != 0 && l != 0;
                                st[MERGE_SAME] += both && (v < 0) == (l < 0);
                                st[MERGE_OPP] += both && (v < 0) != (l < 0);
                            } else {
                                const int nv = merge_value(l, v, fill, l_min, l_max);
                                st[MERGE_CHANGED] += nv != l;
                                L[(size_t)Y * W + X] = (int16_t)nv;
                            }
                        }
                }
            }
        }
        for (int n : seen) bad += n != 1;
    }
    std::printf("%ld %d", bad, flags);
    for (int k = 0; k < 8; k++) std::printf(" %d", st[k]);
    std::printf("\n");
    for (size_t i = 0; i < L.size(); i++) std::printf("%d ", (int)L[i]);
    std::printf("\n");
    return bad != 0;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("gridmerge_plan")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


def run_prog(exe, src, dst, xform, so, do, want=1, cell=20.0, **kw):
    p = dict(gm.DEFAULTS, **kw)
    args = [dst.shape[0], src.shape[0], want, p["occ_min"], int(p["mode"] == gm.FILL), int(p["dry_run"]), p["l_min"], p["l_max"],
            p["min_support"], p["max_contra_permille"]]
    nums = [cell] + list(xform) + list(do) + list(so)
    text = " ".join(str(int(v)) for v in src.ravel()) + "\n" + " ".join(str(int(v)) for v in dst.ravel()) + "\n"
    out = subprocess.run([exe] + [str(a) for a in args] + [repr(float(v)) for v in nums], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[:300] + out.stderr[-4000:]
    head, body = out.stdout.splitlines()[:2]
    head = [int(v) for v in head.split()]
    assert head[0] == 0
    return {"flags": head[1], "stats": np.array(head[2:], np.int32),
            "dst": np.array(body.split(), np.int64).astype(np.int16).reshape(dst.shape)}


def rot(th, tx=0.0, ty=0.0):
    return (float(np.cos(th)), float(np.sin(th)), tx, ty)


CASES = [
    # W, Sw, transform, source origin, destination origin, slices wanted, params
    (16, 16, rot(0.0), (0.0, 0.0), (0.0, 0.0), 1, {}),
    (24, 40, rot(0.4, 130.0, -75.0), (-400.0, -400.0), (-240.0, -240.0), 3, {}),
    (52, 16, rot(3.1, 40.0, 10.0), (-160.0, -160.0), (-520.0, -520.0), 2, dict(mode=gm.FILL)),
    (70, 80, rot(-2.0, 0.0, 333.3), (-800.0, -800.0), (-700.0, -700.0), 5, {}),
    (130, 40, (0.0, 1.0, 0.0, 0.0), (-400.0, -400.0), (-1300.0, -1300.0), 7, {}),       # an exact quarter turn
    (64, 16, rot(0.4, 1e5, 0.0), (0.0, 0.0), (0.0, 0.0), 1000, {}),                     # wholly off the source
    (33, 16, (1.0, 0.0, 1e300, -1e300), (0.0, 0.0), (0.0, 0.0), 4, {}),                 # far: nothing converts
    (33, 16, (1e300, 1e300, 1e300, 1e300), (0.0, 0.0), (0.0, 0.0), 4, {}),              # inf - inf: a NaN fails the test
    (16, 16, (float("nan"), 0.0, 0.0, 0.0), (0.0, 0.0), (0.0, 0.0), 1, {}),
    (16, 16, rot(0.3), (float("inf"), 0.0), (0.0, 0.0), 1, {}),
    (40, 40, rot(0.2, 3.0, 4.0), (-400.0, -400.0), (-400.0, -400.0), 2, dict(dry_run=True)),
    (40, 40, rot(0.2, 3.0, 4.0), (-400.0, -400.0), (-400.0, -400.0), 2, dict(min_support=10 ** 6)),
    (40, 40, rot(0.2, 3.0, 4.0), (-400.0, -400.0), (-400.0, -400.0), 2, dict(max_contra_permille=0)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_program_is_the_reference(plan_exe, case):
    W, Sw, xf, so, do, want, kw = CASES[case]
    rng = np.random.default_rng(100 + case)
    # sparse and signed, like a map: most cells free or unknown, some occupied, values beyond the clamps too
    src = np.where(rng.random((Sw, Sw)) < 0.3, rng.integers(-400, 401, (Sw, Sw)), 0).astype(np.int16)
    dst = np.where(rng.random((W, W)) < 0.5, rng.integers(-400, 401, (W, W)), 0).astype(np.int16)
    kw = dict(dict(min_support=0, max_contra_permille=1000), **kw)
    got = run_prog(plan_exe, src, dst, xf, so, do, want=want, **kw)
    ref = gm.merge(src, so, dst, do, xf, **kw)
    assert got["flags"] == ref["flags"] and got["stats"].tolist() == ref["stats"].tolist(), (got["flags"], got["stats"], ref["stats"])
    assert np.array_equal(got["dst"], ref["dst"])


def test_tiles_of_every_width(plan_exe):
    """Widths from 16 to 130, on and off the tile sides: the program's own count of visits (once a cell)
    passes for the slice counts a launch can ask for."""
    src = np.ones((16, 16), np.int16)
    for W in list(range(16, 131, 7)) + [128, 129]:
        for want in (1, 2, W):
            got = run_prog(plan_exe, src, np.zeros((W, W), np.int16), rot(0.0), (0.0, 0.0), (0.0, 0.0), want=want, mode=gm.FILL,
                           min_support=0)
            assert got["stats"][0] == 256 and got["stats"][7] == 256
