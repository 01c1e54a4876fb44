"""The plain C++ of lslam_pose_graph (lidar_slam_amd/csrc/lslam_posegraph_core.h), compiled with g++ on the
CPU: the text the kernel compiles.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

The program is one evaluation and one step as posegraph_kernel makes them, serially: every block of H walks
the edge list in ascending order (posegraph_add_diag, posegraph_add_off), the damping, then the packed LDL^T
column by column through the same element functions (posegraph_col_scale, posegraph_col_element,
posegraph_col_update) and the substitutions.  H, g, the undivided column and chi live in heap arrays of
exactly the packed sizes, so an index outside the triangle is the sanitizer's error.  The bits of the damped
H, of g, of delta and of chi2 must equal tests/posegraph_ref.py's: the NumPy form and the kernel's C++ are
held to each other without a device.  N = 2 and 3 are the smallest systems, 22 and 23 give n = 63 and 66
(either side of a wave), 64 the largest triangle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import posegraph_ref as pg
from lidar_slam_amd import posegraph  # noqa: F401  (the feature under test ships this header)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_posegraph_core.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static void put(const double *v, size_t n) {
    for (size_t i = 0; i < n; i++) {
        uint64_t b;
        std::memcpy(&b, v + i, 8);
        std::printf("%016" PRIx64 " ", b);
    }
    std::printf("\n");
}

// stdin: N E damp_t damp_r, then N poses (3), N (cos, sin), E edges (i j z[3] info[6]), all as hex bit patterns
static double rd() {
    uint64_t b;
    if (std::scanf("%" SCNx64, &b) != 1) std::exit(3);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

int main() {
    int N, E;
    if (std::scanf("%d %d", &N, &E) != 2) return 3;
    const double damp_t = rd(), damp_r = rd();
    std::vector<double> P((size_t)3 * N), cs((size_t)2 * N), z((size_t)3 * E), om((size_t)6 * E), chi((size_t)E);
    std::vector<int> ij((size_t)2 * E);
    for (auto &v : P) v = rd();
    for (auto &v : cs) v = rd();
    for (int e = 0; e < E; e++) {
        if (std::scanf("%d %d", &ij[2 * e], &ij[2 * e + 1]) != 2) return 3;
        for (int q = 0; q < 3; q++) z[3 * e + q] = rd();
        for (int q = 0; q < 6; q++) om[6 * e + q] = rd();
    }
    const int n = posegraph_dim(N), nb = N - 1;
    std::vector<double> H((size_t)posegraph_tri_size(n)), g((size_t)n), u((size_t)n);
    double chi2 = 0.0;
    for (int e = 0; e < E; e++) {
        PosegraphEdge t;
        posegraph_edge(&P[3 * ij[2 * e]], &P[3 * ij[2 * e + 1]], cs[2 * ij[2 * e]], cs[2 * ij[2 * e] + 1], &z[3 * e], &om[6 * e], t);
        chi[e] = t.chi;
    }
    for (int e = 0; e < E; e++) chi2 = chi2 + chi[e];
    for (int blk = 0; blk < nb * (nb + 1) / 2; blk++) {
        int rn, cn;
        posegraph_col_element(-1, blk, rn, cn);
        if (cn > rn || rn >= nb || cn < 0) return 4;
        const int vr = rn + 1, vc = cn + 1;
        if (rn == cn) {
            double h[6] = {0, 0, 0, 0, 0, 0}, gg[3] = {0, 0, 0};
            for (int e = 0; e < E; e++) {
                const int i = ij[2 * e], j = ij[2 * e + 1];
                if (i != vr && j != vr) continue;
                PosegraphEdge t;
                posegraph_edge(&P[3 * i], &P[3 * j], cs[2 * i], cs[2 * i + 1], &z[3 * e], &om[6 * e], t);
                posegraph_add_diag(t, i == vr, h, gg);
            }
            h[0] = h[0] + damp_t, h[2] = h[2] + damp_t, h[5] = h[5] + damp_r;
            const int r0 = 3 * rn;
            int q = 0;
            for (int r = 0; r < 3; r++) {
                for (int k = 0; k <= r; k++) H.at(posegraph_tri(r0 + r, r0 + k)) = h[q++];
                g.at(r0 + r) = gg[r];
            }
        } else {
            double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int e = 0; e < E; e++) {
                const int i = ij[2 * e], j = ij[2 * e + 1];
                if (!((i == vr && j == vc) || (i == vc && j == vr))) continue;
                PosegraphEdge t;
                posegraph_edge(&P[3 * i], &P[3 * j], cs[2 * i], cs[2 * i + 1], &z[3 * e], &om[6 * e], t);
                posegraph_add_off(t, i == vr, h);
            }
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) H.at(posegraph_tri(3 * rn + r, 3 * cn + k)) = h[3 * r + k];
        }
    }
    put(H.data(), H.size());
    put(g.data(), g.size());
    // (raw pointers into vectors of the exact sizes: the sanitizer watches the element functions' indices)
    const bool ok = posegraph_solve_serial(H.data(), g.data(), u.data(), n);
    std::printf("%d\n", ok ? 1 : 0);
    for (auto &v : g) v = -v;
    put(g.data(), g.size());
    put(&chi2, 1);
    return 0;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("posegraph_core")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


def hx(v):
    return " ".join("%016x" % int(b) for b in np.ascontiguousarray(v, np.float64).reshape(-1).view(np.uint64))


def run_prog(exe, pose, cs, ij, z, info, damp_t, damp_r):
    lines = ["%d %d %s" % (len(pose), len(ij), hx([damp_t, damp_r])), hx(pose), hx(cs)]
    for e in range(len(ij)):
        lines.append("%d %d %s %s" % (ij[e, 0], ij[e, 1], hx(z[e]), hx(info[e])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[:300] + out.stderr[-4000:]
    H, g, ok, delta, chi2 = out.stdout.splitlines()[:5]
    bits = lambda s: np.array([int(v, 16) for v in s.split()], np.uint64)  # noqa: E731
    return bits(H), bits(g), int(ok), bits(delta), bits(chi2)


@pytest.mark.parametrize("N", (2, 3, 22, 23, 64))
def test_program_is_the_reference(core_exe, N):
    rng = np.random.default_rng(700 + N)
    for extra, damp in ((0, (1e-6, 1e-3)), (2 * N, (0.0, 0.0))):
        pose, ij, z, info = pg.random_graph(N, rng, extra)
        ref = pg.solve(pose, ij, z, info, n_iter=1, damp_t=damp[0], damp_r=damp[1])
        Hr, gr, delta, chi2 = ref["first"]
        cs = ref["trace"][0]
        H, g, ok, d, c2 = run_prog(core_exe, pose, cs, ij, z, info, *damp)
        n = 3 * (N - 1)
        assert ok == 1 and delta is not None
        assert np.array_equal(H, np.ascontiguousarray(Hr[np.tril_indices(n)]).view(np.uint64))
        assert np.array_equal(g, np.ascontiguousarray(gr).view(np.uint64))
        assert np.array_equal(d, np.ascontiguousarray(delta).view(np.uint64))
        assert c2[0] == np.float64(chi2).view(np.uint64)


def test_a_bad_pivot_ends_the_solve(core_exe):
    pose, ij, z, info = pg.random_graph(3, np.random.default_rng(9), 0)
    ij, z, info = ij[:1], z[:1], info[:1]  # node 2 is isolated: its pivot is +0.0 without damping
    ref = pg.solve(pose, ij, z, info, n_iter=1, damp_t=0.0, damp_r=0.0)
    assert ref["flags"] == pg.SINGULAR
    assert run_prog(core_exe, pose, ref["trace"][0], ij, z, info, 0.0, 0.0)[2] == 0
