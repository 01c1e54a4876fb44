"""The plain C++ of lslam_pose_graph_gate (lidar_slam_amd/csrc/lslam_posegate_core.h), compiled with g++ on the
CPU: the text the kernel compiles.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them; nothing loaded into
Python is built that way.

The program is posegate_graph_serial, the whole call for one graph as posegate_kernel makes it, serially: the
evaluation and the packed LDL^T through lslam_posegraph_core.h's element functions, then the candidates a block
at a time through posegate_rhs, posegate_forward / divide / backward and posegate_tail, then the append.  H, the
undivided column, the block of right-hand sides, chi, the poses, the candidates and every output live in heap
arrays of exactly the packed sizes, so an index outside them is the sanitizer's error.  The bits of chi2, cov,
e, d2, the flags and the appended edges must equal tests/posegate_ref.py's, whatever the number of candidates
solved together.  N = 2 and 3 are the smallest systems, 22 and 23 give n = 63 and 66 (either side of a wave),
64 the largest triangle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import posegate_ref as gr
import posegraph_ref as pg
from lidar_slam_amd import posegraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_posegate_core.h"
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
static void puti(const int32_t *v, size_t n) {
    for (size_t i = 0; i < n; i++) std::printf("%d ", v[i]);
    std::printf("\n");
}
static double rd() {
    uint64_t b;
    if (std::scanf("%" SCNx64, &b) != 1) std::exit(3);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

// stdin: N E C E_cap slots append, damp_t damp_r nis_max, N poses (3), N (cos, sin), E edges and C candidates
// (i j z[3] info[6]); the doubles as hex bit patterns
int main() {
    int N, E, C, Ec, slots, append;
    if (std::scanf("%d %d %d %d %d %d", &N, &E, &C, &Ec, &slots, &append) != 6) return 3;
    const double damp_t = rd(), damp_r = rd(), nis_max = rd();
    std::vector<double> P((size_t)3 * N), cs((size_t)2 * N), ez((size_t)3 * Ec), eo((size_t)6 * Ec), cz((size_t)3 * C), co((size_t)6 * C);
    std::vector<int32_t> eij((size_t)2 * Ec), cij((size_t)2 * C);
    for (auto &v : P) v = rd();
    for (auto &v : cs) v = rd();
    for (int e = 0; e < E + C; e++) {
        int32_t *ij = e < E ? &eij[2 * e] : &cij[2 * (e - E)];
        double *z = e < E ? &ez[3 * e] : &cz[3 * (e - E)], *o = e < E ? &eo[6 * e] : &co[6 * (e - E)];
        if (std::scanf("%d %d", ij, ij + 1) != 2) return 3;
        for (int q = 0; q < 3; q++) z[q] = rd();
        for (int q = 0; q < 6; q++) o[q] = rd();
    }
    const int n = posegraph_dim(N);
    std::vector<double> H((size_t)posegraph_tri_size(n)), u((size_t)n), X((size_t)n * 3 * slots), chi((size_t)E);
    std::vector<double> nis((size_t)C), err((size_t)3 * C), cov((size_t)6 * C);
    std::vector<int32_t> cf((size_t)C);
    double chi2 = 0.0;
    int32_t ne = E;
    // (raw pointers into vectors of the exact sizes: the sanitizer watches the element functions' indices)
    const PosegateWork wk = {H.data(), u.data(), X.data(), chi.data()};
    const int flags = posegate_graph_serial(N, E, C, N, Ec, C, slots, P.data(), cs.data(), eij.data(), ez.data(), eo.data(),
                                            cij.data(), cz.data(), co.data(), damp_t, damp_r, nis_max, append, wk, &chi2,
                                            nis.data(), err.data(), cov.data(), cf.data(), &ne);
    std::printf("%d %d\n", flags, ne);
    put(&chi2, 1);
    put(nis.data(), nis.size());
    put(err.data(), err.size());
    put(cov.data(), cov.size());
    puti(cf.data(), cf.size());
    puti(eij.data(), (size_t)2 * ne);
    put(ez.data(), (size_t)3 * ne);
    put(eo.data(), (size_t)6 * ne);
    return 0;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    assert hasattr(posegraph.PoseGraph, "gate")  # (the feature under test ships this header)
    d = tmp_path_factory.mktemp("posegate_core")
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


def run_prog(exe, pose, cs, ij, z, info, cij, cz, cinfo, Ec, slots, append, damp_t, damp_r, nis_max):
    lines = ["%d %d %d %d %d %d %s" % (len(pose), len(ij), len(cij), Ec, slots, append, hx([damp_t, damp_r, nis_max])), hx(pose), hx(cs)]
    for a, b, c in ((ij, z, info), (cij, cz, cinfo)):
        for e in range(len(a)):
            lines.append("%d %d %s %s" % (a[e][0], a[e][1], hx(b[e]), hx(c[e])))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[:300] + out.stderr[-4000:]
    rows = out.stdout.split("\n")
    bits = lambda s: np.array([int(v, 16) for v in s.split()], np.uint64)  # noqa: E731
    ints = lambda s: np.array([int(v) for v in s.split()], np.int64)  # noqa: E731
    flags, ne = ints(rows[0])
    return dict(flags=flags, n_edges=ne, chi2=bits(rows[1]), nis=bits(rows[2]), err=bits(rows[3]), cov=bits(rows[4]),
                cand_flags=ints(rows[5]), edge_ij=ints(rows[6]), edge_z=bits(rows[7]), edge_info=bits(rows[8]))


def candidates(N, pose, rng, C):
    """C candidates on a graph of N nodes: random pairs (i > j, into node 0 and repeated ones among them), near and
    far from the poses' own relative pose, with full information matrices; one on a node that is not there and one
    with a negative Omega where C allows."""
    cij = np.array([(rng.choice(N, 2, replace=False) if N > 2 else ((1, 0), (0, 1))[c % 2]) for c in range(C)], np.int32).reshape(C, 2)
    cz = pg.relative_pose(pose[cij[:, 0]], pose[cij[:, 1]]) + rng.normal(0, 1, (C, 3)) * [20.0, 20.0, 0.02]
    cz[1::3, 0] += 1e6  # (far outside any of these graphs' covariances)
    A = rng.normal(0, 1, (C, 3, 3)) * [0.1, 0.1, 10.0]
    O = np.einsum("eij,ekj->eik", A, A) + np.diag([1e-3, 1e-3, 10.0])
    cinfo = np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], 1)
    if C >= 4:
        cij[2] = (0, N)
        cinfo[3] = -cinfo[3]
    if C >= 6:
        cij[5], cz[5], cinfo[5] = cij[4], cz[4], cinfo[4]  # two equal candidates
    return cij, cz, cinfo


def same(got, ref, E_out):
    assert got["flags"] == ref["flags"] and got["n_edges"] == ref["n_edges"] == E_out
    u = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)  # noqa: E731
    assert got["chi2"][0] == np.float64(ref["chi2"]).view(np.uint64)
    assert np.array_equal(got["cand_flags"], ref["cand_flags"])
    assert np.array_equal(got["nis"], u(ref["cand_nis"])) and np.array_equal(got["err"], u(ref["cand_err"]))
    assert np.array_equal(got["cov"], u(ref["cand_cov"]))
    assert np.array_equal(got["edge_ij"], ref["edge_ij"][:E_out].reshape(-1))
    assert np.array_equal(got["edge_z"], u(ref["edge_z"][:E_out])) and np.array_equal(got["edge_info"], u(ref["edge_info"][:E_out]))


@pytest.mark.parametrize("N", (2, 3, 22, 23, 64))
def test_program_is_the_reference(core_exe, N):
    rng = np.random.default_rng(900 + N)
    C = 9
    for extra, damp, nis_max in ((0, (1e-6, 1e-3), 16.27), (2 * N, (0.0, 0.0), np.inf)):
        pose, ij, z, info = pg.random_graph(N, rng, extra)
        cij, cz, cinfo = candidates(N, pose, rng, C)
        E, Ec = len(ij), len(ij) + 2  # (room for two: the third accepted candidate finds none)
        pad = lambda a: np.concatenate([a, np.zeros((2,) + a.shape[1:], a.dtype)])  # noqa: E731
        ref = gr.gate(pose, pad(ij), pad(z), pad(info), cij, cz, cinfo, n_edges=E, damp_t=damp[0], damp_r=damp[1],
                      nis_max=nis_max, append=1)
        assert ref["flags"] == 0
        cs = ref["trace"]
        outs = [run_prog(core_exe, pose, cs, ij, z, info, cij, cz, cinfo, Ec, slots, 1, damp[0], damp[1], nis_max)
                for slots in (1, 4, 9)]
        for got in outs:
            same(got, ref, ref["n_edges"])
        f = ref["cand_flags"]
        assert f[2] == gr.BAD_EDGE and f[3] == gr.BAD_INFO and (f[5] & 15) == (f[4] & 15)
        if np.isinf(nis_max):
            assert ((f & gr.APPENDED) != 0).sum() == 2 and (f & gr.NO_ROOM).any() and not (f & gr.OUTLIER).any()
        else:
            assert (f & gr.OUTLIER).any()
        # append = 0: the same verdicts, the edges as given
        got = run_prog(core_exe, pose, cs, ij, z, info, cij, cz, cinfo, Ec, 4, 0, damp[0], damp[1], nis_max)
        ref0 = gr.gate(pose, pad(ij), pad(z), pad(info), cij, cz, cinfo, n_edges=E, damp_t=damp[0], damp_r=damp[1], nis_max=nis_max)
        same(got, ref0, E)
        assert np.array_equal(ref0["cand_flags"], f & ~(gr.APPENDED | gr.NO_ROOM))


def test_a_bad_pivot_ends_the_call(core_exe):
    pose, ij, z, info = pg.random_graph(3, np.random.default_rng(9), 0)
    ij, z, info = ij[:1], z[:1], info[:1]  # node 2 is isolated: its pivot is +0.0 without damping
    cij, cz, cinfo = candidates(3, pose, np.random.default_rng(10), 2)
    ref = gr.gate(pose, ij, z, info, cij, cz, cinfo, damp_t=0.0, damp_r=0.0, append=1)
    assert ref["flags"] == gr.SINGULAR and not ref["cand_flags"].any() and not ref["cand_nis"].any()
    got = run_prog(core_exe, pose, ref["trace"], ij, z, info, cij, cz, cinfo, 1, 2, 1, 0.0, 0.0, 16.27)
    assert got["flags"] == gr.SINGULAR and got["n_edges"] == 1 and not got["cand_flags"].any() and not got["nis"].any()
