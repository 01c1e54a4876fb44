"""The plain C++ of a map read as a revolution (lidar_slam_amd/csrc/lslam_gridpoints_plan.h), compiled with
g++ on the CPU: the text the kernels compile.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

The program is the kernels' two passes over heap arrays of exactly the sizes of the grid and of the
robot's slots: band after band, a wave's 64 lanes an iteration, a unit of 8 cells (or of 1) a lane.  The
count pass fills the per-band pairs; the write pass takes each band's first ordinal from them and places
every in-range cell by the ballots of its iteration, as gridpoints_kernel does (gp_below stands for mbcnt).
An index outside either array is an error there (the sanitizer's, and the program's own count).  It also
counts how often each cell is visited: the bands' units must cover the grid once.  Its xy (compared as bit
patterns), counts and flags must equal tests/gridpoints_ref.py's, so the NumPy form and the kernels' C++
are held to each other without a device.

Widths 16, 24, 72 and 520 straddle the 8-cell unit (24 = 3 units a row, 520 = 65), the 64-lane wave (a
row of 72 in units of 1 is 64 + 8 lanes; a row of 520 in units of 8 is 65 lanes) and the band height (1 row
to the whole grid, by `want`).  Runs of 63, 64 and 65 occupied cells end at a row's end and so, for every
band height that divides that row's number, at a band's seam."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gridpoints_ref as gp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_gridpoints_plan.h"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static std::vector<int16_t> L;
static std::vector<int> seen;
static long bad = 0;
static int W, CELLS, occ_min;
static GpAnchor A;

// a lane's unit: the masks of its occupied cells and of those in range (0 for a lane beyond the band)
static void lane_masks(const GpBand &q, int u, bool count, int &X0, int &Y, uint32_t &occ, uint32_t &in, double &dy) {
    occ = in = 0;
    X0 = Y = 0;
    dy = 0.0;
    if (u >= q.n) return;
    gp_unit(W, q.y0, u, CELLS, X0, Y);
    if (X0 < 0 || X0 + CELLS > W || Y < 0 || Y >= W) { bad++; return; }
    for (int j = 0; j < CELLS; j++) {
        if (count) seen[(size_t)Y * W + X0 + j]++;
        occ |= ((int)L[(size_t)Y * W + X0 + j] >= occ_min ? 1u : 0u) << j;
    }
    dy = gp_offset(A.oy, Y, A.cell, A.ay);
    for (uint32_t m = occ; m;) {
        const int j = __builtin_ctz(m);
        m &= m - 1;
        in |= (gp_in_range(gp_offset(A.ox, X0 + j, A.cell, A.ax), dy, A.r2) ? 1u : 0u) << j;
    }
}

// argv: W cells want cap occ_min cell radius ox oy ax ay c s; stdin: W*W values
int main(int argc, char **argv) {
    if (argc != 14) return 2;
    W = std::atoi(argv[1]), CELLS = std::atoi(argv[2]);
    const int want = std::atoi(argv[3]), cap = std::atoi(argv[4]);
    occ_min = std::atoi(argv[5]);
    A.cell = std::atof(argv[6]);
    const double radius = std::atof(argv[7]);
    A.r2 = radius * radius;
    A.ox = std::atof(argv[8]), A.oy = std::atof(argv[9]), A.ax = std::atof(argv[10]), A.ay = std::atof(argv[11]);
    A.c = std::atof(argv[12]), A.s = std::atof(argv[13]);
    if (W % CELLS) return 2;
    L.resize((size_t)W * W);
    seen.assign((size_t)W * W, 0);
    for (auto &v : L) { int x; if (std::scanf("%d", &x) != 1) return 3; v = (int16_t)x; }
    std::vector<double> xy((size_t)cap * 2, 0.0);  // (the launcher's memset)
    const int rows = gp_band_rows(W, want), nb = gp_bands(W, rows);
    if (rows < 1 || nb < 1 || nb > GP_BANDS || (long)nb * rows < W || (long)(nb - 1) * rows >= W) bad++;
    std::vector<int> bc((size_t)nb * 2, -1);
    const bool ok = gp_anchor_finite(A);
    int counts[4] = {0, 0, 0, 0}, flags = 0;

    // the count pass
    for (int band = 0; band < nb; band++) {
        if (!ok) { bc[2 * band] = bc[2 * band + 1] = 0; continue; }
        const GpBand q = gp_band(W, rows, band, CELLS);
        int c_occ = 0, c_in = 0;
        for (int u0 = 0; u0 < q.n; u0 += GP_WAVE)
            for (int lane = 0; lane < GP_WAVE; lane++) {
                int X0, Y;
                uint32_t occ, in;
                double dy;
                lane_masks(q, u0 + lane, true, X0, Y, occ, in, dy);
                c_occ += __builtin_popcount(occ), c_in += __builtin_popcount(in);
            }
        bc[2 * band] = c_occ, bc[2 * band + 1] = c_in;
    }
    // the write pass
    for (int band = 0; band < nb; band++) {
        int n_occ = 0, n_in = 0, ord = 0;
        for (int k = 0; k < nb; k++) n_occ += bc[2 * k], n_in += bc[2 * k + 1], ord += k < band ? bc[2 * k + 1] : 0;
        const int stride = gp_stride(n_in, cap);
        if (band == 0) {
            const int n_out = gp_n_out(n_in, stride);
            counts[0] = n_occ, counts[1] = n_in, counts[2] = ok ? stride : 0, counts[3] = n_out;
            flags = ok ? gp_flags(n_out, stride) : 1;
        }
        if (!ok || bc[2 * band + 1] == 0) continue;
        const GpBand q = gp_band(W, rows, band, CELLS);
        for (int u0 = 0; u0 < q.n; u0 += GP_WAVE) {
            int X0[GP_WAVE], Y[GP_WAVE];
            uint32_t occ[GP_WAVE], in[GP_WAVE];
            double dy[GP_WAVE];
            uint64_t bj[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int total = 0;
            for (int lane = 0; lane < GP_WAVE; lane++) {
                lane_masks(q, u0 + lane, false, X0[lane], Y[lane], occ[lane], in[lane], dy[lane]);
                for (int j = 0; j < CELLS; j++) bj[j] |= (uint64_t)((in[lane] >> j) & 1u) << lane;
            }
            for (int j = 0; j < CELLS; j++) total += __builtin_popcountll(bj[j]);
            for (int lane = 0; lane < GP_WAVE; lane++) {
                int below = 0;
                for (int j = 0; j < CELLS; j++) below += gp_below(bj[j], lane);
                int i = ord + below;
                for (uint32_t m = in[lane]; m; i++) {
                    const int j = __builtin_ctz(m);
                    m &= m - 1;
                    const int slot = gp_slot(i, stride);
                    if (slot < 0) continue;
                    if (slot >= cap || slot >= counts[3]) { bad++; continue; }
                    double px, py;
                    gp_point(A, gp_offset(A.ox, X0[lane] + j, A.cell, A.ax), dy[lane], px, py);
                    if (xy[2 * (size_t)slot] != 0.0 || xy[2 * (size_t)slot + 1] != 0.0) bad++;  // a slot is written once
                    xy[2 * (size_t)slot] = px, xy[2 * (size_t)slot + 1] = py;
                }
            }
            ord += total;
        }
        if (ord > counts[1]) bad++;
    }
    if (ok) for (int n : seen) bad += n != 1;
    std::printf("%ld %d %d %d %d %d\n", bad, flags, counts[0], counts[1], counts[2], counts[3]);
    for (double v : xy) { uint64_t b; std::memcpy(&b, &v, 8); std::printf("%" PRIx64 " ", b); }
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
    d = tmp_path_factory.mktemp("gridpoints_plan")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


def run_prog(exe, L, origin, anchor, cells, want, **kw):
    p = dict(gp.DEFAULTS, **kw)
    W = L.shape[0]
    args = [W, cells, want, p["cap"], p["occ_min"]]
    nums = [p["cell"], p["radius"]] + list(origin) + list(anchor)
    text = " ".join(str(int(v)) for v in L.ravel()) + "\n"
    out = subprocess.run([exe] + [str(a) for a in args] + [repr(float(v)) for v in nums], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[:300] + out.stderr[-4000:]
    head, body = out.stdout.splitlines()[:2]
    head = [int(v) for v in head.split()]
    assert head[0] == 0
    return {"flags": head[1], "counts": np.array(head[2:], np.int32),
            "xy": np.array([int(v, 16) for v in body.split()], np.uint64).reshape(-1, 2)}


def same(got, ref):
    assert got["flags"] == ref["flags"] and got["counts"].tolist() == ref["counts"].tolist(), (got["flags"], got["counts"], ref["flags"], ref["counts"])
    assert np.array_equal(got["xy"], np.ascontiguousarray(ref["xy"]).view(np.uint64))


def seam_map(W, rng):
    """Runs of 63, 64 and 65 occupied cells (row-major) that end at a row's end, on rows whose numbers + 1
    have many divisors, over a sprinkle of single cells."""
    L = np.where(rng.random(W * W) < 0.01, 100, 0).astype(np.int16)
    n_rows = -(-65 // W) + 1
    ends = [y for y in (6, 12, 24, 36, 48, 60, 120, 240, 360, 480) if n_rows <= y <= W][:6] + [W]
    for k, y in enumerate(ends):
        run = (63, 64, 65)[k % 3]
        L[y * W - run:y * W] = 200
    return L.reshape(W, W)


def rot(th):
    return (float(np.cos(th)), float(np.sin(th)))


WIDTHS = (16, 24, 72, 520)


@pytest.mark.parametrize("W", WIDTHS)
def test_program_is_the_reference(plan_exe, W):
    rng = np.random.default_rng(200 + W)
    half = 0.5 * W * 20.0
    origin = (-half + 40.0, -half - 60.0)
    for k, (occupancy, cap, radius, anchor) in enumerate((
            (0.01, 1024, 8000.0, (13.0, -7.0) + rot(0.3)),
            (0.30, 64, 0.4 * W * 20.0, (half / 3, -half / 5) + rot(-2.0)),     # decimated, a radius inside the grid
            (1.00, 1024, 8000.0, (0.0, 0.0) + rot(1.0)),                          # every cell: n_in far above the cap
            (0.30, 65536, 1e6, (1e5, 0.0) + (0.0, 1.0)))):                        # an anchor off the map, a quarter turn
        L = np.where(rng.random((W, W)) < occupancy, rng.integers(85, 351, (W, W)), rng.integers(-200, 85, (W, W))).astype(np.int16)
        ref = gp.points(L, origin, anchor, cap=cap, radius=radius)
        for cells in (8, 1):
            for want in ((1, 3, W, 256) if W < 520 else (2, 256)):
                if W == 520 and cells == 1 and k != 1:
                    continue  # (the slow form of the large width: one map is enough)
                same(run_prog(plan_exe, L, origin, anchor, cells, want, cap=cap, radius=radius), ref)


@pytest.mark.parametrize("W", WIDTHS)
def test_runs_across_lanes_rows_and_bands(plan_exe, W):
    rng = np.random.default_rng(300 + W)
    L = seam_map(W, rng)
    half = 0.5 * W * 20.0
    origin, anchor = (-half, -half), (10.0, 10.0) + rot(0.7)  # (the anchor is on a cell centre: that cell is left out if occupied)
    for cap in (1024, 50):
        ref = gp.points(L, origin, anchor, cap=cap)
        assert ref["counts"][1] >= 3 * 63
        for cells in (8, 1):
            for want in ((1, 2, 3, 4, 6, W) if W < 520 else (4, 130, 256)):
                same(run_prog(plan_exe, L, origin, anchor, cells, want, cap=cap), ref)


def test_bad_anchor_and_empty(plan_exe):
    L = np.full((16, 16), 100, np.int16)
    for bad in range(6):
        v = [0.0, 0.0, 5.0, 5.0, 1.0, 0.0]
        v[bad] = (float("nan"), float("inf"), -float("inf"))[bad % 3]
        got = run_prog(plan_exe, L, v[:2], v[2:], 8, 4)
        same(got, gp.points(L, v[:2], v[2:]))
        assert got["flags"] == gp.BAD_ANCHOR and not got["counts"].any() and not got["xy"].any()
    got = run_prog(plan_exe, np.zeros((16, 16), np.int16), (0.0, 0.0), (5.0, 5.0, 1.0, 0.0), 8, 4)
    assert got["flags"] == gp.EMPTY and not got["counts"][[0, 1, 3]].any() and got["counts"][2] == 1
    # coordinates at 1e300: finite inputs, d2 overflows to inf, nothing is in range
    got = run_prog(plan_exe, L, (1e300, 0.0), (5.0, 5.0, 1.0, 0.0), 8, 4)
    same(got, gp.points(L, (1e300, 0.0), (5.0, 5.0, 1.0, 0.0)))
    assert got["flags"] == gp.EMPTY and got["counts"].tolist() == [256, 0, 1, 0]
