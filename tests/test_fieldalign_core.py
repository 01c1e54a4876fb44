"""The per-point arithmetic and the 3 x 3 solve of lslam_field_align
(lidar_slam_amd/csrc/lslam_fieldalign_core.h), compiled with g++ on the CPU: the text the kernel
compiles.  The program has its own main and is built with -fsanitize=address,undefined when the
compiler here can link an empty program with them, and with -ffp-contract=off as the library is.

It is fed the inputs of tests/fieldalign_ref.py point by point (a frame, the valid points in range, the
field) and held to the reference bit for bit: which points lie on the map and which are used, the cell
and the fractions, m, gx, gy, the ten fixed-point terms, their sums, and the step that
fieldalign_solve makes of them; the distance of every uint16 against math.isqrt.  The frames are the
evaluations of the reference's own iteration in the five-revolution room, and random fields under
points on cell centres and boundaries, off the map, and from poses far outside any integer's range.

What the GPU tests alone cover is the kernel around these functions: the gathers, the reduction, the
iteration and the outputs.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dist_ref as dr
import fieldalign_ref as far
from test_fieldscore_ref import ROOM_DIST
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, build_room, room_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_fieldalign_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int64_t bits(double v) { int64_t b; std::memcpy(&b, &v, 8); return b; }

// in: doubles (n, W, px, py, c, s, ox, oy, inv, trunc, damp_t, damp_r), x[n], y[n], d2[W W]
// out: int64 rows of 19 per point (on, used, ix, iy, fu, fv, m, gx, gy as bits, ten terms), then the ten
//      sums, then (dx, dy, dt as bits, ok)
static int frame(const char *in, const char *out) {
    FILE *f = std::fopen(in, "rb");
    if (!f) return 2;
    double h[12];
    if (std::fread(h, 8, 12, f) != 12) return 2;
    const int n = (int)h[0], W = (int)h[1];
    std::vector<double> x(n), y(n), d(size_t(W) * W);
    if (std::fread(x.data(), 8, n, f) != (size_t)n || std::fread(y.data(), 8, n, f) != (size_t)n ||
        std::fread(d.data(), 8, d.size(), f) != d.size())
        return 2;
    std::fclose(f);
    std::vector<uint16_t> D(d.size());  // exactly sized: ASan sees any read outside
    for (size_t i = 0; i < d.size(); i++) D[i] = (uint16_t)d[i];
    FieldAlignFrame fr;
    fr.px = h[2], fr.py = h[3], fr.c = h[4], fr.s = h[5], fr.ox = h[6], fr.oy = h[7], fr.inv = h[8];
    std::vector<int64_t> o(size_t(n) * 19 + 14, 0);
    uint64_t sum[10] = {0};
    for (int p = 0; p < n; p++) {
        int64_t *row = o.data() + size_t(p) * 19;
        double rx, ry, fu, fv;
        int ix, iy;
        if (!fieldalign_locate(fr, x[p], y[p], W, rx, ry, ix, iy, fu, fv)) continue;
        const uint16_t *Dc = D.data() + size_t(iy) * W + ix;
        double m, gx, gy;
        fieldalign_bilinear(fieldalign_dq(Dc[0]), fieldalign_dq(Dc[1]), fieldalign_dq(Dc[W]), fieldalign_dq(Dc[W + 1]), fu, fv,
                            m, gx, gy);
        row[0] = 1, row[2] = ix, row[3] = iy, row[4] = bits(fu), row[5] = bits(fv), row[6] = bits(m), row[7] = bits(gx),
        row[8] = bits(gy);
        if (m > h[9]) continue;
        row[1] = 1;
        fieldalign_terms(m, gx, gy, rx, ry, fr.inv, row + 9);
        for (int i = 0; i < 10; i++) sum[i] += (uint64_t)row[9 + i];
    }
    int64_t *tail = o.data() + size_t(n) * 19;
    for (int i = 0; i < 10; i++) tail[i] = (int64_t)sum[i];
    double delta[3];
    tail[13] = fieldalign_solve(tail, h[10], h[11], delta) ? 1 : 0;
    for (int i = 0; i < 3; i++) tail[10 + i] = bits(delta[i]);
    f = std::fopen(out, "wb");
    if (!f || std::fwrite(o.data(), 8, o.size(), f) != o.size()) return 2;
    std::fclose(f);
    return 0;
}

// in: int64 rows of (ten sums) then doubles' bits (damp_t, damp_r); out: rows of (dx, dy, dt as bits, ok)
static int solves(const char *in, const char *out) {
    FILE *f = std::fopen(in, "rb"), *g = std::fopen(out, "wb");
    if (!f || !g) return 2;
    int64_t row[12];
    while (std::fread(row, 8, 12, f) == 12) {
        double damp[2], delta[3];
        std::memcpy(damp, row + 10, 16);
        int64_t o[4];
        o[3] = fieldalign_solve(row, damp[0], damp[1], delta) ? 1 : 0;
        for (int i = 0; i < 3; i++) o[i] = bits(delta[i]);
        std::fwrite(o, 8, 4, g);
    }
    std::fclose(f);
    std::fclose(g);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !std::strcmp(argv[1], "frame")) return frame(argv[2], argv[3]);
    if (argc == 4 && !std::strcmp(argv[1], "solve")) return solves(argv[2], argv[3]);
    if (argc == 2 && !std::strcmp(argv[1], "isqrt")) {
        for (uint32_t v = 0; v < 65536u; v++) std::printf("%u\n", fieldalign_isqrt16(v));
        return 0;
    }
    return 2;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("fieldalign_core")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe), d


def run_frame(core, d2, x, y, px, py, c, s, ox, oy, inv, trunc, damp_t, damp_r):
    """One frame through the program and through the reference; everything compared bit for bit.  Returns
    (points on the map, points used)."""
    exe, d = core
    W = d2.shape[0]
    head = np.array([len(x), W, px, py, c, s, ox, oy, inv, trunc, damp_t, damp_r], np.float64)
    np.concatenate([head, x, y, d2.astype(np.float64).reshape(-1)]).tofile(str(d / "in.bin"))
    out = subprocess.run([exe, "frame", str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    o = np.fromfile(str(d / "out.bin"), np.int64)
    rows, tail = o[:len(x) * 19].reshape(len(x), 19), o[len(x) * 19:]
    t = far.point_terms(d2.astype(np.int64), x, y, px, py, c, s, ox, oy, inv, trunc)
    on = rows[:, 0] == 1
    assert int(on.sum()) == len(t["ix"]) and not rows[~on].any()
    got = rows[on]
    assert np.array_equal(got[:, 1], t["used"].astype(np.int64))
    assert np.array_equal(got[:, 2], t["ix"]) and np.array_equal(got[:, 3], t["iy"])
    for col, name in ((4, "fu"), (5, "fv"), (6, "m"), (7, "gx"), (8, "gy")):
        assert np.array_equal(got[:, col], t[name].view(np.int64)), name
    assert np.array_equal(got[:, 9:], t["terms"])
    N, n_used = far.evaluate(d2.astype(np.int64), x, y, px, py, c, s, ox, oy, inv, trunc)
    assert tail[:10].tolist() == N
    delta, ok = far.solve(N, damp_t, damp_r)
    assert tail[13] == int(ok) and tail[10:13].tolist() == np.array(delta, np.float64).view(np.int64).tolist()
    return int(on.sum()), n_used


def test_isqrt(core):
    out = subprocess.run([core[0], "isqrt"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = np.array(out.stdout.split(), np.int64)
    assert np.array_equal(got / 256.0, far.DQ) and len(got) == 65536


def test_room_frames(core):
    """Every evaluation of the reference's iteration for two robots of the room."""
    poses, revs = room_run()
    L = build_room(poses, revs)
    d2 = dr.field_batch(L, **ROOM_DIST)[0]
    rev = revs[4]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    q = far.DEFAULTS
    total = 0
    for r in (0, 4):
        pts = rev["xy"][off[r]:off[r + 1]]
        x, y = far.used_points(pts, 8000.0)
        out = far.align(d2[r], pts, poses[4][r] + np.array([-30.0, 30.0, 0.03]), None, ROOM_ORIGIN, ROOM_KW)
        for k in range(out["iters"] + 1):
            px, py, _, c, s = out["trace"][k]
            on, used = run_frame(core, d2[r], x, y, px, py, c, s, ROOM_ORIGIN[0], ROOM_ORIGIN[1], 1.0 / 20.0, q["trunc"],
                                 q["damp_t"], q["damp_r"])
            assert used >= 690
            total += 1
    assert total >= 12


def test_nasty_frames(core):
    rng = np.random.default_rng(59)
    W, cell = 32, 100.0
    for case in range(12):
        d2 = rng.choice([0, 1, 2, 3, 5, 9, 100, 625, 626, 4096, 65025], (W, W)).astype(np.uint16)
        n = 300
        x, y = rng.uniform(-2000.0, 2000.0, n), rng.uniform(-2000.0, 2000.0, n)
        x[:60] = rng.integers(-20, 20, 60) * cell          # on cell boundaries
        y[60:120] = rng.integers(-20, 20, 60) * cell + 50.0  # on cell centres
        th = rng.uniform(-3.0, 3.0) if case % 3 else 0.0
        px, py = ((0.0, 0.0), (150.0, -250.0), (1e300, 0.0), (-4e9, 7e12), (1550.0, 1550.0), (-1600.0, 1600.0))[case % 6]
        trunc = (25.0, 0.0, 255.0, 1.5)[case % 4]
        on, used = run_frame(core, d2, x, y, px, py, np.cos(th), np.sin(th), -1600.0, -1600.0, 1.0 / cell, trunc,
                             (1.0, 0.0)[case % 2], (100.0, 0.0)[case % 2])
        assert (on == 0) == (abs(px) > 1e6) and used <= on


def test_solves(core):
    """fieldalign_solve alone: singular and near-singular systems, sums at the ends of int64."""
    exe, d = core
    rng = np.random.default_rng(61)
    rows = []
    for _ in range(200):
        J = rng.normal(size=(rng.integers(1, 6), 3)) * rng.choice([1e-3, 1.0, 300.0], 3)
        m = rng.normal(size=len(J))
        H, g = J.T @ J, J.T @ m
        N = [H[0, 0], H[0, 1], H[0, 2], H[1, 1], H[1, 2], H[2, 2], g[0], g[1], g[2], m @ m]
        rows.append(([int(round(v * 2 ** 20)) for v in N], rng.choice([0.0, 1e-6, 1.0]), rng.choice([0.0, 1e-6, 100.0])))
    big = 2 ** 62
    rows += [([0] * 10, 0.0, 0.0), ([0] * 10, 1.0, 100.0), ([1, 0, 0, 0, 0, 0, 1, 1, 1, 1], 0.0, 0.0),
             ([big, big, big, big, big, big, -big, big, -big, big], 0.0, 0.0),
             ([big, 0, 0, big, 0, big, -big, big, -big, big], 1.0, 1.0),
             ([-5, 0, 0, 7, 0, 9, 1, 2, 3, 4], 0.0, 0.0), ([4, 2, 0, 1, 0, 9, 1, 2, 3, 4], 0.0, 0.0),
             ([2 ** 63 - 1] * 10, 0.0, 0.0), ([-2 ** 63] * 10, 1.0, 1.0)]
    buf = np.zeros((len(rows), 12), np.int64)
    for i, (N, dt, dr_) in enumerate(rows):
        buf[i, :10] = N
        buf[i, 10:] = np.array([dt, dr_], np.float64).view(np.int64)
    buf.tofile(str(d / "sin.bin"))
    out = subprocess.run([exe, "solve", str(d / "sin.bin"), str(d / "sout.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(str(d / "sout.bin"), np.int64).reshape(len(rows), 4)
    n_ok = 0
    for i, (N, dt, dr_) in enumerate(rows):
        delta, ok = far.solve(N, float(dt), float(dr_))
        assert got[i, 3] == int(ok) and got[i, :3].tolist() == np.array(delta, np.float64).view(np.int64).tolist(), (i, N)
        n_ok += int(ok)
    assert 100 < n_ok < len(rows)
