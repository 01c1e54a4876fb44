"""The strips of a paged recentre (lidar_slam_amd/csrc/lslam_page_plan.h), compiled with g++ on the
CPU: the text the kernels compile.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

For W = 16 and Cw = 24, every (sx, sy) in [-W-1, W+1]^2 and a spread of win (inside the canvas, half
off each edge, wholly off, negative, past the canvas, the ends of int32) the program prints the four
rectangles of the leaving set (the two strips, whole and clipped to the canvas) and the four of the
entering set.  Here they are painted: the whole strips must cover every cell of the reference's
leaving (entering) set once and no other cell, the clipped ones every cell of that set that is on the
canvas once and no other.  The program itself visits every cell of the clipped rectangles in a
window and a canvas allocated at their exact sizes, as the kernels' copies do, so a cell outside
either is an error there.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import page_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
W, CW = 16, 24
WINS = [(4, 4), (0, 0), (CW - W, CW - W), (-8, 3), (CW - 8, 3), (5, -8), (5, CW - 8), (-3, CW - 5), (-W, 2), (CW, 2),
        (2, -W - 1), (2, CW + 1), (-W + 1, -W + 1), (CW - 1, CW - 1), (-1000, 1000), (8, 16), (-16, 8),
        (2 ** 31 - 1, 0), (0, 2 ** 31 - 1), (-2 ** 31, 0), (3, -2 ** 31)]

PROG = r"""
#include "lslam_page_plan.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static long bad = 0, checked = 0;

static void emit(const PageRect &q) { std::printf(" %d %d %d %d", q.x0, q.x1, q.y0, q.y1); }

// every cell of a clipped rectangle, in a window and a canvas of exactly their sizes
static void visit(const PageRect &q, int W, int Cw, int64_t ox, int64_t oy, std::vector<int> &win, std::vector<int> &canvas) {
    for (int y = q.y0; y < q.y1; y++)
        for (int x = q.x0; x < q.x1; x++) {
            checked++;
            if (!page_on_canvas(ox, oy, x, y, Cw) || x < 0 || x >= W || y < 0 || y >= W) {
                bad++;
                continue;
            }
            win[(size_t)y * W + x]++;
            canvas[(size_t)(oy + y) * Cw + (size_t)(ox + x)]++;
        }
}

int main(int argc, char **argv) {
    const int W = std::atoi(argv[1]), Cw = std::atoi(argv[2]);
    const long long wx = std::atoll(argv[3]), wy = std::atoll(argv[4]);
    std::vector<int> win((size_t)W * W), canvas((size_t)Cw * Cw);
    for (int sy = -W - 1; sy <= W + 1; sy++)
        for (int sx = -W - 1; sx <= W + 1; sx++) {
            const PageStrips out = page_leaving(W, sx, sy), in = page_entering(W, sx, sy);
            const PageRect c[4] = {page_clip(out.h, wx, wy, Cw), page_clip(out.v, wx, wy, Cw),
                                   page_clip(in.h, wx + sx, wy + sy, Cw), page_clip(in.v, wx + sx, wy + sy, Cw)};
            std::printf("%d %d", sx, sy);
            emit(out.h), emit(out.v), emit(c[0]), emit(c[1]), emit(in.h), emit(in.v), emit(c[2]), emit(c[3]);
            std::printf(" %d %d\n", page_area(c[0]) + page_area(c[1]), page_area(c[2]) + page_area(c[3]));
            visit(c[0], W, Cw, wx, wy, win, canvas);
            visit(c[1], W, Cw, wx, wy, win, canvas);
            visit(c[2], W, Cw, wx + sx, wy + sy, win, canvas);
            visit(c[3], W, Cw, wx + sx, wy + sy, win, canvas);
            checked++;
        }
    std::printf("%ld %ld\n", checked, bad);
    return bad != 0 || checked == 0;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("page_plan")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


def paint(rects):
    """How often each window cell is covered by the rectangles (x0, x1, y0, y1); a rectangle must lie on the window."""
    n = np.zeros((W, W), np.int64)
    for x0, x1, y0, y1 in rects:
        if x0 < x1 and y0 < y1:
            assert 0 <= x0 and x1 <= W and 0 <= y0 and y1 <= W, (x0, x1, y0, y1)
            n[y0:y1, x0:x1] += 1
    return n


@pytest.mark.parametrize("win", WINS, ids=["win_%d_%d" % w for w in WINS])
def test_strips_tile_the_reference_sets(plan_exe, win):
    out = subprocess.run([plan_exe, str(W), str(CW), str(win[0]), str(win[1])], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.splitlines()
    checked, bad = map(int, lines[-1].split())
    assert checked > 0 and bad == 0
    rows = np.array([[int(v) for v in ln.split()] for ln in lines[:-1]], np.int64)
    assert len(rows) == (2 * W + 3) ** 2
    seen = set()
    for row in rows:
        sx, sy = int(row[0]), int(row[1])
        seen.add((sx, sy))
        r = row[2:34].reshape(8, 4)
        leave, enter = pr.leaving(W, sx, sy), pr.entering(W, sx, sy)
        on0, on1 = pr.on_canvas(W, CW, win[0], win[1]), pr.on_canvas(W, CW, win[0] + sx, win[1] + sy)
        assert np.array_equal(paint(r[0:2]), leave.astype(np.int64)), (sx, sy)
        assert np.array_equal(paint(r[2:4]), (leave & on0).astype(np.int64)), (sx, sy)
        assert np.array_equal(paint(r[4:6]), enter.astype(np.int64)), (sx, sy)
        assert np.array_equal(paint(r[6:8]), (enter & on1).astype(np.int64)), (sx, sy)
        assert (row[34], row[35]) == ((leave & on0).sum(), (enter & on1).sum()), (sx, sy)
        if 0 < abs(sx) < W and 0 < abs(sy) < W:  # the L: |sy| full rows, |sx| columns over the remaining rows
            (hx0, hx1, hy0, hy1), (vx0, vx1, vy0, vy1) = r[0], r[1]
            assert (hx0, hx1, hy1 - hy0) == (0, W, abs(sy)) and (vx1 - vx0, vy1 - vy0) == (abs(sx), W - abs(sy))
    assert len(seen) == (2 * W + 3) ** 2
