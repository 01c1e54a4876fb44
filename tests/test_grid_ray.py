"""The integer ray of the occupancy-grid update and its clip to a tile
(lidar_slam_amd/csrc/lslam_grid_ray.h), compiled with g++ on the CPU: the text the kernel compiles.
The program is built with -fsanitize=address,undefined when the compiler here can link an empty
program with them.

For every ray end in [-24, 24]^2 around a robot cell at every offset 0..7 inside its tile, and
every tile of 8 x 8 cells that the ray can meet plus a ring of tiles that it cannot, the clipped
step interval must visit exactly the steps that a brute-force walk finds inside the tile."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_grid_ray.h"
#include <cstdio>
#include <cstring>

static long bad = 0, checked = 0;
#define CHECK(x) do { if (!(x)) { if (bad++ < 20) std::printf("line %d: %s (X0 %d Y0 %d dx %d dy %d tile %d %d)\n", \
    __LINE__, #x, X0, Y0, dx, dy, tx, ty); } } while (0)

enum { TS = 8, LO = -5, HI = 5, NT = HI - LO + 1 };  // tiles -5 .. 5 a side: cells -40 .. 47
static int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the walk: every step's cell, the tile it lies in; per tile the first and last step and their number
static void clip_case(int base) {
    for (int oy = 0; oy < TS; oy++)
        for (int ox = 0; ox < TS; ox++)
            for (int dy = -24; dy <= 24; dy++)
                for (int dx = -24; dx <= 24; dx++) {
                    const int X0 = base + ox, Y0 = base + oy;
                    const int n = grid_ray_steps(dx, dy);
                    int first[NT][NT], last[NT][NT], cnt[NT][NT];
                    std::memset(cnt, 0, sizeof(cnt));
                    int tx = 0, ty = 0;
                    for (int i = 0; i <= n; i++) {
                        int x, y;
                        grid_ray_cell(X0, Y0, dx, dy, n, i, x, y);
                        tx = fdiv(x - base, TS) - LO;
                        ty = fdiv(y - base, TS) - LO;
                        CHECK(tx >= 0 && tx < NT && ty >= 0 && ty < NT);
                        if (!cnt[ty][tx]++) first[ty][tx] = i;
                        last[ty][tx] = i;
                    }
                    for (ty = 0; ty < NT; ty++)
                        for (tx = 0; tx < NT; tx++) {
                            const int x0 = base + (tx + LO) * TS, y0 = base + (ty + LO) * TS;
                            int ilo = -7, ihi = -7;
                            const bool in = grid_ray_clip(X0, Y0, dx, dy, x0, y0, x0 + TS, y0 + TS, ilo, ihi);
                            checked++;
                            CHECK(in == (cnt[ty][tx] > 0));
                            if (in && cnt[ty][tx]) {
                                CHECK(ilo == first[ty][tx] && ihi == last[ty][tx]);
                                CHECK(ihi - ilo + 1 == cnt[ty][tx]);  // one interval, nothing skipped
                            }
                        }
                }
}

// the ray itself: step 0 is the robot cell, step n the hit cell, neighbours one Chebyshev step apart
static void walk_case() {
    const int X0 = 3, Y0 = -2, tx = 0, ty = 0;
    for (int dy = -40; dy <= 40; dy++)
        for (int dx = -40; dx <= 40; dx++) {
            const int n = grid_ray_steps(dx, dy);
            int px = 0, py = 0;
            for (int i = 0; i <= n; i++) {
                int x, y;
                grid_ray_cell(X0, Y0, dx, dy, n, i, x, y);
                if (i == 0) CHECK(x == X0 && y == Y0);
                if (i == n) CHECK(x == X0 + dx && y == Y0 + dy);
                if (i > 0) {
                    const int cx = grid_iabs(x - px), cy = grid_iabs(y - py);
                    CHECK((cx > cy ? cx : cy) == 1);
                }
                px = x;
                py = y;
                checked++;
            }
        }
}

// the division-free walk from any first step gives the closed form's offsets
static void carry_case() {
    const int X0 = 0, Y0 = 0, tx = 0, ty = 0;
    for (int dy = 0; dy <= 40; dy++)
        for (int dx = 0; dx <= 40; dx++) {
            const int n = grid_ray_steps(dx, dy);
            for (int i0 = 0; i0 <= n; i0++) {
                GridAxisWalk wx = grid_walk_begin(i0, dx, n), wy = grid_walk_begin(i0, dy, n);
                for (int i = i0; i <= n; i++) {
                    CHECK(wx.off == grid_ray_offset(i, dx, n) && wy.off == grid_ray_offset(i, dy, n));
                    grid_walk_next(wx);
                    grid_walk_next(wy);
                    checked++;
                }
            }
        }
    const int big[3][2] = {{4098, 4097}, {4098, 1}, {4097, 4098}};
    for (int e = 0; e < 3; e++) {
        const int dx = big[e][0], dy = big[e][1], n = grid_ray_steps(dx, dy);
        GridAxisWalk wx = grid_walk_begin(5, dx, n), wy = grid_walk_begin(5, dy, n);
        for (int i = 5; i <= n; i++) {
            CHECK(wx.off == grid_ray_offset(i, dx, n) && wy.off == grid_ray_offset(i, dy, n));
            grid_walk_next(wx);
            grid_walk_next(wy);
            checked++;
        }
    }
}

// the longest rays the parameter ranges allow, far from the origin: the products stay inside int32
static void far_case() {
    const int big = (1 << 20) - 1, tx = 0, ty = 0;
    const int ends[5][2] = {{4098, 4097}, {-4098, 1}, {4097, -4098}, {-3, -4098}, {-4098, -4098}};
    for (int s = 0; s < 2; s++)
        for (int e = 0; e < 5; e++) {
            const int X0 = s ? big : 100, Y0 = s ? -big : 2000, dx = ends[e][0], dy = ends[e][1];
            const int n = grid_ray_steps(dx, dy);
            int inside = 0, ilo, ihi, lo = -1, hi = -1;
            for (int i = 0; i <= n; i++) {
                int x, y;
                grid_ray_cell(X0, Y0, dx, dy, n, i, x, y);
                if (x >= 0 && x < 2048 && y >= 0 && y < 2048) {
                    if (!inside++) lo = i;
                    hi = i;
                }
            }
            const bool in = grid_ray_clip(X0, Y0, dx, dy, 0, 0, 2048, 2048, ilo, ihi);
            checked++;
            CHECK(in == (inside > 0));
            if (in) CHECK(ilo == lo && ihi == hi && hi - lo + 1 == inside);
        }
}

int main(int argc, char **argv) {
    const char *w = argc > 1 ? argv[1] : "";
    if (!std::strcmp(w, "clip")) clip_case(0);
    else if (!std::strcmp(w, "clip_negative")) clip_case(-131071 * TS);
    else if (!std::strcmp(w, "walk")) walk_case();
    else if (!std::strcmp(w, "far")) far_case();
    else if (!std::strcmp(w, "carry")) carry_case();
    std::printf("%ld %ld\n", checked, bad);
    return bad != 0 || checked == 0;
}
"""

CASES = ["clip", "clip_negative", "walk", "far", "carry"]


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def ray_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("grid_ray")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("case", CASES)
def test_grid_ray(ray_exe, case):
    out = subprocess.run([ray_exe, case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    checked, bad = map(int, out.stdout.split()[-2:])
    assert checked > 0 and bad == 0, out.stdout
