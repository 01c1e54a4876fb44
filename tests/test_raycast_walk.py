"""One beam of lslam_grid_raycast (lidar_slam_amd/csrc/lslam_raycast_walk.h), compiled with g++ on the
CPU: the text the kernel compiles.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

The header's walk carries the ray's remainders and the squared radius along; the brute force here
takes every step from the closed form in 64-bit integers, tests the cap by multiplying, and reads the
map with a bounds test.  They must agree on (kind, ox, oy, i_h) for every far offset in [-24, 24]^2,
every Rc in 0..24 and random 2-bit maps of width 5, 8 and 37 with the robot on every kind of place
(inside, on the border, off the map); and for the largest offsets the parameter ranges allow
(|D| = 8192, Rc = 4096), where 2 i |D| + n and ox ox + oy oy come closest to the end of int32.
The class table (step 4) is checked against its definition written out case by case."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_raycast_walk.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long bad = 0, checked = 0;
#define CHECK(x) do { if (!(x)) { if (bad++ < 20) std::printf("line %d: %s (Dx %d Dy %d Rc %d W %d X0 %d Y0 %d)\n", \
    __LINE__, #x, Dx, Dy, Rc, W, X0, Y0); } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct Map {  // codes [W][W]; the robot cell (X0, Y0)
    const std::vector<unsigned char> *m;
    int W, X0, Y0;
    int operator()(int ox, int oy) const {
        const int X = X0 + ox, Y = Y0 + oy;
        if (X < 0 || X >= W || Y < 0 || Y >= W) return RAYCAST_UNKNOWN;
        return (*m)[(size_t)Y * W + X];
    }
};
struct AllFree { int operator()(int, int) const { return RAYCAST_FREE; } };

// the definition, step by step, in int64
template <class Code>
static int brute(int Dx, int Dy, int Rc, const Code &code, int &ox, int &oy, int &ih) {
    const long long ax = Dx < 0 ? -(long long)Dx : Dx, ay = Dy < 0 ? -(long long)Dy : Dy, n = ax > ay ? ax : ay;
    const int sx = (Dx > 0) - (Dx < 0), sy = (Dy > 0) - (Dy < 0);
    ox = oy = 0;
    for (long long i = 0; i <= n; i++) {
        const long long fx = n ? (2 * i * ax + n) / (2 * n) : 0, fy = n ? (2 * i * ay + n) / (2 * n) : 0;
        ox = (int)(sx * fx);
        oy = (int)(sy * fy);
        ih = (int)i;
        if (fx * fx + fy * fy > (long long)Rc * Rc) return RAYCAST_K_NONE;
        const int v = code(ox, oy);
        if (v == RAYCAST_OCC) return RAYCAST_K_OCC;
        if (v != RAYCAST_FREE) return RAYCAST_K_UNKNOWN;
    }
    ih = (int)n + 1;
    return RAYCAST_K_NONE;
}

template <class Code>
static void compare(int Dx, int Dy, int Rc, const Code &code, int W, int X0, int Y0) {
    int ox = -7, oy = -7, ih = -7, bx, by, bh;
    const int k = raycast_walk(Dx, Dy, Rc, code, ox, oy, ih), kb = brute(Dx, Dy, Rc, code, bx, by, bh);
    checked++;
    CHECK(k == kb && ox == bx && oy == by && ih == bh);
}

static void maps_case(int W, int density) {
    std::vector<unsigned char> m((size_t)W * W);
    for (int rep = 0; rep < 3; rep++) {
        // mostly free, so that rays run: 1 in `density` cells is occupied, as many unknown
        for (auto &c : m) { const uint32_t r = rnd() % (uint32_t)density; c = r == 0 ? RAYCAST_OCC : (r == 1 ? RAYCAST_UNKNOWN : RAYCAST_FREE); }
        const int places[6][2] = {{W / 2, W / 2}, {0, 0}, {W - 1, 0}, {1, W - 2}, {-1, W / 2}, {W / 2, W + 3}};
        for (int pl = 0; pl < 6; pl++) {
            Map map = {&m, W, places[pl][0], places[pl][1]};
            for (int Rc = 0; Rc <= 24; Rc++)
                for (int Dy = -24; Dy <= 24; Dy++)
                    for (int Dx = -24; Dx <= 24; Dx++) compare(Dx, Dy, Rc, map, W, map.X0, map.Y0);
        }
    }
}

static void free_case() {  // nothing but the cap stops a ray; Rc beyond the ray's end: nothing stops it
    const int W = 0, X0 = 0, Y0 = 0;
    for (int Rc = 0; Rc <= 40; Rc++)
        for (int Dy = -24; Dy <= 24; Dy++)
            for (int Dx = -24; Dx <= 24; Dx++) compare(Dx, Dy, Rc, AllFree(), W, X0, Y0);
}

static void big_case() {
    const int W = 0, X0 = 0, Y0 = 0;
    const int D = RAYCAST_D_MAX;
    const int ends[8][2] = {{D, D}, {-D, D - 1}, {D, -1}, {1, -D}, {-D, -D}, {D - 1, D}, {4100, -4099}, {0, D}};
    const int caps[4] = {4096, 4095, 1 << 14, 0};
    for (int e = 0; e < 8; e++)
        for (int c = 0; c < 4; c++) compare(ends[e][0], ends[e][1], caps[c], AllFree(), W, X0, Y0);
}

static void class_case() {
    const int Dx = 0, Dy = 0, W = 0, X0 = 0, Y0 = 0, Rc = 0;
    for (int tol = 0; tol <= 64; tol += (tol < 4 ? 1 : 15))
        for (int ih = 0; ih <= 140; ih++) {
            for (int im = 0; im <= 300; im++) {
                const bool early = im < ih - tol, late = im > ih + tol;
                checked++;
                CHECK(raycast_class(RAYCAST_K_OCC, ih, im, tol) == (early ? RAYCAST_C_NOVEL : late ? RAYCAST_C_THROUGH : RAYCAST_C_MATCH));
                CHECK(raycast_class(RAYCAST_K_UNKNOWN, ih, im, tol) == (early ? RAYCAST_C_NOVEL : RAYCAST_C_UNMAPPED));
                CHECK(raycast_class(RAYCAST_K_NONE, ih, im, tol) == (early ? RAYCAST_C_NOVEL : RAYCAST_C_MATCH));
            }
            // a beyond point, and the longest ray: i_h - tol and i_h + tol do not wrap
            CHECK(raycast_class(RAYCAST_K_OCC, ih, RAYCAST_I_BEYOND, tol) == RAYCAST_C_THROUGH);
            CHECK(raycast_class(RAYCAST_K_UNKNOWN, ih, RAYCAST_I_BEYOND, tol) == RAYCAST_C_UNMAPPED);
            CHECK(raycast_class(RAYCAST_K_NONE, RAYCAST_D_MAX + 1, RAYCAST_I_BEYOND, tol) == RAYCAST_C_MATCH);
        }
    CHECK(raycast_code(-32768, -32767, -32768) == RAYCAST_FREE && raycast_code(-32767, -32767, -32768) == RAYCAST_OCC);
    CHECK(raycast_code(32767, 32767, 32766) == RAYCAST_OCC && raycast_code(32766, 32767, 32766) == RAYCAST_FREE);
    CHECK(raycast_code(0, 85, -41) == RAYCAST_UNKNOWN && raycast_code(-41, 85, -41) == RAYCAST_FREE && raycast_code(85, 85, -41) == RAYCAST_OCC);
}

static void far_case() {  // step 2: the beam's far cell lies far / cell away along its longer axis
    const int Rc = 0, W = 0, X0 = 0, Y0 = 0;
    RaycastPose r = {1050.0, 1050.0, 1.0, 0.0, 0.0, 0.0, 1.0 / 100.0, 10.0, 10.0};
    int Dx = 0, Dy = 0;
    CHECK(raycast_far_cell(r, 500.0, 0.0, 3200.0, Dx, Dy) && Dx == 32 && Dy == 0);
    CHECK(raycast_far_cell(r, -1.0, -2.0, 3200.0, Dx, Dy) && Dx == -16 && Dy == -32);
    CHECK(raycast_far_cell(r, 1e300, -1e300, 3200.0, Dx, Dy) && Dx == 32 && Dy == -32);
    CHECK(!raycast_far_cell(r, 1e-310, 0.0, 3200.0, Dx, Dy));   // q overflows: x q = inf
    CHECK(!raycast_far_cell(r, 0.0, -4e-320, 3200.0, Dx, Dy));  // 0 inf = NaN
    checked += 5;
}

int main(int argc, char **argv) {
    const char *w = argc > 1 ? argv[1] : "";
    if (!std::strcmp(w, "map5")) maps_case(5, 9);
    else if (!std::strcmp(w, "map8")) maps_case(8, 12);
    else if (!std::strcmp(w, "map37")) maps_case(37, 60);
    else if (!std::strcmp(w, "free")) free_case();
    else if (!std::strcmp(w, "big")) big_case();
    else if (!std::strcmp(w, "class")) class_case();
    else if (!std::strcmp(w, "far")) far_case();
    std::printf("%ld %ld\n", checked, bad);
    return bad != 0 || checked == 0;
}
"""

CASES = ["map5", "map8", "map37", "free", "big", "class", "far"]


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def walk_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("raycast_walk")
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
def test_raycast_walk(walk_exe, case):
    out = subprocess.run([walk_exe, case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    checked, bad = map(int, out.stdout.split()[-2:])
    assert checked > 0 and bad == 0, out.stdout
