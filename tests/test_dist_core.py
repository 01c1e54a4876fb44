"""The two 1-D passes of lslam_grid_distance (lidar_slam_amd/csrc/lslam_dist_core.h), compiled with
g++ on the CPU: the text the kernel compiles.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them.

A map of W x W source bits is packed as the kernel packs it (32 rows of a column to a word, words of
a row block side by side, from a base row that need not be 0), dist_column_g gives g for every cell
into a row of bytes, dist_row_d2 gives d2 (searching from r = 1, and from the nearest unsaturated
column that dist_nearest_col finds in the row's bit mask, as the kernel does), and the result must
equal the brute-force minimum over all sources, saturated: for every W in {1, 5, 8, 16, 37, 64}, d_max in {1, 2, 3, W - 1, W, 255}, random
maps at six densities and hand-made ones (no source, one source at each end of a row and of a column,
all sources).  The bitmap is given only the rows within d_max - 1 of the band asked for, as the
kernel's bands are, for bands of every 8 rows and for the whole map.  dist_border2 is checked against
its definition.

Both passes of the shipped kernel are these functions; what the GPU tests alone cover is the packing
of the bitmap from logodds, the bands' seams and the stores.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_dist_core.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long bad = 0, checked = 0;
static uint32_t rng_state = 2468u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int brute(const std::vector<unsigned char> &src, int W, int x, int y, int d_max) {
    long best = (long)d_max * d_max;
    for (int yy = 0; yy < W; yy++)
        for (int xx = 0; xx < W; xx++)
            if (src[(size_t)yy * W + xx]) {
                const long d = (long)(x - xx) * (x - xx) + (long)(y - yy) * (y - yy);
                if (d < best) best = d;
            }
    return (int)best;
}

// rows [y0, y1) of the field from a bitmap of rows [base, top) only, exactly sized: ASan sees any read outside
static void band(const std::vector<unsigned char> &src, int W, int d_max, int y0, int y1, const char *what) {
    const int hal = (d_max < W ? d_max : W) - 1;
    const int base = y0 - hal > 0 ? y0 - hal : 0, top = y1 + hal < W ? y1 + hal : W;
    const int nblk = (top - base + 31) >> 5;
    std::vector<uint32_t> bits((size_t)nblk * W, 0u);
    for (int y = base; y < top; y++)
        for (int x = 0; x < W; x++)
            if (src[(size_t)y * W + x]) bits[(size_t)((y - base) >> 5) * W + x] |= 1u << ((y - base) & 31);
    std::vector<uint8_t> g(W);
    for (int y = y0; y < y1; y++) {
        for (int x = 0; x < W; x++) {
            const int v = dist_column_g(bits.data() + x, W, nblk, y - base, d_max);
            int want = d_max;  // the column's nearest source, over the whole map
            for (int yy = 0; yy < W; yy++)
                if (src[(size_t)yy * W + x] && abs(yy - y) < want) want = abs(yy - y);
            checked++;
            if (v != want && bad++ < 20) std::printf("%s: g W %d d_max %d (%d, %d): %d, want %d\n", what, W, d_max, x, y, v, want);
            g[x] = (uint8_t)v;
        }
        // the row's unsaturated columns as the kernel's ballots give them, exactly sized
        std::vector<uint64_t> mask((size_t)(W + 63) >> 6, 0);
        for (int x = 0; x < W; x++)
            if (g[x] < d_max) mask[(size_t)x >> 6] |= (uint64_t)1 << (x & 63);
        for (int x = 0; x < W; x++) {
            const int want = brute(src, W, x, y, d_max);
            const int v = dist_row_d2(g.data(), W, x, d_max);  // the search from r = 1
            int r0 = d_max;  // the nearest unsaturated column, x included
            for (int xx = 0; xx < W; xx++)
                if (g[xx] < d_max && abs(xx - x) < r0) r0 = abs(xx - x);
            const int n = dist_nearest_col(mask.data(), (W + 63) >> 6, x, d_max);
            const int u = n < d_max ? dist_row_d2(g.data(), W, x, d_max, n) : d_max * d_max;  // as the kernel: from the mask
            checked += 3;
            if (v != want && bad++ < 20) std::printf("%s: d2 W %d d_max %d (%d, %d): %d, want %d\n", what, W, d_max, x, y, v, want);
            if (n != r0 && bad++ < 20) std::printf("%s: nearest W %d d_max %d (%d, %d): %d, want %d\n", what, W, d_max, x, y, n, r0);
            if (u != want && bad++ < 20) std::printf("%s: d2 from the mask W %d d_max %d (%d, %d): %d, want %d\n", what, W, d_max, x, y, u, want);
        }
    }
}

static void one_map(const std::vector<unsigned char> &src, int W, const char *what) {
    const int dm[6] = {1, 2, 3, W - 1, W, 255};
    for (int k = 0; k < 6; k++) {
        if (dm[k] < 1) continue;
        band(src, W, dm[k], 0, W, what);
        for (int y0 = 0; y0 < W; y0 += 8) band(src, W, dm[k], y0, y0 + 8 < W ? y0 + 8 : W, what);
    }
}

static void width(int W) {
    std::vector<unsigned char> src((size_t)W * W);
    const int per_mille[6] = {0, -1, 1, 30, 500, 1000};  // -1: one cell
    for (int d = 0; d < 6; d++) {
        for (auto &c : src) c = per_mille[d] > 0 && (int)(rnd() % 1000u) < per_mille[d];
        if (per_mille[d] < 0) src[(size_t)(rnd() % (uint32_t)W) * W + rnd() % (uint32_t)W] = 1;
        one_map(src, W, "random");
    }
    // one source at each end of a row and of a column; both ends at once
    const int ends[5][2] = {{0, W / 2}, {W - 1, W / 2}, {W / 2, 0}, {W / 2, W - 1}, {0, 0}};
    for (int e = 0; e < 5; e++) {
        std::fill(src.begin(), src.end(), 0);
        src[(size_t)ends[e][1] * W + ends[e][0]] = 1;
        if (e == 4) src[(size_t)(W - 1) * W + W - 1] = 1;
        one_map(src, W, "ends");
    }
}

static void border() {
    for (int W = 1; W <= 40; W++)
        for (int y = 0; y < W; y++)
            for (int x = 0; x < W; x++) {
                int b = 1 << 30;  // the nearest cell off the map along an axis
                for (int t = -1; t <= W; t += W + 1) {
                    if (abs(x - t) < b) b = abs(x - t);
                    if (abs(y - t) < b) b = abs(y - t);
                }
                checked++;
                if (dist_border2(x, y, W) != b * b && bad++ < 20) std::printf("border W %d (%d, %d)\n", W, x, y);
            }
}

int main(int argc, char **argv) {
    const char *w = argc > 1 ? argv[1] : "";
    if (!std::strcmp(w, "border")) border();
    else if (std::atoi(w) > 0) width(std::atoi(w));
    std::printf("%ld %ld\n", checked, bad);
    return bad != 0 || checked == 0;
}
"""

CASES = ["1", "5", "8", "16", "37", "64", "border"]


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("dist_core")
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
def test_dist_core(core_exe, case):
    out = subprocess.run([core_exe, case], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    checked, bad = map(int, out.stdout.split()[-2:])
    assert checked > 0 and bad == 0, out.stdout
