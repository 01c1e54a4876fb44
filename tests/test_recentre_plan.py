"""The plan of a grid recentre (lidar_slam_amd/csrc/lslam_recentre_plan.h), compiled with g++ on the
CPU: the text the kernel compiles.  The program is built with -fsanitize=address,undefined when the
compiler here can link an empty program with them, so a source index off the map is an error, not a
wrong cell.

The program executes the plan IN PLACE on a plain array whose cells hold their own flat index: band
after band in the plan's order, each band read completely into a buffer and only then stored.  The
result is compared with an out-of-place shift for W in {5, 8, 16, 37, 52, 64}, every (sx, sy) in
[-W-2, W+2]^2 and band heights 1, 3 and the shipped recentre_band_rows(W); a row that a later band
reads after an earlier one stored it shows as a wrong index.  The shift rule is held to a
loop-by-loop form for every c in [-3W, 3W], margin 0 .. W/2 and quantum 1 .. 64."""
import os
import shutil
import subprocess

import pytest

import recentre_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

PROG = r"""
#include "lslam_recentre_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long bad = 0, checked = 0;
#define CHECK(x, ...) do { if (!(x)) { if (bad++ < 20) { std::printf("line %d: %s: ", __LINE__, #x); std::printf(__VA_ARGS__); \
    std::printf("\n"); } } } while (0)

// the plan in place: a band is read completely, then stored
static void run_plan(std::vector<int> &a, int W, int sx, int sy, int B) {
    const RecentrePlan p = recentre_plan(W, sx, sy, B);
    std::vector<int> buf((size_t)B * W);  // exactly a band: a larger one is an out-of-bounds write
    int rows_done = 0, prev_y0 = -1;
    for (int k = 0; k < p.nbands; k++) {
        const RecentreBand b = recentre_band(p, k);
        CHECK(b.y0 >= 0 && b.y0 < b.y1 && b.y1 <= W && b.y1 - b.y0 <= B, "band %d rows [%d, %d)", k, b.y0, b.y1);
        CHECK(b.y0 <= b.cy0 && b.cy0 <= b.cy1 && b.cy1 <= b.y1, "band %d copy rows [%d, %d)", k, b.cy0, b.cy1);
        if (k > 0) CHECK(sy >= 0 ? b.y0 > prev_y0 : b.y0 < prev_y0, "order at band %d", k);
        prev_y0 = b.y0;
        for (int y = b.y0; y < b.y1; y++)
            for (int x = 0; x < W; x++) {
                int src = -1;
                const bool copy = recentre_source(p, b, y, x, src);
                buf[(size_t)(y - b.y0) * W + x] = copy ? a[(size_t)src] : 0;
            }
        for (int y = b.y0; y < b.y1; y++)
            for (int x = 0; x < W; x++) a[(size_t)y * W + x] = buf[(size_t)(y - b.y0) * W + x];
        rows_done += b.y1 - b.y0;
    }
    CHECK(rows_done == W, "rows stored %d of %d", rows_done, W);
}

static void plan_case(int W, int Bforce) {
    const int B = Bforce > 0 ? Bforce : recentre_band_rows(W);
    for (int sy = -W - 2; sy <= W + 2; sy++)
        for (int sx = -W - 2; sx <= W + 2; sx++) {
            std::vector<int> a((size_t)W * W), want((size_t)W * W);
            for (int i = 0; i < W * W; i++) a[i] = i + 1;  // (0 is the fill)
            for (int y = 0; y < W; y++)
                for (int x = 0; x < W; x++) {
                    const int ys = y + sy, xs = x + sx;
                    want[(size_t)y * W + x] = (ys >= 0 && ys < W && xs >= 0 && xs < W) ? ys * W + xs + 1 : 0;
                }
            run_plan(a, W, sx, sy, B);
            checked++;
            CHECK(a == want, "W %d B %d shift (%d, %d)", W, B, sx, sy);
        }
}

// far shifts: what a robot cell near +-2^20 gives; nothing overflows, nothing is copied
static void far_case() {
    const int far[4] = {5000, -5000, (1 << 20) + 2048, -(1 << 20) - 2048};
    for (int W = 5; W <= 64; W += 59)
        for (int i = 0; i < 4; i++)
            for (int j = -1; j <= 1; j++) {
                std::vector<int> a((size_t)W * W, 7), zero((size_t)W * W, 0), b = a;
                run_plan(a, W, far[i], j * 3, recentre_band_rows(W));
                run_plan(b, W, j * 3, far[i], 3);
                checked += 2;
                CHECK(a == zero && b == zero, "W %d far %d", W, far[i]);
            }
}

static void band_rows_case() {
    for (int W = 1; W <= 2048; W++) {
        const int B = recentre_band_rows(W);
        checked++;
        CHECK(B >= 1 && B <= W && (B * W <= RECENTRE_BAND_CELLS || B == 1), "W %d B %d", W, B);
        CHECK(B == W || (B + 1) * W > RECENTRE_BAND_CELLS, "W %d B %d is not the most", W, B);
        if (W >= 16) CHECK(B >= 8 && B * W <= RECENTRE_BAND_CELLS, "W %d B %d", W, B);
    }
    std::printf("rows %d %d %d %d %d\n", recentre_band_rows(52), recentre_band_rows(64), recentre_band_rows(256),
                recentre_band_rows(512), recentre_band_rows(2048));
}

// the shift rule against a search: the multiple of quantum that brings c nearest W/2, ties and
// signs as floor((c - W/2 + quantum/2) / quantum) has them
static void shift_case(int W) {
    for (int q = 1; q <= 64; q++)
        for (int c = -3 * W; c <= 3 * W; c++) {
            // loop form of floordiv: the largest m with m q <= c - W/2 + q/2
            const int t = c - W / 2 + q / 2;
            int m = -8 * W - 64;
            while ((m + 1) * q <= t) m++;
            const int s = recentre_axis_shift(c, W, q);
            checked++;
            CHECK(s == m * q, "W %d q %d c %d: %d != %d", W, q, c, s, m * q);
            // what it is for: the robot cell lands within q/2 of the middle
            const int left = c - s - W / 2;
            CHECK(left >= -(q / 2) && left < q - q / 2, "W %d q %d c %d leaves %d", W, q, c, left);
            for (int margin = 0; margin <= W / 2; margin++) {
                const int other = W / 2;  // the other axis sits in the middle: only c can trigger
                const bool inside = margin <= c && c < W - margin && margin <= other && other < W - margin;
                int sx = 99, sy = 99, tx = 99, ty = 99;
                recentre_shift(c, other, W, margin, q, sx, sy);
                recentre_shift(other, c, W, margin, q, tx, ty);
                const int so = q * ((other - W / 2 + q / 2) / q);  // (non-negative: plain division)
                CHECK(sx == (inside ? 0 : s) && sy == (inside ? 0 : so), "W %d q %d c %d margin %d", W, q, c, margin);
                CHECK(ty == (inside ? 0 : s) && tx == (inside ? 0 : so), "W %d q %d c %d margin %d (y)", W, q, c, margin);
            }
        }
}

int main(int argc, char **argv) {
    const char *w = argc > 1 ? argv[1] : "";
    const int W = argc > 2 ? std::atoi(argv[2]) : 0, B = argc > 3 ? std::atoi(argv[3]) : 0;
    if (!std::strcmp(w, "plan")) plan_case(W, B);
    else if (!std::strcmp(w, "far")) far_case();
    else if (!std::strcmp(w, "rows")) band_rows_case();
    else if (!std::strcmp(w, "shift")) shift_case(W);
    std::printf("%ld %ld\n", checked, bad);
    return bad != 0 || checked == 0;
}
"""

WIDTHS = [5, 8, 16, 37, 52, 64]


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("recentre_plan")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe)


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    checked, bad = map(int, out.stdout.split()[-2:])
    assert checked > 0 and bad == 0, out.stdout
    return out.stdout


@pytest.mark.parametrize("band", [1, 3, 0], ids=["band1", "band3", "shipped"])
@pytest.mark.parametrize("W", WIDTHS)
def test_plan_in_place(plan_exe, W, band):
    _run(plan_exe, "plan", W, band)


def test_far_shifts_clear(plan_exe):
    _run(plan_exe, "far")


def test_band_rows(plan_exe):
    """The most whole rows that 16384 cells hold, and the Python mirrors of it."""
    from lidar_slam_amd import mapping
    out = _run(plan_exe, "rows")
    rows = [int(v) for v in out.splitlines()[0].split()[1:]]
    assert rows == [52, 64, 64, 32, 8]
    assert rows == [mapping.recentre_band_rows(w) for w in (52, 64, 256, 512, 2048)]
    assert rows == [rr.band_rows(w) for w in (52, 64, 256, 512, 2048)]


@pytest.mark.parametrize("W", WIDTHS)
def test_shift_rule(plan_exe, W):
    _run(plan_exe, "shift", W)
