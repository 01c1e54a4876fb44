"""lslam_raycast_walk.h against tests/raycast_ref.py on the CPU: the per-beam text that the kernel
compiles (far cell, walk, class), built with g++ into a small shared object behind a plain-C++ map
accessor, must give the reference's cls and stop byte for byte on the nasty inputs of the GPU tests.
What is left to tests/test_gpu_raycast.py is the kernel's own part: the window load, the slices,
the counts.  (tests/test_raycast_walk.py runs the same header under the sanitizers in a program of
its own.)"""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

import raycast_ref as rcr
from test_gpu_occgrid import nasty_points
from test_gpu_raycast import NASTY_POSES, random_map, sparse_map
from test_raycast_walk import CSRC

SRC = r"""
#include "lslam_raycast_walk.h"
#include <math.h>

struct Grid {
    const int16_t *L;
    int X0, Y0, W, occ_min, free_max;
    int operator()(int ox, int oy) const {
        const int X = X0 + ox, Y = Y0 + oy;
        if (X < 0 || X >= W || Y < 0 || Y >= W) return RAYCAST_UNKNOWN;
        return raycast_code(L[(long)Y * W + X], occ_min, free_max);
    }
};

// one robot with a usable pose: cls [n], stop [n][3]
extern "C" void cast(const int16_t *L, int W, const double *xy, int n, const double *pose, const double *rot,
                     const double *origin, double cell, double max_range, int occ_min, int free_max, int tol,
                     unsigned char *cls, int *stop) {
    RaycastPose r;
    r.px = pose[0]; r.py = pose[1]; r.c = rot[0]; r.s = rot[1]; r.ox = origin[0]; r.oy = origin[1];
    r.inv = 1.0 / cell;
    r.X0d = floor((r.px - r.ox) * r.inv);
    r.Y0d = floor((r.py - r.oy) * r.inv);
    const Grid g = {L, (int)r.X0d, (int)r.Y0d, W, occ_min, free_max};
    const int Rc = (int)floor(max_range * r.inv);
    for (int p = 0; p < n; p++) {
        const double x = xy[2 * p], y = xy[2 * p + 1];
        int cl = 0, ox = 0, oy = 0, ih = 0;
        bool beyond = false;
        if (isfinite(x) && isfinite(y) && !(x == 0.0 && y == 0.0))
            cl = raycast_point(r, x, y, max_range * max_range, max_range + 2.0 * cell, Rc, tol, g, ox, oy, ih, beyond);
        cls[p] = (unsigned char)cl;
        stop[3 * p] = ox; stop[3 * p + 1] = oy; stop[3 * p + 2] = ih;
    }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("raycast_walk_ref")
    (d / "cast.cpp").write_text(SRC)
    # (-ffp-contract=off as the library is built: no fused multiply-add where the definition has two roundings)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC,
                           str(d / "cast.cpp"), "-o", str(d / "cast.so")])
    return C.CDLL(str(d / "cast.so"))


def compare(lib, L, xy, pose, origin, **kw):
    p = rcr.params(**kw)
    xy = np.ascontiguousarray(xy, np.float64)
    L = np.ascontiguousarray(L, np.int16)
    pose, origin = np.ascontiguousarray(pose, np.float64), np.ascontiguousarray(origin, np.float64)
    rot = np.array([np.cos(pose[2]), np.sin(pose[2])])
    cls, stop = np.zeros(len(xy), np.uint8), np.zeros((len(xy), 3), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    lib.cast(vp(L), C.c_int(L.shape[0]), vp(xy), C.c_int(len(xy)), vp(pose), vp(rot), vp(origin), C.c_double(p["cell"]),
             C.c_double(p["max_range"]), C.c_int(p["occ_min"]), C.c_int(p["free_max"]), C.c_int(p["tol"]), vp(cls), vp(stop))
    rc, rs, _, flags = rcr.cast(L, xy, pose, rot, origin, **kw)
    assert flags == 0
    bad = np.flatnonzero((cls != rc) | (stop != rs).any(1))
    assert bad.size == 0, (kw, len(bad), xy[bad[:5]], cls[bad[:5]], rc[bad[:5]], stop[bad[:5]], rs[bad[:5]])
    return rc


@pytest.mark.parametrize("tol", [0, 3, 64])
def test_header_equals_reference_on_nasty_robots(lib, tol):
    rng = np.random.default_rng(51)
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0, tol=tol)
    L = random_map(rng, 7, 80)
    seen = np.zeros(5, np.int64)
    for r in (0, 2, 3, 4, 5, 6):  # (robot 1's pose is bad: the kernel's part)
        pts = nasty_points(rng, 1500, 80, 100.0, 3000.0)
        pts[:3] = [[1e-310, 0.0], [0.0, -4e-320], [1e300, -1e300]]
        seen += np.bincount(compare(lib, L[r], pts, NASTY_POSES[r], (-4000.0, -4000.0), **kw) & 15, minlength=5)
    assert np.all(seen[[0, 1, 3, 4]] > 0) and (seen[2] > 0) == (tol < 30), seen  # (no ray here is longer than tol = 64)


@pytest.mark.parametrize("kw,pose,n", [
    (dict(grid_w=2048, cell=5.0, max_range=8000.0), (100.0, -50.0, 0.7), 400),
    (dict(grid_w=1024, cell=10.0, max_range=2795.0), (5115.0, -5100.0, 2.0), 600),
    (dict(grid_w=52, cell=100.0, max_range=3000.0, occ_min=1, free_max=-1), (2599.0, -10.0, 2.5), 600),
])
def test_header_equals_reference_on_long_rays(lib, kw, pose, n):
    rng = np.random.default_rng(52)
    W = kw["grid_w"]
    L = sparse_map(rng, 1, W, W * 3, W)[0]
    half = 0.5 * W * kw["cell"]
    compare(lib, L, nasty_points(rng, n, W, kw["cell"], kw["max_range"]), pose, (-half, -half), **kw)
