"""GPU parity of the distance field (lslam_grid_distance, lidar_slam_amd.mapping.DistanceField) against
its NumPy definition, tests/dist_ref.py.  The transform is integers from end to end: d2, n_src and
flags are compared EXACTLY.  In every case d2 is pre-filled with 0xFFFF, which no field can hold (the
largest cap is 65025), so an unwritten cell shows; and logodds is read back unchanged.

The kernel has one form and two paths into it: 16-byte groups of 8 cells where grid_w is a multiple of
8, a lane per column otherwise (grid_w 52).  A robot's rows go to one workgroup when the robots alone
fill the chip (the 600-robot case) and to up to 16 bands otherwise; the bands' seams lie at multiples
of 8 rows and every small case crosses them.
"""
import numpy as np
import pytest

import dist_ref as dr
from test_dist_ref import DENSITIES, random_map

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def make(ctx, L, **kw):
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    R, W = L.shape[0], L.shape[1]
    g = OccupancyGrid(ctx, R, grid_w=W)
    g.upload(L)
    return g, DistanceField(g, **kw)


def run(ctx, L, calls=1, **kw):
    """`calls` transforms of freshly uploaded grids into a d2 pre-filled with 0xFFFF, each compared with
    the reference; returns the device's results."""
    g, f = make(ctx, L, **kw)
    f.d2.upload(np.full(L.shape, 0xFFFF, np.uint16))
    want = dr.field_batch(L, **kw)
    for call in range(calls):
        f.step()
        res = f.results()
        assert np.array_equal(res["n_src"], want[1]), (kw, call, res["n_src"], want[1])
        assert np.array_equal(res["flags"], want[2]), (kw, call, res["flags"], want[2])
        bad = np.argwhere(res["d2"] != want[0])
        assert bad.size == 0, (kw, call, len(bad), bad[:5], [res["d2"][tuple(b)] for b in bad[:5]], [want[0][tuple(b)] for b in bad[:5]])
    assert g.logodds.download().tobytes() == np.ascontiguousarray(L, np.int16).tobytes()  # the grid is read only
    return res


def density_maps(rng, W):
    """Seven robots: one map per density of test_dist_ref, and one of random int16 values."""
    maps = [random_map(rng, W, d) for d in DENSITIES]
    maps[0] = np.minimum(maps[0], -1).astype(np.int16)  # no source in either mode
    maps.append(rng.integers(-32768, 32768, (W, W)).astype(np.int16))
    return np.stack(maps)


@pytest.mark.parametrize("mode", [dr.OCC, dr.NOT_FREE])
@pytest.mark.parametrize("W", [16, 24, 52, 64, 80])
def test_small(ctx, W, mode):
    L = density_maps(np.random.default_rng(7 * W + mode), W)
    for d_max in (1, 2, 7, 64, 255):
        res = run(ctx, L, mode=mode, d_max=d_max)
        assert res["flags"][0] == dr.EMPTY and res["flags"][1] == 0 and res["n_src"][5] > W * W // 2
    # thresholds other than the defaults, the int16 ends among them
    for kw in (dict(occ_min=-32768), dict(occ_min=32767), dict(occ_min=1), dict(free_max=32767), dict(free_max=-32768),
               dict(free_max=-42)):
        run(ctx, L, mode=mode, d_max=7, **kw)


@pytest.mark.parametrize("W", [24, 52])
def test_sources_on_the_borders(ctx, W):
    maps = []
    for k in range(9):
        L = np.full((W, W), -41, np.int16)
        if k == 0:
            L[0, :] = 85
        elif k == 1:
            L[W - 1, :] = 85
        elif k == 2:
            L[:, 0] = 85
        elif k == 3:
            L[:, W - 1] = 85
        else:  # a single corner; all four
            for c in ([(0, 0)], [(0, W - 1)], [(W - 1, 0)], [(W - 1, W - 1)], [(0, 0), (0, W - 1), (W - 1, 0), (W - 1, W - 1)])[k - 4]:
                L[c] = 85
        maps.append(L)
    L = np.stack(maps)
    for mode in (dr.OCC, dr.NOT_FREE):
        for d_max in (3, 64):
            run(ctx, L, mode=mode, d_max=d_max, free_max=84)
    res = run(ctx, L, d_max=255)
    assert res["d2"][7, 0, 0] == 2 * (W - 1) ** 2 and res["d2"][4, W - 1, W - 1] == 2 * (W - 1) ** 2


def test_saturation(ctx):
    L = np.zeros((2, 256, 256), np.int16)
    L[0, 0, 0] = 85
    L[1, 255, 255] = 350
    d2 = run(ctx, L, d_max=255)["d2"]
    assert d2[0, 0, 254] == 254 * 254 and d2[0, 0, 255] == 65025 and d2[0, 255, 0] == 65025
    assert d2[0, 200, 150] == 62500 and d2[0, 200, 160] == 65025 and d2[0, 255, 255] == 65025
    assert d2[1, 255, 1] == 254 * 254 and d2[1, 255, 0] == 65025 and d2[1, 55, 105] == 62500
    # per robot the cells outside a quarter disc of radius 255: about 256^2 - pi 255^2 / 4 = 14,465
    assert 2 * 14000 < (d2 == 65025).sum() < 2 * 15000


def room_like(W=512):
    """Walls two cells thick around a free interior, unknown outside: int16 [W, W]."""
    L = np.zeros((W, W), np.int16)
    L[100:400, 120:330] = -200
    for a, b in ((100, 102), (398, 400)):
        L[a:b, 120:330] = 350
    for a, b in ((120, 122), (328, 330)):
        L[100:400, a:b] = 170
    L[250, 200:240] = 85  # a piece of furniture, one hit thick
    return L


def test_defaults(ctx):
    from lidar_slam_amd import _lib
    rng = np.random.default_rng(5)
    L = np.stack([room_like(), np.full((512, 512), -41, np.int16), random_map(rng, 512, 0.5)])
    g, f = make(ctx, L)
    assert (f.p.mode, f.p.occ_min, f.p.free_max, f.p.d_max, f.q.off2) == (0, 85, -1, 64, 4096)
    res = run(ctx, L)
    assert res["flags"].tolist() == [0, _lib.DIST_EMPTY, 0] and res["n_src"][1] == 0
    assert np.all(res["d2"][1] == 4096) and res["d2"][0, 250, 225] == 0 and res["d2"][0, 240, 225] == 100
    assert res["d2"][0, 0, 0] == 4096 and res["d2"][2].max() <= 25
    run(ctx, L, mode=dr.NOT_FREE)


def test_largest(ctx):
    rng = np.random.default_rng(2048)
    L = np.full((1, 2048, 2048), -41, np.int16)
    n = 600
    L[0, rng.integers(0, 2048, n), rng.integers(0, 2048, n)] = 200
    L[0, 2047, 2047] = L[0, 0, 2047] = 85
    res = run(ctx, L, d_max=40)
    assert res["n_src"][0] > 590 and res["d2"].max() == 1600 and res["d2"][0, 2047, 2040] <= 49


def test_batch_and_one_robot_alone(ctx):
    rng = np.random.default_rng(130)
    L = np.stack([random_map(rng, 64, DENSITIES[2 + r % 3]) for r in range(130)])
    res = run(ctx, L, d_max=20)
    alone = run(ctx, L[77:78], d_max=20)
    assert alone["d2"].tobytes() == res["d2"][77:78].tobytes() and alone["n_src"][0] == res["n_src"][77]
    # enough robots that each gets one workgroup: the band is the whole map (40 rows: five groups of 8)
    Lm = np.stack([random_map(rng, 40, DENSITIES[1 + r % 5]) for r in range(600)])
    for mode in (dr.OCC, dr.NOT_FREE):
        run(ctx, Lm, mode=mode, d_max=9)
    run(ctx, Lm[:, :36, :36], d_max=9)  # and a lane per column


def test_repeat_and_a_changed_grid(ctx):
    rng = np.random.default_rng(9)
    L = density_maps(rng, 80)
    a = run(ctx, L, calls=2, d_max=33)
    # the field follows the grid: a new map into the same buffers
    g, f = make(ctx, L, d_max=33)
    f.step()
    L2 = density_maps(rng, 80)[::-1].copy()
    g.upload(L2)
    f.step(sync=False)
    f.ctx.sync()
    res = f.results()
    want = dr.field_batch(L2, d_max=33)
    assert np.array_equal(res["d2"], want[0]) and np.array_equal(res["n_src"], want[1]) and np.array_equal(res["flags"], want[2])
    assert not np.array_equal(res["d2"], a["d2"])


def test_overlap_and_parameters_are_refused(ctx):
    import ctypes as C
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    g = OccupancyGrid(ctx, 2, grid_w=64)
    with pytest.raises(ValueError):
        DistanceField(g, d_max=256)
    with pytest.raises(ValueError):
        DistanceField(g, mode=2)
    with pytest.raises(TypeError):
        DistanceField(g, tol=3)
    f = DistanceField(g)
    with pytest.raises(ValueError):
        f.results()
    b = _lib.DistBatch()
    b.n_robots = 2
    b.logodds, b.n_src, b.flags = g.logodds.addr, f.n_src.addr, f.flags.addr
    b.d2 = g.logodds.addr + 64 * 64 * 2  # the second robot's grid
    st = _lib.load().lslam_grid_distance(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.p))
    assert st == _lib.LSLAM_ERR_ARG and b"overlaps" in _lib.load().lslam_last_error()
    # grid_w 2048 holds a bitmap of d_max up to 205
    big = OccupancyGrid(ctx, 1, grid_w=2048)
    fb = DistanceField(big, d_max=206)
    with pytest.raises(_lib.HIPLibraryError, match="does not fit LDS"):
        fb.step()
    # the largest that fits, around one source: the disc of radius 205 and nothing else
    L = np.zeros((1, 2048, 2048), np.int16)
    L[0, 1000, 1100] = 85
    big.upload(L)
    fl = DistanceField(big, d_max=205)
    fl.d2.upload(np.full(L.shape, 0xFFFF, np.uint16))
    fl.step()
    d2 = fl.results()["d2"][0].astype(np.int64)
    y, x = np.mgrid[:2048, :2048]
    assert np.array_equal(d2, np.minimum((x - 1100) ** 2 + (y - 1000) ** 2, 205 * 205))
