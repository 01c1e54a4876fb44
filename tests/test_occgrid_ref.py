"""The occupancy-grid definition (include/lidarslam.h, lslam_grid_update) on the CPU: properties of
the integer ray, the clamp that is applied once per revolution, the quality of the map it builds of
the synthetic room, and the ABI checks that need no device.  tests/occgrid_ref.py is the NumPy form
of the definition; tests/test_gpu_occgrid.py holds the kernel to it bit for bit.

Room quality.  Robots 200-207 drive five revolutions (synth.trajectory with u = (146, 174), steps
0-4) in the 4000 x 3000 mm room; grid_w 256 at 20 mm, origin (-560, -1060).  Per robot, at the
true poses and at poses moved by 10 mm and pi/720 rad (the bounds that
test_gpu_scanmatch.test_end_to_end_without_odometry asserts of the filter):
  * of the cells with L >= 170 (two hits' worth), the fraction whose centre lies within 80 mm of a
    wall line: >= 99 %  (measured here: >= 99.86 %, both runs; seven robots of eight at 100 %);
  * of the interior cells (centre more than 100 mm inside the room), the fraction with L < 0:
    >= 99 %  (measured: >= 99.82 % at the true poses, >= 99.85 % at the moved ones);
  * interior cells with L >= 170: none (measured: none).
"""
import ctypes as C

import numpy as np
import pytest

import occgrid_ref as ogr
from lidar_slam_amd import _lib, synth

ROOM_ROBOTS = list(range(200, 208))
ROOM_KW = dict(grid_w=256)
ROOM_ORIGIN = (-560.0, -1060.0)


def room_run():
    """The five revolutions of the room test: (poses [5, R, 3], revolutions)."""
    poses = synth.trajectory(ROOM_ROBOTS, 4, u=(146.0, 174.0))
    return poses, [synth.revolutions_at(poses[k], k, ROOM_ROBOTS) for k in range(5)]


def moved(poses):
    """Every pose moved by 10 mm (in a direction that changes with robot and step) and pi/720 rad."""
    out = np.array(poses, np.float64)
    K, R = out.shape[:2]
    k, i = np.meshgrid(np.arange(K), np.arange(R), indexing="ij")
    a = 2.4 * (R * k + i)
    out[..., 0] += 10.0 * np.cos(a)
    out[..., 1] += 10.0 * np.sin(a)
    out[..., 2] += np.where((k + i) % 2 == 0, 1.0, -1.0) * (np.pi / 720)
    return out


def room_stats(L, origin=ROOM_ORIGIN, cell=20.0):
    """One robot's grid -> (fraction of the L >= 170 cells within 80 mm of a wall line, fraction of
    the interior cells with L < 0, number of interior cells with L >= 170)."""
    W = L.shape[0]
    cx = origin[0] + (np.arange(W) + 0.5) * cell
    cy = origin[1] + (np.arange(W) + 0.5) * cell
    X, Y = np.meshgrid(cx, cy)  # row Y
    d_wall = np.minimum(np.minimum(np.abs(X), np.abs(X - synth.ROOM_W)), np.minimum(np.abs(Y), np.abs(Y - synth.ROOM_H)))
    interior = (X > 100.0) & (X < synth.ROOM_W - 100.0) & (Y > 100.0) & (Y < synth.ROOM_H - 100.0)
    occ = L >= 170
    assert occ.any() and interior.any()
    return (float(np.mean(d_wall[occ] <= 80.0)), float(np.mean(L[interior] < 0)), int(np.sum(occ & interior)))


def assert_room(L, what):
    for i in range(L.shape[0]):
        near, free, ghosts = room_stats(L[i])
        print("%s robot %d: occupied near a wall %.4f, interior free %.4f, interior occupied %d"
              % (what, ROOM_ROBOTS[i], near, free, ghosts))
        assert near >= 0.99 and free >= 0.99 and ghosts == 0, (what, i, near, free, ghosts)


def test_ray_properties():
    for X1 in range(-40, 41):
        for Y1 in range(-40, 41):
            free, hit = ogr.ray_cells(0, 0, X1, Y1)
            n = max(abs(X1), abs(Y1))
            assert len(free) == n and hit == (X1, Y1)
            if n == 0:
                continue
            assert tuple(free[0]) == (0, 0)
            path = np.concatenate([free, [hit]])
            assert np.all(np.max(np.abs(np.diff(path, axis=0)), axis=1) == 1), (X1, Y1)
            if X1 >= 0 and Y1 >= X1:  # one octant against its seven images
                for sx in (1, -1):
                    for sy in (1, -1):
                        f2, _ = ogr.ray_cells(0, 0, sx * X1, sy * Y1)
                        assert np.array_equal(f2, free * [sx, sy]), (X1, Y1, sx, sy)
                        f3, _ = ogr.ray_cells(0, 0, sy * Y1, sx * X1)
                        assert np.array_equal(f3, (free * [sx, sy])[:, ::-1]), (X1, Y1, sx, sy)
    # a robot cell away from the origin only shifts the ray
    free, hit = ogr.ray_cells(-7, 12, -7 + 9, 12 - 30)
    f0, _ = ogr.ray_cells(0, 0, 9, -30)
    assert np.array_equal(free, f0 + [-7, 12]) and hit == (2, -18)


KW = dict(grid_w=32, cell=100.0, max_range=3000.0)


def test_clamp_once_per_revolution():
    p = ogr.params(**KW)
    pose, origin = (1050.0, 1050.0, 0.0), (0.0, 0.0)  # robot cell (10, 10), heading +x
    a = np.arange(720) * (2 * np.pi / 720)
    ring = np.stack([500.0 * np.cos(a), 500.0 * np.sin(a)], -1)
    L, n_used, flags = ogr.update(np.zeros((32, 32), np.int16), ring, pose, None, origin, **KW)
    assert n_used.tolist() == [720, 0] and flags == 0
    assert L[10, 10] == p["l_min"]  # 720 passes, clamped once
    assert L.min() == p["l_min"] and L.max() <= p["l_max"]

    # one hit in cell (15, 10) and three rays that pass it on their way to (18..20, 10)
    pts = np.array([[500.0, 0.0], [800.0, 0.0], [900.0, 0.0], [1000.0, 0.0]])
    L0 = np.zeros((32, 32), np.int16)
    L0[10, 15] = p["l_max"] - 10
    L0[3, 3], L0[4, 4] = 5000, -7000  # outside the clamp range, untouched by any ray
    L, n_used, flags = ogr.update(L0, pts, pose, None, origin, **KW)
    assert L[10, 15] == p["l_max"] - 10 + 85 - 123 == 302
    assert L[3, 3] == 5000 and L[4, 4] == -7000
    assert L[10, 10] == 4 * p["l_miss"] and L[10, 20] == p["l_hit"]
    # the same four rays one at a time clamp in between: a different, order-dependent answer
    Ls = L0
    for q in pts:
        Ls = ogr.update(Ls, q[None], pose, None, origin, **KW)[0]
    assert Ls[10, 15] == p["l_max"] - 123


def test_flags_and_counts():
    L0 = np.full((32, 32), 7, np.int16)
    pts = np.array([[500.0, 0.0], [0.0, 0.0], [np.nan, 1.0], [np.inf, 1.0], [2999.0, 0.0], [3001.0, 0.0], [0.0, -1200.0]])
    L, n_used, flags = ogr.update(L0, pts, (1050.0, 1050.0, 0.0), None, (0.0, 0.0), **KW)
    assert n_used.tolist() == [3, 1] and flags == ogr.CLIPPED  # (2999, 0) ends in cell 40; (0, -1200) in row -2
    assert L[10, 31] == 7 - 41 and L[0, 10] == 7 - 41 and L[10, 15] == 7 + 85 - 41
    for pose in [(np.nan, 0.0, 0.0), (0.0, 0.0, np.inf), (100.0 * 2.0 ** 20, 0.0, 0.0)]:
        L, n_used, flags = ogr.update(L0, pts, pose, None, (0.0, 0.0), **KW)
        assert flags == ogr.BAD_POSE and n_used.tolist() == [0, 0] and np.array_equal(L, L0)
    L, n_used, flags = ogr.update(L0, pts, (0.0, 0.0, 0.0), None, (np.nan, 0.0), **KW)
    assert flags == ogr.BAD_POSE
    # a robot outside the grid, its ray entering it
    L, n_used, flags = ogr.update(L0, [[1000.0, 0.0]], (-450.0, 1050.0, 0.0), None, (0.0, 0.0), **KW)
    assert flags == ogr.CLIPPED and L[10, 5] == 7 + 85 and L[10, 0] == 7 - 41 and n_used.tolist() == [1, 0]


def build_room(poses, revs):
    R = len(ROOM_ROBOTS)
    L = np.zeros((R, 256, 256), np.int16)
    for k, rev in enumerate(revs):
        off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
        L, n_used, flags = ogr.update_batch(L, rev["xy"], off, poses[k], None, np.tile(ROOM_ORIGIN, (R, 1)), **ROOM_KW)
        # (an outlier return may end outside the grid: CLIPPED is legitimate here)
        assert not (flags & ogr.BAD_POSE).any() and np.all(n_used[:, 0] == 720)
    return L


@pytest.fixture(scope="module")
def room():
    return room_run()


def test_room_quality_at_true_poses(room):
    poses, revs = room
    assert_room(build_room(poses, revs), "true poses")


def test_room_quality_at_moved_poses(room):
    poses, revs = room
    m = moved(poses)
    d = m - poses
    assert np.allclose(np.hypot(d[..., 0], d[..., 1]), 10.0) and np.allclose(np.abs(d[..., 2]), np.pi / 720)
    assert_room(build_room(m, revs), "moved poses")


def test_grid_params_default():
    p = _lib.grid_params()
    got = {k: getattr(p, k) for k in ogr.DEFAULTS}
    assert got == ogr.DEFAULTS == dict(cell=20.0, max_range=8000.0, grid_w=512, l_hit=85, l_miss=-41, l_min=-200,
                                       l_max=350)
    assert p.reserved == 0
    assert _lib.GRID_BAD_POSE == ogr.BAD_POSE == 1 and _lib.GRID_CLIPPED == ogr.CLIPPED == 2 and _lib.K_GRID == 10


def test_grid_struct_sizes():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_grid_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.GridParams) == 40
    assert got[1] == C.sizeof(_lib.GridBatch) == 72
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_grid_abi_sizes(one, 1) == 2 and list(one) == [40, -1]
    nine = (C.c_int64 * 9)()
    assert L.lslam_abi_sizes(nine, 9) == 9
    assert _lib.ABI_VERSION == 6


BAD_FIELDS = [("cell", 0.0), ("cell", -1.0), ("cell", float("nan")), ("max_range", 0.0), ("max_range", float("inf")),
              ("max_range", 20.0 * 4096 + 1.0), ("grid_w", 15), ("grid_w", 2049), ("l_hit", 0), ("l_hit", 1025),
              ("l_miss", 0), ("l_miss", -1025), ("l_min", 0), ("l_min", -32769), ("l_max", 0), ("l_max", 32768)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_grid_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    L = _lib.load()
    b = _lib.GridBatch()
    assert L.lslam_grid_update(None, C.byref(b), C.byref(_lib.grid_params())) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()  # valid parameters, an empty batch: only the context is missing
    p = _lib.grid_params(**{field: value})
    assert L.lslam_grid_update(None, C.byref(b), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert field.encode() in L.lslam_last_error()


def test_grid_accepts_the_ends_of_the_ranges():
    L = _lib.load()
    b = _lib.GridBatch()
    for kw in (dict(grid_w=16, l_hit=1, l_miss=-1, l_min=-1, l_max=1), dict(max_range=20.0 * 4096),
               dict(grid_w=2048, l_hit=1024, l_miss=-1024, l_min=-32768, l_max=32767)):
        assert L.lslam_grid_update(None, C.byref(b), C.byref(_lib.grid_params(**kw))) == _lib.LSLAM_ERR_ARG
        assert b"ctx" in L.lslam_last_error(), kw


def test_grid_missing_pointers():
    L = _lib.load()
    p = _lib.grid_params()
    b = _lib.GridBatch()
    b.n_robots = 1
    assert L.lslam_grid_update(None, C.byref(b), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    b.xy = b.pt_off = b.pose = b.origin = 4096
    assert L.lslam_grid_update(None, C.byref(b), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing output" in L.lslam_last_error()
    b.n_robots = -1
    assert L.lslam_grid_update(None, C.byref(b), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_update(None, None, C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_update(None, C.byref(b), None) == _lib.LSLAM_ERR_ARG
