"""GPU parity of the Gauss-Newton alignment in the distance field (lslam_field_align,
DistanceField.align) against its NumPy definition, tests/fieldalign_ref.py, over fields that the device
made (lslam_grid_distance, held to tests/dist_ref.py in the same breath).

Every double operation of the definition is rounded on its own and the sums are integers, so pose_out,
trace, normal, n_used, iters and flags are compared EXACTLY (the doubles as bit patterns), the reference
being fed the (cos, sin) that the device wrote to trace; those are themselves held to 1e-15 against
NumPy's, as test_gpu_occgrid.assert_rot holds rot.  The end-to-end case repeats the cap of
tests/test_fieldalign_ref.py on the device's own grid.
"""
import ctypes as C

import numpy as np
import pytest

import dist_ref as dr
import fieldalign_ref as far
from oracle import cpu as orc
from test_fieldalign_ref import assert_room_align
from test_fieldscore_ref import ROOM_DIST
from test_gpu_fieldscore import field_of
from test_gpu_occgrid import csr, nasty_points
from test_gpu_raycast import NASTY_POSES, NASTY_SIZES, random_map
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, room_run

pytestmark = pytest.mark.gpu

ALIGN_KEYS = tuple(far.DEFAULTS)


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_trace_rot(trace, iters, flags):
    """(cos, sin) of every evaluation made against NumPy's of the traced heading: 1e-15."""
    worst = 0.0
    for r in range(len(trace)):
        if flags[r] & far.BAD_POSE:
            continue
        rows = trace[r, :iters[r] + 1]
        worst = max(worst, np.abs(rows[:, 3] - np.cos(rows[:, 2])).max(), np.abs(rows[:, 4] - np.sin(rows[:, 2])).max())
    print("trace (cos, sin) error", worst)
    assert worst <= 1e-15


def check_align(f, d2, xy, sco, cpo, poses, grid_kw, pose=None, pose_out=None):
    """One align compared with the reference; returns the device's results.  pose: what the device is
    given (default: the host array poses)."""
    f.align(xy, sco, cpo, pose=poses if pose is None else pose, pose_out=pose_out)
    res = f.align_results()
    q = {k: getattr(f.a, k) for k in ALIGN_KEYS}
    want = far.align_batch(d2, xy, cpo[sco], poses, res["trace"], f.grid.origin_host, grid_kw, **q)
    assert np.array_equal(res["flags"], want["flags"]), (q, res["flags"], want["flags"])
    assert np.array_equal(res["iters"], want["iters"]), (q, res["iters"], want["iters"])
    assert np.array_equal(res["n_used"], want["n_used"]), (q, res["n_used"], want["n_used"])
    assert np.array_equal(res["normal"], want["normal"]), (q, res["normal"], want["normal"])
    assert same_bits(res["trace"], want["trace"]), (q, np.argwhere(res["trace"] != want["trace"])[:5])
    assert same_bits(res["pose_out"], want["pose_out"]), (q, res["pose_out"], want["pose_out"])
    assert_trace_rot(res["trace"], res["iters"], res["flags"])
    H, g = f.align_information()
    Hw, gw = far.information(want["normal"])
    assert np.array_equal(H, Hw) and np.array_equal(g, gw)
    return res


@pytest.mark.parametrize("W", [16, 24, 80])
def test_small_and_nasty(ctx, W):
    """The map spans -4000 .. 4000 mm whatever W is (at W 24 the cell, 1000 / 3, and its inverse are no
    binary fractions).  The nasty poses and points of the ray caster's tests, then the ends of n_iter
    and of trunc, no damping, and no floor on the points."""
    cell = 8000.0 / W
    kw = dict(grid_w=W, cell=cell, max_range=3000.0)
    rng = np.random.default_rng(470 + W)
    arrays = [nasty_points(rng, n, W, cell, 3000.0) for n in NASTY_SIZES]
    arrays[0][:4] = [[1e-310, 0.0], [0.0, -4e-320], [3000.0, 0.0], [1e300, -1e300]]  # denormals; at and beyond max_range
    L0 = random_map(rng, 7, W, occupied=0.06)
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=max(4, W // 4), min_points=3), **kw)
    xy, sco, cpo = csr(arrays)
    res = check_align(f, d2, xy, sco, cpo, NASTY_POSES, kw)
    assert res["flags"][1] == far.BAD_POSE and same_bits(res["pose_out"][1], NASTY_POSES[1]) and not res["trace"][1].any()
    assert res["flags"][4] & far.FEW and res["n_used"][4].tolist() == [0, 0, 0]  # the robot with no points
    assert res["iters"].max() >= 2 and (res["n_used"][[0, 3], 0] > 10).all()
    assert np.all(res["n_used"][:, 1] <= res["n_used"][:, 2])
    for over in (dict(n_iter=1), dict(n_iter=2), dict(n_iter=32, eps_t=0.0, eps_r=0.0), dict(trunc=0.0), dict(trunc=255.0),
                 dict(damp_t=0.0, damp_r=0.0), dict(min_points=0, min_permille=0, max_shift=np.inf, max_turn=np.inf),
                 dict(max_shift=0.0), dict(min_permille=1000)):
        old = {k: getattr(f.a, k) for k in over}
        for k, v in over.items():
            setattr(f.a, k, v)
        res = check_align(f, d2, xy, sco, cpo, NASTY_POSES, kw)
        if "n_iter" in over:
            assert res["trace"].shape[1] == over["n_iter"] + 1 and res["iters"].max() == over["n_iter"]
        if over.get("min_points") == 0:  # the robot with no points: zero sums, a zero step, CONVERGED
            assert res["flags"][4] == far.CONVERGED and res["iters"][4] == 1
        for k, v in old.items():
            setattr(f.a, k, v)
    assert np.array_equal(f.results()["d2"], d2) and g.logodds.download().tobytes() == L0.tobytes()  # both are read only


def test_long_revolution(ctx):
    """4096 points on one robot: 64 rounds of the lane-strided loop add up."""
    kw = dict(grid_w=64, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(481)
    L0 = random_map(rng, 1, 64, occupied=0.05)
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=12, trunc=12.0), **kw)
    xy, sco, cpo = csr([nasty_points(rng, 4096, 64, 100.0, 3000.0)])
    res = check_align(f, d2, xy, sco, cpo, np.array([[310.0, -420.0, 0.7]]), kw)
    assert res["n_used"][0, 0] > 1500 and res["iters"][0] >= 2 and not res["flags"][0] & far.BAD_POSE


def test_many_robots_one_map_and_empty_fields(ctx):
    """130 robots are 33 workgroups, the last with two waves at work.  Robot 77 alone has a map: the
    others' fields are EMPTY, without a gradient, so their step is exactly zero and CONVERGED comes
    with the first; robot 77 moves."""
    kw = dict(grid_w=32, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(482)
    R = 130
    L0 = np.zeros((R, 32, 32), np.int16)
    L0[77] = random_map(rng, 1, 32, occupied=0.08)[0]
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=10, trunc=10.0, min_points=0, min_permille=0), **kw)
    assert (f.results()["flags"] == dr.EMPTY).sum() == R - 1
    poses = np.stack([rng.uniform(-800, 800, R), rng.uniform(-800, 800, R), rng.uniform(-3, 3, R)], -1)
    xy, sco, cpo = csr([nasty_points(rng, 65, 32, 100.0, 3000.0) for _ in range(R)])
    res = check_align(f, d2, xy, sco, cpo, poses, kw)
    others = np.arange(R) != 77
    assert np.all(res["flags"][others] == far.CONVERGED) and np.all(res["iters"][others] == 1)
    assert same_bits(res["pose_out"][others], poses[others]) and not res["normal"][others, :9].any()
    assert res["iters"][77] >= 2 and res["normal"][77, :6].any() and not same_bits(res["trace"][77, 1, :3], poses[77])


def test_singular_without_damping(ctx):
    """One source cell, d_max 3: far from it the field is saturated and J is zero; without damping the
    first pivot is zero.  Around it the system has its three pivots and the iteration runs."""
    kw = dict(grid_w=32, cell=100.0, max_range=3000.0)
    L0 = np.full((2, 32, 32), -100, np.int16)
    L0[:, 20, 20] = 200
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=3, trunc=3.0, damp_t=0.0, damp_r=0.0, min_points=3), **kw)
    rng = np.random.default_rng(483)
    near = np.array([450.0, 450.0]) + rng.uniform(-220.0, 220.0, (40, 2))  # around the source, seen from (0, 0)
    xy, sco, cpo = csr([rng.uniform(-900.0, -100.0, (40, 2)), near])
    res = check_align(f, d2, xy, sco, cpo, np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), kw)
    assert res["flags"][0] & far.SINGULAR and res["iters"][0] == 0 and not res["trace"][0, 1:].any()
    assert not res["flags"][1] & far.SINGULAR and res["iters"][1] >= 1


def test_aliasing_device_pose_and_stale_rows(ctx):
    """pose_out on the pose it was read from gives what a separate pose_out gives; a device pose is read
    in place; a second call into the same outputs leaves no row of the first behind."""
    kw = dict(grid_w=64, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(484)
    R = 9
    L0 = random_map(rng, R, 64, occupied=0.05)
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=12, trunc=12.0, eps_t=0.0, eps_r=0.0, min_points=3), **kw)
    poses = np.stack([rng.uniform(-2000, 2000, R), rng.uniform(-2000, 2000, R), rng.uniform(-3, 3, R)], -1)
    poses[3] = [np.nan, 1.0, 2.0]
    xy, sco, cpo = csr([nasty_points(rng, 200, 64, 100.0, 3000.0) for _ in range(R)])
    first = check_align(f, d2, xy, sco, cpo, poses, kw)  # eps 0: all eleven rows of trace are written
    assert first["iters"].max() == 10 and first["trace"][first["iters"] == 10][:, 10].any()
    f.a.eps_t, f.a.eps_r = 5.0, 1.0  # any step converges: rows 2 .. 10 must be zeros again
    second = check_align(f, d2, xy, sco, cpo, poses, kw)
    assert second["iters"].max() == 1 and not second["trace"][:, 2:].any()
    f.a.eps_t, f.a.eps_r = 0.01, 1e-4
    want = check_align(f, d2, xy, sco, cpo, poses, kw)
    dpose = ctx.to_device(poses)
    got = check_align(f, d2, xy, sco, cpo, poses, kw, pose=dpose)  # read in place
    assert same_bits(dpose.download(), poses)
    alias = check_align(f, d2, xy, sco, cpo, poses, kw, pose=dpose, pose_out=dpose)
    for k in want:
        assert same_bits(want[k], got[k]) and same_bits(want[k], alias[k]), k
    assert same_bits(dpose.download(), want["pose_out"]) and not same_bits(want["pose_out"], poses)


def test_refusals(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    g = OccupancyGrid(ctx, 2, grid_w=32, cell=100.0, max_range=3000.0)
    for bad in (dict(trunc=-1.0), dict(trunc=256.0), dict(n_iter=0), dict(n_iter=33), dict(damp_t=-1.0), dict(eps_r=np.nan),
                dict(min_permille=1001), dict(max_turn=-1.0)):
        with pytest.raises(ValueError):
            DistanceField(g, **bad)
    f = DistanceField(g)
    xy, sco, cpo = csr([np.ones((5, 2)), np.ones((5, 2))])
    with pytest.raises(ValueError):
        f.align(xy, sco, cpo, pose=np.zeros((2, 3)))  # no field yet
    with pytest.raises(ValueError):
        f.align_results()
    f.step()
    with pytest.raises(ValueError):
        f.align(xy, sco, cpo, pose=np.zeros((2, 3)), pose_out=np.zeros((2, 3)))  # pose_out lives on the device
    with pytest.raises(ValueError):
        f.align(xy, sco, cpo, pose=np.zeros((2, 3)), pose_out=ctx.empty((1, 3), np.float64))
    L = _lib.load()
    b = _lib.FieldAlignBatch()  # n_robots 0 does nothing, whatever the pointers
    assert L.lslam_field_align(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a)) == 0
    b.n_robots = 2
    b.xy = f.d2.addr
    assert L.lslam_field_align(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a)) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    f.align(xy, sco, cpo, pose=np.zeros((2, 3)))  # and the context still works
    assert f.align_results()["flags"].tolist() == [far.FEW | far.WEAK] * 2  # the field is EMPTY at d_max 64: beyond trunc


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The five-revolution device chain of test_gpu_fieldscore.test_end_to_end: the field of the device's
    own grid, the alignment from the filter's pose read in place on the device (exact against the
    reference fed that grid's field), the room's cap of test_fieldalign_ref from the displaced true
    poses, and after a recentre that moves the robots the alignment in the moved grid with the moved
    origin, exact again."""
    from lidar_slam_amd.mapping import FIELDALIGN_REJECTED, DistanceField, OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    field = DistanceField(grid, **ROOM_DIST)
    for step, rev in enumerate(revs):
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm, sync=False)
    rev = revs[4]
    sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
    field.step(sync=False)
    x = lm.x.download()
    d2 = dr.field_batch(grid.results()["logodds"], **ROOM_DIST)[0]
    assert np.array_equal(field.results()["d2"], d2)
    res = check_align(field, d2, rev["xy"], sco, cpo, x, ROOM_KW, pose=lm)
    assert not (res["flags"] & FIELDALIGN_REJECTED).any() and same_bits(lm.x.download(), x)
    err = res["pose_out"] - poses[4]
    print("from the filter's poses: error mm", np.hypot(err[:, 0], err[:, 1]).round(2), "mrad", (1e3 * err[:, 2]).round(3),
          "iters", res["iters"])

    def align_fn(guess):
        field.align(rev["xy"], sco, cpo, pose=guess)
        return field.align_results()
    assert_room_align(align_fn, poses[4])

    guess = poses[4] + np.array([-30.0, 30.0, 0.03])
    before = check_align(field, d2, rev["xy"], sco, cpo, guess, ROOM_KW)
    grid.recentre(pose=lm, margin=128, quantum=8, sync=False)
    field.step(sync=False)
    assert grid.recentre_results()["shift"].any(1).sum() >= R // 2
    d2m = dr.field_batch(grid.results()["logodds"], **ROOM_DIST)[0]
    after = check_align(field, d2m, rev["xy"], sco, cpo, guess, ROOM_KW)
    assert not same_bits(grid.origin_host, np.tile(ROOM_ORIGIN, (R, 1))) and not np.array_equal(d2m, d2)
    # (walls further than half a map from a robot have scrolled off: the descent need not end where it did)
    print("after the recentre: moved by mm", np.abs(after["pose_out"] - before["pose_out"])[:, :2].max(1).round(2),
          "flags", after["flags"])
