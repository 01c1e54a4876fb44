"""GPU parity of the occupancy-grid update (lslam_grid_update, lidar_slam_amd/mapping.py) against its
NumPy definition, tests/occgrid_ref.py.

The grid is integers and every double operation of the definition is rounded on its own, so
logodds, n_used and flags are compared EXACTLY, the reference being fed the (cos, sin) that the
device wrote to rot: those bits are the definition's input.  rot itself is held to
|rot - (np.cos, np.sin)| <= 1e-15: OCML documents 2 ulp for cos and sin, glibc stays below 1 ulp,
both at magnitude <= 1 (ulp 1.1e-16), which gives 3.3e-16; 1e-15 leaves a factor of 3.
"""
import numpy as np
import pytest

import occgrid_ref as ogr
from lidar_slam_amd import synth
from oracle import cpu as orc
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, assert_room, room_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def csr(arrays):
    """One chunk per robot: (xy, scan_chunk_off, chunk_pt_off)."""
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)
    xy = np.concatenate([np.asarray(a, np.float64).reshape(-1, 2) for a in arrays] + [np.zeros((0, 2))])
    return xy, np.arange(len(arrays) + 1, dtype=np.int32), off


def assert_rot(rot, poses):
    th = np.asarray(poses, np.float64).reshape(-1, 3)[:, 2]
    ok = np.isfinite(th)
    want = np.stack([np.cos(th[ok]), np.sin(th[ok])], -1)
    err = np.abs(rot[ok] - want)
    print("rot error", err.max(initial=0.0))
    assert err.max(initial=0.0) <= 1e-15


def check(ctx, arrays, poses, origin=None, L0=None, calls=1, **kw):
    """`calls` updates of a fresh grid (preloaded with L0) from the same revolutions, each compared
    with the reference; returns the last device results and the OccupancyGrid."""
    from lidar_slam_amd.mapping import OccupancyGrid
    R = len(arrays)
    xy, sco, cpo = csr(arrays)
    g = OccupancyGrid(ctx, R, origin=origin, **kw)
    L = np.zeros((R, g.W, g.W), np.int16)
    if L0 is not None:
        g.upload(L0)
        L = np.array(L0, np.int16)
    res = None
    for call in range(calls):
        g.step(xy, sco, cpo, pose=poses)
        res = g.results()
        Lr, n_used, flags = ogr.update_batch(L, xy, cpo, poses, res["rot"], g.origin_host, **kw)
        assert np.array_equal(res["flags"], flags), (call, res["flags"], flags)
        assert np.array_equal(res["n_used"], n_used), (call, res["n_used"], n_used)
        bad = np.argwhere(res["logodds"] != Lr)
        assert bad.size == 0, (call, len(bad), bad[:5])
        assert_rot(res["rot"], poses)
        L = Lr
    return res, g


def nasty_points(rng, n, grid_w, cell, max_range):
    """Robot-frame points: anywhere within 1.2 max_range; exactly on cell boundaries of the world
    frame for a pose with theta = 0 on a cell corner (negative ones included); in the robot's own
    cell; NaN, inf and (0, 0)."""
    kinds = rng.integers(0, 5, n)
    r = rng.uniform(0.0, 1.2 * max_range, n)
    a = rng.uniform(-np.pi, np.pi, n)
    xy = np.stack([r * np.cos(a), r * np.sin(a)], -1)
    onb = rng.integers(-grid_w // 3, grid_w // 3, (n, 2)) * cell
    own = rng.uniform(0.0, 0.4 * cell, (n, 2))
    xy = np.where((kinds == 1)[:, None], onb, xy)
    xy = np.where((kinds == 2)[:, None], own, xy)
    junk = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0], [-np.inf, np.nan], [100.0, np.nan]])
    sel = kinds == 3
    xy[sel] = junk[rng.integers(0, len(junk), int(sel.sum()))]
    return xy


def test_small_and_nasty(ctx):
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(41)
    sizes = [37, 64, 65, 200, 0, 3, 50]
    poses = np.array([[200.0, -300.0, 0.0],      # on a cell corner, theta = 0: points on cell boundaries
                      [np.nan, 10.0, 0.2],       # BAD_POSE
                      [-5200.0, 350.0, 0.3],     # the robot outside the grid (it spans -4000 .. 4000)
                      [1234.5, -777.25, 1e6],    # a huge heading
                      [10.0, 20.0, -2.0],
                      [-1500.0, 3900.0, 3.0],
                      [3950.0, 3950.0, 0.8]])    # in the corner cell: most rays leave the grid
    arrays = [nasty_points(rng, n, 80, 100.0, 3000.0) for n in sizes]
    arrays[5] = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0]])
    L0 = rng.integers(-200, 351, (7, 80, 80)).astype(np.int16)
    far = rng.integers(0, 80, (40, 3))
    L0[far[:, 0] % 7, far[:, 1], far[:, 2]] = rng.choice([-32768, -5000, -201, 351, 9000, 32767], 40)
    res, _ = check(ctx, arrays, poses, L0=L0, calls=2, **kw)
    assert res["flags"][1] == ogr.BAD_POSE and res["n_used"][1].tolist() == [0, 0]
    assert res["logodds"][1].tobytes() == L0[1].tobytes()
    assert res["flags"][2] == ogr.CLIPPED and res["flags"][6] == ogr.CLIPPED
    assert res["n_used"][4].tolist() == [0, 0] and res["n_used"][5].tolist() == [0, 0]
    assert res["logodds"][5].tobytes() == L0[5].tobytes() and res["flags"][5] == 0
    assert res["n_used"][:, 1].sum() > 0 and res["n_used"][3, 0] > 100
    assert np.any(res["logodds"][2] != L0[2])  # the outside robot's rays enter the grid


def seam_rays(W, T):
    """Robots on and beside every tile seam and in the corners; per robot, rays to every such cell
    (axis-parallel along the seams, corner to corner), exact diagonals, and slopes 1/2 and 2, whose
    rounding (2 i |d| + n) div 2n lands on a boundary at every other step."""
    c = sorted({0, W - 1} | {s for k in (1, 2) for s in (k * T - 1, k * T, k * T + 1) if 0 < s < W})
    starts = [(x, y) for x in c for y in c]
    ends_all = []
    for (X0, Y0) in starts:
        ends = [(x, y) for x in c for y in c]
        for m in (1, 2, 3, T // 2, T - 1, T, T + 1, W - 1):
            for sx in (1, -1):
                for sy in (1, -1):
                    ends += [(X0 + sx * m, Y0 + sy * m), (X0 + sx * 2 * m, Y0 + sy * m), (X0 + sx * m, Y0 + sy * 2 * m)]
        ends_all.append(np.array([e for e in ends if e != (X0, Y0)], np.float64))
    return np.array(starts, np.float64), ends_all


@pytest.mark.parametrize("W", ["16", "T+2", "2T", "2T+2"])
def test_tile_seams(ctx, W):
    from lidar_slam_amd.mapping import TILE as T
    W = {"16": 16, "T+2": T + 2, "2T": 2 * T, "2T+2": 2 * T + 2}[W]
    cell = 10.0
    kw = dict(grid_w=W, cell=cell, max_range=4096 * cell)
    starts, ends = seam_rays(W, T)
    # theta = 0, the robot on its cell's centre, the returns on theirs: every sum below is exact
    poses = np.concatenate([(starts + 0.5) * cell, np.zeros((len(starts), 1))], 1)
    arrays = [(e - s) * cell for s, e in zip(starts, ends)]
    res, _ = check(ctx, arrays, poses, origin=(0.0, 0.0), **kw)
    assert np.all(res["rot"] == [1.0, 0.0])
    L = res["logodds"]
    for i in (0, len(starts) - 1):  # the corner robots' own cells: passed by every ray
        x, y = starts[i].astype(int)
        assert L[i, y, x] == -200


def test_saturation_and_long_revolutions(ctx):
    pose1 = synth.scan_polar(510)[2]
    long_rev = synth.polar_to_xy_ref(*synth.scan_polar_at(pose1, 77, n_beams=4096))
    same = np.tile([[1000.0, 250.0]], (300, 1))
    poses = np.array([[1500.0, 1500.0, 0.4], pose1])
    res, _ = check(ctx, [same, long_rev], poses, origin=ROOM_ORIGIN, calls=3, **ROOM_KW)
    assert res["n_used"][0].tolist() == [300, 0] and res["n_used"][1].sum() == 4096
    for r in range(2):
        assert res["logodds"][r].min() == -200 and res["logodds"][r].max() == 350


def test_defaults(ctx):
    from lidar_slam_amd.mapping import OccupancyGrid
    robots = [300, 301, 302]
    poses = synth.trajectory(robots, 1, u=(146.0, 174.0))
    g = OccupancyGrid.centred_on(ctx, poses[0])
    assert g.W == 512 and np.array_equal(g.origin_host, poses[0][:, :2] - 5120.0)
    L = np.zeros((3, 512, 512), np.int16)
    for k in range(2):
        rev = synth.revolutions_at(poses[k], k, robots)
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        g.step(rev["xy"], sco, cpo, pose=poses[k])
        res = g.results()
        L, n_used, flags = ogr.update_batch(L, rev["xy"], cpo[sco], poses[k], res["rot"], g.origin_host)
        assert np.array_equal(res["logodds"], L) and np.array_equal(res["n_used"], n_used)
        assert np.array_equal(res["flags"], flags) and not flags.any()
        assert_rot(res["rot"], poses[k])
    assert (L < 0).sum() > 3 * 20000 and (L >= 170).sum() > 3 * 100
    p = g.probability()
    assert p.shape == L.shape and np.all(p[L == 0] == 0.5)
    assert np.allclose(p[L == -200], 1 - 1 / (1 + np.exp(-2.0))) and np.allclose(p[L == 170], 1 - 1 / (1 + np.exp(1.7)))


def test_inputs(ctx):
    """Host arrays, a device array read in place, and a staged MapInput give the same grids; clear
    zeroes them; two asynchronous steps equal two synchronous ones."""
    from lidar_slam_amd.mapping import OccupancyGrid
    from lidar_slam_amd.slam import LandmarkMap
    robots = [310, 311]
    poses = synth.trajectory(robots, 1, u=(146.0, 174.0))
    revs = [synth.revolutions_at(poses[k], k, robots) for k in range(2)]
    kw = dict(grid_w=256)
    host, dev, staged, asyn = (OccupancyGrid(ctx, 2, origin=ROOM_ORIGIN, **kw) for _ in range(4))
    lm = LandmarkMap(ctx, 2)
    dpose = ctx.empty((2, 3), np.float64)
    for k, rev in enumerate(revs):
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        host.step(rev["xy"], sco, cpo, pose=poses[k])
        dxy = ctx.to_device(rev["xy"])
        dpose.upload(poses[k])
        dev.step(dxy, sco, cpo, pose=dpose)
        staged.step(lm.upload(rev["xy"], sco, cpo), pose=poses[k])
        asyn.step(rev["xy"], sco, cpo, pose=poses[k], sync=False)
    ctx.sync()
    a = host.results()
    assert a["logodds"].any()
    for other in (dev, staged, asyn):
        b = other.results()
        for key in ("logodds", "rot", "n_used", "flags"):
            assert np.array_equal(a[key], b[key]), key
    host.clear()
    assert not host.results()["logodds"].any()
    with pytest.raises(ValueError):
        OccupancyGrid(ctx, 2, grid_w=4096)
    with pytest.raises(ValueError):
        host.step(revs[0]["xy"], revs[0]["scan_chunk_off"], revs[0]["chunk_pt_off"])  # no pose


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The chain of test_gpu_scanmatch.test_end_to_end_without_odometry with the grid behind it:
    revolutions -> odometry -> map and filter -> grid, the pose read on the device from lm.x.  Every
    step is exact against the reference given the downloaded lm.x; the finished grids meet the room
    caps of test_occgrid_ref (measured on an MI355X, worst robot: 99.86 % of the occupied cells
    within 80 mm of a wall, 99.87 % of the interior free, no interior cell occupied; pose errors
    at most 7.3 mm and 0.0024 rad)."""
    from lidar_slam_amd.mapping import OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    L = np.zeros((R, 256, 256), np.int16)
    for step, rev in enumerate(revs):
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm)
        x = lm.x.download()
        res = grid.results()
        L, n_used, flags = ogr.update_batch(L, rev["xy"], cpo[sco], x, res["rot"], grid.origin_host, **ROOM_KW)
        assert np.array_equal(res["logodds"], L), step
        assert np.array_equal(res["n_used"], n_used) and np.array_equal(res["flags"], flags), step
        assert_rot(res["rot"], x)
        dpos = np.hypot(x[:, 0] - poses[step][:, 0], x[:, 1] - poses[step][:, 1])
        print("step", step, "pose error", dpos.max(), np.abs(x[:, 2] - poses[step][:, 2]).max())
    assert_room(res["logodds"], "device, filter poses")
