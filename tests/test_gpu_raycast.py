"""GPU parity of grid ray casting (lslam_grid_raycast, lidar_slam_amd.mapping.GridRayCaster) against its
NumPy definition, tests/raycast_ref.py.

Every double operation of the definition is rounded on its own and the rest is integers, so cls, stop,
counts and flags are compared EXACTLY, the reference being fed the (cos, sin) that the device wrote
to rot: those bits are the definition's input.  rot itself is held to 1e-15 as in
test_gpu_occgrid.assert_rot.

The kernel has two forms.  The HBM form (the cells read from HBM as the walk goes) ships.  The LDS
form (the window's codes loaded into LDS first) is selected by LSLAM_RAYCAST_FORM=lds, read at every
call, while min(2 Rc + 1, grid_w), Rc = floor(max_range / cell), is at most 558 cells (its rows of
ceil((win + 2) / 16) | 1 dwords, win + 2 of them, fit 80 KiB); beyond that the HBM form runs whatever
the variable says.  With 2 Rc + 1 odd the largest LDS window is 557 (Rc = 278) and the first that does
not fit 559 (Rc = 279).  Every case here runs under both settings and both must be exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

import raycast_ref as rcr
from test_gpu_occgrid import assert_rot, csr, nasty_points
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, room_run
from test_raycast_ref import (assert_control, assert_far_pose, assert_room_caps, far_off)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def lds_bytes(win):
    return 32 + (((win + 2) * (((win + 2 + 15) >> 4) | 1) * 4 + 15) & ~15)


def random_map(rng, R, W, occupied=0.03, unknown=0.03):
    """Mostly free, so that rays run; some occupied cells; some never seen (0) or with little evidence
    either way (values around the thresholds); values outside any clamp range."""
    L = rng.integers(-200, -40, (R, W, W)).astype(np.int16)
    u = rng.random((R, W, W))
    L = np.where(u < occupied, rng.integers(85, 351, L.shape), L)
    weak = np.where(rng.random(L.shape) < 0.6, 0, rng.integers(-3, 4, L.shape))
    L = np.where((u >= occupied) & (u < occupied + unknown), weak, L).astype(np.int16)
    far = rng.integers(0, W, (60, 2))
    L[rng.integers(0, R, 60), far[:, 0], far[:, 1]] = rng.choice([-32768, -5000, -201, 351, 9000, 32767, 1, -1], 60)
    return L


FORMS = ("hbm", "lds")


class kernel_form:
    """LSLAM_RAYCAST_FORM for the calls inside (the library reads it at every call)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.get("LSLAM_RAYCAST_FORM")
        os.environ["LSLAM_RAYCAST_FORM"] = self.form

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("LSLAM_RAYCAST_FORM", None)
        else:
            os.environ["LSLAM_RAYCAST_FORM"] = self.old


def check(ctx, arrays, poses, L0, origin=None, rc_kw=None, **grid_kw):
    """One cast of the revolutions through the uploaded grids in each form, compared with the reference;
    returns the last device results (with the raw cls byte) and the GridRayCaster."""
    from lidar_slam_amd.mapping import GridRayCaster, OccupancyGrid
    rc_kw = rc_kw or {}
    R = len(arrays)
    xy, sco, cpo = csr(arrays)
    g = OccupancyGrid(ctx, R, origin=origin, **grid_kw)
    g.upload(L0)
    rc = GridRayCaster(g, **rc_kw)
    ref = None
    for form in FORMS:
        with kernel_form(form):
            rc.step(xy, sco, cpo, pose=poses)
        res = rc.results()
        res["raw"] = res["cls"] | (res["kind"] << 4)
        if ref is None:  # (both forms write the same rot: the same instructions)
            ref = rcr.cast_batch(L0, xy, cpo, poses, res["rot"], g.origin_host, **grid_kw, **rc_kw), res["rot"]
        (cls, stop, counts, flags), rot = ref
        assert np.array_equal(res["rot"], rot, equal_nan=True), form
        assert np.array_equal(res["flags"], flags), (form, res["flags"], flags)
        bad = np.flatnonzero(res["raw"] != cls)
        assert bad.size == 0, (form, len(bad), bad[:5], res["raw"][bad[:5]], cls[bad[:5]], xy[bad[:5]])
        bad = np.flatnonzero((res["stop"] != stop).any(1))
        assert bad.size == 0, (form, len(bad), bad[:5], res["stop"][bad[:5]], stop[bad[:5]])
        assert np.array_equal(res["counts"], counts), (form, res["counts"], counts)
        assert_rot(res["rot"], poses)
    assert not np.any(np.asarray(g.results()["logodds"]) != L0)  # the grid is read only
    return res, rc


NASTY_POSES = np.array([[200.0, -300.0, 0.0],      # on a cell corner, theta = 0: points on cell boundaries
                        [np.nan, 10.0, 0.2],       # BAD_POSE
                        [-5200.0, 350.0, 0.3],     # the robot off the map (it spans -4000 .. 4000)
                        [1234.5, -777.25, 1e6],    # a huge heading
                        [10.0, 20.0, -2.0],
                        [-1500.0, 3900.0, 3.0],
                        [3950.0, 3950.0, 0.8]])    # in the corner cell: most rays leave the map
NASTY_SIZES = [63, 64, 65, 257, 0, 1, 3]


@pytest.mark.parametrize("tol", [0, 3])
def test_small_and_nasty(ctx, tol):
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(43)
    arrays = [nasty_points(rng, n, 80, 100.0, 3000.0) for n in NASTY_SIZES]
    arrays[0][:4] = [[1e-310, 0.0], [0.0, -4e-320], [3000.0, 0.0], [1e300, -1e300]]  # denormal: INVALID; at and beyond max_range
    L0 = random_map(rng, 7, 80)
    res, rc = check(ctx, arrays, NASTY_POSES, L0, rc_kw=dict(tol=tol), **kw)
    off = np.concatenate([[0], np.cumsum(NASTY_SIZES)])
    assert res["flags"].tolist() == [0, rcr.BAD_POSE, 0, 0, 0, 0, 0]
    assert not res["raw"][off[1]:off[2]].any() and not res["counts"][1].any() and not res["stop"][off[1]:off[2]].any()
    r2 = slice(off[2], off[3])  # off the map: every valid beam stops at step 0, unknown
    valid = res["cls"][r2] != rcr.INVALID
    assert valid.sum() > 30 and np.all(res["kind"][r2][valid] == rcr.UNKNOWN) and not res["stop"][r2].any()
    assert res["cls"][0] == rcr.INVALID and res["cls"][1] == rcr.INVALID and res["counts"][0, 5] >= 1
    assert res["counts"][4].tolist() == [0] * 8
    for k in (rcr.MATCH, rcr.NOVEL, rcr.THROUGH, rcr.UNMAPPED):  # every class and kind occurs
        assert (res["cls"] == k).any(), k
    for k in (rcr.NONE, rcr.UNKNOWN, rcr.OCC):
        assert (res["kind"][res["cls"] != rcr.INVALID] == k).any(), k
    # the Python helpers against the reference's
    assert np.array_equal(rc.expected_range(), rcr.expected_range(res["raw"], res["stop"], 100.0))
    assert np.array_equal(rc.novel_mask(), res["cls"] == rcr.NOVEL)
    assert np.array_equal(rc.inconsistency(), rcr.inconsistency(res["counts"]))


def test_width_52(ctx):
    """grid_w is not a multiple of 8: the lane-per-cell window load."""
    kw = dict(grid_w=52, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(44)
    poses = np.array([[0.0, 0.0, 0.5], [-2550.0, 2549.0, -1.0], [2599.0, -10.0, 2.5]])
    arrays = [nasty_points(rng, n, 52, 100.0, 3000.0) for n in (130, 64, 77)]
    res, _ = check(ctx, arrays, poses, random_map(rng, 3, 52), **kw)
    assert (res["kind"] == rcr.OCC).sum() > 20


def test_small_window_in_a_big_map(ctx):
    """Rc = 10 in a 512-cell map: the window is clipped at every edge and corner."""
    kw = dict(grid_w=512, cell=20.0, max_range=205.0)
    rng = np.random.default_rng(45)
    e = 5120.0
    poses = np.array([[0.0, 0.0, 0.1], [-e + 5.0, 0.0, 1.0], [e - 5.0, 30.0, 2.0], [7.0, -e + 1.0, 3.0], [-9.0, e - 1.0, 4.0],
                      [-e + 70.0, -e + 130.0, 5.0], [e - 1.0, e - 1.0, 6.0], [e - 150.0, -e + 45.0, 0.0]])
    arrays = [nasty_points(rng, 150, 24, 20.0, 205.0) for _ in poses]
    res, _ = check(ctx, arrays, poses, random_map(rng, len(poses), 512, occupied=0.01, unknown=0.01), **kw)
    assert (res["kind"] == rcr.NONE).sum() > 100 and (res["kind"] == rcr.UNKNOWN).sum() > 50


def sparse_map(rng, R, W, n_occ, n_unk):
    L = np.full((R, W, W), -100, np.int16)
    for n, lo, hi in ((n_occ, 1, 351), (n_unk, 0, 1)):  # (0: never seen)
        c = rng.integers(0, W, (n, 2))
        L[rng.integers(0, R, n), c[:, 0], c[:, 1]] = rng.integers(lo, hi, n)
    return L


def test_hbm_form(ctx):
    """grid_w 2048 at 5 mm with max_range 8000: Rc = 1600, the window is the whole map and its codes
    do not fit LDS: the HBM form whatever is asked for.  A sparse map, so that rays run for hundreds of
    steps."""
    kw = dict(grid_w=2048, cell=5.0, max_range=8000.0)
    assert lds_bytes(2048) > 80 * 1024
    rng = np.random.default_rng(46)
    poses = np.array([[100.0, -50.0, 0.7]])
    arrays = [nasty_points(rng, 300, 2048, 5.0, 8000.0)]
    res, _ = check(ctx, arrays, poses, sparse_map(rng, 1, 2048, 6000, 3000), **kw)
    walked = res["stop"][res["cls"] != rcr.INVALID, 2]
    assert walked.max() > 600 and (res["kind"] == rcr.OCC).sum() > 10 and (res["kind"] == rcr.UNKNOWN).sum() > 10


@pytest.mark.parametrize("max_range,win,form", [(2785.0, 557, "lds"), (2795.0, 559, "hbm")])
def test_largest_lds_window(ctx, max_range, win, form):
    """The largest window whose codes fit LDS and the first that does not (module docstring), robots in
    the middle of a 1024-cell map (the whole window) and at its edge."""
    kw = dict(grid_w=1024, cell=10.0, max_range=max_range)
    assert min(2 * int(np.floor(max_range * (1.0 / 10.0))) + 1, 1024) == win
    assert (lds_bytes(win) <= 80 * 1024) == (form == "lds") and lds_bytes(557) <= 80 * 1024 < lds_bytes(559)
    rng = np.random.default_rng(47)
    poses = np.array([[3.0, -4.0, 0.3], [5115.0, -5100.0, 2.0]])
    arrays = [nasty_points(rng, 200, 1024, 10.0, max_range) for _ in poses]
    res, _ = check(ctx, arrays, poses, sparse_map(rng, 2, 1024, 3000, 1500), **kw)
    # (a ray that nothing stops leaves the circle after 197 steps, on the diagonal, to Rc + 1, along an axis)
    assert res["stop"][:200, 2].max() >= 197 and (res["kind"][:200] == rcr.NONE).sum() > 20


def test_slices(ctx):
    """A robot's points are split over workgroups by the batch's size: one robot of 4096 points, 64 robots
    of 65, and a robot of those alone give the same bytes."""
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(48)
    check(ctx, [nasty_points(rng, 4096, 80, 100.0, 3000.0)], np.array([[10.0, 20.0, -2.0]]), random_map(rng, 1, 80), **kw)
    R = 64
    poses = np.concatenate([rng.uniform(-3900.0, 3900.0, (R, 2)), rng.uniform(-3.0, 3.0, (R, 1))], 1)
    arrays = [nasty_points(rng, 65, 80, 100.0, 3000.0) for _ in range(R)]
    L0 = random_map(rng, R, 80)
    res, _ = check(ctx, arrays, poses, L0, **kw)
    for r in (0, 17, 63):
        alone, _ = check(ctx, [arrays[r]], poses[r:r + 1], L0[r:r + 1], **kw)
        s = slice(65 * r, 65 * r + 65)
        assert alone["raw"].tobytes() == res["raw"][s].tobytes() and alone["stop"].tobytes() == res["stop"][s].tobytes()
        assert alone["counts"].tobytes() == res["counts"][r:r + 1].tobytes()


def test_edge_calls(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import GridRayCaster
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(49)
    arrays = [nasty_points(rng, n, 80, 100.0, 3000.0) for n in (100, 30)]
    poses = np.array([[10.0, 20.0, -2.0], [-1500.0, 3900.0, 3.0]])
    res, rc = check(ctx, arrays, poses, random_map(rng, 2, 80), **kw)
    xy, sco, cpo = csr(arrays)
    # stop = NULL
    rc.step(xy, sco, cpo, pose=poses, want_stop=False)
    r2 = rc.results()
    assert r2["stop"] is None and np.array_equal(r2["cls"], res["cls"]) and np.array_equal(r2["counts"], res["counts"])
    with pytest.raises(ValueError):
        rc.expected_range()
    # n_robots = 0: nothing is touched, nothing is needed
    L = _lib.load()
    b = _lib.RaycastBatch()
    assert L.lslam_grid_raycast(ctx.handle, C.byref(b), C.byref(rc.grid.p), C.byref(rc.p)) == _lib.LSLAM_OK
    ctx.sync()
    assert np.array_equal(rc.results()["counts"], res["counts"])
    # the timing id brackets the whole call
    ctx.set_timing(True, kernels=[_lib.K_RAYCAST, _lib.K_GRID])
    ctx.timing_reset()
    try:
        rc.step(xy, sco, cpo, pose=poses)
        assert ctx.timing(_lib.K_RAYCAST)[1] == 1 and ctx.timing(_lib.K_GRID)[1] == 0
        rc.step(xy, sco, cpo, pose=poses)
        ms, n = ctx.timing(_lib.K_RAYCAST)
        assert n == 2 and ms > 0.0
    finally:
        ctx.set_timing(False)
    with pytest.raises(ValueError):
        GridRayCaster(rc.grid, tol=65)
    with pytest.raises(ValueError):
        GridRayCaster(rc.grid, free_max=85)
    with pytest.raises(ValueError):
        rc.step(xy, sco, cpo)  # no pose


@pytest.fixture
def loose():
    from oracle import cpu as orc
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The chain of test_gpu_occgrid.test_end_to_end, then the fifth revolution cast through the
    device's own grids at the filter's poses, read on the device from lm.x: exact against the reference
    given the downloaded grid and lm.x; the room caps of test_raycast_ref hold; the shortened sector
    comes back as the NOVEL mask; lm.x moved by (700, -600) mm and 0.5 rad is at least five times as
    inconsistent."""
    from lidar_slam_amd.mapping import GridRayCaster, OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    for rev in revs:
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm)
    rev = revs[4]
    sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
    Ld, x = grid.results()["logodds"], lm.x.download()
    rc = GridRayCaster(grid)
    dpose = ctx.empty((R, 3), np.float64)

    def cast_fn(xy, p):
        """p None: the filter's poses, read on the device from lm.x."""
        for form in FORMS[::-1]:  # (the shipped form last: its results stay in rc)
            with kernel_form(form):
                if p is None:
                    rc.step(xy, sco, cpo, pose=lm)
                else:
                    dpose.upload(p)
                    rc.step(xy, sco, cpo, pose=dpose)
            res = rc.results()
            raw = res["cls"] | (res["kind"] << 4)
            q = x if p is None else p
            cls, stop, counts, flags = rcr.cast_batch(Ld, xy, cpo[sco], q, res["rot"], grid.origin_host, **ROOM_KW)
            assert np.array_equal(raw, cls) and np.array_equal(res["stop"], stop), form
            assert np.array_equal(res["counts"], counts) and not res["flags"].any() and not flags.any(), form
            assert_rot(res["rot"], q)
        return raw, res["counts"]

    # (the filter's poses stand in both places: they ARE the moved poses, within 10 mm of the truth)
    assert_room_caps(cast_fn, rev, None, None)
    cls, idx = assert_control(cast_fn, rev, None, 0.6, rcr.NOVEL)
    mask = rc.novel_mask()  # of the control's cast, the last one
    assert mask[idx].mean() >= 0.9 and np.array_equal(mask, (cls & 15) == rcr.NOVEL)
    assert_far_pose(cast_fn, rev, None, far_off(x, 700.0, -600.0, 0.5))
