"""GPU parity of the grid recentre (lslam_grid_recentre, OccupancyGrid.recentre) against its NumPy
definition, tests/recentre_ref.py.

The shift is integers, the new origin two rounded operations and the cells 16-bit patterns that are
moved, so logodds, the origin's bits, shift and flags are compared EXACTLY.

The kernel shifts a grid in place, band of rows after band of rows (lslam_recentre_plan.h), on one of
two paths per robot: 16-byte groups where grid_w and sx are multiples of 8, a lane per cell otherwise.
With margin = W / 2 and quantum = 1 the pose chooses any shift, so one batch holds every class of
shift: none, smaller than a group, a group, around a band's height B = recentre_band_rows(W), around
the map's width, far beyond it, with both signs on both axes.  The grids hold a permutation of all
65,536 int16 values (W = 256) or random ones, so a source cell that was overwritten before it was read
cannot go unnoticed."""
import ctypes as C

import numpy as np
import pytest

import mapmatch_ref as mmr
import occgrid_ref as ogr
import raycast_ref as rcr
import recentre_ref as rr
from test_gpu_occgrid import csr
from test_recentre_ref import (MOVED, BAD_POSE, CLEARED, WALK_MOVE, WALKS, WALK_STEPS, assert_walk_match, bits,
                               walk_origin, walk_poses, walk_revolutions)

pytestmark = pytest.mark.gpu

CELL = 20.0


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def run(ctx, L0, pose, origin, margin, quantum, **grid_kw):
    """One recentre of freshly uploaded grids, compared with the reference; returns (the device's
    results, the reference's, the OccupancyGrid)."""
    from lidar_slam_amd.mapping import OccupancyGrid
    R = len(pose)
    g = OccupancyGrid(ctx, R, origin=origin, **grid_kw)
    g.upload(L0)
    g.recentre(pose, margin=margin, quantum=quantum)
    res = g.recentre_results()
    res["logodds"] = g.logodds.download()
    given = {k: v for k, v in (("margin", margin), ("quantum", quantum)) if v is not None}  # None: the defaults
    ref = rr.recentre_batch(L0, pose, origin, **given, **grid_kw)
    assert_same(res, ref)
    assert np.array_equal(bits(g.origin.download()), bits(ref[1]))
    return res, ref, g


def assert_same(res, ref, what=""):
    L, origin, shift, flags = ref
    assert np.array_equal(res["shift"], shift), (what, np.argwhere(res["shift"] != shift)[:5])
    assert np.array_equal(res["flags"], flags), (what, res["flags"], flags)
    bad = np.argwhere(bits(res["origin"]) != bits(origin))
    assert bad.size == 0, (what, bad[:5], res["origin"][bad[:5, 0]], origin[bad[:5, 0]])
    bad = np.argwhere(res["logodds"] != L)
    assert bad.size == 0, (what, len(bad), bad[:5], shift[np.unique(bad[:, 0])[:8]].tolist())


def shift_classes(W):
    """(sx, sy) of one batch: every magnitude on each axis with both signs of the other axis, the
    partner cycling through the magnitudes; the pure cases; (0, 0)."""
    from lidar_slam_amd.mapping import recentre_band_rows
    B = recentre_band_rows(W)
    mags = sorted({1, 7, 8, 9, B - 1, B, B + 1, W - 1, W, W + 1, 5000} - {0})
    out = [(0, 0)]
    for i, m in enumerate(mags):
        u = mags[(3 * i + 1) % len(mags)]
        for v in (m, -m):
            out += [(v, u), (v, -u), (u, v), (-u, v), (v, 0), (0, v)]
    # a column shift on the 16-byte groups with every kind of row shift, and the reverse
    out += [(8, 1), (-8, -7), (16, B - 1), (-24, -(B + 1)), (8, B), (-8, -B), (1, 8), (-7, -16), (9, B), (-9, -B)]
    return np.array(sorted(set(out)), np.int64)


def batch_for(rng, W, shifts, permutation=False):
    R = len(shifts)
    origin = CELL * rng.integers(-50, 50, (R, 2)).astype(np.float64)
    pose = np.stack([np.append(rr.pose_for_shift(origin[r], CELL, W, *shifts[r]), rng.uniform(-3, 3)) for r in range(R)])
    if permutation:
        assert W == 256
        L0 = np.stack([rng.permutation(65536).astype(np.uint16).view(np.int16).reshape(W, W) for _ in range(R)])
    else:
        L0 = rng.integers(-32768, 32768, (R, W, W)).astype(np.int16)
    return L0, pose, origin


@pytest.mark.parametrize("W", [256, 64, 52])
def test_every_shift_class(ctx, W):
    rng = np.random.default_rng(W)
    shifts = shift_classes(W)
    L0, pose, origin = batch_for(rng, W, shifts, permutation=W == 256)
    res, ref, g = run(ctx, L0, pose, origin, W // 2, 1, grid_w=W, cell=CELL)
    assert np.array_equal(res["shift"], shifts)  # the pose chose the shift
    far = np.abs(shifts).max(1) >= W
    assert np.array_equal(res["flags"], np.where(shifts.any(1), MOVED | np.where(far, CLEARED, 0), 0))
    groups = shifts.any(1) & (shifts[:, 0] % 8 == 0) & (W % 8 == 0)
    print("W %d: %d robots, %d on 16-byte groups, %d a lane per cell, %d of them cleared"
          % (W, len(shifts), groups.sum(), (shifts.any(1) & ~groups).sum(), far.sum()))
    # a second recentre with the same poses continues from the moved origin: the robot is in the middle now
    g.recentre(pose, margin=W // 2, quantum=1)
    again = g.recentre_results()
    assert not again["shift"].any() and not again["flags"].any()
    assert np.array_equal(g.logodds.download(), ref[0]) and np.array_equal(bits(again["origin"]), bits(ref[1]))


def test_largest_map(ctx):
    """grid_w 2048: 4 KiB rows, bands of 8 rows, on both paths."""
    W = 2048
    rng = np.random.default_rng(11)
    shifts = np.array([(8, 9), (-16, -7), (3, 9)], np.int64)
    L0, pose, origin = batch_for(rng, W, shifts)
    res, ref, g = run(ctx, L0, pose, origin, W // 2, 1, grid_w=W, cell=CELL)
    assert np.array_equal(res["shift"], shifts)


def test_quantum_and_margin_at_the_defaults(ctx):
    """Quantum 8, margin 128, grid_w 512: robots on both sides of each margin edge, and 65 that all move."""
    W, m = 512, 128
    rng = np.random.default_rng(5)
    edge = [(m - 1, 300), (m, 300), (W - m - 1, 200), (W - m, 200), (300, m - 1), (300, m), (200, W - m - 1), (200, W - m)]
    cells = []
    while len(cells) < 65:
        c = rng.integers(-300, W + 300, 2)
        if not (m <= c[0] < W - m and m <= c[1] < W - m):
            cells.append(tuple(int(v) for v in c))
    cells = np.array(cells + edge, np.float64)
    R = len(cells)
    origin = CELL * rng.integers(-50, 50, (R, 2)).astype(np.float64)
    pose = np.concatenate([origin + (cells + rng.uniform(0.05, 0.95, (R, 2))) * CELL, rng.uniform(-3, 3, (R, 1))], 1)
    L0 = rng.integers(-32768, 32768, (R, W, W)).astype(np.int16)
    res, ref, g = run(ctx, L0, pose, origin, None, None, grid_w=W, cell=CELL)
    assert np.all(res["flags"][:65] & MOVED) and np.all(res["shift"] % 8 == 0)
    assert (res["flags"][65:] != 0).tolist() == [True, False, False, True] * 2
    left = cells - res["shift"] - W // 2
    assert np.all((left[res["flags"] != 0] >= -4) & (left[res["flags"] != 0] < 4))  # back within quantum / 2 of the middle


def test_what_must_be_left_alone(ctx):
    W = 64
    rng = np.random.default_rng(9)
    shifts = np.array([(0, 0), (8, -8), (0, 0), (-3, 5), (0, 0), (0, 0), (0, 0), (16, 0), (0, 0)], np.int64)
    L0, pose, origin = batch_for(rng, W, shifts)
    L0[:, :2, :8] = np.array([-32768, 32767, -201, 351, -5000, 9000, 1, -1], np.int16)  # outside any clamp range
    pose[0, :2] = origin[0] + (np.array([W // 2 + 3, W // 2 - 4]) + 0.5) * CELL  # triggered (margin W/2), rounds to zero at quantum 8
    pose[2, 0] = np.nan
    origin[4, 1] = np.inf
    pose[5, 0] = origin[5, 0] + (2.0 ** 20 + 0.5) * CELL
    pose[6, 1] = origin[6, 1] - (2.0 ** 20 - 0.5) * CELL
    res, ref, g = run(ctx, L0, pose, origin, W // 2, 8, grid_w=W, cell=CELL)
    assert res["flags"].tolist() == [0, MOVED, BAD_POSE, MOVED, BAD_POSE, BAD_POSE, BAD_POSE, MOVED, 0]
    assert res["shift"].tolist() == [[0, 0], [8, -8], [0, 0], [0, 8], [0, 0], [0, 0], [0, 0], [16, 0], [0, 0]]
    still = [0, 2, 4, 5, 6, 8]
    assert np.array_equal(res["logodds"][still], L0[still]) and np.array_equal(bits(res["origin"][still]), bits(origin[still]))
    assert np.array_equal(res["logodds"][1, 8:, :W - 8], L0[1, :W - 8, 8:])  # the patterns moved as they were
    # the same at quantum 1, where robot 3 takes the lane-per-cell path beside the others
    res, ref, g = run(ctx, L0, pose, origin, W // 2, 1, grid_w=W, cell=CELL)
    assert res["shift"][[0, 3]].tolist() == [[3, -4], [-3, 5]]
    assert np.array_equal(res["logodds"][[2, 4, 5, 6]], L0[[2, 4, 5, 6]])


def test_timing_slot_empty_batch_and_arguments(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import OccupancyGrid
    W = 64
    rng = np.random.default_rng(2)
    L0, pose, origin = batch_for(rng, W, np.array([(8, 0), (0, 0)], np.int64))
    g = OccupancyGrid(ctx, 2, origin=origin, grid_w=W, cell=CELL)
    with pytest.raises(ValueError):
        g.recentre_results()
    before = g.origin_host
    assert before is g.origin_host  # no recentre yet: the array given at construction, no copy
    g.upload(L0)
    ctx.set_timing(True, kernels=[_lib.K_RECENTRE, _lib.K_GRID])
    ctx.timing_reset()
    try:
        g.recentre(pose, margin=W // 2, quantum=8)
        assert ctx.timing(_lib.K_RECENTRE)[1] == 1 and ctx.timing(_lib.K_GRID)[1] == 0
        g.recentre(pose, margin=W // 2, quantum=8)
        ms, n = ctx.timing(_lib.K_RECENTRE)
        assert n == 2 and ms > 0.0
    finally:
        ctx.set_timing(False)
    assert g.recentre_results()["shift"].tolist() == [[0, 0], [0, 0]]  # the second call found the robots centred
    assert np.array_equal(g.origin_host, origin + [[8 * CELL, 0.0], [0.0, 0.0]]) and np.array_equal(before, origin)
    # n_robots = 0: nothing is touched, nothing is needed
    L = _lib.load()
    b = _lib.RecentreBatch()
    q = _lib.recentre_params(margin=W // 2)
    assert L.lslam_grid_recentre(ctx.handle, C.byref(b), C.byref(g.p), C.byref(q)) == _lib.LSLAM_OK
    # (its parameters are still checked: the default margin of 128 cells does not fit a map of 64)
    assert L.lslam_grid_recentre(ctx.handle, C.byref(b), C.byref(g.p), C.byref(_lib.recentre_params())) == _lib.LSLAM_ERR_ARG
    ctx.sync()
    assert np.array_equal(g.logodds.download(), np.stack([rr.shifted(L0[0], 8, 0), L0[1]]))
    for kw in (dict(margin=W // 2 + 1), dict(quantum=0), dict(quantum=65), dict(margin=-1)):
        with pytest.raises(ValueError):
            g.recentre(pose, **kw)
    with pytest.raises(ValueError):
        g.recentre(None)
    with pytest.raises(ValueError):
        g.recentre(pose[:1])


@pytest.mark.parametrize("device_pose", [False, True], ids=["host_pose", "device_pose"])
def test_walk_1_on_the_device(ctx, device_pose):
    """recentre then step per revolution, every step held to the reference chain (fed the rot the
    device wrote); then the readers on the rolled grid: they follow the moved origin."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import GridRayCaster, OccupancyGrid
    w = WALKS[1]
    gkw, R = w["grid"], 3
    poses, revs = walk_poses(1), walk_revolutions(1)
    grid = OccupancyGrid(ctx, R, origin=walk_origin(1), **gkw)
    L = np.zeros((R, gkw["grid_w"], gkw["grid_w"]), np.int16)
    origin = walk_origin(1)
    dpose = ctx.empty((R, 3), np.float64)
    moved_at = []
    for k in range(WALK_STEPS):
        xy, sco, cpo = csr(revs[k])
        if device_pose:
            dpose.upload(poses[k])
        p = dpose if device_pose else poses[k]
        grid.recentre(p, margin=w["margin"], quantum=w["quantum"], sync=False)
        grid.step(xy, sco, cpo, pose=p)
        rc = grid.recentre_results()
        res = grid.results()
        L, origin, shift, rflags = rr.recentre_batch(L, poses[k], origin, margin=w["margin"], quantum=w["quantum"], **gkw)
        ups = [ogr.update(L[r], revs[k][r], poses[k, r], res["rot"][r], origin[r], **gkw) for r in range(R)]
        L = np.stack([u[0] for u in ups])
        assert np.array_equal(rc["shift"], shift) and np.array_equal(rc["flags"], rflags), k
        assert np.array_equal(bits(rc["origin"]), bits(origin)), k
        assert np.array_equal(res["logodds"], L), (k, np.argwhere(res["logodds"] != L)[:5])
        assert not res["flags"].any(), k  # never CLIPPED
        if shift[0].any():
            moved_at.append((k, shift[0].tolist()))
    assert moved_at == [(3, [32, 0]), (6, [32, 0]), (9, [24, 0]), (12, [32, 0])]
    assert np.array_equal(bits(grid.origin_host), bits(grid.origin.download())) and np.array_equal(grid.origin_host, origin)

    xy, sco, cpo = csr(revs[-1])
    guess = poses[-1] + WALK_MOVE
    loc = GridLocalizer(ctx, R, win_w=256)
    loc.step(xy, sco, cpo, grid=grid, pose=guess)
    got = loc.results()
    ref = mmr.match_batch(L, origin, guess, xy, cpo, rot0=got["rot0"], rot=loc.rot_host, grid_w=256, win_w=256, cell=20.0)
    for key in ("delta", "best", "n_valid", "flags"):
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(bits(got["pose"]), bits(ref["pose_out"]))
    assert_walk_match([dict(pose_out=got["pose"][r], flags=int(got["flags"][r])) for r in range(R)])

    caster = GridRayCaster(grid)
    caster.step(xy, sco, cpo, pose=poses[-1])
    c = caster.results()
    cls, stop, counts, flags = rcr.cast_batch(L, xy, cpo, poses[-1], c["rot"], origin, **gkw)
    assert np.array_equal(c["cls"] | (c["kind"] << 4), cls) and np.array_equal(c["stop"], stop)
    assert np.array_equal(c["counts"], counts) and np.array_equal(c["flags"], flags) and not flags.any()
    assert counts[:, rcr.MATCH].min() > 300  # the beams do land on the rolled map's walls
