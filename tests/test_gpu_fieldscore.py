"""GPU parity of the field read under a revolution (lslam_field_score, DistanceField.score) against its
NumPy definition, tests/fieldscore_ref.py, over fields that the device made (lslam_grid_distance, held
to tests/dist_ref.py in the same breath).

Every double operation of the definition is rounded on its own and the rest is integers, so stats,
clear2 and flags are compared EXACTLY, the reference being fed the (cos, sin) that the device wrote to
rot; rot itself is held to 1e-15 as in test_gpu_occgrid.assert_rot.  The end-to-end case repeats the
physical caps of tests/test_fieldscore_ref.py on the device's own grid and follows a recentred grid.
"""
import numpy as np
import pytest

import dist_ref as dr
import fieldscore_ref as fr
from oracle import cpu as orc
from test_fieldscore_ref import ROOM_DIST, ROOM_SCORE, assert_room_caps
from test_gpu_occgrid import assert_rot, csr, nasty_points
from test_gpu_raycast import NASTY_POSES, NASTY_SIZES, random_map
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, room_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def field_of(ctx, L0, origin=None, dist_kw=None, **grid_kw):
    """The device's field of uploaded grids, held to the reference: (OccupancyGrid, DistanceField, d2)."""
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    dist_kw = dist_kw or {}
    g = OccupancyGrid(ctx, len(L0), origin=origin, **grid_kw)
    g.upload(L0)
    f = DistanceField(g, **dist_kw)
    f.d2.upload(np.full(L0.shape, 0xFFFF, np.uint16))
    f.step()
    res = f.results()
    want = dr.field_batch(L0, **{k: v for k, v in dist_kw.items() if k in dr.DEFAULTS})
    assert np.array_equal(res["d2"], want[0]) and np.array_equal(res["n_src"], want[1]) and np.array_equal(res["flags"], want[2])
    return g, f, res["d2"]


def check_score(f, d2, xy, sco, cpo, poses, grid_kw):
    """One score compared with the reference; returns the device's results."""
    f.score(xy, sco, cpo, pose=poses)
    res = f.score_results()
    q = dict(trunc2=int(f.q.trunc2), near2=int(f.q.near2), off2=int(f.q.off2))
    stats, clear2, flags = fr.score_batch(d2, xy, cpo[sco], poses, res["rot"], f.grid.origin_host, grid_kw, **q)
    assert np.array_equal(res["flags"], flags), (res["flags"], flags)
    assert np.array_equal(res["stats"], stats), (q, res["stats"], stats)
    assert np.array_equal(res["clear2"], clear2), (res["clear2"], clear2)
    assert_rot(res["rot"], poses)
    cell = float(f.grid.p.cell)
    assert np.array_equal(f.clearance_mm(), fr.clearance_mm(clear2, cell))
    assert np.array_equal(f.near_share(), fr.near_share(stats)) and np.array_equal(f.mean_d2(), fr.mean_d2(stats))
    return res


def test_small_and_nasty(ctx):
    kw = dict(grid_w=80, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(47)
    arrays = [nasty_points(rng, n, 80, 100.0, 3000.0) for n in NASTY_SIZES]
    arrays[0][:4] = [[1e-310, 0.0], [0.0, -4e-320], [3000.0, 0.0], [1e300, -1e300]]  # denormals; at and beyond max_range
    L0 = random_map(rng, 7, 80)
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=20, trunc2=100, near2=2), **kw)
    assert f.q.off2 == 400
    xy, sco, cpo = csr(arrays)
    res = check_score(f, d2, xy, sco, cpo, NASTY_POSES, kw)
    assert res["flags"].tolist() == [0, fr.BAD_POSE, 0, 0, 0, 0, 0]
    assert not res["stats"][1].any() and res["clear2"][1] == 0 and not res["stats"][4].any()
    assert res["clear2"][2] == 400 and res["stats"][2, 3] > 0   # the robot off the map: off2; some of its points too
    assert res["stats"][6, 3] > 0 and res["stats"][0, 1] > 30   # in the corner cell: points leave the map
    assert np.all(res["stats"][:, 2] <= res["stats"][:, 1]) and np.all(res["stats"][:, 0] <= 100 * res["stats"][:, 1])
    # the ends of the ranges
    for trunc2, near2, off2 in ((1, 0, 0), (65025, 65025, 65025), (1, 65025, 65025), (65025, 0, 1), (625, 4, 0)):
        f.q.trunc2, f.q.near2, f.q.off2 = trunc2, near2, off2
        res = check_score(f, d2, xy, sco, cpo, NASTY_POSES, kw)
        if near2 == 65025:
            assert np.array_equal(res["stats"][:, 2], res["stats"][:, 1])
        if trunc2 == 1 and off2 == 0:  # a point on a source or off the map adds nothing, any other one
            assert np.all(res["stats"][:, 0] <= res["stats"][:, 1] - res["stats"][:, 3])
    # a device pose read in place gives the same
    dpose = ctx.to_device(NASTY_POSES)
    want = f.score_results()
    f.score(xy, sco, cpo, pose=dpose)
    got = f.score_results()
    for k in want:
        assert np.array_equal(want[k], got[k], equal_nan=True), k
    assert np.array_equal(f.results()["d2"], d2) and g.logodds.download().tobytes() == L0.tobytes()  # both are read only


def test_long_revolution_and_many_robots(ctx):
    """4096 points on one robot are cut into slices that add up; 64 robots of 65 points get one slice each
    or a few: the sums do not depend on the cut."""
    kw = dict(grid_w=64, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(48)
    for sizes in ([4096], [65] * 64):
        R = len(sizes)
        L0 = random_map(rng, R, 64, occupied=0.05)
        poses = np.stack([rng.uniform(-2500, 2500, R), rng.uniform(-2500, 2500, R), rng.uniform(-3, 3, R)], -1)
        g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=12), **kw)
        xy, sco, cpo = csr([nasty_points(rng, n, 64, 100.0, 3000.0) for n in sizes])
        res = check_score(f, d2, xy, sco, cpo, poses, kw)
        assert res["stats"][:, 1].sum() > 0.5 * sum(sizes) and not res["flags"].any()


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The five-revolution device chain of test_gpu_occgrid.test_end_to_end (the pose read on the device
    from lm.x) with the field behind it: the field and the score are exact against the references fed
    the device's grid and rot; the physical caps of test_fieldscore_ref hold on the device's own grid;
    and after a recentre that moves the robots, step() plus score() are exact against the references
    fed the moved grid and origin."""
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    field = DistanceField(grid, trunc2=ROOM_SCORE["trunc2"], near2=ROOM_SCORE["near2"], **ROOM_DIST)
    assert field.q.off2 == ROOM_SCORE["off2"]
    for step, rev in enumerate(revs):
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm, sync=False)
    rev = revs[4]
    sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
    field.d2.upload(np.full((R, 256, 256), 0xFFFF, np.uint16))
    field.step(sync=False)
    field.score(rev["xy"], sco, cpo, pose=lm)
    x = lm.x.download()
    L = grid.results()["logodds"]

    def exact(L, what):
        d2, n_src, flags = dr.field_batch(L, **ROOM_DIST)
        fres = field.results()
        assert np.array_equal(fres["d2"], d2) and np.array_equal(fres["n_src"], n_src) and np.array_equal(fres["flags"], flags), what
        res = field.score_results()
        stats, clear2, sflags = fr.score_batch(d2, rev["xy"], cpo[sco], x, res["rot"], grid.origin_host, ROOM_KW, **ROOM_SCORE)
        assert np.array_equal(res["stats"], stats) and np.array_equal(res["clear2"], clear2), (what, res["stats"], stats)
        assert np.array_equal(res["flags"], sflags) and not sflags.any(), what
        assert_rot(res["rot"], x)
        return res

    res = exact(L, "the chain's grid")
    print("n_src", field.results()["n_src"], "near share at the filter's poses", field.near_share().round(3),
          "clearance mm", field.clearance_mm().round(1))

    def score_fn(p):
        field.score(rev["xy"], sco, cpo, pose=p)
        r = field.score_results()
        assert not r["flags"].any()
        return r["stats"], r["clear2"]
    assert_room_caps(score_fn, poses[4])

    # the rolling grid: margin = W / 2 recentres every robot; the room's robots are not in the middle
    grid.recentre(pose=lm, margin=128, quantum=8, sync=False)
    field.step(sync=False)
    field.score(rev["xy"], sco, cpo, pose=lm)
    rr = grid.recentre_results()
    assert rr["shift"].any(1).sum() >= R // 2 and not np.array_equal(grid.origin_host, np.tile(ROOM_ORIGIN, (R, 1)))
    L2 = grid.results()["logodds"]
    assert not np.array_equal(L2, L)
    res2 = exact(L2, "the recentred grid")
    # what stayed on the map reads the same: the robot's clearance, unless it was saturated by the map's edge
    same = res["clear2"] < 128 * 128
    assert same.any() and np.array_equal(res2["clear2"][same], res["clear2"][same])
