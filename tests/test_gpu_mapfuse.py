"""GPU parity of the match fusion (lslam_map_fuse, GridLocalizer.fuse) against its NumPy definition,
tests/mapfuse_ref.py.

The moments are integers and every double operation of the definition is rounded on its own, so
pose_out, P_out, z, Rm, nis, moments, delta, best, n_valid, flags and the whole score volume are
compared EXACTLY (the FP64 outputs as bit patterns), the reference being fed the (cos, sin) that the
device wrote to rot0, as in test_gpu_mapmatch.  That the division and the int64 -> double conversion
of the kernel are single roundings is what these comparisons show.
"""
import numpy as np
import pytest

import mapfuse_ref as mfr
from lidar_slam_amd import _lib
from oracle import cpu as orc
from test_gpu_occgrid import assert_rot, csr
from test_mapfuse_ref import CORR, HAND, P_ROOM, corridor, nan_payload
from test_mapmatch_ref import KW, at_cell, cells, grid_with, pose_bits, room_setup
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, assert_room, room_run

pytestmark = pytest.mark.gpu

INT_KEYS = ("moments", "delta", "best", "n_valid", "flags", "scores")
BIT_KEYS = (("pose", "pose_out"), ("P", "P_out"), ("z", "z"), ("Rm", "Rm"), ("nis", "nis"))
GKW = dict(grid_w=KW["grid_w"], cell=KW["cell"])
MKW = {k: KW[k] for k in ("win_w", "smear", "k_trans", "k_theta")}


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def assert_equal(res, ref, what=""):
    for key in INT_KEYS:
        if key == "scores" and key not in res:
            continue
        got = res[key] if key != "delta" else pose_bits(res[key])
        want = ref[key] if key != "delta" else pose_bits(ref[key])
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, key, len(bad), bad[:5], res[key][tuple(bad[0])], ref[key][tuple(bad[0])])
    for key, rkey in BIT_KEYS:
        bad = np.argwhere(pose_bits(res[key]) != pose_bits(ref[rkey]))
        assert bad.size == 0, (what, key, len(bad), bad[:5], res[key][tuple(bad[0])], ref[rkey][tuple(bad[0])])


def run(ctx, L, origin, poses, P, arrays, gkw, mkw, alias=False, want_scores=True):
    """One fuse on fresh objects: (device results, the localizer, the grid, (x, P) on the device)."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    R = len(arrays)
    xy, sco, cpo = csr(arrays)
    grid = OccupancyGrid(ctx, R, origin=origin, **gkw)
    grid.upload(L)
    loc = GridLocalizer(ctx, R, **mkw)
    dx = ctx.to_device(np.ascontiguousarray(poses, np.float64).reshape(R, 3))
    dP = ctx.to_device(np.ascontiguousarray(P, np.float64).reshape(R, 9))
    loc.fuse(xy, sco, cpo, grid=grid, x=dx, P=dP, write_back=alias, want_scores=want_scores)
    return loc.results(), loc, grid, (dx, dP)


def check(ctx, L, origin, poses, P, arrays, gkw, mkw, what=""):
    """A fuse into separate buffers, compared with the reference; returns (device results, reference)."""
    R = len(arrays)
    res, loc, grid, (dx, dP) = run(ctx, L, origin, poses, P, arrays, gkw, mkw)
    xy, _, cpo = csr(arrays)
    ref = mfr.fuse_batch(L, grid.origin_host, poses, P, xy, cpo, rot0=res["rot0"], rot=loc.rot_host, **gkw, **mkw)
    assert_equal(res, ref, what)
    assert_rot(res["rot0"], poses)
    # the inputs are only read
    assert np.array_equal(grid.logodds.download(), L)
    assert np.array_equal(pose_bits(dx.download()), pose_bits(np.asarray(poses, np.float64).reshape(R, 3)))
    assert np.array_equal(pose_bits(dP.download()), pose_bits(np.asarray(P, np.float64).reshape(R, 9)))
    return res, ref


def prior(sx, st, R):
    d = np.array([sx, sx, st])
    return np.tile(CORR * d[:, None] * d[None, :], (R, 1, 1))


def random_case(seed, R, W=40, ww=32, cell=50.0, npts=60, reach=None):
    """R robots somewhere on a sparse random map of W cells, scans of about npts points."""
    rng = np.random.default_rng(seed)
    origin = np.tile([-300.0, 450.0], (R, 1))
    X0, Y0 = rng.integers(W // 2 - 4, W // 2 + 4, R), rng.integers(W // 2 - 4, W // 2 + 4, R)
    f = rng.uniform(0.01, 0.99, (R, 2))
    poses = np.stack([origin[:, 0] + (X0 + f[:, 0]) * cell, origin[:, 1] + (Y0 + f[:, 1]) * cell,
                      rng.uniform(-np.pi, np.pi, R)], -1)
    L = np.where(rng.random((R, W, W)) < 0.12, 120, -41).astype(np.int16)
    reach = (ww // 2) * cell if reach is None else reach
    arrays = [rng.uniform(-reach, reach, (npts - r % 5, 2)) for r in range(R)]
    return L, origin, poses, arrays


@pytest.mark.parametrize("smear,kt,kth", [(0, 0, 0), (0, 1, 1), (2, 4, 1), (2, 10, 20), (2, 15, 31)])
def test_volume_shapes(ctx, smear, kt, kth):
    """One candidate (a single lane), 27 (a partly filled wave), 243, the defaults' 18,081 (no multiple
    of 256) and the largest volume, 60,543 candidates."""
    R = 5
    L, origin, poses, arrays = random_case(100 * smear + 10 * kt + kth, R)
    mkw = dict(win_w=32, smear=smear, k_trans=kt, k_theta=kth, theta_step=0.01, min_permille=20)
    P = prior((kt + 1) * 50.0, (kth + 1) * 0.01, R)
    res, _ = check(ctx, L, origin, poses, P, arrays, dict(grid_w=40, cell=50.0), mkw)
    assert res["scores"].shape == (R, 2 * kth + 1, 2 * kt + 1, 2 * kt + 1) and res["scores"].any()
    updated = (res["flags"] & ~mfr.EDGE) == 0
    print("flags", res["flags"].tolist(), "nis", res["nis"].tolist(), "W", res["moments"][:, 0].tolist())
    assert updated.any() and np.all(np.diagonal(res["P"][updated], axis1=1, axis2=2) < np.diagonal(P[updated], axis1=1, axis2=2))


def corner_case():
    """Five points that only the rotation k = 2 and the shift (+4, +4), the far corner of the volume, lay
    onto the occupied cells; with cut_permille 0 every candidate that scores weighs in, all of them at
    negative offsets."""
    step = 0.2
    T = [(-2, -1), (-1, 2), (1, -3), (0, 1), (-3, -3)]
    L = grid_with(32, [(16 + i, 16 + j) for i, j in T])
    U = np.array([(i - 4, j - 4) for i, j in T], np.float64) * 100.0  # cell centres, from the robot on its cell's centre
    c, s = np.cos(-step), np.sin(-step)
    pts = np.stack([c * U[:, 0] - s * U[:, 1], s * U[:, 0] + c * U[:, 1]], -1)
    return L, at_cell(16, 16), pts, dict(MKW, theta_step=step, cut_permille=0)


def test_winner_in_a_corner(ctx):
    L, pose, pts, mkw = corner_case()
    P = np.diag([500.0 ** 2, 500.0 ** 2, 0.3 ** 2])
    res, _ = check(ctx, L[None], np.zeros((1, 2)), pose[None], P[None], [pts], GKW, mkw)
    assert res["best"][0].tolist() == [2, 8, 8, 5] and res["flags"][0] == mfr.EDGE
    assert np.all(res["moments"][0, 1:4] < 0) and res["moments"][0, 0] > 5
    assert res["pose"][0, 0] > pose[0] + 100.0  # updated towards the corner


def test_corridor(ctx):
    L, pose, pts = corridor()
    res, _ = check(ctx, L[None], np.zeros((1, 2)), pose[None], np.diag([1e4, 1e4, 1e-2])[None], [pts], GKW, MKW)
    assert res["moments"][0].tolist() == [54, 0, 0, 0, 360, 0, 0, 0, 0, 36]
    assert res["Rm"][0, 1, 1] == (100.0 * 100.0) / 12.0 and res["Rm"][0, 0, 0] >= 10.0 * res["Rm"][0, 1, 1]


def test_largest_moments(ctx):
    """A fully occupied map under a 4096-point scan at the largest search window: every candidate ties at
    3 x points, the centre wins and all 60,543 weigh in: the largest moments a test-sized input reaches."""
    rng = np.random.default_rng(41)
    W, cell = 64, 50.0
    L = np.full((1, W, W), 200, np.int16)
    pose = np.array([[(W // 2 + 0.5) * cell, (W // 2 + 0.5) * cell, 0.4]])
    pts = rng.uniform(-15.0 * cell, 15.0 * cell, (4096, 2))
    pts[np.hypot(pts[:, 0], pts[:, 1]) > 15.0 * cell] *= 0.5  # (a rotation keeps every point 15 cells inside the window)
    mkw = dict(win_w=64, smear=2, k_trans=15, k_theta=31, theta_step=0.005)
    P = np.diag([400.0 ** 2, 400.0 ** 2, 0.1 ** 2])[None]
    res, _ = check(ctx, L, np.zeros((1, 2)), pose, P, [pts], dict(grid_w=W, cell=cell), mkw)
    assert res["best"][0].tolist() == [31, 15, 15, 3 * 4096] and res["flags"][0] == 0
    assert np.all(res["scores"] == 3 * 4096)
    w = 3 * 4096 - (3 * 4096 * 900) // 1000
    assert res["moments"][0, 0] == w * 63 * 31 * 31 and res["moments"][0, 9] == w * 31 * 31 * 2 * sum(c * c for c in range(32))
    assert not res["moments"][0, [1, 2, 3, 5, 6, 8]].any()


@pytest.mark.parametrize("R", [1, 300])
def test_batch_sizes(ctx, R):
    L, origin, poses, arrays = random_case(500 + R, R, W=32, ww=16, cell=100.0, npts=24)
    mkw = dict(MKW, smear=2, min_permille=100)
    res, _ = check(ctx, L, origin, poses, prior(400.0, 0.02, R), arrays, dict(grid_w=32, cell=100.0), mkw)
    assert np.count_nonzero((res["flags"] & ~mfr.EDGE) == 0) > R // 2


def states_case():
    """Six robots, each ending in another state: accepted, EDGE and accepted, EMPTY, WEAK, BAD_POSE,
    OUTLIER.  The robots that must stay untouched carry NaNs with a payload in P (and BAD_POSE in x)."""
    nan = nan_payload()
    full = np.full((32, 32), 300, np.int16)
    big = np.diag([1e4, 1e4, 1e-2])
    Ls = [HAND["L"], grid_with(32, [(23, 16)]), full, grid_with(32, [(18, 17), (12, 12)]), full,
          grid_with(32, [(19, 17), (20, 17), (19, 19)])]
    poses = np.array([HAND["pose"], at_cell(16, 16), at_cell(60, 8, 0.1), at_cell(16, 16), [nan, 1650.0, 0.1], at_cell(16, 16)])
    arrays = [HAND["xy"], cells((11, 0)), cells((1, 1)), cells((2, 1), (5, 5), (-5, 5), (5, -5), (-6, -6)), cells((1, 1)),
              HAND["xy"]]
    P = np.array([big, np.diag([1e6, 1e4, 1e-2]), big, big, big, np.diag([1.0, 1.0, 1e-6])])
    P[2, 0, 1] = P[4, 2, 2] = nan
    want = [0, mfr.EDGE, mfr.EMPTY, mfr.WEAK, mfr.BAD_POSE, mfr.OUTLIER]
    return np.array(Ls), np.zeros((6, 2)), poses, P, arrays, want


def test_six_states_and_bad_cov(ctx):
    L, origin, poses, P, arrays, want = states_case()
    res, _ = check(ctx, L, origin, poses, P, arrays, GKW, MKW, "states")
    assert res["flags"].tolist() == want
    keep = [2, 3, 4, 5]
    assert np.array_equal(pose_bits(res["pose"][keep]), pose_bits(poses[keep]))
    assert np.array_equal(pose_bits(res["P"][keep]), pose_bits(P[keep]))
    assert np.all(np.any(res["pose"][:2] != poses[:2], axis=1))
    assert np.all(np.diagonal(res["P"][:2], axis1=1, axis2=2) < np.diagonal(P[:2], axis1=1, axis2=2))
    assert not res["moments"][[2, 4]].any() and not res["Rm"][[2, 4]].any() and not res["nis"][[2, 4]].any()
    assert np.array_equal(pose_bits(res["z"][[2, 4]]), pose_bits(poses[[2, 4]]))
    assert res["nis"][5] > 16.27 and res["moments"][3, 0] > 0 and res["Rm"][3, 0, 0] > 0
    # a second batch: the accepted robot between two whose covariance is refused
    Pb = np.array([P[0], P[0], P[0]])
    Pb[0, 0, 1] = nan_payload()
    Pb[2, 1, 1] = -1e4
    resb, _ = check(ctx, L[[0, 0, 0]], origin[:3], poses[[0, 0, 0]], Pb, [arrays[0]] * 3, GKW, MKW, "bad cov")
    assert resb["flags"].tolist() == [mfr.BAD_COV, 0, mfr.BAD_COV] and resb["nis"][[0, 2]].tolist() == [0.0, 0.0]
    assert np.array_equal(pose_bits(resb["P"][[0, 2]]), pose_bits(Pb[[0, 2]]))
    assert np.array_equal(pose_bits(resb["pose"][[0, 2]]), pose_bits(poses[[0, 0]]))
    assert np.array_equal(pose_bits(resb["pose"][1]), pose_bits(res["pose"][0])) and resb["moments"][0, 0] > 0


def test_outputs_may_alias_the_inputs(ctx):
    L, origin, poses, P, arrays, want = states_case()
    plain, _, _, _ = run(ctx, L, origin, poses, P, arrays, GKW, MKW)
    alias, _, _, (dx, dP) = run(ctx, L, origin, poses, P, arrays, GKW, MKW, alias=True)
    assert plain["flags"].tolist() == want
    for key in INT_KEYS + ("pose", "P", "z", "Rm", "nis", "rot0"):
        assert np.array_equal(pose_bits(plain[key]) if plain[key].dtype == np.float64 else plain[key],
                              pose_bits(alias[key]) if alias[key].dtype == np.float64 else alias[key]), key
    assert np.array_equal(pose_bits(dx.download()), pose_bits(plain["pose"]))
    assert np.array_equal(pose_bits(dP.download().reshape(-1, 3, 3)), pose_bits(plain["P"]))


def test_map_match_is_the_same_before_and_after_a_fuse(ctx):
    """lslam_map_match and lslam_map_fuse share the context's scratch volume and its timers: a match
    gives the same bits before and after a fuse as on its own, and each call is timed under its own id."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    R = 7
    L, origin, poses, arrays = random_case(77, R)
    gkw, mkw = dict(grid_w=40, cell=50.0), dict(win_w=32, k_trans=4, k_theta=3, theta_step=0.01, min_permille=100)
    xy, sco, cpo = csr(arrays)
    grid = OccupancyGrid(ctx, R, origin=origin, **gkw)
    grid.upload(L)
    own = GridLocalizer(ctx, R, **mkw)
    own.step(xy, sco, cpo, grid=grid, pose=poses, want_scores=True)
    alone = own.results()
    loc = GridLocalizer(ctx, R, **mkw)
    dx, dP = ctx.to_device(poses), ctx.to_device(prior(250.0, 0.04, R).reshape(R, 9))
    ctx.set_timing(True, kernels=[_lib.K_MAPMATCH, _lib.K_MAPFUSE])
    ctx.timing_reset()
    try:
        loc.step(xy, sco, cpo, grid=grid, pose=poses)  # (no scores asked for: the scratch volume)
        before = loc.results()
        assert ctx.timing(_lib.K_MAPMATCH)[1] == 1 and ctx.timing(_lib.K_MAPFUSE)[1] == 0
        loc.fuse(xy, sco, cpo, grid=grid, x=dx, P=dP, write_back=False)
        fused = loc.results()
        assert ctx.timing(_lib.K_MAPMATCH)[1] == 1 and ctx.timing(_lib.K_MAPFUSE)[1] == 1
        loc.step(xy, sco, cpo, grid=grid, pose=poses)
        after = loc.results()
        assert ctx.timing(_lib.K_MAPMATCH)[1] == 2 and ctx.timing(_lib.K_MAPFUSE)[1] == 1
    finally:
        ctx.set_timing(False)
    assert "P" in fused and "P" not in before and "P" not in after and "scores" not in fused
    for key in ("pose", "delta", "rot0"):
        assert np.array_equal(pose_bits(before[key]), pose_bits(alone[key])), key
        assert np.array_equal(pose_bits(after[key]), pose_bits(alone[key])), key
    for key in ("best", "n_valid", "flags"):
        assert np.array_equal(before[key], alone[key]) and np.array_equal(after[key], alone[key]), key
    # the fuse between them is the reference's, scratch volume and all
    ref = mfr.fuse_batch(L, grid.origin_host, poses, prior(250.0, 0.04, R), xy, cpo, rot0=fused["rot0"], rot=loc.rot_host,
                         **gkw, **mkw)
    assert_equal(fused, ref)
    assert np.array_equal(fused["best"], alone["best"]) and np.array_equal(pose_bits(fused["delta"]), pose_bits(alone["delta"]))


def test_parameters_and_arguments(ctx):
    from lidar_slam_amd.localize import GridLocalizer
    with pytest.raises(ValueError, match="cut_permille"):
        GridLocalizer(ctx, 2, cut_permille=1000)
    with pytest.raises(ValueError, match="nis_max"):
        GridLocalizer(ctx, 2, nis_max=0.0)
    loc = GridLocalizer(ctx, 2, r_scale=2.0, nis_max=float("inf"), cut_permille=0, k_trans=3)
    assert (loc.fp.r_scale, loc.fp.nis_max, loc.fp.cut_permille, loc.p.k_trans) == (2.0, float("inf"), 0, 3)
    with pytest.raises(ValueError):
        loc.fuse(np.zeros((0, 2)), [0, 0, 0], [0], grid=None, x=ctx.empty((2, 3), np.float64), P=ctx.empty((2, 9), np.float64))
    with pytest.raises(ValueError):
        loc.fuse(np.zeros((0, 2)), [0, 0, 0], [0], grid=None, x=np.zeros((2, 3)), P=np.zeros((2, 9)))  # host arrays


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The chain of test_gpu_mapmatch.test_end_to_end for five revolutions; then lm.x is moved by
    (120, -90) mm and 0.08 rad on the device, lm.P set to diag(150^2, 150^2, 0.12^2), and the revolution
    of step 5 is fused into the filter in place: exact against the reference given the downloaded
    inputs, every pose within 20 mm and pi/360 rad of the truth, the diagonal of lm.P shrunk; a grid
    update from the fused poses still meets the room caps.  Measured on an MI355X: fused to within
    7.3 mm and 0.0040 rad, nis at most 1.48, standard deviations after the update at most 13.7 mm,
    11.5 mm and 0.0080 rad."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    truth, rev5 = room_setup()[:2]
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    loc = GridLocalizer(ctx, R)
    for rev in revs:
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm, sync=False)
    L = grid.logodds.download()
    guess = truth + [120.0, -90.0, 0.08]
    P = np.tile(P_ROOM, (R, 1, 1))
    lm.x.upload(guess)
    lm.P.upload(P.reshape(R, 9))
    sco, cpo = rev5["scan_chunk_off"], rev5["chunk_pt_off"]
    loc.fuse(rev5["xy"], sco, cpo, grid=grid, lm=lm, want_scores=True)
    res = loc.results()
    ref = mfr.fuse_batch(L, grid.origin_host, guess, P, rev5["xy"], cpo[sco], rot0=res["rot0"], **ROOM_KW)
    assert_equal(res, ref)
    assert_rot(res["rot0"], guess)
    x, P1 = lm.x.download(), lm.P.download().reshape(R, 3, 3)
    assert np.array_equal(pose_bits(x), pose_bits(res["pose"])) and np.array_equal(pose_bits(P1), pose_bits(res["P"]))
    dpos = np.hypot(x[:, 0] - truth[:, 0], x[:, 1] - truth[:, 1])
    dth = np.abs(x[:, 2] - truth[:, 2])
    print("fused from (120, -90) mm, 0.08 rad off: worst", dpos.max(), "mm", dth.max(), "rad; nis at most", res["nis"].max(),
          "; sd after", np.sqrt(np.diagonal(P1, axis1=1, axis2=2)).max(0))
    assert not res["flags"].any(), res["flags"]
    assert dpos.max() <= 20.0 and dth.max() <= np.pi / 360
    assert np.all(np.diagonal(P1, axis1=1, axis2=2) < np.diag(P_ROOM))
    grid.step(rev5["xy"], sco, cpo, pose=lm)
    assert_room(grid.results()["logodds"], "device, fused poses")
