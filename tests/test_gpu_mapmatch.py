"""GPU parity of the scan-to-map matcher (lslam_map_match, lidar_slam_amd/localize.py) against its
NumPy definition, tests/mapmatch_ref.py.

Scores are integers and every double operation of the definition is rounded on its own, so pose_out,
delta, best, n_valid, flags and the whole score volume are compared EXACTLY, the reference being fed
the (cos, sin) that the device wrote to rot0: those bits are the definition's input.  rot0 itself is
held to 1e-15 as in test_gpu_occgrid (OCML's 2 ulp and glibc's 1 ulp at magnitude <= 1: 3.3e-16).
"""
import numpy as np
import pytest

import mapmatch_ref as mmr
from oracle import cpu as orc
from test_gpu_occgrid import assert_rot, csr
from test_mapmatch_ref import BAD_POSES, ROOM_BAD, ROOM_EDGE, pose_bits, room_setup
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, assert_room, room_run

pytestmark = pytest.mark.gpu

KEYS = ("delta", "best", "n_valid", "flags", "scores")


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def assert_equal(res, ref, what=""):
    for key in KEYS:
        bad = np.argwhere(res[key] != ref[key])
        assert bad.size == 0, (what, key, len(bad), bad[:5])
    bad = np.argwhere(pose_bits(res["pose"]) != pose_bits(ref["pose_out"]))
    assert bad.size == 0, (what, "pose", bad[:5], res["pose"][bad[:5, 0]], ref["pose_out"][bad[:5, 0]])


def check(ctx, L, origin, poses, arrays, gkw, mkw, what=""):
    """One call on fresh objects, compared with the reference; returns (device results, reference)."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    R = len(arrays)
    xy, sco, cpo = csr(arrays)
    grid = OccupancyGrid(ctx, R, origin=origin, **gkw)
    grid.upload(L)
    loc = GridLocalizer(ctx, R, **mkw)
    loc.step(xy, sco, cpo, grid=grid, pose=poses, want_scores=True)
    res = loc.results()
    ref = mmr.match_batch(L, grid.origin_host, poses, xy, cpo, rot0=res["rot0"], rot=loc.rot_host, **gkw, **mkw)
    assert_equal(res, ref, what)
    assert_rot(res["rot0"], poses)
    assert np.array_equal(grid.logodds.download(), L)  # read only
    return res, ref


def pose_in_cell(rng, X0, Y0, origin, cell):
    """A pose somewhere inside map cell (X0, Y0) (not within 1 % of its border), any heading."""
    f = rng.uniform(0.01, 0.99, (len(X0), 2))
    return np.stack([origin[:, 0] + (X0 + f[:, 0]) * cell, origin[:, 1] + (Y0 + f[:, 1]) * cell,
                     rng.uniform(-np.pi, np.pi, len(X0))], -1)


@pytest.mark.parametrize("W", [48, 20, 100, 24])
def test_alignment_sweep(ctx, W):
    """Window 16 on a map of W cells: the window's first column X0 - 8 (and row) takes every residue
    mod 16, hence mod 8, against the dwords of G and the 16-byte groups of the map's rows; W = 20 and
    100 take the cell-per-lane path.  Map values lie around occ_min."""
    rng = np.random.default_rng(100 + W)
    R, cell = 32, 100.0
    gkw = dict(grid_w=W, cell=cell)
    mkw = dict(win_w=16, k_trans=3, k_theta=1, smear=2, occ_min=85, min_permille=300)
    i = np.arange(R)
    lo = max(0, (W - 20) // 2 - 2)  # the window of the first robots hangs over the map's edge when W is small
    X0 = lo + 2 + i % 16
    Y0 = lo + 2 + (5 * i + i // 16) % 16
    assert len(set((X0 - 8) % 16)) == 16 and len(set((Y0 - 8) % 16)) == 16
    origin = np.where((i < 16)[:, None], [0.0, 0.0], [-1234.5, 777.25])
    poses = pose_in_cell(rng, X0, Y0, origin, cell)
    L = (85 + rng.integers(-2, 3, (R, W, W))).astype(np.int16)
    L[rng.random((R, W, W)) < 0.7] = -20  # mostly free: scores that tell the candidates apart
    arrays = [rng.uniform(-1250.0, 1250.0, (40 + r, 2)) for r in range(R)]
    res, ref = check(ctx, L, origin, poses, arrays, gkw, mkw)
    assert np.all(res["n_valid"][:, 0] > 0) and not np.any(res["flags"] & (mmr.BAD_POSE | mmr.EMPTY))


@pytest.mark.parametrize("W", [16, 20])
def test_overhang(ctx, W):
    """The window over each edge and corner of the map, wholly outside it, and larger than it
    (W = 16: 16-byte groups; W = 20: a lane per cell)."""
    rng = np.random.default_rng(7 + W)
    cell = 100.0
    gkw = dict(grid_w=W, cell=cell)
    c = [-3, W // 2, W + 2]
    cellsxy = [(x, y) for x in c for y in c] + [(W + 100, 3), (5, -9), (W + 8, W + 8), (W + 7, W + 7)]
    R = len(cellsxy)
    X0, Y0 = np.array(cellsxy).T
    origin = np.tile([300.0, -4100.0], (R, 1))
    poses = pose_in_cell(rng, X0, Y0, origin, cell)
    L = (85 + rng.integers(-1, 2, (R, W, W))).astype(np.int16)
    arrays = [rng.uniform(-1400.0, 1400.0, (50, 2)) for _ in range(R)]
    res, _ = check(ctx, L, origin, poses, arrays, gkw, dict(win_w=16, k_trans=4, k_theta=2, min_permille=100))
    assert res["flags"][9:12].tolist() == [mmr.EMPTY] * 3 and not res["n_valid"][9:12, 0].any()
    assert np.array_equal(pose_bits(res["pose"][9:12]), pose_bits(poses[9:12]))
    assert res["n_valid"][12, 0] <= 1  # the window's corner cell is the map's
    # a window of 64 on this map: all of it, wherever it is seen from
    big, _ = check(ctx, L, origin, poses, arrays, gkw, dict(win_w=64, k_trans=2, k_theta=1, min_permille=100))
    assert np.array_equal(big["n_valid"][:9, 0], (L[:9] >= 85).sum(axis=(1, 2)))


@pytest.mark.parametrize("smear,kt,kth", [(0, 0, 0), (1, 15, 2), (2, 3, 31), (2, 15, 0)])
def test_search_window(ctx, smear, kt, kth):
    """Every smear with occupied cells on the window's and the map's borders; the smallest and the
    largest translation window (Nt = 31: two groups of 16 jx, the largest LDS) and rotation window."""
    rng = np.random.default_rng(31 * smear + kt + kth)
    W, ww, cell = 40, 32, 50.0
    gkw = dict(grid_w=W, cell=cell)
    mkw = dict(win_w=ww, smear=smear, k_trans=kt, k_theta=kth, theta_step=0.01, min_permille=200)
    cellsxy = [(20, 20), (16, 16), (24, 17), (3, 36), (37, 2)]
    R = len(cellsxy)
    X0, Y0 = np.array(cellsxy).T
    origin = np.zeros((R, 2))
    poses = pose_in_cell(rng, X0, Y0, origin, cell)
    L = np.full((R, W, W), -41, np.int16)
    L[:, [0, W - 1], :] = 200   # the map's border
    L[:, :, [0, W - 1]] = 200
    for r in range(R):          # the window's border cells that lie on the map
        for e in (0, ww - 1):
            y, x = Y0[r] - ww // 2 + e, X0[r] - ww // 2 + e
            if 0 <= y < W:
                L[r, y, ::3] = 90
            if 0 <= x < W:
                L[r, 1::3, x] = 90
    L[rng.random((R, W, W)) < 0.05] = 85
    arrays = [rng.uniform(-(ww // 2 + kt + 2) * cell, (ww // 2 + kt + 2) * cell, (150, 2)) for _ in range(R)]
    res, _ = check(ctx, L, origin, poses, arrays, gkw, mkw)
    assert res["scores"].shape == (R, 2 * kth + 1, 2 * kt + 1, 2 * kt + 1) and res["scores"].any()


def test_bad_poses(ctx):
    """Every bad pose of the CPU test in one batch, between two good robots: BAD_POSE alone, zero
    scores and counts, the centre as best, the pose's bits (NaN payloads included) returned."""
    rng = np.random.default_rng(9)
    R = len(BAD_POSES) + 2
    poses = np.array([[1650.0, 1650.0, 0.1]] + [p for p, _ in BAD_POSES] + [[1250.0, 1850.0, -2.0]])
    origin = np.array([[0.0, 0.0]] + [o for _, o in BAD_POSES] + [[0.0, 0.0]])
    poses[2, 0] = np.frombuffer(np.uint64(0x7FF80000DEADBEEF).tobytes(), np.float64)[0]  # a NaN with a payload
    L = np.where(rng.random((R, 32, 32)) < 0.3, 100, -41).astype(np.int16)
    arrays = [rng.uniform(-900.0, 900.0, (30, 2)) for _ in range(R)]
    res, _ = check(ctx, L, origin, poses, arrays, dict(grid_w=32, cell=100.0),
                   dict(win_w=16, k_trans=4, k_theta=2, min_permille=100))
    bad = slice(1, R - 1)
    assert np.all(res["flags"][bad] == mmr.BAD_POSE) and not np.any(res["flags"][[0, R - 1]] & mmr.BAD_POSE)
    assert not res["scores"][bad].any() and not res["n_valid"][bad].any() and not res["delta"][bad].any()
    assert np.all(res["best"][bad] == [2, 4, 4, 0])
    assert np.array_equal(pose_bits(res["pose"][bad]), pose_bits(poses[bad]))
    assert np.all(np.isnan(res["rot0"][~np.isfinite(poses[:, 2])]))
    assert res["best"][0, 3] > 0 and res["best"][R - 1, 3] > 0


def test_slices(ctx):
    """One robot's inputs alone (a slice per rotation), in a batch of 3 and in a batch of more than
    two workgroups per CU (one slice): the same results."""
    rng = np.random.default_rng(55)
    W, cell = 24, 100.0
    gkw = dict(grid_w=W, cell=cell)
    mkw = dict(win_w=16, k_trans=4, k_theta=5, min_permille=200)
    Rbig = 520
    L = np.where(rng.random((Rbig, W, W)) < 0.25, 100, -30).astype(np.int16)
    origin = rng.uniform(-500.0, 500.0, (Rbig, 2))
    poses = pose_in_cell(rng, rng.integers(6, 18, Rbig), rng.integers(6, 18, Rbig), origin, cell)
    arrays = [rng.uniform(-900.0, 900.0, (8, 2)) for _ in range(Rbig)]
    for at in (0, 2, Rbig - 1):  # the robot under test, where each batch holds it
        L[at], origin[at], poses[at], arrays[at] = L[0], origin[0], poses[0], arrays[0]
    alone, _ = check(ctx, L[:1], origin[:1], poses[:1], arrays[:1], gkw, mkw, "alone")
    three, _ = check(ctx, L[:3], origin[:3], poses[:3], arrays[:3], gkw, mkw, "three")
    many, _ = check(ctx, L, origin, poses, arrays, gkw, mkw, "many")
    assert alone["best"][0, 3] > 0
    for key in KEYS + ("pose", "rot0"):
        for res, at in ((three, 0), (three, 2), (many, 0), (many, 2), (many, Rbig - 1)):
            assert np.array_equal(pose_bits(alone[key][0]) if key in ("pose", "rot0") else alone[key][0],
                                  pose_bits(res[key][at]) if key in ("pose", "rot0") else res[key][at]), (key, at)


def test_long_and_ragged_scans(ctx):
    """Revolutions of 4100, 513, 512, 1 and 0 points (tiles of 512) with NaN, inf, (0, 0) and 1e300
    points, and points up to k_trans cells outside the window, which only some translations bring
    in (the packed-coordinate list)."""
    rng = np.random.default_rng(77)
    W, ww, kt, cell = 64, 32, 4, 50.0
    gkw = dict(grid_w=W, cell=cell)
    mkw = dict(win_w=ww, k_trans=kt, k_theta=3, min_permille=100)
    sizes = [4100, 513, 512, 1, 0]
    R = len(sizes)
    origin = np.tile([-1600.0, -1600.0], (R, 1))
    poses = pose_in_cell(rng, rng.integers(24, 40, R), rng.integers(24, 40, R), origin, cell)
    L = np.where(rng.random((R, W, W)) < 0.2, 120, -41).astype(np.int16)
    junk = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0], [-np.inf, np.nan], [1e300, 1e300], [-1e300, 3.0],
                     [1e300, -1e300]])
    arrays = []
    for n in sizes:
        reach = (ww // 2 + kt + 1) * cell
        a = rng.uniform(-reach, reach, (n, 2))
        ring = rng.random(n) < 0.3          # in the ring just outside the window
        side = rng.integers(0, 2, n) * 2 - 1
        a[ring, 0] = side[ring] * rng.uniform(ww // 2 * cell, reach, int(ring.sum()))
        bad = rng.random(n) < 0.05
        a[bad] = junk[rng.integers(0, len(junk), int(bad.sum()))]
        arrays.append(a)
    arrays[3] = np.array([[120.0, -260.0]])
    res, _ = check(ctx, L, origin, poses, arrays, gkw, mkw)
    assert res["n_valid"][4, 1] == 0 and res["flags"][4] == mmr.EMPTY and res["n_valid"][3, 1] == 1
    assert 3800 < res["n_valid"][0, 1] < 4100 and res["best"][0, 3] > 0


def test_default_window_on_the_room(ctx):
    """Batches of test_mapmatch_ref's room tests at the default window (two of its guess draws, its
    far guess and its guess beyond the translation window): exact against the reference, and the caps
    asserted there hold for the device's results: 20 mm, pi/360 rad and flags 0 for the draws, WEAK
    and an untouched pose for the far guess, EDGE and a corrected pose for the last."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    truth, rev5, off, L5, L1, origin, guesses = room_setup()
    R = len(ROOM_ROBOTS)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    grid.upload(L5)
    loc = GridLocalizer(ctx, R)
    sco, cpo = rev5["scan_chunk_off"], rev5["chunk_pt_off"]
    for which, g in (("draw 0", guesses[0]), ("draw 1", guesses[1]), ("bad", truth + ROOM_BAD), ("edge", truth + ROOM_EDGE)):
        loc.step(rev5["xy"], sco, cpo, grid=grid, pose=g, want_scores=True)
        res = loc.results()
        ref = mmr.match_batch(L5, origin, g, rev5["xy"], off, rot0=res["rot0"], **ROOM_KW)
        assert_equal(res, ref, which)
        assert_rot(res["rot0"], g)
        dpos = np.hypot(res["pose"][:, 0] - truth[:, 0], res["pose"][:, 1] - truth[:, 1])
        dth = np.abs(res["pose"][:, 2] - truth[:, 2])
        print(which, "flags", res["flags"].tolist(), "worst", dpos.max(), "mm", dth.max(), "rad")
        if which == "bad":
            assert np.all(res["flags"] & mmr.WEAK) and np.array_equal(pose_bits(res["pose"]), pose_bits(g))
        elif which == "edge":
            assert np.all(res["flags"] == mmr.EDGE) and np.all(res["pose"][:, 0] == g[:, 0] + 200.0)
        else:
            assert not res["flags"].any() and dpos.max() <= 20.0 and dth.max() <= np.pi / 360


def test_pose_out_may_alias_pose(ctx):
    """write_back on a DeviceArray: accepted robots move, WEAK, EMPTY and BAD_POSE robots keep their
    bits, and everything equals the call that does not alias."""
    from lidar_slam_amd.localize import GridLocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    truth, rev5, off, L5, L1, origin, guesses = room_setup()
    R = len(ROOM_ROBOTS)
    g = np.array(guesses[1])
    g[1] = truth[1] + ROOM_BAD                    # WEAK
    g[2] = (-90000.0, 40000.0, 0.3)               # the window is off the map: EMPTY
    g[3] = (np.nan, truth[3, 1], truth[3, 2])     # BAD_POSE
    g[4, 2] = -np.inf                             # BAD_POSE
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    grid.upload(L5)
    sco, cpo = rev5["scan_chunk_off"], rev5["chunk_pt_off"]
    plain, alias = GridLocalizer(ctx, R), GridLocalizer(ctx, R)
    plain.step(rev5["xy"], sco, cpo, grid=grid, pose=g, want_scores=True)
    a = plain.results()
    ref = mmr.match_batch(L5, grid.origin_host, g, rev5["xy"], off, rot0=a["rot0"], **ROOM_KW)
    assert_equal(a, ref)
    assert a["flags"][1] & mmr.WEAK  # (the far guess's winner may lie on the border as well)
    assert a["flags"][[0, 2, 3, 4, 5, 6, 7]].tolist() == [0, mmr.EMPTY, mmr.BAD_POSE, mmr.BAD_POSE, 0, 0, 0]
    dpose = ctx.to_device(g)
    alias.step(rev5["xy"], sco, cpo, grid=grid, pose=dpose, write_back=True, want_scores=True)
    b = alias.results()
    got = dpose.download()
    assert np.array_equal(pose_bits(got), pose_bits(b["pose"]))
    for key in KEYS:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(pose_bits(a["pose"]), pose_bits(got)) and np.array_equal(pose_bits(a["rot0"]), pose_bits(b["rot0"]))
    assert np.array_equal(pose_bits(got[1:5]), pose_bits(g[1:5]))
    moved = [0, 5, 6, 7]
    assert np.all(np.any(got[moved] != g[moved], axis=1)) and np.all(got[moved] == g[moved] + a["delta"][moved])
    with pytest.raises(ValueError):
        alias.step(rev5["xy"], sco, cpo, grid=grid, pose=g, write_back=True)  # a host pose cannot be written back
    with pytest.raises(ValueError):
        GridLocalizer(ctx, R, win_w=15)


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The chain of test_gpu_occgrid.test_end_to_end for five revolutions; then the filter's poses
    are moved by (120, -90) mm and 0.08 rad on the device and the revolution of step 5 is localised
    in the grid, written back into lm.x: exact against the reference given the downloaded inputs,
    every pose within 20 mm and pi/360 rad of the truth, flags 0; a grid update from the corrected
    poses still meets the room caps.  Measured on an MI355X: filter poses 2.1 mm and 0.0014 rad off
    after the five revolutions; localised to within 7.1 mm and 0.0037 rad, score ratio at least 0.88."""
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
    x = lm.x.download()
    print("filter pose error after five revolutions",
          np.hypot(x[:, 0] - poses[4][:, 0], x[:, 1] - poses[4][:, 1]).max(), np.abs(x[:, 2] - poses[4][:, 2]).max())
    guess = truth + [120.0, -90.0, 0.08]
    lm.x.upload(guess)
    sco, cpo = rev5["scan_chunk_off"], rev5["chunk_pt_off"]
    loc.step(rev5["xy"], sco, cpo, grid=grid, pose=lm, write_back=True, want_scores=True)
    res = loc.results()
    ref = mmr.match_batch(L, grid.origin_host, guess, rev5["xy"], cpo[sco], rot0=res["rot0"], **ROOM_KW)
    assert_equal(res, ref)
    assert_rot(res["rot0"], guess)
    x = lm.x.download()
    assert np.array_equal(pose_bits(x), pose_bits(res["pose"]))
    dpos = np.hypot(x[:, 0] - truth[:, 0], x[:, 1] - truth[:, 1])
    dth = np.abs(x[:, 2] - truth[:, 2])
    print("localised from (120, -90) mm, 0.08 rad off: worst", dpos.max(), "mm", dth.max(), "rad; score ratio",
          (res["best"][:, 3] / (3.0 * res["n_valid"][:, 1])).min())
    assert not res["flags"].any(), res["flags"]
    assert dpos.max() <= 20.0 and dth.max() <= np.pi / 360
    grid.step(rev5["xy"], sco, cpo, pose=lm)
    assert_room(grid.results()["logodds"], "device, localised poses")
