"""The scan-to-map definition (include/lidarslam.h, lslam_map_match) on the CPU: how well it finds
a robot again in the map of the synthetic room, the acceptance gate, hand-made edge cases held
against a second, loop-by-loop form of the definition, and the ABI checks that need no device.
tests/mapmatch_ref.py is the NumPy form of the definition; tests/test_gpu_mapmatch.py holds the
kernels to it bit for bit.

Room recovery.  The room of test_occgrid_ref (robots 200-207, grid_w 256 at 20 mm, origin
(-560, -1060)), the map built from revolutions 0-4 at the true poses; the revolution of step 5 is
matched from guesses off by up to +-150 mm per axis and +-0.12 rad (three seeded draws per robot and
the true pose itself), default parameters.  Caps, one search quantum each: every result within
20 mm (one cell) and pi/360 rad (one step) of the truth, flags == 0.  Measured here: 4.6 mm and
0.0047 rad at worst.  Score over 3 x (valid points): 0.881-0.909 on the five-revolution map, at
least 0.767 for the same guesses on a one-revolution map, at most 0.093 for a guess 700 mm, -600 mm
and 0.5 rad away: the gate of 0.5 separates them.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mapmatch_ref as mmr
from lidar_slam_amd import _lib, synth
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, build_room, room_run

ROOM_BAD = np.array([700.0, -600.0, 0.5])    # a guess this far off must be refused
ROOM_EDGE = np.array([-215.0, 0.0, 0.0])     # more than k_trans cells off along x: the winner lies on the border


def pose_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def room_setup():
    """(truth [R, 3] at step 5, the revolution of step 5, offsets, map of five revolutions, map of
    one, origin [R, 2], guesses [4, R, 3])."""
    poses, revs = room_run()
    poses6 = synth.trajectory(ROOM_ROBOTS, 5, u=(146.0, 174.0))
    assert np.array_equal(poses6[:5], poses)
    rev5 = synth.revolutions_at(poses6[5], 5, ROOM_ROBOTS)
    off = rev5["chunk_pt_off"][rev5["scan_chunk_off"]]
    R = len(ROOM_ROBOTS)
    L5 = build_room(poses, revs)
    L1 = build_room(poses[:1], revs[:1])
    rng = np.random.default_rng(20)
    d = rng.uniform(-1.0, 1.0, (3, R, 3)) * [150.0, 150.0, 0.12]
    guesses = np.concatenate([poses6[5][None] + d, poses6[5][None]])
    return poses6[5], rev5, off, L5, L1, np.tile(ROOM_ORIGIN, (R, 1)), guesses


@functools.lru_cache(maxsize=None)
def room_case(which, draw=0):
    """Reference results of one batch of the room: which = "good" (guess set `draw` on the
    five-revolution map), "one" (the same on the one-revolution map), "bad", "edge".  Returns
    (L, guesses [R, 3], results); shared with test_gpu_mapmatch."""
    truth, rev5, off, L5, L1, origin, guesses = room_setup()
    L = L1 if which == "one" else L5
    g = {"good": guesses[draw], "one": guesses[draw], "bad": truth + ROOM_BAD, "edge": truth + ROOM_EDGE}[which]
    return L, g, mmr.match_batch(L, origin, g, rev5["xy"], off, **ROOM_KW)


def ratio(res):
    return res["best"][:, 3] / (3.0 * res["n_valid"][:, 1])


def test_room_recovery():
    truth = room_setup()[0]
    worst_d = worst_t = 0.0
    ratios = []
    for draw in range(4):
        _, g, res = room_case("good", draw)
        dpos = np.hypot(res["pose_out"][:, 0] - truth[:, 0], res["pose_out"][:, 1] - truth[:, 1])
        dth = np.abs(res["pose_out"][:, 2] - truth[:, 2])
        print("draw", draw, "guess off by", np.hypot(g[:, 0] - truth[:, 0], g[:, 1] - truth[:, 1]).max(), "mm ->",
              dpos.max(), "mm,", dth.max(), "rad; ratio", ratio(res).min(), ratio(res).max())
        assert np.all(res["flags"] == 0), res["flags"]
        assert dpos.max() <= 20.0 and dth.max() <= np.pi / 360
        assert np.all(res["n_valid"][:, 1] == 720) and np.all(res["n_valid"][:, 0] > 100)
        worst_d, worst_t = max(worst_d, dpos.max()), max(worst_t, dth.max())
        ratios += list(ratio(res))
    print("worst", worst_d, "mm", worst_t, "rad; ratios", min(ratios), max(ratios))


def test_gate_refuses_a_far_guess_and_keeps_the_good_ones():
    _, g, res = room_case("bad")
    print("bad guesses: ratio at most", ratio(res).max())
    assert np.all(res["flags"] & mmr.WEAK) and not np.any(res["flags"] & (mmr.EMPTY | mmr.BAD_POSE))
    assert np.array_equal(pose_bits(res["pose_out"]), pose_bits(g))
    assert np.any(res["delta"] != 0.0)  # reported all the same
    lo = 1.0
    for draw in range(4):
        _, g, res = room_case("one", draw)
        lo = min(lo, ratio(res).min())
        assert not np.any(res["flags"] & (mmr.WEAK | mmr.EMPTY | mmr.BAD_POSE)), (draw, res["flags"])
        assert np.all(res["pose_out"] == g + res["delta"])
    print("good guesses on a one-revolution map: ratio at least", lo)


def test_edge_still_corrects():
    truth = room_setup()[0]
    _, g, res = room_case("edge")
    assert np.all(res["flags"] == mmr.EDGE), res["flags"]
    assert np.all(res["best"][:, 2] == 20)  # jx on the window's border
    assert np.all(res["pose_out"] == g + res["delta"]) and np.all(res["delta"][:, 0] == 200.0)
    assert np.abs(res["pose_out"][:, 0] - truth[:, 0]).max() <= 15.0 + 20.0


# ---- hand-made cases: cells of 100 mm, window 16, the robot on the centre of its cell ----

# (k_theta 1: with a single rotation the winner is on the border of that axis, which is EDGE)
KW = dict(cell=100.0, grid_w=32, win_w=16, smear=0, k_trans=4, k_theta=1)


def at_cell(X0, Y0, th=0.0, cell=100.0):
    return np.array([(X0 + 0.5) * cell, (Y0 + 0.5) * cell, th])


def cells(*ij, cell=100.0):
    """Robot-frame points that, seen from at_cell(X0, Y0), fall into map cells (X0 + i, Y0 + j)."""
    return np.array([[i * cell + 10.0, j * cell + 10.0] for i, j in ij], np.float64).reshape(-1, 2)


def grid_with(W, occupied, value=100):
    L = np.zeros((W, W), np.int16)
    for x, y in occupied:
        L[y, x] = value
    return L


def naive(L, origin, pose, xy, **kw):
    """The definition once more, a loop per index and Python floats: (G, n_occupied, S)."""
    p = mmr.params(**kw)
    gw, ww, sm, kt, kth = (int(p[k]) for k in ("grid_w", "win_w", "smear", "k_trans", "k_theta"))
    half, inv = ww // 2, 1.0 / float(p["cell"])
    Nt, Nth = 2 * kt + 1, 2 * kth + 1
    px, py, th = (float(v) for v in pose)
    ox, oy = (float(v) for v in origin)
    X0, Y0 = int(np.floor((px - ox) * inv)), int(np.floor((py - oy) * inv))
    occ = [(gy, gx) for gy in range(ww) for gx in range(ww)
           if 0 <= Y0 - half + gy < gw and 0 <= X0 - half + gx < gw and L[Y0 - half + gy, X0 - half + gx] >= p["occ_min"]]
    G = np.zeros((ww, ww), np.int64)
    for gy in range(ww):
        for gx in range(ww):
            for (y, x) in occ:
                G[gy, gx] = max(G[gy, gx], sm + 1 - max(abs(gy - y), abs(gx - x)))
    c, s = float(np.cos(th)), float(np.sin(th))
    rot = mmr.rot_table(kth, p["theta_step"])
    S = np.zeros((Nth, Nt, Nt), np.int64)
    for k in range(Nth):
        cc = c * float(rot[k, 0]) - s * float(rot[k, 1])
        ss = s * float(rot[k, 0]) + c * float(rot[k, 1])
        for x, y in np.asarray(xy, np.float64).reshape(-1, 2):
            x, y = float(x), float(y)
            if not (np.isfinite(x) and np.isfinite(y)) or (x == 0.0 and y == 0.0):
                continue
            with np.errstate(invalid="ignore", over="ignore"):
                wx = np.float64(px) + (np.float64(cc) * x - np.float64(ss) * y)
                wy = np.float64(py) + (np.float64(ss) * x + np.float64(cc) * y)
                ax = np.floor((wx - ox) * inv) - X0
                ay = np.floor((wy - oy) * inv) - Y0
            if not (-half - kt <= ax < half + kt and -half - kt <= ay < half + kt):
                continue
            for jy in range(Nt):
                for jx in range(Nt):
                    gy, gx = int(ay) + jy - kt + half, int(ax) + jx - kt + half
                    if 0 <= gy < ww and 0 <= gx < ww:
                        S[k, jy, jx] += G[gy, gx]
    return G, len(occ), S


def assert_same_as_naive(L, origin, pose, xy, **kw):
    m = mmr.match(L, origin, pose, xy, **kw)
    G, n_occ, S = naive(L, origin, pose, xy, **kw)
    assert np.array_equal(m["G"], G) and m["n_valid"][0] == n_occ
    assert np.array_equal(m["scores"], S)
    return m


def test_tie_break_order():
    # one point; occupied cells 1 to the right and 3 to the left of it: both score 1, the nearer wins
    m = mmr.match(grid_with(32, [(17, 16), (13, 16)]), (0.0, 0.0), at_cell(16, 16), cells((0, 0)), **KW)
    assert m["best"].tolist() == [1, 4, 5, 1] and m["flags"] == 0
    assert m["delta"].tolist() == [100.0, 0.0, 0.0]
    # equal distances: the smaller flat index (jy, then jx)
    m = mmr.match(grid_with(32, [(18, 16), (14, 16), (16, 18), (16, 14)]), (0.0, 0.0), at_cell(16, 16), cells((0, 0)), **KW)
    assert m["best"].tolist() == [1, 2, 4, 1]
    assert m["delta"].tolist() == [0.0, -200.0, 0.0]


def test_window_over_the_map_borders():
    rng = np.random.default_rng(3)
    kw = dict(KW, grid_w=16, smear=1, k_theta=1, occ_min=85)
    L = (85 + rng.integers(-2, 3, (16, 16))).astype(np.int16)
    pts = rng.uniform(-1300.0, 1300.0, (40, 2))
    for X0 in (-3, 2, 8, 14, 18):
        for Y0 in (-3, 2, 8, 14, 18):
            m = assert_same_as_naive(L, (0.0, 0.0), at_cell(X0, Y0, 0.3), pts, **kw)
            nx, ny = (min(16, X0 + 8) - max(0, X0 - 8)), (min(16, Y0 + 8) - max(0, Y0 - 8))
            assert 0 < m["n_valid"][0] <= nx * ny < 256 or (X0, Y0) == (8, 8)
    # with occ_min at the bottom of the range the occupied cells are exactly the window's cells on the map
    m = mmr.match(L, (0.0, 0.0), at_cell(-3, 14), pts, **dict(kw, occ_min=-32768))
    assert m["n_valid"][0] == 5 * 10


def test_window_outside_the_map_is_empty():
    L = np.full((16, 16), 300, np.int16)
    for X0, Y0 in ((40, 8), (8, -9), (-100, -100), (24, 24)):
        pose = at_cell(X0, Y0, 0.1)
        m = mmr.match(L, (0.0, 0.0), pose, cells((1, 1), (2, -3)), **dict(KW, grid_w=16))
        assert m["flags"] == mmr.EMPTY and m["n_valid"].tolist() == [0, 2]
        assert m["best"].tolist() == [1, 4, 4, 0] and not m["delta"].any() and not m["scores"].any()
        assert np.array_equal(pose_bits(m["pose_out"]), pose_bits(pose))
    # one cell further in, the window's corner cell is on the map
    m = mmr.match(L, (0.0, 0.0), at_cell(23, 23), cells((-8, -8)), **dict(KW, grid_w=16))
    assert m["n_valid"].tolist() == [1, 1] and m["flags"] == 0 and m["best"].tolist() == [1, 4, 4, 1]


def test_window_larger_than_the_map():
    rng = np.random.default_rng(4)
    L = (85 + rng.integers(-1, 2, (16, 16))).astype(np.int16)
    kw = dict(KW, grid_w=16, win_w=32, smear=2, k_trans=2)
    pts = rng.uniform(-1200.0, 1200.0, (30, 2))
    for X0, Y0 in ((8, 8), (3, 12), (-10, 20)):
        m = assert_same_as_naive(L, (0.0, 0.0), at_cell(X0, Y0, -0.2), pts, **kw)
    m = assert_same_as_naive(L, (0.0, 0.0), at_cell(8, 8), pts, **kw)
    assert m["n_valid"][0] == int((L >= 85).sum())  # the whole map is inside the window


def test_occ_min_thresholds():
    pose, pts = at_cell(16, 16), cells((2, 1))
    L = grid_with(32, [(18, 17)], value=100)
    for occ_min, hit in ((99, True), (100, True), (101, False)):
        m = mmr.match(L, (0.0, 0.0), pose, pts, **dict(KW, occ_min=occ_min))
        assert (m["best"][3] == 1 and m["n_valid"][0] == 1 and m["flags"] == 0) == hit, occ_min
        assert (m["flags"] == mmr.EMPTY) == (not hit)
    L = np.full((32, 32), -32768, np.int16)
    L[17, 18] = 32767
    m = mmr.match(L, (0.0, 0.0), pose, pts, **dict(KW, occ_min=32767))
    assert m["n_valid"][0] == 1 and m["best"].tolist() == [1, 4, 4, 1]
    m = mmr.match(L, (0.0, 0.0), pose, pts, **dict(KW, occ_min=-32768))
    assert m["n_valid"][0] == 256 and m["best"][3] == 1  # every cell of the window counts, -32768 included
    m = mmr.match(L, (0.0, 0.0), pose, pts, **dict(KW, occ_min=-32767))
    assert m["n_valid"][0] == 1


def test_smear_is_clipped_to_the_window():
    # window = map cells 8..23; occupied: its corner cell (8, 8), and (7, 12), (24, 20), (15, 24) just outside it
    L = grid_with(32, [(8, 8), (7, 12), (24, 20), (15, 24)])
    m = assert_same_as_naive(L, (0.0, 0.0), at_cell(16, 16), cells((-8, -8)), **dict(KW, smear=2))
    G = m["G"]
    assert m["n_valid"][0] == 1
    assert G[:3, :3].tolist() == [[3, 2, 1], [2, 2, 1], [1, 1, 1]] and G.sum() == 3 + 3 * 2 + 5
    # the same cell one to the left is outside: nothing is smeared back in
    m = mmr.match(grid_with(32, [(7, 8)]), (0.0, 0.0), at_cell(16, 16), cells((-8, -8)), **dict(KW, smear=2))
    assert not m["G"].any() and m["flags"] == mmr.EMPTY


def _bad_poses():
    """NaN, +inf and -inf in each of the five inputs, then robot cells 2^20 or more cells off."""
    good = [1650.0, 1650.0, 0.1, 0.0, 0.0]
    out = []
    for i in range(5):
        for v in (np.nan, np.inf, -np.inf):
            w = list(good)
            w[i] = v
            out.append((tuple(w[:3]), tuple(w[3:])))
    far = 100.0 * 2.0 ** 20
    return out + [((far, 1650.0, 0.1), (0.0, 0.0)), ((1650.0, -far, 0.1), (0.0, 0.0)),
                  ((1650.0, 1650.0, 0.1), (0.0, far + 1700.0)), ((1650.0, 1650.0, 0.1), (-far, 0.0))]


BAD_POSES = _bad_poses()


@pytest.mark.parametrize("pose,origin", BAD_POSES)
def test_bad_pose(pose, origin):
    L = np.full((32, 32), 300, np.int16)
    m = mmr.match(L, origin, pose, cells((1, 1), (2, 2)), **dict(KW, k_theta=2))
    assert m["flags"] == mmr.BAD_POSE
    assert np.array_equal(pose_bits(m["pose_out"]), pose_bits(np.array(pose)))
    assert m["delta"].tolist() == [0.0, 0.0, 0.0] and m["best"].tolist() == [2, 4, 4, 0]
    assert m["n_valid"].tolist() == [0, 0] and m["scores"].shape == (5, 9, 9) and not m["scores"].any()
    th = float(pose[2])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(m["rot0"], [np.cos(th), np.sin(th)], equal_nan=True)


def test_last_good_robot_cell():
    """|X0| = 2^20 - 1 is still a pose: the window lies outside the map, which is EMPTY, not BAD_POSE."""
    m = mmr.match(np.full((32, 32), 300, np.int16), (0.0, 0.0), (100.0 * (2.0 ** 20 - 1), 1650.0, 0.0), cells((1, 1)), **KW)
    assert m["flags"] == mmr.EMPTY and m["n_valid"].tolist() == [0, 1]


def test_no_points_invalid_points_huge_points():
    L = grid_with(32, [(18, 17), (12, 12)])
    pose = at_cell(16, 16)
    m = mmr.match(L, (0.0, 0.0), pose, np.zeros((0, 2)), **KW)
    assert m["flags"] == mmr.EMPTY and m["n_valid"].tolist() == [2, 0]
    assert np.array_equal(pose_bits(m["pose_out"]), pose_bits(pose))
    junk = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0], [-np.inf, np.nan], [100.0, np.nan]])
    m = mmr.match(L, (0.0, 0.0), pose, junk, **KW)
    assert m["flags"] == mmr.EMPTY and m["n_valid"].tolist() == [2, 0]
    huge = np.array([[1e300, 1e300], [-1e300, 5.0], [1e300, -1e300], [3e9, 100.0]])
    pts = np.concatenate([junk, huge, cells((2, 1))])
    for th in (0.0, 0.7):
        m = assert_same_as_naive(L, (0.0, 0.0), at_cell(16, 16, th), pts, **dict(KW, k_theta=1))
        assert m["n_valid"].tolist() == [2, 5]  # finite means valid; only the last one can reach the window
    m = mmr.match(L, (0.0, 0.0), pose, pts, **KW)
    assert m["best"].tolist() == [1, 4, 4, 1] and m["flags"] == mmr.WEAK  # 1 of 5 points: below the gate of 0.5


def test_points_reachable_only_under_some_translations():
    # the point falls 3 cells right of the window (map cells 8..23): shifts of -3 and -4 bring it in
    L = grid_with(32, [(23, 16), (22, 16)])
    m = assert_same_as_naive(L, (0.0, 0.0), at_cell(16, 16), cells((10, 0)), **KW)
    assert m["scores"][1, 4].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    assert m["best"].tolist() == [1, 4, 1, 1] and m["flags"] == 0  # (jx = 1: not on the border)
    m = mmr.match(L, (0.0, 0.0), at_cell(16, 16), cells((12, 0)), **KW)  # k_trans cells out: counted ...
    assert m["flags"] == mmr.EMPTY                                      # ... but no shift reaches a cell
    m = mmr.match(grid_with(32, [(23, 16)]), (0.0, 0.0), at_cell(16, 16), cells((11, 0)), **KW)
    assert m["best"].tolist() == [1, 4, 0, 1] and m["flags"] == mmr.EDGE


def test_gate_at_equality():
    pose = at_cell(16, 16)
    pts = cells((1, 0), (3, 2), (-4, 5), (6, -6))
    kw = dict(KW, min_permille=500)
    m = mmr.match(grid_with(32, [(17, 16), (19, 18)]), (0.0, 0.0), pose, pts, **kw)
    assert m["best"].tolist() == [1, 4, 4, 2] and m["n_valid"].tolist() == [2, 4]
    assert m["flags"] == 0  # 1000 * 2 == 500 * 1 * 4: accepted
    assert np.array_equal(m["pose_out"], pose)  # (the correction is zero)
    m = mmr.match(grid_with(32, [(17, 16)]), (0.0, 0.0), pose, pts, **kw)
    assert m["best"][3] == 1 and m["flags"] == mmr.WEAK
    m = mmr.match(grid_with(32, [(17, 16)]), (0.0, 0.0), pose, pts, **dict(kw, min_permille=250))
    assert m["flags"] == 0
    m = mmr.match(grid_with(32, [(17, 16)]), (0.0, 0.0), pose, pts, **dict(kw, min_permille=251))
    assert m["flags"] == mmr.WEAK
    # with a smear the full score of a point is smear + 1
    m = mmr.match(grid_with(32, [(17, 16), (19, 18)]), (0.0, 0.0), pose, pts, **dict(kw, smear=2))
    assert m["best"][3] == 6 and m["flags"] == 0
    m = mmr.match(grid_with(32, [(17, 16), (19, 19)]), (0.0, 0.0), pose, pts, **dict(kw, smear=2))
    assert m["best"][3] == 5 and m["flags"] == mmr.WEAK
    # min_permille 0 accepts any non-zero score, 1000 only a perfect one
    m = mmr.match(grid_with(32, [(17, 16)]), (0.0, 0.0), pose, pts, **dict(kw, min_permille=0))
    assert m["flags"] == 0
    full = grid_with(32, [(17, 16), (19, 18), (12, 21), (22, 10)])
    assert mmr.match(full, (0.0, 0.0), pose, pts, **dict(kw, min_permille=1000))["flags"] == 0


def test_accepted_pose_is_the_guess_plus_delta():
    L = grid_with(32, [(18, 17), (19, 17), (18, 19)])
    pose = at_cell(16, 16)
    m = mmr.match(L, (0.0, 0.0), pose, cells((1, 1), (2, 1), (1, 3)), **KW)
    assert m["flags"] == 0 and m["best"].tolist() == [1, 4, 5, 3]
    assert m["pose_out"].tolist() == [1750.0, 1650.0, 0.0]


# ---- ABI, no device ----

def test_mapmatch_params_default():
    p = _lib.mapmatch_params()
    got = {k: getattr(p, k) for k in ("theta_step", "win_w", "smear", "k_trans", "k_theta", "occ_min", "min_permille")}
    assert got == dict(theta_step=np.pi / 360, win_w=512, smear=2, k_trans=10, k_theta=20, occ_min=85, min_permille=500)
    assert {k: mmr.DEFAULTS[k] for k in got} == got
    assert mmr.DEFAULTS["cell"] == _lib.grid_params().cell and mmr.DEFAULTS["grid_w"] == _lib.grid_params().grid_w
    assert (_lib.MAPMATCH_EMPTY, _lib.MAPMATCH_EDGE, _lib.MAPMATCH_BAD_POSE, _lib.MAPMATCH_WEAK) == (1, 2, 4, 8)
    assert (mmr.EMPTY, mmr.EDGE, mmr.BAD_POSE, mmr.WEAK) == (1, 2, 4, 8)
    assert _lib.K_MAPMATCH == 11 and _lib.ABI_VERSION == 6


def test_mapmatch_struct_sizes():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_mapmatch_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.MapMatchParams) == 32
    assert got[1] == C.sizeof(_lib.MapMatchBatch) == 112
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_mapmatch_abi_sizes(one, 1) == 2 and list(one) == [32, -1]
    assert L.lslam_mapmatch_abi_sizes(None, 2) == 2
    two, nine = (C.c_int64 * 2)(), (C.c_int64 * 9)()
    assert L.lslam_grid_abi_sizes(two, 2) == 2 and list(two) == [40, 72]  # the earlier tables are as they were
    assert L.lslam_abi_sizes(nine, 9) == 9


def call(b, g, m):
    L = _lib.load()
    st = L.lslam_map_match(None, None if b is None else C.byref(b), None if g is None else C.byref(g),
                           None if m is None else C.byref(m))
    return st, L.lslam_last_error()


BAD_FIELDS = [("theta_step", 0.0), ("theta_step", -1.0), ("theta_step", float("nan")), ("theta_step", float("inf")),
              ("win_w", 14), ("win_w", 514), ("win_w", 129), ("smear", -1), ("smear", 3), ("k_trans", -1), ("k_trans", 16),
              ("k_theta", -1), ("k_theta", 32), ("occ_min", -32769), ("occ_min", 32768), ("min_permille", -1),
              ("min_permille", 1001)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_mapmatch_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    b = _lib.MapMatchBatch()
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params())
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg  # valid parameters, an empty batch: only the context is missing
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(**{field: value}))
    assert st == _lib.LSLAM_ERR_ARG and field.encode() in msg


@pytest.mark.parametrize("field,value", [("cell", 0.0), ("cell", float("nan")), ("grid_w", 15), ("grid_w", 2049),
                                         ("max_range", 0.0), ("l_hit", 0)])
def test_mapmatch_checks_the_grid_params_as_the_grid_update_does(field, value):
    st, msg = call(_lib.MapMatchBatch(), _lib.grid_params(**{field: value}), _lib.mapmatch_params())
    assert st == _lib.LSLAM_ERR_ARG and field.encode() in msg


def test_mapmatch_accepts_the_ends_of_the_ranges():
    b = _lib.MapMatchBatch()
    for kw in (dict(win_w=16, smear=0, k_trans=0, k_theta=0, occ_min=-32768, min_permille=0, theta_step=1e-300),
               dict(win_w=512, smear=2, k_trans=15, k_theta=31, occ_min=32767, min_permille=1000, theta_step=1e300)):
        for gkw in (dict(grid_w=16), dict(grid_w=2048)):
            st, msg = call(b, _lib.grid_params(**gkw), _lib.mapmatch_params(**kw))
            assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg, (kw, gkw)


INPUTS = ("xy", "pt_off", "pose", "origin", "logodds", "rot")
OUTPUTS = ("pose_out", "delta", "best", "n_valid", "rot0", "flags")


def test_mapmatch_missing_pointers():
    g, m = _lib.grid_params(), _lib.mapmatch_params()

    def batch(without=None):
        b = _lib.MapMatchBatch()
        b.n_robots = 1
        for f in INPUTS + OUTPUTS:
            if f != without:
                setattr(b, f, 4096)
        return b

    for f in INPUTS:
        st, msg = call(batch(f), g, m)
        assert st == _lib.LSLAM_ERR_ARG and b"missing input" in msg and f.encode() in msg, f
    for f in OUTPUTS:
        st, msg = call(batch(f), g, m)
        assert st == _lib.LSLAM_ERR_ARG and b"missing output" in msg and f.encode() in msg, f
    st, msg = call(batch(), g, m)  # scores is optional: only the context is missing
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg
    b = batch()
    b.n_robots = -1
    assert call(b, g, m)[0] == _lib.LSLAM_ERR_ARG
    assert call(None, g, m)[0] == _lib.LSLAM_ERR_ARG
    assert call(batch(), None, m)[0] == _lib.LSLAM_ERR_ARG
    assert call(batch(), g, None)[0] == _lib.LSLAM_ERR_ARG
