"""The Gauss-Newton alignment in the distance field (include/lidarslam.h, lslam_field_align) on the
CPU: tests/fieldalign_ref.py against a plain float64 Gauss-Newton, a hand-made case per rule of the
definition, what the alignment is worth on the five-revolution room of test_occgrid_ref, and the ABI
checks that need no device.  tests/test_gpu_fieldalign.py holds the kernel to the reference bit for bit
and repeats the room's cap on the device's own grid.

The quantisation bound (test_against_plain_gauss_newton).  The reference sums each of the ten terms as
rint(t 2^20): a term moves by at most 2^-21, a sum of n <= 2^16 used points by at most e = n 2^-21
(<= 2^-5).  Let H d = -g be the plain, damped system and (H + dH) d' = -(g + dg) the quantised one, every
entry of dH and dg at most e in magnitude: ||dH||_2 <= ||dH||_F <= 3 e and ||dg||_2 <= sqrt(3) e.  Then
d' - d = -(H + dH)^-1 (dg + dH d), so with lmin the smallest eigenvalue of H,
    ||d' - d||_2 <= (sqrt(3) e + 3 e ||d||_2) / (lmin - 3 e),
in the units of d (cells, cells, rad).  The plain solver's own rounding (a different order of the same
float64 operations) is far below that: 1e-9 (1 + ||d||) is added for it.  Nothing here is taken from
what the reference gives.

The room.  Robots 200-207, ROOM_KW, ROOM_ORIGIN, the map built at the true poses, occ_min 85, d_max 128,
the fifth revolution, the defaults of lslam_fieldalign_params.  The true step-4 poses displaced by
(30, -25) mm and 0.01 rad, and by (-30, 30) mm (one and a half cells) and 0.03 rad.  Measured on the
reference, per robot, the error to the true pose after the alignment:
  * first displacement: 1.5 .. 4.1 mm and 0.06 .. 2.51 mrad, 5 .. 10 steps, seven of eight CONVERGED;
  * second displacement: 1.5 .. 4.1 mm and 0.06 .. 2.51 mrad, 6 .. 10 steps, seven of eight CONVERGED;
no robot sets a rejecting flag.  tests/mapmatch_ref.py from the same guesses (printed beside them by
test_room): 0.4 .. 4.1 mm and 0.10 .. 1.82 mrad from the first, 1.2 .. 3.1 mm and 0.26 .. 2.43 mrad from
the second.  The cap: the reference's worst, 4.1 mm, plus the margin that
test_fieldscore_ref.assert_room_caps allows a clearance, half a cell diagonal and the 5 mm of range
noise: 4.1 + 14.2 + 5 = 23.3 mm; for the heading the worst, 2.6 mrad, plus that margin seen from the
1500 mm between the room's centre and its nearer walls, 19.2 / 1500 = 12.8 mrad: 15.4 mrad.
"""
import ctypes as C
import math

import numpy as np
import pytest

import dist_ref as dr
import fieldalign_ref as far
import mapmatch_ref as mmr
from lidar_slam_amd import _lib
from test_fieldscore_ref import ROOM_DIST
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, build_room, room_run

KW = dict(grid_w=32, cell=100.0, max_range=3000.0)
ROOM_DISPLACEMENTS = ((30.0, -25.0, 0.01), (-30.0, 30.0, 0.03))
ROOM_CAP_MM = 4.1 + 0.5 * math.hypot(20.0, 20.0) + 5.0
ROOM_CAP_RAD = 2.6e-3 + (0.5 * math.hypot(20.0, 20.0) + 5.0) / 1500.0


def assert_room_align(align_fn, poses_true):
    """align_fn(guesses [R, 3]) -> dict(pose_out, flags, iters, ..), the reference here and the device in
    test_gpu_fieldalign.  The caps of the module's docstring."""
    for disp in ROOM_DISPLACEMENTS:
        out = align_fn(poses_true + np.array(disp))
        err = out["pose_out"] - poses_true
        mm, rad = np.hypot(err[:, 0], err[:, 1]), np.abs(err[:, 2])
        print("displaced by", disp, "error mm", mm.round(2), "mrad", (1e3 * rad).round(3), "iters", out["iters"],
              "flags", out["flags"])
        assert not (out["flags"] & far.KEEP).any(), out["flags"]
        assert np.all(mm <= ROOM_CAP_MM) and np.all(rad <= ROOM_CAP_RAD), (mm, rad)


@pytest.fixture(scope="module")
def room():
    poses, revs = room_run()
    L = build_room(poses, revs)
    d2, _, flags = dr.field_batch(L, **ROOM_DIST)
    assert not flags.any()
    return poses, revs, L, d2


def test_room(room):
    poses, revs, L, d2 = room
    rev = revs[4]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    origin = np.tile(ROOM_ORIGIN, (len(ROOM_ROBOTS), 1))
    assert_room_align(lambda guess: far.align_batch(d2, rev["xy"], off, guess, None, origin, ROOM_KW), poses[4])
    for disp in ROOM_DISPLACEMENTS:  # the correlative matcher from the same guesses, for DESIGN's table
        m = mmr.match_batch(L, origin, poses[4] + np.array(disp), rev["xy"], off, **ROOM_KW)
        err = m["pose_out"] - poses[4]
        print("mapmatch_ref from", disp, "error mm", np.hypot(err[:, 0], err[:, 1]).round(2), "mrad",
              (1e3 * np.abs(err[:, 2])).round(3), "flags", m["flags"])


def plain_step(d2, x, y, pose, origin, cell, trunc, damp_t, damp_r):
    """One Gauss-Newton step in float64 with nothing quantised: the textbook bilinear weights on the same
    corner distances, np.linalg.solve.  -> (delta (3,), H damped, points used)."""
    W = d2.shape[0]
    px, py, th = pose
    c, s = np.cos(th), np.sin(th)
    rx, ry = c * x - s * y, s * x + c * y
    u, v = (px + rx - origin[0]) / cell - 0.5, (py + ry - origin[1]) / cell - 0.5
    ix, iy = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    on = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= W - 2)
    rx, ry, u, v, ix, iy = (a[on] for a in (rx, ry, u, v, ix, iy))
    fu, fv = u - ix, v - iy
    d00, d10, d01, d11 = (far.DQ[d2[iy + j, ix + i]] for j, i in ((0, 0), (0, 1), (1, 0), (1, 1)))
    m = (1 - fu) * (1 - fv) * d00 + fu * (1 - fv) * d10 + (1 - fu) * fv * d01 + fu * fv * d11
    gx = (1 - fv) * (d10 - d00) + fv * (d11 - d01)
    gy = (1 - fu) * (d01 - d00) + fu * (d11 - d10)
    keep = m <= trunc
    J = np.stack([gx, gy, (gy * rx - gx * ry) / cell], -1)[keep]
    H = J.T @ J + np.diag([damp_t, damp_t, damp_r])
    return np.linalg.solve(H, -(J.T @ m[keep])), H, int(keep.sum())


def test_against_plain_gauss_newton(room):
    """Every step that the reference takes in the room, from both displacements, against the plain step
    from the same pose: within the module docstring's bound."""
    poses, revs, L, d2 = room
    rev = revs[4]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    q = far.DEFAULTS
    worst = 0.0
    for r in range(len(ROOM_ROBOTS)):
        x, y = far.used_points(rev["xy"][off[r]:off[r + 1]], 8000.0)
        for disp in ROOM_DISPLACEMENTS:
            out = far.align(d2[r], rev["xy"][off[r]:off[r + 1]], poses[4][r] + np.array(disp), None, ROOM_ORIGIN, ROOM_KW)
            assert out["iters"] >= 5 and len(out["deltas"]) == out["iters"]
            for k, delta in enumerate(out["deltas"]):
                want, H, n = plain_step(d2[r].astype(np.int64), x, y, out["trace"][k, :3], ROOM_ORIGIN, 20.0, q["trunc"],
                                        q["damp_t"], q["damp_r"])
                assert 16 <= n <= 2 ** 16
                e = n * 2.0 ** -21
                lmin = np.linalg.eigvalsh(H)[0]
                norm = np.linalg.norm(want)
                bound = (math.sqrt(3.0) * e + 3.0 * e * norm) / (lmin - 3.0 * e) + 1e-9 * (1.0 + norm)
                diff = np.linalg.norm(np.array(delta) - want)
                worst = max(worst, diff / bound)
                assert lmin > 3.0 * e and diff <= bound, (r, disp, k, diff, bound)
    print("largest share of the bound", worst)


def flat(value, W=32):
    return np.full((W, W), value, np.int64)


def test_fu_zero_and_the_cell_centre_convention():
    """A field value belongs to its cell's centre: a point on the centre of cell (10, 12) has fu = fv = 0
    exactly and reads that cell's distance alone; gx and gy are the differences to the next cells."""
    d2 = flat(400)
    d2[12, 10], d2[12, 11], d2[13, 10], d2[13, 11] = 9, 16, 25, 36
    x, y = np.array([1050.0 - 500.0]), np.array([1250.0 - 700.0])
    t = far.point_terms(d2, x, y, 500.0, 700.0, 1.0, 0.0, 0.0, 0.0, 0.01, 25.0)
    assert (t["ix"][0], t["iy"][0], t["fu"][0], t["fv"][0]) == (10, 12, 0.0, 0.0)
    assert (t["m"][0], t["gx"][0], t["gy"][0]) == (3.0, 1.0, 2.0) and t["used"][0]
    assert t["jt"][0] == (2.0 * 550.0 - 1.0 * 550.0) * 0.01
    assert t["terms"][0].tolist() == [int(v * 2 ** 20) for v in (1.0, 2.0, 5.5, 4.0, 11.0, 30.25, 3.0, 6.0, 16.5, 9.0)]
    # a quarter of a cell further along x: fu = 0.25, m = 3 + 0.25, gy between the two columns' differences
    t = far.point_terms(d2, x + 25.0, y, 500.0, 700.0, 1.0, 0.0, 0.0, 0.0, 0.01, 25.0)
    assert (t["fu"][0], t["fv"][0], t["m"][0], t["gx"][0], t["gy"][0]) == (0.25, 0.0, 3.25, 1.0, 2.0)
    # dq floors: isqrt(65536 * 2) / 256 = 362 / 256
    assert far.DQ[2] == 362.0 / 256.0 and far.DQ[65025] == 255.0 and far.DQ[0] == 0.0


def test_corners_off_the_map_are_skipped():
    d2 = flat(4)
    # cell centres lie at 50, 150, .. 3150: u < 0 below 50 and iu = W - 1 from 3150 on
    x = np.array([49.0, 50.0, 3149.0, 3150.0, 1000.0, 1000.0, 1000.0])
    y = np.array([1000.0, 1000.0, 1000.0, 1000.0, 49.0, 3149.99, 3150.0])
    t = far.point_terms(d2, x, y, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.01, 25.0)
    assert t["ix"].tolist() == [0, 30, 9] and t["iy"].tolist() == [9, 9, 30]
    out = far.align(d2, np.stack([x, y], -1), (0.0, 0.0, 0.0), None, (0.0, 0.0), dict(KW, max_range=8000.0), min_points=0)
    assert out["n_used"].tolist() == [3, 3, 7]


def test_trunc_is_inclusive():
    d2 = flat(9)  # m = 3.0 exactly, wherever the point lies
    x, y = np.array([1000.0, 1234.5]), np.array([1000.0, 777.25])
    at = far.point_terms(d2, x, y, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.01, 3.0)
    above = far.point_terms(d2, x, y, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.01, math.nextafter(3.0, 0.0))
    assert at["m"].tolist() == [3.0, 3.0] and at["used"].all() and not above["used"].any()
    assert at["terms"][:, 9].tolist() == [9 << 20] * 2 and not above["terms"].any()


def ring(n, radius, phase=0.1):
    a = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a)], -1)


def test_empty_field_converges_at_once():
    """No gradient: every sum of J is zero, the step is exactly zero and CONVERGED comes with the first."""
    d2 = flat(16 * 16)
    pose = (1600.0, 1500.0, 0.3)
    out = far.align(d2, ring(40, 800.0), pose, None, (0.0, 0.0), KW)
    assert (out["flags"], out["iters"]) == (far.CONVERGED, 1) and out["deltas"] == [(-0.0, -0.0, -0.0)]
    assert out["pose_out"].tolist() == list(pose) and np.array_equal(out["trace"][1, :3], pose) and not out["trace"][2:].any()
    assert out["normal"][:9].tolist() == [0] * 9 and out["normal"][9] == 40 * 256 << 20 and out["n_used"].tolist() == [40, 40, 40]
    # with trunc below d_max every point is skipped: FEW, or with min_points 0 still CONVERGED; WEAK either way
    assert far.align(d2, ring(40, 800.0), pose, None, (0.0, 0.0), KW, trunc=15.0)["flags"] == far.FEW | far.WEAK
    out = far.align(d2, ring(40, 800.0), pose, None, (0.0, 0.0), KW, trunc=15.0, min_points=0)
    assert out["flags"] == far.CONVERGED | far.WEAK and out["n_used"].tolist() == [0, 0, 40]


def corridor_field(W=32):
    L = np.full((W, W), -100, np.int16)
    L[6, :] = L[25, :] = 200  # two walls along x
    return dr.field(L, d_max=16)[0].astype(np.int64)


def test_corridor_does_not_move_along_the_walls():
    """The field depends on y alone: gx is exactly 0, the damped system decouples, and x never moves."""
    d2 = corridor_field()
    pts = np.array([[dx, wy] for dx in np.arange(-900.0, 901.0, 150.0) for wy in (650.0 - 1600.0, 2550.0 - 1600.0)])
    pose = (1600.0, 1600.0 + 60.0, 0.0)  # the walls' centres lie at y = 650 and 2550: the guess is 60 mm off
    out = far.align(d2, pts, pose, None, (0.0, 0.0), KW)
    assert not out["flags"] & far.KEEP and out["iters"] >= 1
    assert np.all(out["trace"][:out["iters"] + 1, 0] == 1600.0) and all(d[0] == 0.0 for d in out["deltas"])
    assert out["normal"][[0, 1, 2, 6]].tolist() == [0, 0, 0, 0] and out["normal"][3] > 0
    assert abs(out["pose_out"][1] - 1600.0) < 10.0 and abs(out["pose_out"][2]) < 0.01, out["pose_out"]


def test_flags():
    d2 = corridor_field()
    pts = np.array([[dx, wy] for dx in np.arange(-900.0, 901.0, 150.0) for wy in (650.0 - 1600.0, 2550.0 - 1600.0)])
    pose = (1600.0, 1660.0, 0.0)
    run = lambda p=pose, pts=pts, d2=d2, **kw: far.align(d2, pts, p, None, (0.0, 0.0), KW, **kw)
    # FEW: 26 points
    out = run(min_points=27)
    assert (out["flags"], out["iters"]) == (far.FEW, 0) and out["pose_out"].tolist() == list(pose) and out["normal"][3] > 0
    assert run(min_points=26)["flags"] & far.FEW == 0
    # SINGULAR: without damping the corridor's x has no pivot
    out = run(damp_t=0.0, damp_r=0.0)
    assert (out["flags"], out["iters"]) == (far.SINGULAR, 0) and out["pose_out"].tolist() == list(pose)
    assert not out["trace"][1:].any() and out["trace"][0].tolist() == [1600.0, 1660.0, 0.0, 1.0, 0.0]
    # DIVERGED: the alignment moves by some 60 mm; the gate is per axis
    out = run(max_shift=20.0)
    assert out["flags"] & far.DIVERGED and out["pose_out"].tolist() == list(pose) and abs(out["trace"][out["iters"], 1] - 1600.0) < 10.0
    assert run(p=(1600.0, 1660.0, 0.02), max_turn=0.0)["flags"] & far.DIVERGED and not run(max_shift=math.inf, max_turn=math.inf)["flags"] & far.DIVERGED
    # WEAK: two of 28 points lie 8 cells from a wall, beyond trunc 5
    far_pts = np.concatenate([pts, [[0.0, -150.0], [100.0, -150.0]]])
    out = run(pts=far_pts, trunc=5.0, min_permille=1000)
    assert out["flags"] & far.WEAK and out["n_used"].tolist() == [26, 26, 28] and out["pose_out"].tolist() == list(pose)
    assert not run(pts=far_pts, trunc=5.0, min_permille=900)["flags"] & far.KEEP
    # BAD_POSE: by lslam_grid_update's rule; pose_out keeps the bits
    for bad in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, np.nan), (1e9, 0.0, 0.0)):
        out = run(p=bad)
        assert out["flags"] == far.BAD_POSE and out["pose_out"].tobytes() == np.array(bad).tobytes()
        assert not out["trace"].any() and not out["normal"].any() and not out["n_used"].any() and out["iters"] == 0
    out = far.align(d2, pts, pose, None, (np.nan, 0.0), KW)
    assert out["flags"] == far.BAD_POSE


def test_n_iter_bounds_the_steps():
    d2 = corridor_field()
    pts = np.array([[dx, wy] for dx in np.arange(-900.0, 901.0, 150.0) for wy in (650.0 - 1600.0, 2550.0 - 1600.0)])
    for n_iter in (1, 2, 32):
        out = far.align(d2, pts, (1600.0, 1660.0, 0.02), None, (0.0, 0.0), KW, n_iter=n_iter, eps_t=0.0, eps_r=0.0)
        assert out["iters"] == n_iter and out["trace"].shape == (n_iter + 1, 5) and out["trace"][n_iter, 3] != 0.0
        assert not out["flags"] & far.CONVERGED


def test_information():
    normal = np.arange(1, 11, dtype=np.int64)[None] << 20
    H, g = far.information(normal)
    assert H[0].tolist() == [[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]] and g[0].tolist() == [7.0, 8.0, 9.0]


# ---- the ABI checks that need no device ----

def test_params_default_and_struct_sizes():
    p = _lib.fieldalign_params()
    got = {k: getattr(p, k) for k in far.DEFAULTS}
    assert got == far.DEFAULTS and p.reserved == 0
    assert p.trunc ** 2 == _lib.fieldscore_params().trunc2
    sizes = (C.c_int64 * 2)()
    assert _lib.load().lslam_fieldalign_abi_sizes(sizes, 2) == 2
    assert list(sizes) == [C.sizeof(_lib.FieldAlignParams), C.sizeof(_lib.FieldAlignBatch)] == [72, 96]
    assert (_lib.FIELDALIGN_BAD_POSE, _lib.FIELDALIGN_CONVERGED, _lib.FIELDALIGN_SINGULAR, _lib.FIELDALIGN_FEW,
            _lib.FIELDALIGN_DIVERGED, _lib.FIELDALIGN_WEAK) == (far.BAD_POSE, far.CONVERGED, far.SINGULAR, far.FEW,
                                                                far.DIVERGED, far.WEAK)


BAD_FIELDS = [("trunc", -1.0), ("trunc", 255.5), ("trunc", float("nan")), ("damp_t", -1.0), ("damp_t", float("inf")),
              ("damp_r", -1e-3), ("damp_r", float("nan")), ("eps_t", -1.0), ("eps_r", float("inf")), ("max_shift", -1.0),
              ("max_shift", float("nan")), ("max_turn", -0.1), ("n_iter", 0), ("n_iter", 33), ("min_points", -1),
              ("min_permille", -1), ("min_permille", 1001)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_validation_needs_no_device(field, value):
    L = _lib.load()
    b, g = _lib.FieldAlignBatch(), _lib.grid_params()
    st = L.lslam_field_align(None, C.byref(b), C.byref(g), C.byref(_lib.fieldalign_params(**{field: value})))
    assert st == _lib.LSLAM_ERR_ARG and field in L.lslam_last_error().decode()


def test_accepts_the_ends_of_the_ranges_and_names_missing_pointers():
    L = _lib.load()
    g = _lib.grid_params()
    ends = dict(trunc=0.0, damp_t=0.0, damp_r=0.0, eps_t=0.0, eps_r=0.0, max_shift=float("inf"), max_turn=float("inf"),
                n_iter=32, min_points=0, min_permille=1000)
    for kw in (ends, dict(trunc=255.0, n_iter=1, max_shift=0.0, max_turn=0.0, min_permille=0)):
        # (an empty batch: the parameters are checked, then the missing context is named)
        st = L.lslam_field_align(None, C.byref(_lib.FieldAlignBatch()), C.byref(g), C.byref(_lib.fieldalign_params(**kw)))
        assert st == _lib.LSLAM_ERR_ARG and b"ctx is NULL" in L.lslam_last_error()
    p = _lib.fieldalign_params()
    assert L.lslam_field_align(None, None, C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG and b"batch is NULL" in L.lslam_last_error()
    assert L.lslam_field_align(None, C.byref(_lib.FieldAlignBatch()), C.byref(g), None) == _lib.LSLAM_ERR_ARG
    assert b"params is NULL" in L.lslam_last_error()
    b = _lib.FieldAlignBatch()
    b.n_robots = -1
    assert L.lslam_field_align(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG and b"negative" in L.lslam_last_error()
    names = ("xy", "pt_off", "pose", "origin", "d2", "pose_out", "trace", "normal", "n_used", "iters", "flags")
    for missing in names:
        b = _lib.FieldAlignBatch()
        b.n_robots = 1
        for n in names:
            if n != missing:
                setattr(b, n, 4096)
        assert L.lslam_field_align(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
        assert missing.encode() in L.lslam_last_error() and b"missing" in L.lslam_last_error()
    bad_grid = _lib.grid_params(cell=0.0)
    assert L.lslam_field_align(None, C.byref(_lib.FieldAlignBatch()), C.byref(bad_grid), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"cell" in L.lslam_last_error()
