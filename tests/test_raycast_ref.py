"""The grid ray-cast definition (include/lidarslam.h, lslam_grid_raycast) on the CPU: every rule on
hand-made maps, the classes it gives in the synthetic room, and the ABI checks that need no device.
tests/raycast_ref.py is the NumPy form of the definition; tests/test_gpu_raycast.py holds the kernel
to it bit for bit, tests/test_raycast_walk.py the kernel's per-beam header to a brute-force walk
(n = 0, a far cell equal to the robot cell, cannot come out of step 2, whose far cell lies at least
two cells away: that case is the header test's).

The room.  The five-revolution map of test_occgrid_ref.build_room at the true poses (robots 200-207,
grid_w 256 at 20 mm); the fifth revolution is classed against it with the defaults (occ_min 1,
free_max -1, tol 3).  Over the eight robots' 5760 beams the reference gives, at the true poses,
  MATCH share m_ref = 0.9599 (worst robot 0.9472), NOVEL + THROUGH share e_ref = 0.0300 (worst 0.0375);
the other 1.0 % are UNMAPPED, stopped by a cell that was never seen.  m_ref is above 0.9, so the
default tol stands.
The poses moved by 10 mm and pi/720 rad (test_occgrid_ref.moved) must keep MATCH >= m_ref - 0.03 and
NOVEL + THROUGH <= e_ref + 0.02 (measured 0.9597 and 0.0319); the margins cover walls that are one to
two cells thick.  Controls: a 30-beam sector (the robot's nearest wall) shortened to 60 % turns
>= 90 % NOVEL, lengthened to 1.5 x (inside max_range) >= 90 % THROUGH (measured 100 % both, and for
every other robot's such sector at least 29 of 30); a pose 700 mm and 0.5 rad off has at least 5 x
the inconsistency of the true one (measured: at least 0.854 against at most 0.038).

Why the defaults are 1 and -1.  With the matchers' occ_min = 85 (one hit) and free_max = -41 (one
pass) the same map gives MATCH 0.6931 and 28.5 % UNMAPPED: beside a wall the cells hold one hit and
one to three passes (L = 44, 3, -38), inside the band (-41, 85), so the ray stops at an unknown cell a
step or two in front of the wall, and a beam that an unknown cell stops can be neither MATCH nor
THROUGH (the lengthened control then gives 26 of 30).  tol does not reach it: tol = 64, the end of
its range, gives 0.7045 (test_room_with_the_matchers_thresholds).  A cell with any net evidence is
therefore read: p > 0.5 occupied, p < 0.5 free, L = 0 unknown."""
import ctypes as C

import numpy as np
import pytest

import raycast_ref as rcr
from lidar_slam_amd import _lib
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, build_room, moved, room_run

M_REF, E_REF = 0.9599, 0.0300  # the reference's shares at the true poses (docstring)

KW = dict(grid_w=32, cell=100.0, max_range=3000.0)
POSE = (1050.0, 1050.0, 0.0)  # robot cell (10, 10), heading +x, on its cell's centre
FREE, UNK, OCCV = -100, 0, 200


def one(L, pts, pose=POSE, **kw):
    k = dict(KW)
    k.update(kw)
    cls, stop, counts, flags = rcr.cast(L, np.asarray(pts, np.float64).reshape(-1, 2), pose, None, (0.0, 0.0), **k)
    return (cls & 15).tolist(), (cls >> 4).tolist(), stop.tolist(), counts.tolist(), flags


def free_map(wall_x=None):
    L = np.full((32, 32), FREE, np.int16)
    if wall_x is not None:
        L[:, wall_x] = OCCV
    return L


def test_stop_order_cap_before_cell():
    # max_range 500: Rc = 5, far = 700, the ray along +x has n = 7; the cap fires at ox = 6
    for wall, want in ((16, (rcr.NONE, [6, 0, 6])), (15, (rcr.OCC, [5, 0, 5])), (17, (rcr.NONE, [6, 0, 6]))):
        c, k, s, _, _ = one(free_map(wall), [[300.0, 0.0]], max_range=500.0)
        assert (k[0], s[0]) == want, (wall, k, s)
    # the unknown cell too comes after the cap
    L = free_map()
    L[10, 16] = UNK
    assert one(L, [[300.0, 0.0]], max_range=500.0)[1:3] == ([rcr.NONE], [[6, 0, 6]])
    L[10, 15] = UNK
    assert one(L, [[300.0, 0.0]], max_range=500.0)[1:3] == ([rcr.UNKNOWN], [[5, 0, 5]])


@pytest.mark.parametrize("tol", [0, 3])
def test_tol_edges(tol):
    L = free_map(18)  # the map stops the +x beam at i_h = 8
    steps = [8 - tol - 1, 8 - tol, 8, 8 + tol, 8 + tol + 1]
    c, k, s, counts, flags = one(L, [[100.0 * i, 0.0] for i in steps], tol=tol)
    assert k == [rcr.OCC] * 5 and s == [[8, 0, 8]] * 5 and flags == 0
    assert c == [rcr.NOVEL, rcr.MATCH, rcr.MATCH, rcr.MATCH, rcr.THROUGH]
    assert counts == [0, 3, 1, 1, 0, 0, 0, 0]
    # an unknown stop: early is NOVEL, everything else UNMAPPED
    L[:, 18] = UNK
    c, k, _, counts, _ = one(L, [[100.0 * i, 0.0] for i in steps], tol=tol)
    assert k == [rcr.UNKNOWN] * 5 and c == [rcr.NOVEL] + [rcr.UNMAPPED] * 4
    # no stop inside the range circle (max_range 800: Rc = 8, the cap fires at i_h = 9)
    steps = [9 - tol - 1, 9 - tol, 9]  # (the last is beyond)
    c, k, s, counts, _ = one(free_map(), [[0.0, 100.0 * i] for i in steps], tol=tol, max_range=800.0)
    assert k == [rcr.NONE] * 3 and s == [[0, 9, 9]] * 3 and c == [rcr.NOVEL, rcr.MATCH, rcr.MATCH]
    assert counts[:5] == [0, 2, 1, 0, 0] and counts[5] == steps.count(9) and counts[6:] == [3, 0]


def test_beyond_points_under_each_kind():
    L = free_map(18)
    # +x: the wall (OCC); -x: the ray leaves the map at ox = -11 (UNKNOWN); +y with max_range 800: NONE
    c, k, s, counts, _ = one(L, [[3500.0, 0.0], [-3500.0, 0.0]])
    assert k == [rcr.OCC, rcr.UNKNOWN] and c == [rcr.THROUGH, rcr.UNMAPPED]
    assert s == [[8, 0, 8], [-11, 0, 11]] and counts == [0, 0, 0, 1, 1, 2, 0, 0]
    c, k, s, counts, _ = one(L, [[0.0, 900.0], [0.0, 1e200]], max_range=800.0)
    assert k == [rcr.NONE] * 2 and c == [rcr.MATCH] * 2 and s == [[0, 9, 9]] * 2 and counts == [0, 2, 0, 0, 0, 2, 2, 0]
    # exactly at max_range is not beyond
    assert one(L, [[0.0, 800.0]], max_range=800.0)[3][5] == 0


def test_robot_off_the_map():
    c, k, s, counts, flags = one(free_map(18), [[500.0, 0.0], [3500.0, 0.0]], pose=(-450.0, 1050.0, 0.0))
    assert flags == 0 and k == [rcr.UNKNOWN] * 2 and s == [[0, 0, 0]] * 2
    assert c == [rcr.UNMAPPED] * 2 and counts == [0, 0, 0, 0, 2, 1, 0, 0]


def test_shortest_ray_and_rc_zero():
    # max_range below one cell: Rc = 0, far = 2.5 cells; step 0 is the robot's own cell, step 1 leaves the circle
    c, k, s, _, _ = one(free_map(), [[30.0, 0.0], [0.0, -20.0]], max_range=50.0)
    assert k == [rcr.NONE] * 2 and s == [[1, 0, 1], [0, -1, 1]] and c == [rcr.MATCH] * 2
    L = free_map()
    L[10, 10] = OCCV  # the robot's own cell
    assert one(L, [[30.0, 0.0]], max_range=50.0)[1:3] == ([rcr.OCC], [[0, 0, 0]])


def test_thresholds_at_the_int16_ends():
    L = free_map()
    L[10, 13], L[10, 14] = 32766, 32767
    assert one(L, [[100.0, 0.0]], occ_min=32767, free_max=32766)[1:3] == ([rcr.OCC], [[4, 0, 4]])
    assert one(L, [[100.0, 0.0]], occ_min=32767, free_max=32765)[1:3] == ([rcr.UNKNOWN], [[3, 0, 3]])
    L = np.full((32, 32), -32768, np.int16)
    L[10, 13], L[10, 14] = -32767, -32768
    assert one(L, [[100.0, 0.0]], occ_min=-32767, free_max=-32768)[1:3] == ([rcr.OCC], [[3, 0, 3]])
    assert one(L, [[100.0, 0.0]], occ_min=-32766, free_max=-32768)[1:3] == ([rcr.UNKNOWN], [[3, 0, 3]])
    L[10, 13] = -32768
    L[10, 20] = 32767
    assert one(L, [[100.0, 0.0]], occ_min=32767, free_max=-32768)[1:3] == ([rcr.OCC], [[10, 0, 10]])


def test_invalid_points_and_bad_poses():
    pts = [[np.nan, 1.0], [0.0, 0.0], [1e-310, 0.0], [0.0, -4e-320], [np.inf, 2.0], [400.0, 0.0]]
    c, k, s, counts, flags = one(free_map(18), pts)
    assert c == [0, 0, 0, 0, 0, rcr.NOVEL] and k[:5] == [0] * 5 and s[:5] == [[0, 0, 0]] * 5
    assert counts == [5, 0, 1, 0, 0, 0, 0, 0] and flags == 0
    for pose in [(np.nan, 0.0, 0.0), (0.0, 0.0, np.inf), (100.0 * 2.0 ** 20, 0.0, 0.0)]:
        c, k, s, counts, flags = one(free_map(18), pts, pose=pose)
        assert flags == rcr.BAD_POSE and c == [0] * 6 and s == [[0, 0, 0]] * 6 and counts == [0] * 8


def test_batch_and_helpers():
    L = np.stack([free_map(18), free_map(15)])
    xy = np.array([[400.0, 0.0], [800.0, 0.0], [500.0, 0.0]])
    cls, stop, counts, flags = rcr.cast_batch(L, xy, [0, 2, 3], [POSE, POSE], None, None, **KW)
    assert (cls & 15).tolist() == [rcr.NOVEL, rcr.MATCH, rcr.MATCH] and stop[:, 2].tolist() == [8, 8, 5]
    assert np.array_equal(rcr.expected_range(cls, stop, 100.0), [800.0, 800.0, 500.0])
    assert np.allclose(rcr.inconsistency(counts), [0.5, 0.0])
    cls, stop, counts, flags = rcr.cast_batch(L, xy[:0], [0, 0, 0], [POSE, POSE], None, None, **KW)
    assert cls.size == 0 and stop.shape == (0, 3) and not counts.any()


# ---- the room ----

def shares(counts):
    """(MATCH share, NOVEL + THROUGH share) of all robots' valid beams."""
    c = np.asarray(counts, np.int64).sum(0)
    valid = c[1:5].sum()
    return c[rcr.MATCH] / valid, (c[rcr.NOVEL] + c[rcr.THROUGH]) / valid


def room_cast(L, rev, poses, rot=None, **kw):
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    return rcr.cast_batch(L, rev["xy"], off, poses, rot, np.tile(ROOM_ORIGIN, (len(ROOM_ROBOTS), 1)), **ROOM_KW, **kw), off


def sector(rev, off, robot=0, n=30):
    """The control sector: the `n` consecutive beams of a robot whose farthest return is nearest, the
    piece of wall the robot sees best (chosen from the revolution alone, before anything is cast)."""
    xy = rev["xy"][off[robot]:off[robot + 1]]
    r = np.hypot(xy[:, 0], xy[:, 1])
    far = np.array([r[i:i + n].max() if np.all(np.isfinite(r[i:i + n])) else np.inf for i in range(len(r) - n + 1)])
    first = int(np.argmin(far))
    assert 1.5 * far[first] < 8000.0
    return off[robot] + first + np.arange(n)


def assert_room_caps(cast_fn, rev, poses_true, poses_moved):
    """cast_fn(xy, poses) -> (cls, counts), the reference here and the device in test_gpu_raycast.
    Returns the shares at the true poses."""
    _, counts0 = cast_fn(rev["xy"], poses_true)
    m0, e0 = shares(counts0)
    _, counts1 = cast_fn(rev["xy"], poses_moved)
    m1, e1 = shares(counts1)
    per = np.asarray(counts0, np.float64)
    print("true poses: MATCH %.4f, NOVEL + THROUGH %.4f (worst robot %.4f, %.4f); moved poses: %.4f, %.4f"
          % (m0, e0, (per[:, 1] / per[:, 1:5].sum(1)).min(), ((per[:, 2] + per[:, 3]) / per[:, 1:5].sum(1)).max(), m1, e1))
    assert m1 >= M_REF - 0.03 and e1 <= E_REF + 0.02, (m1, e1)
    return m0, e0


def assert_control(cast_fn, rev, poses_true, scale, want):
    """The control sector's returns scaled: at least 90 % of it turns `want`, no other beam changes."""
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    idx = sector(rev, off)
    cls0, _ = cast_fn(rev["xy"], poses_true)
    xy = rev["xy"].copy()
    xy[idx] *= scale
    cls, _ = cast_fn(xy, poses_true)
    share = np.mean((cls[idx] & 15) == want)
    print("sector scaled by %.1f: %s share %.3f; its classes %s" % (scale, rcr.CLASS_NAMES[want], share,
                                                                   np.bincount(cls[idx] & 15, minlength=5).tolist()))
    other = np.setdiff1d(np.arange(len(xy)), idx)
    assert np.array_equal(cls[other], cls0[other])  # beams do not depend on one another
    assert share >= 0.9, (scale, share)
    return cls, idx


def assert_far_pose(cast_fn, rev, poses_true, poses_far):
    _, counts0 = cast_fn(rev["xy"], poses_true)
    _, counts2 = cast_fn(rev["xy"], poses_far)
    i0, i2 = rcr.inconsistency(counts0), rcr.inconsistency(counts2)
    print("inconsistency: true poses", i0.round(4), "far poses", i2.round(4))
    assert np.all(i2 >= 5.0 * i0) and np.all(i2 > 0.0), (i0, i2)


@pytest.fixture(scope="module")
def room():
    poses, revs = room_run()
    return poses, revs, build_room(poses, revs)


def far_off(poses, dx=700.0, dy=0.0, dth=0.5):
    out = np.array(poses, np.float64)
    out[:, 0] += dx
    out[:, 1] += dy
    out[:, 2] += dth
    return out


def ref_cast_fn(room):
    poses, revs, L = room

    def cast_fn(xy, p):
        (cls, stop, counts, flags), _ = room_cast(L, dict(revs[4], xy=xy), p)
        assert not flags.any()
        return cls, counts
    return cast_fn


def test_room_caps(room):
    poses, revs, L = room
    m0, e0 = assert_room_caps(ref_cast_fn(room), revs[4], poses[4], moved(poses)[4])
    # the figures the caps are made of: the reference at the true poses
    assert abs(m0 - M_REF) < 5e-4 and abs(e0 - E_REF) < 5e-4, (m0, e0)


def test_room_control_shortened_sector_is_novel(room):
    poses, revs, L = room
    assert_control(ref_cast_fn(room), revs[4], poses[4], 0.6, rcr.NOVEL)


def test_room_control_lengthened_sector_is_through(room):
    poses, revs, L = room
    assert_control(ref_cast_fn(room), revs[4], poses[4], 1.5, rcr.THROUGH)


def test_room_far_pose_is_inconsistent(room):
    poses, revs, L = room
    assert_far_pose(ref_cast_fn(room), revs[4], poses[4], far_off(poses[4]))


def test_room_with_the_matchers_thresholds(room):
    """What the defaults are not (module docstring): with occ_min = 85 and free_max = -41 the cells beside
    a wall are unknown and MATCH stays near 0.7 whatever tol is; the defaults lift it above 0.9."""
    poses, revs, L = room
    for kw, lo, hi in ((dict(occ_min=85, free_max=-41), 0.0, 0.75), (dict(occ_min=85, free_max=-41, tol=64), 0.0, 0.75),
                       (dict(), 0.9, 1.0)):
        (cls, stop, counts, flags), _ = room_cast(L, revs[4], moved(poses)[4], **kw)
        m, e = shares(counts)
        print(kw, "moved poses: MATCH %.4f, NOVEL + THROUGH %.4f" % (m, e))
        assert lo <= m <= hi and e <= 0.05, (kw, m, e)


def test_expected_scan_of_the_room(room):
    """The map rendered as a scan: unit vectors times max_range; the stop cells lie on the walls."""
    poses, revs, L = room
    a = np.arange(360) * (2 * np.pi / 360)
    xy = 8000.0 * np.stack([np.cos(a), np.sin(a)], -1)
    cls, stop, counts, flags = rcr.cast(L[0], xy, poses[4][0], None, ROOM_ORIGIN, **ROOM_KW)
    assert np.all((cls & 15) != rcr.INVALID)  # (the classes mean nothing here: rounding puts some points beyond)
    occ = (cls >> 4) == rcr.OCC
    assert occ.mean() > 0.9
    rng = rcr.expected_range(cls, stop, 20.0)
    # the true range of each direction in the room's outline, from the same pose
    px, py, th = poses[4][0]
    from lidar_slam_amd import synth
    d = np.stack([np.cos(a + th), np.sin(a + th)], -1)
    with np.errstate(divide="ignore"):
        tx = np.where(d[:, 0] > 0, (synth.ROOM_W - px) / d[:, 0], np.where(d[:, 0] < 0, -px / d[:, 0], np.inf))
        ty = np.where(d[:, 1] > 0, (synth.ROOM_H - py) / d[:, 1], np.where(d[:, 1] < 0, -py / d[:, 1], np.inf))
    true = np.minimum(tx, ty)
    err = np.abs(rng[occ] - true[occ])
    print("expected range against the outline: median %.1f mm, 95 %% %.1f mm" % (np.median(err), np.percentile(err, 95)))
    assert np.median(err) <= 40.0 and np.percentile(err, 95) <= 120.0


# ---- ABI ----

def test_raycast_params_default():
    p = _lib.raycast_params()
    assert {k: getattr(p, k) for k in rcr.DEFAULTS} == rcr.DEFAULTS == dict(occ_min=1, free_max=-1, tol=3)
    assert p.reserved == 0
    assert _lib.RAYCAST_BAD_POSE == rcr.BAD_POSE == 1 and _lib.K_RAYCAST == 14 and _lib.ABI_VERSION == 6
    assert (_lib.RAYCAST_INVALID, _lib.RAYCAST_MATCH, _lib.RAYCAST_NOVEL, _lib.RAYCAST_THROUGH,
            _lib.RAYCAST_UNMAPPED) == (rcr.INVALID, rcr.MATCH, rcr.NOVEL, rcr.THROUGH, rcr.UNMAPPED) == (0, 1, 2, 3, 4)
    assert (_lib.RAYCAST_KIND_NONE, _lib.RAYCAST_KIND_UNKNOWN, _lib.RAYCAST_KIND_OCC) == (rcr.NONE, rcr.UNKNOWN, rcr.OCC)


def test_raycast_struct_sizes():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_raycast_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.RaycastParams) == 16
    assert got[1] == C.sizeof(_lib.RaycastBatch) == 88
    one_ = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_raycast_abi_sizes(one_, 1) == 2 and list(one_) == [16, -1]
    assert L.lslam_raycast_abi_sizes(None, 2) == 2
    # the older tables are unchanged
    nine = (C.c_int64 * 9)()
    assert L.lslam_abi_sizes(nine, 9) == 9 and list(nine) == [112, 56, 56, 128, 232, 48, 48, 32, 96]
    for fn, want in ((L.lslam_grid_abi_sizes, [40, 72]), (L.lslam_mapmatch_abi_sizes, [32, 112]),
                     (L.lslam_mapfuse_abi_sizes, [24, 160]), (L.lslam_reloc_abi_sizes, [56, 176])):
        two = (C.c_int64 * 2)()
        assert fn(two, 2) == 2 and list(two) == want


BAD_FIELDS = [("occ_min", 32768), ("occ_min", -32769), ("free_max", 32767), ("free_max", -32769), ("free_max", 85),
              ("free_max", 100), ("tol", -1), ("tol", 65)]
BAD_GRID_FIELDS = [("cell", 0.0), ("max_range", float("inf")), ("grid_w", 2049)]


@pytest.mark.parametrize("field,value", BAD_FIELDS + BAD_GRID_FIELDS)
def test_raycast_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    L = _lib.load()
    b = _lib.RaycastBatch()
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(_lib.grid_params()), C.byref(_lib.raycast_params())) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()  # valid parameters, an empty batch: only the context is missing
    g, p = _lib.grid_params(), _lib.raycast_params()
    setattr(g if (field, value) in BAD_GRID_FIELDS else p, field, value)
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert field.encode() in L.lslam_last_error()


def test_raycast_accepts_the_ends_of_the_ranges():
    L = _lib.load()
    b = _lib.RaycastBatch()
    for kw in (dict(occ_min=32767, free_max=32766, tol=64), dict(occ_min=-32767, free_max=-32768, tol=0)):
        assert L.lslam_grid_raycast(None, C.byref(b), C.byref(_lib.grid_params()), C.byref(_lib.raycast_params(**kw))) == _lib.LSLAM_ERR_ARG
        assert b"ctx" in L.lslam_last_error(), kw


def test_raycast_missing_pointers():
    L = _lib.load()
    g, p = _lib.grid_params(), _lib.raycast_params()
    b = _lib.RaycastBatch()
    b.n_robots = 1
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    b.xy = b.pt_off = b.pose = b.origin = b.logodds = 4096
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing output" in L.lslam_last_error()
    b.cls = b.counts = b.rot = b.flags = 4096  # stop stays NULL: it is optional
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()
    b.n_robots = -1
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_raycast(None, None, C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_raycast(None, C.byref(b), None, C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_raycast(None, C.byref(b), C.byref(g), None) == _lib.LSLAM_ERR_ARG
