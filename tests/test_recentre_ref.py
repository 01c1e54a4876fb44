"""The grid-recentre definition (include/lidarslam.h, lslam_grid_recentre) on the CPU: the NumPy form
tests/recentre_ref.py held to a cell-by-cell loop form, a hand-made case for every rule, the ABI checks
that need no device, and two walks through the synthetic room in which a rolled grid is compared with
fixed, larger grids fed the same revolutions.  tests/test_gpu_recentre.py holds the kernel to
recentre_ref bit for bit; tests/test_recentre_plan.py the kernel's in-place plan to an out-of-place
shift.

The walks.  Three robots with (y, theta, dy) = WALK_ROBOTS drive poses (800 + 200 k, y + dy k,
theta + 0.05 k), k = 0 .. 12, across the 4000 x 3000 mm room; revolution ids 5000 + 100 robot + k;
origin = floor((p0 - W cell / 2) / cell) cell; every step is recentre, then occgrid_ref.update.
  Walk 1: grid_w 256 at 20 mm, max_range 2000, margin 104, quantum 8.  Robot 0 moves at steps 3, 6, 9
    and 12 by (32, 0), (32, 0), (24, 0), (32, 0), the others also in y; CLIPPED is never set, and with
    this margin no cell of the final window was written, scrolled off and came back: the final grid EQUALS the matching
    window of a fixed 512-cell grid (origin (-3120, -3620)) fed the same revolutions.  The scan-to-map
    matcher, run on the rolled grid and origin from the last true pose moved by (60, -40) mm and
    0.03 rad, comes back within 20 mm and pi/360 rad (the caps of test_mapmatch_ref; measured 4.1 mm
    and 0.0018 rad) with flags 0.
  Walk 2: dy = (0, 60, -50), grid_w 128, max_range 1000, margin 32: cells do scroll off.  Each cell of
    the final grid equals the cell of the fixed 256-cell grid (origin (-560, -1060)) that started
    accumulating at the step the cell last entered the window: what scrolls off is lost, what scrolls
    in starts unknown, and nothing else differs."""
import ctypes as C
import functools

import numpy as np
import pytest

import mapmatch_ref as mmr
import occgrid_ref as ogr
import recentre_ref as rr
from lidar_slam_amd import _lib, synth

BAD_POSE, MOVED, CLEARED = rr.BAD_POSE, rr.MOVED, rr.CLEARED


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the loop form ----

def loop_recentre(L, pose, origin, grid_w, cell, margin, quantum):
    """The definition once more, cell by cell and without NumPy's slicing or floor division."""
    W = grid_w
    inv = 1.0 / cell
    vals = [float(v) for v in pose] + [float(v) for v in origin]
    if not all(np.isfinite(v) for v in vals):
        return [row[:] for row in L], list(origin), (0, 0), BAD_POSE
    cells = []
    for p, o in zip(pose[:2], origin):
        f = float(np.floor((float(p) - float(o)) * inv))
        if not abs(f) < 2.0 ** 20:
            return [row[:] for row in L], list(origin), (0, 0), BAD_POSE
        cells.append(int(f))
    if all(margin <= c < W - margin for c in cells):
        return [row[:] for row in L], list(origin), (0, 0), 0
    s = []
    for c in cells:
        t = c - W // 2 + quantum // 2
        m = 0
        while m * quantum > t:
            m -= 1
        while (m + 1) * quantum <= t:
            m += 1
        s.append(m * quantum)
    sx, sy = s
    if sx == 0 and sy == 0:
        return [row[:] for row in L], list(origin), (0, 0), 0
    new = [float(origin[0]) + float(sx) * cell, float(origin[1]) + float(sy) * cell]
    if not all(np.isfinite(v) for v in new):
        return [row[:] for row in L], list(origin), (0, 0), BAD_POSE
    out = [[0] * W for _ in range(W)]
    for y in range(W):
        for x in range(W):
            if 0 <= y + sy < W and 0 <= x + sx < W:
                out[y][x] = L[y + sy][x + sx]
    return out, new, (sx, sy), MOVED | (CLEARED if abs(sx) >= W or abs(sy) >= W else 0)


def test_ref_against_the_loop_form():
    rng = np.random.default_rng(7)
    seen = set()
    for trial in range(300):
        W = int(rng.choice([16, 19, 24, 33]))
        cell = float(rng.choice([20.0, 12.5, 7.3]))
        margin = int(rng.integers(0, W // 2 + 1))
        quantum = int(rng.choice([1, 2, 3, 5, 8, 16, 64]))
        origin = rng.uniform(-500.0, 500.0, 2)
        span = W * cell
        pose = np.concatenate([origin + rng.uniform(-1.2 * span, 2.2 * span, 2), [rng.uniform(-3, 3)]])
        L = rng.integers(-32768, 32768, (W, W)).astype(np.int16)
        got = rr.recentre(L, pose, origin, grid_w=W, cell=cell, margin=margin, quantum=quantum)
        want = loop_recentre(L.tolist(), pose.tolist(), origin.tolist(), W, cell, margin, quantum)
        assert np.array_equal(got[0], np.array(want[0], np.int16)), trial
        assert np.array_equal(bits(got[1]), bits(want[1])), trial
        assert tuple(got[2]) == want[2] and got[3] == want[3], trial
        seen.add(got[3])
    assert seen == {0, MOVED, MOVED | CLEARED}


# ---- a case per rule: cells of 100 mm, W = 32, origin (0, 0); the robot on its cell's centre ----

KW = dict(grid_w=32, cell=100.0, margin=6, quantum=8)


def at_cell(cx, cy, th=0.0):
    return (100.0 * cx + 50.0, 100.0 * cy + 50.0, th)


def one(pose, origin=(0.0, 0.0), L=None, **kw):
    k = dict(KW)
    k.update(kw)
    W = k["grid_w"]
    if L is None:
        L = (np.arange(W * W, dtype=np.int64) - 500).astype(np.int16).reshape(W, W)
    out, new, shift, flags = rr.recentre(L, pose, origin, **k)
    return L, out, new, tuple(int(v) for v in shift), flags


def test_margin_edges():
    W, m = 32, 6
    for c, moves in ((m - 1, True), (m, False), (W - m - 1, False), (W - m, True)):
        for pose in (at_cell(c, 16), at_cell(16, c)):
            L, out, new, shift, flags = one(pose)
            assert (flags == MOVED) == moves and (shift != (0, 0)) == moves, (c, pose, shift, flags)
            if not moves:
                assert flags == 0 and np.array_equal(out, L) and np.array_equal(bits(new), bits((0.0, 0.0)))
    # a trigger on one axis recentres both: the other axis sits 5 cells off the middle, inside the margin
    L, out, new, shift, flags = one(at_cell(W - m, 21))
    assert shift == (8, 8) and flags == MOVED
    L, out, new, shift, flags = one(at_cell(20, 21))
    assert shift == (0, 0) and flags == 0


def test_quantum_rounding():
    """d = c - W/2 from -20 to 20 at quantum 8 (margin W/2: every cell triggers): the multiple of 8
    nearest d, the tie at +-4 going up."""
    for d in range(-20, 21):
        L, out, new, shift, flags = one(at_cell(16 + d, 16 + d), margin=16)
        want = 8 * int(np.floor((d + 4) / 8.0))
        assert shift == (want, want), (d, shift)
        assert abs(d - want) <= 4 and (d - want) != 4
        assert flags == (MOVED if want else 0)
        assert np.array_equal(new, np.array([100.0 * want] * 2))
        assert np.array_equal(out, rr.shifted(L, want, want))
    assert [rr.axis_shift(c, 32, 8) for c in (11, 12, 19, 20)] == [-8, 0, 0, 8]
    assert [rr.axis_shift(c, 33, 3) for c in (14, 15, 16, 17, 18)] == [-3, 0, 0, 0, 3]  # integer halves: 16 and 1


def test_zero_shift_after_a_trigger_writes_nothing():
    # margin 16 = W/2 triggers everywhere; three cells off the middle round to zero at quantum 8
    L, out, new, shift, flags = one(at_cell(19, 13), origin=(0.1, -0.3), margin=16)
    assert shift == (0, 0) and flags == 0
    assert np.array_equal(out, L) and np.array_equal(bits(new), bits((0.1, -0.3)))


def test_bad_poses_are_untouched():
    inf, nan = float("inf"), float("nan")
    cases = [((nan, 1650.0, 0.0), (0.0, 0.0)), ((1650.0, inf, 0.0), (0.0, 0.0)), ((1650.0, 1650.0, nan), (0.0, 0.0)),
             ((1650.0, 1650.0, 0.0), (inf, 0.0)), ((1650.0, 1650.0, 0.0), (0.0, -inf)),
             (at_cell(2 ** 20, 16), (0.0, 0.0)), (at_cell(16, -2 ** 20), (0.0, 0.0))]
    for pose, origin in cases:
        L, out, new, shift, flags = one(pose, origin)
        assert flags == BAD_POSE and shift == (0, 0), (pose, origin)
        assert np.array_equal(out, L) and np.array_equal(bits(new), bits(origin))
    # one cell inside the bound the robot is merely far away: everything scrolls off
    for pose, want in ((at_cell(2 ** 20 - 1, 16), (2 ** 20 - 16, 0)), (at_cell(16, -2 ** 20 + 1), (0, -2 ** 20 - 16))):
        L, out, new, shift, flags = one(pose)
        assert flags == MOVED | CLEARED and shift == want and not out.any(), (pose, shift)
        assert np.array_equal(new, 100.0 * np.array(want, np.float64))


def test_origin_overflow_is_a_bad_pose():
    """fl(s cell) overflows (a cell size no grid accepts, but the rule is the definition's): untouched."""
    big = 1.0e305
    pose = (big * 2000.5, 16.5 * big, 0.0)  # robot cell (2000, 16): s = 1984, 1984e305 is not finite
    with np.errstate(over="ignore"):
        L, out, new, shift, flags = one(pose, cell=big)
    assert flags == BAD_POSE and shift == (0, 0) and np.array_equal(out, L) and np.array_equal(new, (0.0, 0.0))
    # at the largest double the sum absorbs the shift and stays finite: a move, not a bad pose
    o = np.finfo(np.float64).max
    pose = (o, o, 0.0)  # robot cell (0, 0): s = -16
    L, out, new, shift, flags = one(pose, origin=(o, o), margin=16, quantum=1)
    assert flags == MOVED and shift == (-16, -16) and np.all(np.isfinite(new))
    L, out, new, shift, flags = one((-o, -o, 0.0), origin=(-o, -o), margin=16, quantum=1)
    assert flags == MOVED and shift == (-16, -16) and np.array_equal(new, (-o, -o))  # (absorbed, finite)


def test_cleared():
    for (cx, cy), want in (((16 + 32, 16), (32, 0)), ((16, 16 - 32), (0, -32)), ((16 + 31, 16), (31, 0)), ((16 + 40, 16 - 5000), (40, -5000))):
        L, out, new, shift, flags = one(at_cell(cx, cy), margin=16, quantum=1)
        assert shift == want
        cleared = max(abs(want[0]), abs(want[1])) >= 32
        assert flags == (MOVED | (CLEARED if cleared else 0))
        assert out.any() != cleared
        assert np.array_equal(out, rr.shifted(L, *want))
    L = np.arange(1, 32 * 32 + 1, dtype=np.int16).reshape(32, 32)
    assert np.array_equal(rr.shifted(L, 31, -31)[31, 0], L[0, 31]) and np.count_nonzero(rr.shifted(L, 31, -31)) == 1


def test_the_two_roundings_of_the_origin():
    """An origin that is no multiple of the cell: fl(origin + fl(s cell)), not a fused multiply-add."""
    cell, origin, s = 0.1, (0.1, -0.7), 24
    W = 64
    pose = (origin[0] + (W // 2 + s + 0.5) * cell, origin[1] + (W // 2 + 0.5) * cell, 0.0)
    L, out, new, shift, flags = one(pose, origin, grid_w=W, cell=cell, margin=8, quantum=8)
    assert shift == (s, 0) and flags == MOVED
    two = np.float64(0.1) + np.float64(24.0) * np.float64(0.1)  # 2.5000000000000004
    from fractions import Fraction
    fused = float(Fraction(0.1) + Fraction(24) * Fraction(0.1))  # one rounding: 2.5
    assert two != fused, "this case does not tell the two apart"
    assert np.array_equal(bits(new), bits((two, -0.7)))
    assert np.array_equal(out, rr.shifted(L, s, 0))


def test_patterns_survive():
    L = np.array([-32768, 32767, -201, 351, 1, -1, 0, 12345], np.int16).repeat(128).reshape(32, 32)
    _, out, new, shift, flags = one(at_cell(27, 16), L=L)
    assert shift == (8, 0) and np.array_equal(out[:, :24], L[:, 8:]) and not out[:, 24:].any()


def test_batch_form():
    rng = np.random.default_rng(3)
    L = rng.integers(-300, 400, (4, 32, 32)).astype(np.int16)
    pose = np.array([at_cell(16, 16), at_cell(30, 2), (np.nan, 0.0, 0.0), at_cell(3, 16)])
    origin = np.zeros((4, 2))
    out, new, shift, flags = rr.recentre_batch(L, pose, origin, **KW)
    assert flags.tolist() == [0, MOVED, BAD_POSE, MOVED] and shift.tolist() == [[0, 0], [16, -16], [0, 0], [-16, 0]]
    assert shift.dtype == np.int32 and flags.dtype == np.int32 and out.dtype == np.int16 and new.dtype == np.float64
    assert np.array_equal(out[1], rr.shifted(L[1], 16, -16)) and np.array_equal(out[0], L[0]) and np.array_equal(out[2], L[2])


# ---- ABI ----

def test_recentre_params_default_and_constants():
    p = _lib.recentre_params()
    assert {k: getattr(p, k) for k in rr.DEFAULTS} == rr.DEFAULTS == dict(margin=128, quantum=8)
    assert list(p.reserved) == [0, 0]
    assert (_lib.RECENTRE_BAD_POSE, _lib.RECENTRE_MOVED, _lib.RECENTRE_CLEARED) == (BAD_POSE, MOVED, CLEARED) == (1, 2, 4)
    assert _lib.K_RECENTRE == 15 and _lib.ABI_VERSION == 6
    L = _lib.load()
    assert b"(abi 6," in L.lslam_version()
    # LSLAM_K_COUNT is 16: slot 15 exists, slot 16 does not (no device needed: a NULL context is refused first,
    # so the header is the witness)
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lidarslam.h")).read()
    assert re.search(r"LSLAM_K_RECENTRE = 15\b", hdr) and re.search(r"LSLAM_K_COUNT = 16\b", hdr)
    assert re.search(r"#define LSLAM_ABI_VERSION\s+6\b", hdr)


def test_recentre_struct_sizes_and_offsets():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_recentre_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.RecentreParams) == 16
    assert got[1] == C.sizeof(_lib.RecentreBatch) == 48
    one_ = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_recentre_abi_sizes(one_, 1) == 2 and list(one_) == [16, -1]
    assert L.lslam_recentre_abi_sizes(None, 2) == 2
    B, P = _lib.RecentreBatch, _lib.RecentreParams
    assert [getattr(B, f).offset for f, _ in B._fields_] == [0, 4, 8, 16, 24, 32, 40]
    assert [f for f, _ in B._fields_] == ["n_robots", "reserved", "pose", "origin", "logodds", "shift", "flags"]
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("margin", 0), ("quantum", 4), ("reserved", 8)]
    # the older tables are unchanged
    nine = (C.c_int64 * 9)()
    assert L.lslam_abi_sizes(nine, 9) == 9 and list(nine) == [112, 56, 56, 128, 232, 48, 48, 32, 96]
    for fn, want in ((L.lslam_grid_abi_sizes, [40, 72]), (L.lslam_mapmatch_abi_sizes, [32, 112]),
                     (L.lslam_mapfuse_abi_sizes, [24, 160]), (L.lslam_reloc_abi_sizes, [56, 176]),
                     (L.lslam_raycast_abi_sizes, [16, 88])):
        two = (C.c_int64 * 2)()
        assert fn(two, 2) == 2 and list(two) == want


BAD_FIELDS = [("margin", -1), ("margin", 257), ("quantum", 0), ("quantum", 65), ("quantum", -8)]
BAD_GRID_FIELDS = [("cell", 0.0), ("grid_w", 2049), ("grid_w", 15)]


@pytest.mark.parametrize("field,value", BAD_FIELDS + BAD_GRID_FIELDS)
def test_recentre_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    L = _lib.load()
    b = _lib.RecentreBatch()
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(_lib.grid_params()), C.byref(_lib.recentre_params())) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()  # valid parameters, an empty batch: only the context is missing
    g, p = _lib.grid_params(), _lib.recentre_params()
    setattr(g if (field, value) in BAD_GRID_FIELDS else p, field, value)
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert field.encode() in L.lslam_last_error()


def test_margin_is_checked_against_the_grid_given():
    L = _lib.load()
    b = _lib.RecentreBatch()
    for grid_w, margin, ok in ((512, 256, True), (64, 32, True), (64, 33, False), (64, 128, False), (2048, 1024, True), (33, 16, True), (33, 17, False)):
        st = L.lslam_grid_recentre(None, C.byref(b), C.byref(_lib.grid_params(grid_w=grid_w)),
                                   C.byref(_lib.recentre_params(margin=margin, quantum=64 if ok else 8)))
        assert st == _lib.LSLAM_ERR_ARG
        assert (b"ctx" if ok else b"margin") in L.lslam_last_error(), (grid_w, margin)
    st = L.lslam_grid_recentre(None, C.byref(b), C.byref(_lib.grid_params()), C.byref(_lib.recentre_params(margin=0, quantum=1)))
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in L.lslam_last_error()


def test_recentre_missing_pointers_and_the_empty_batch():
    L = _lib.load()
    g, p = _lib.grid_params(), _lib.recentre_params()
    b = _lib.RecentreBatch()
    b.n_robots = 1
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    b.pose = b.origin = b.logodds = 4096
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"missing output" in L.lslam_last_error()
    b.shift = b.flags = 4096
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()
    b.n_robots = -1
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"n_robots" in L.lslam_last_error()
    assert L.lslam_grid_recentre(None, None, C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_recentre(None, C.byref(b), None, C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert L.lslam_grid_recentre(None, C.byref(b), C.byref(g), None) == _lib.LSLAM_ERR_ARG
    # an empty batch needs no pointers: its parameters are validated and only the context is then missing
    e = _lib.RecentreBatch()
    assert L.lslam_grid_recentre(None, C.byref(e), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()


def test_mapping_mirrors():
    from lidar_slam_amd import mapping
    assert (mapping.RECENTRE_BAD_POSE, mapping.RECENTRE_MOVED, mapping.RECENTRE_CLEARED) == (1, 2, 4)
    for w in (16, 52, 64, 100, 128, 256, 512, 1000, 2048):
        assert mapping.recentre_band_rows(w) == rr.band_rows(w) == max(1, min(w, 16384 // w))
    assert hasattr(mapping.OccupancyGrid, "recentre") and hasattr(mapping.OccupancyGrid, "recentre_results")
    assert isinstance(mapping.OccupancyGrid.origin_host, property)


# ---- the walks ----

WALK_ROBOTS = ((1500.0, 0.3), (900.0, -1.0), (2200.0, 2.0))  # (y, theta)
WALK_STEPS = 13
WALKS = {1: dict(dy=(0.0, 90.0, -80.0), grid=dict(grid_w=256, cell=20.0, max_range=2000.0), margin=104, quantum=8,
                 fixed_w=512, fixed_origin=(-3120.0, -3620.0)),
         2: dict(dy=(0.0, 60.0, -50.0), grid=dict(grid_w=128, cell=20.0, max_range=1000.0), margin=32, quantum=8,
                 fixed_w=256, fixed_origin=(-560.0, -1060.0))}
WALK_MOVE = np.array([60.0, -40.0, 0.03])  # the matcher's guess: the last true pose moved by this


def walk_poses(which):
    k = np.arange(WALK_STEPS, dtype=np.float64)
    return np.stack([np.stack([800.0 + 200.0 * k, y + dy * k, th + 0.05 * k], -1)
                     for (y, th), dy in zip(WALK_ROBOTS, WALKS[which]["dy"])], 1)  # [step, robot, 3]


@functools.lru_cache(maxsize=None)
def walk_revolutions(which):
    """xy [step][robot] -> [720, 2] in the robot's frame."""
    poses = walk_poses(which)
    return [[synth.polar_to_xy_ref(*synth.scan_polar_at(poses[k, r], 5000 + 100 * r + k)) for r in range(len(WALK_ROBOTS))]
            for k in range(WALK_STEPS)]


def walk_origin(which):
    g = WALKS[which]["grid"]
    p0 = walk_poses(which)[0, :, :2]
    return np.floor((p0 - g["grid_w"] * g["cell"] / 2) / g["cell"]) * g["cell"]


@functools.lru_cache(maxsize=None)
def walk_ref(which):
    """The reference chain: per step the grids [R, W, W] after recentre and update, the origins, the
    shifts and recentre flags, the update's flags; and `entered` [R, W, W], the step at which each
    cell of the final window last came into it.  Shared with test_gpu_recentre."""
    w = WALKS[which]
    g, W, R = w["grid"], w["grid"]["grid_w"], len(WALK_ROBOTS)
    poses, revs = walk_poses(which), walk_revolutions(which)
    L = np.zeros((R, W, W), np.int16)
    origin = walk_origin(which)
    entered = np.zeros((R, W, W), np.int16)
    steps = []
    for k in range(WALK_STEPS):
        L, origin, shift, rflags = rr.recentre_batch(L, poses[k], origin, margin=w["margin"], quantum=w["quantum"], **g)
        for r in range(R):
            if rflags[r] & MOVED:
                e = rr.shifted(entered[r] + 1, *shift[r])
                entered[r] = np.where(e == 0, k, e - 1)
        ups = [ogr.update(L[r], revs[k][r], poses[k, r], None, origin[r], **g) for r in range(R)]
        L = np.stack([u[0] for u in ups])
        steps.append(dict(L=L, origin=origin, shift=shift, rflags=rflags, gflags=np.array([u[2] for u in ups])))
    return steps, entered


def fixed_grid(which, r, first_step):
    """Robot r's fixed grid of the walk, fed the revolutions of the steps from `first_step` on."""
    w = WALKS[which]
    g = dict(w["grid"], grid_w=w["fixed_w"])
    poses, revs = walk_poses(which), walk_revolutions(which)
    F = np.zeros((w["fixed_w"], w["fixed_w"]), np.int16)
    for k in range(first_step, WALK_STEPS):
        F, _, flags = ogr.update(F, revs[k][r], poses[k, r], None, w["fixed_origin"], **g)
        assert flags == 0
    return F


def window_of(F, which, origin):
    """The window of the fixed grid F that a rolled grid with this origin covers."""
    w = WALKS[which]
    W, cell = w["grid"]["grid_w"], w["grid"]["cell"]
    off = (np.asarray(origin) - np.asarray(w["fixed_origin"])) / cell
    assert np.array_equal(off, np.round(off))
    x0, y0 = int(off[0]), int(off[1])
    assert 0 <= x0 and x0 + W <= w["fixed_w"] and 0 <= y0 and y0 + W <= w["fixed_w"]
    return F[y0:y0 + W, x0:x0 + W]


def test_walk_1_equals_a_fixed_grid():
    steps, _ = walk_ref(1)
    sh = np.stack([s["shift"] for s in steps])  # [step, robot, 2]
    moved_at = [k for k in range(WALK_STEPS) if sh[k, 0].any()]
    assert moved_at == [3, 6, 9, 12] and sh[moved_at, 0].tolist() == [[32, 0], [32, 0], [24, 0], [32, 0]]
    for r in (1, 2):
        ys = sh[:, r, 1][sh[:, r, 1] != 0]
        assert len(ys) and set(np.abs(ys).tolist()) <= {8, 16} and np.all(np.sign(ys) == (1 if r == 1 else -1)), ys
    print("shifts per step:", sh.tolist())
    for s in steps:
        assert not np.any(s["gflags"]) and np.all((s["rflags"] & ~MOVED) == 0)  # never CLIPPED, never a bad pose
    for r in range(len(WALK_ROBOTS)):
        F = fixed_grid(1, r, 0)
        Wn = window_of(F, 1, steps[-1]["origin"][r])
        assert np.count_nonzero(Wn) > 1000
        assert np.array_equal(steps[-1]["L"][r], Wn), r


def walk_match_ref(L, origin, rot0=None):
    """The matcher's reference on walk 1's rolled grids, from the displaced guess: per robot results."""
    poses, revs = walk_poses(1), walk_revolutions(1)
    return [mmr.match(L[r], origin[r], poses[-1, r] + WALK_MOVE, revs[-1][r], rot0=None if rot0 is None else rot0[r],
                      grid_w=256, win_w=256, cell=20.0) for r in range(len(WALK_ROBOTS))]


def assert_walk_match(results):
    poses = walk_poses(1)
    for r, res in enumerate(results):
        d = np.hypot(*(np.asarray(res["pose_out"])[:2] - poses[-1, r, :2]))
        dth = abs(float(res["pose_out"][2]) - poses[-1, r, 2])
        print("robot %d: matched on the rolled grid within %.2f mm, %.5f rad, flags %d" % (r, d, dth, res["flags"]))
        assert res["flags"] == 0 and d <= 20.0 and dth <= np.pi / 360, (r, d, dth, res["flags"])


def test_walk_1_matcher_follows_the_rolled_grid():
    steps, _ = walk_ref(1)
    assert_walk_match(walk_match_ref(steps[-1]["L"], steps[-1]["origin"]))


def test_walk_2_cells_restart_where_they_scroll_in():
    steps, entered = walk_ref(2)
    for s in steps:
        assert np.all((s["rflags"] & ~MOVED) == 0)
    for r in range(len(WALK_ROBOTS)):
        moved_at = [k for k in range(WALK_STEPS) if steps[k]["rflags"][r] & MOVED]
        assert len(moved_at) >= 3 and set(np.unique(entered[r]).tolist()) <= set([0] + moved_at)
        want = np.zeros_like(steps[-1]["L"][r])
        for k in [0] + moved_at:
            Wn = window_of(fixed_grid(2, r, k), 2, steps[-1]["origin"][r])
            want = np.where(entered[r] == k, Wn, want)
        n = np.count_nonzero(want)
        print("robot %d: recentred at steps %s, %d non-zero cells" % (r, moved_at, n))
        assert n > 1000 and np.array_equal(steps[-1]["L"][r], want), r
        # and cells did scroll off: the fixed grid from step 0 holds cells the window has lost
        assert np.count_nonzero(fixed_grid(2, r, 0)) > np.count_nonzero(window_of(fixed_grid(2, r, 0), 2, steps[-1]["origin"][r]))
