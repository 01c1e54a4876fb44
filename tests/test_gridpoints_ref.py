"""A map read as a revolution (include/lidarslam.h, lslam_grid_points) on the CPU: the NumPy reference
(tests/gridpoints_ref.py) on a hand-made case per rule, the chain map -> points -> relocalisation ->
merge_transform -> merge on the references in the L-shaped room, and the ABI checks that need no device.
tests/test_gpu_gridpoints.py holds the kernels to the reference bit for bit, and the device chain to this
one.

The room.  Maps A and B of tests/test_gridmerge_ref.py (B's frame is A's turned by 0.4 rad and shifted by
(300, -200) mm), defaults throughout.  B's occupied cells become points about an anchor in B, the
relocaliser's reference finds that anchor in A, merge_transform makes the transform and the merge's
reference judges it in a dry run.  Measured with these references (test_room_chain prints it):

    anchor in B                          cap   in range  stride  points  reloc flags  rival / winner  supported  contradicted
    grid centre, theta 0                 4096       827       1     827            0     1520 / 1992        789             0
    grid centre, theta 0                  256       827       4     207            0      368 /  506        769             0
    (-1120, +880) mm of it, theta 1 rad  4096       827       1     827            0     1587 / 2096        766             0
    (-1120, +880) mm of it, theta 1 rad   256       827       4     207            0      380 /  527        776             0

The true transform supports 779 cells.  The bounds asserted are those that test_room_end_to_end of
tests/test_gridmerge_ref.py holds real revolutions to: no relocalisation flag, no merge flag, at most 25
per thousand contradicted, at least 640 supported."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import gridmerge_ref as gm
import gridpoints_ref as gp
from test_gridmerge_ref import CELL, origin_b, room_maps, share
from test_reloc_ref import SCENE_ORIGIN


def grid16(cells, value=100):
    L = np.zeros((16, 16), np.int16)
    for x, y in cells:
        L[y, x] = value
    return L


# ---- a hand-made case per rule ----

def test_the_radius_edge_is_in_and_the_anchor_cell_is_out():
    """The anchor on the centre of cell (5, 5), radius 5 cells: (10, 5) and (8, 9) lie at d2 == r2 exactly
    and are taken, (9, 9) is out, and the anchor's own cell (d2 == 0) is occupied but not in range."""
    L = grid16([(5, 5), (10, 5), (8, 9), (9, 9)])
    q = gp.points(L, (0.0, 0.0), (110.0, 110.0, 1.0, 0.0), radius=5 * CELL, cap=8)
    assert q["counts"].tolist() == [4, 2, 1, 2] and q["flags"] == 0
    assert q["xy"].tolist() == [[100.0, 0.0], [60.0, 80.0]] + [[0.0, 0.0]] * 6  # row-major: Y = 5 before Y = 9
    # one ulp less of radius and both are out; the anchor cell alone is EMPTY
    q = gp.points(L, (0.0, 0.0), (110.0, 110.0, 1.0, 0.0), radius=np.nextafter(100.0, 0.0), cap=8)
    assert q["counts"].tolist() == [4, 0, 1, 0] and q["flags"] == gp.EMPTY and not q["xy"].any()
    q = gp.points(grid16([(5, 5)]), (0.0, 0.0), (110.0, 110.0, 1.0, 0.0), cap=8)
    assert q["counts"].tolist() == [1, 0, 1, 0] and q["flags"] == gp.EMPTY
    # occ_min is inclusive
    q = gp.points(grid16([(1, 1)], 85) + grid16([(2, 1)], 84), (0.0, 0.0), (110.0, 110.0, 1.0, 0.0))
    assert q["counts"].tolist() == [1, 1, 1, 1]


def test_stride_arithmetic():
    cells = [(x, y) for y in (2, 7, 11) for x in (1, 4, 6, 9, 13)][:13]
    L = grid16(cells)
    full = gp.points(L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), cap=64)
    assert full["counts"].tolist() == [13, 13, 1, 13]
    q = gp.points(L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), cap=13)          # cap == n_in: everything, nothing behind it
    assert q["counts"].tolist() == [13, 13, 1, 13] and q["flags"] == 0 and np.array_equal(q["xy"], full["xy"][:13])
    q = gp.points(L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), cap=12)          # cap == n_in - 1: stride 2, n_out = ceil(13 / 2)
    assert q["counts"].tolist() == [13, 13, 2, 7] and q["flags"] == gp.DECIMATED
    assert np.array_equal(q["xy"][:7], full["xy"][:13:2]) and not q["xy"][7:].any()
    q = gp.points(L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), cap=1)           # one slot: the first cell
    assert q["counts"].tolist() == [13, 13, 13, 1] and q["flags"] == gp.DECIMATED and np.array_equal(q["xy"], full["xy"][:1])
    q = gp.points(L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), cap=5)           # stride 3, n_out = 5 == cap
    assert q["counts"].tolist() == [13, 13, 3, 5] and np.array_equal(q["xy"], full["xy"][:13:3])


def test_empty_and_bad_anchor():
    q = gp.points(np.zeros((16, 16), np.int16), (0.0, 0.0), (100.0, 100.0, 1.0, 0.0), cap=4)
    assert q["counts"].tolist() == [0, 0, 1, 0] and q["flags"] == gp.EMPTY and not q["xy"].any()
    L = np.full((16, 16), 200, np.int16)
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            v = [0.0, 0.0, 100.0, 100.0, 1.0, 0.0]
            v[k] = bad
            q = gp.points(L, v[:2], v[2:], cap=4)
            assert q["flags"] == gp.BAD_ANCHOR and not q["counts"].any(), (k, bad)
            assert q["xy"].shape == (4, 2) and not q["xy"].view(np.uint64).any()  # +0.0, by its bits
    b = gp.points_batch(np.stack([L, L, L]), np.zeros((3, 2)), [(100.0, 100.0, 1.0, 0.0), (np.nan, 0.0, 1.0, 0.0), (100.0, 100.0, 1.0, 0.0)], cap=300)
    assert b["flags"].tolist() == [0, gp.BAD_ANCHOR, 0] and b["pt_off"].tolist() == [0, 300, 600, 900]
    assert np.array_equal(b["xy"][0], b["xy"][2]) and not b["xy"][1].any() and b["counts"][0].tolist() == [256, 256, 1, 256]


def test_a_quarter_turn_anchor_is_rot90():
    """The anchor at the grid's centre (a cell corner) with (c, s) = (0, 1): the points are those of the map
    turned by np.rot90 under an anchor that is not turned.  Cell (X, Y) of L is cell (Y, 15 - X) of the
    turned map; the order differs (row-major in the other map), the set does not."""
    rng = np.random.default_rng(5)
    L = np.where(rng.random((16, 16)) < 0.3, 120, -30).astype(np.int16)
    o, a = (-160.0, -160.0), (0.0, 0.0)
    q = gp.points(L, o, a + (0.0, 1.0), cap=256)
    t = gp.points(np.rot90(L, 1), o, a + (1.0, 0.0), cap=256)
    n = int(q["counts"][3])
    assert n == int((L >= 85).sum()) == int(t["counts"][3]) and q["counts"].tolist() == t["counts"].tolist()

    def rows(p):
        return p[np.lexsort((p[:, 1], p[:, 0]))]
    assert np.array_equal(rows(q["xy"][:n]), rows(t["xy"][:n]))
    # and by hand: the point of cell (X, Y) is (dy, -dx)
    Y, X = np.nonzero(L >= 85)
    assert np.array_equal(q["xy"][:n], np.stack([(Y + 0.5 - 8) * 20.0, -((X + 0.5 - 8) * 20.0)], -1))


# ---- the room: map -> points -> relocalisation -> merge_transform -> merge, on the references ----

def centre_b():
    return np.array(origin_b()) + 0.5 * 512 * CELL


ANCHORS = {"centre": lambda: np.append(centre_b(), 0.0),
           "off_centre_1rad": lambda: np.append(centre_b() + np.array([-1120.0, 880.0]), 1.0)}


@functools.lru_cache(maxsize=None)
def room_chain(anchor, cap):
    """(the points' result, the relocaliser's, the transform, the dry merge's) for B read about ``anchor``."""
    import reloc_ref as rr
    from lidar_slam_amd.mapping import merge_transform
    A, B = room_maps()
    pose = ANCHORS[anchor]()
    q = gp.points(B, origin_b(), gp.anchor_of(pose), cap=cap)
    res = rr.relocalize(A, SCENE_ORIGIN, q["xy"])  # every slot, as the device reads them: the zeros are invalid points
    xf = merge_transform(res["pose_out"], pose)
    return q, res, xf, gm.merge(B, origin_b(), A, SCENE_ORIGIN, xf, dry_run=True)


@pytest.mark.parametrize("cap", [4096, 256])
@pytest.mark.parametrize("anchor", list(ANCHORS))
def test_room_chain(anchor, cap):
    q, res, xf, m = room_chain(anchor, cap)
    st, r = m["stats"], res["result"]
    truth = np.array([np.cos(0.4), np.sin(0.4), 300.0, -200.0])
    print("%-16s cap %4d: counts %s; reloc flags %d, rival %d / winner %d; supported %d contradicted %d (%.1f permille); "
          "transform off by %s" % (anchor, cap, q["counts"].tolist(), res["flags"], r[7], r[5], st[2], st[3], share(st),
                                   np.abs(xf - truth).tolist()))
    assert q["counts"][1] == 827 and q["counts"][2] == (1 if cap == 4096 else 4) and res["n_used"] == q["counts"][3]
    assert res["flags"] == 0 and m["flags"] == 0
    assert share(st) <= 25.0 and st[2] >= 640


def test_an_empty_map_is_lost_and_its_merge_refused():
    """No points: LOST, a NaN pose, a NaN transform, MERGE_BAD_XFORM, the destination bit for bit."""
    import reloc_ref as rr
    from lidar_slam_amd.mapping import merge_transform
    A, _ = room_maps()
    pose = ANCHORS["centre"]()
    q = gp.points(np.zeros((512, 512), np.int16), origin_b(), gp.anchor_of(pose))
    assert q["flags"] == gp.EMPTY
    res = rr.relocalize(A, SCENE_ORIGIN, q["xy"])
    assert res["flags"] == rr.LOST and np.isnan(res["pose_out"]).all()
    xf = merge_transform(res["pose_out"], pose)
    m = gm.merge(np.zeros((512, 512), np.int16), origin_b(), A, SCENE_ORIGIN, xf)
    assert m["flags"] == gm.BAD_XFORM and np.array_equal(m["dst"], A) and not m["stats"].any()


# ---- the ABI, and the refusals that need no device ----

FIELDS = ("logodds", "origin", "anchor", "xy", "pt_off", "counts", "flags", "band_counts")


def _batch(n=1):
    from lidar_slam_amd import _lib
    b = _lib.GridPointsBatch()
    b.n_robots = n
    for i, f in enumerate(FIELDS):
        setattr(b, f, (i + 1) << 32)
    return b


def _err(st):
    from lidar_slam_amd import _lib
    assert st == _lib.LSLAM_ERR_ARG
    return _lib.load().lslam_last_error().decode()


def test_abi_sizes_defaults_and_constants():
    from lidar_slam_amd import _lib, mapping
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_gridpoints_abi_sizes(got, 2) == 2 and list(got) == [16, 72]
    assert list(got) == [C.sizeof(_lib.GridPointsParams), C.sizeof(_lib.GridPointsBatch)]
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_gridpoints_abi_sizes(one, 1) == 2 and list(one) == [16, -1] and L.lslam_gridpoints_abi_sizes(None, 2) == 2
    B = _lib.GridPointsBatch
    assert [(f, getattr(B, f).offset) for f, _ in B._fields_] == [("n_robots", 0), ("reserved", 4)] + [(f, 8 + 8 * i) for i, f in enumerate(FIELDS)]
    P = _lib.GridPointsParams
    assert [(f, getattr(P, f).offset) for f, _ in P._fields_] == [("radius", 0), ("occ_min", 8), ("cap", 12)]
    p = _lib.gridpoints_params()
    assert (p.radius, p.occ_min, p.cap) == (8000.0, 85, 1024) == tuple(gp.DEFAULTS[k] for k in ("radius", "occ_min", "cap"))
    assert L.lslam_gridpoints_params_default(None) == _lib.LSLAM_ERR_ARG
    assert (_lib.GRIDPOINTS_BAD_ANCHOR, _lib.GRIDPOINTS_EMPTY, _lib.GRIDPOINTS_DECIMATED) == \
        (mapping.GRIDPOINTS_BAD_ANCHOR, mapping.GRIDPOINTS_EMPTY, mapping.GRIDPOINTS_DECIMATED) == (gp.BAD_ANCHOR, gp.EMPTY, gp.DECIMATED) == (1, 2, 4)
    assert _lib.ABI_VERSION == 6 and b"(abi 6," in L.lslam_version()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lidarslam.h")).read()
    assert re.search(r"LSLAM_K_COUNT = 16\b", hdr) and re.search(r"#define LSLAM_ABI_VERSION\s+6\b", hdr)  # no new timing slot
    for name, v in (("BAD_ANCHOR", 1), ("EMPTY", 2), ("DECIMATED", 4)):
        assert re.search(r"LSLAM_GRIDPOINTS_%s = %d\b" % (name, v), hdr)
    assert re.search(r"#define LSLAM_GRIDPOINTS_BANDS %d\b" % _lib.GRIDPOINTS_BANDS, hdr)
    # the older tables are unchanged
    two = (C.c_int64 * 2)()
    assert L.lslam_gridmerge_abi_sizes(two, 2) == 2 and list(two) == [32, 72]
    assert all(hasattr(mapping.GridScan, m) for m in ("step", "results")) and hasattr(mapping, "align_maps")


def test_checks_come_before_the_context():
    """Every call with ctx = NULL: the message says how far it came (the order of tests/test_map_entry_frame.py)."""
    from lidar_slam_amd import _lib
    L = _lib.load()
    g, p = _lib.grid_params(grid_w=64), _lib.gridpoints_params()
    ref = C.byref

    def call(b, g=g, p=p):
        return _err(L.lslam_grid_points(None, b and ref(b), g and ref(g), p and ref(p)))

    assert call(_batch()) == "gridpoints: ctx is NULL"
    assert call(_batch(0)) == "gridpoints: ctx is NULL"
    assert call(None) == "gridpoints: batch is NULL"
    assert call(_batch(), p=None) == "gridpoints: params is NULL" and call(_batch(), g=None) == "grid: params is NULL"
    assert call(None, p=None) == "gridpoints: params is NULL"  # params before the batch
    assert "grid_w" in call(_batch(), g=_lib.grid_params(grid_w=8)) and "cell" in call(_batch(), g=_lib.grid_params(cell=0.0))
    assert call(_batch(-1)) == "gridpoints: negative n_robots"
    for kw, word in ((dict(radius=0.0), "radius must be > 0 and finite"), (dict(radius=-1.0), "radius"), (dict(radius=float("inf")), "radius"),
                     (dict(radius=float("nan")), "radius"), (dict(occ_min=40000), "occ_min must be in [-32768, 32767]"),
                     (dict(occ_min=-32769), "occ_min"), (dict(cap=0), "cap must be in [1, 65536]"), (dict(cap=65537), "cap")):
        assert word in call(_batch(), p=_lib.gridpoints_params(**kw)), kw
    for kw in (dict(occ_min=-32768), dict(occ_min=32767), dict(cap=1), dict(cap=65536), dict(radius=1e-3)):
        assert call(_batch(), p=_lib.gridpoints_params(**kw)) == "gridpoints: ctx is NULL", kw
    for f in FIELDS[:3]:
        b = _batch()
        setattr(b, f, None)
        assert call(b) == "gridpoints: missing input (logodds, origin, anchor)"
    for f in FIELDS[3:]:
        b = _batch()
        setattr(b, f, None)
        assert call(b) == "gridpoints: missing output (xy, pt_off, counts, flags, band_counts)"
    b = _batch(-1)
    b.logodds = None
    assert call(b) == "gridpoints: negative n_robots"  # the size before the pointers
    # pt_off is 32 bits wide: R * cap must stay below 2^31
    assert call(_batch(32768), p=_lib.gridpoints_params(cap=65536)) == "gridpoints: n_robots * cap must be below 2^31"
    assert call(_batch(32767), p=_lib.gridpoints_params(cap=65536)) == "gridpoints: ctx is NULL"
    b = _batch(32768)
    b.xy = None
    assert "missing output" in call(b, p=_lib.gridpoints_params(cap=65536))  # the pointers before the product
    # an empty batch needs no pointers
    assert call(_lib.GridPointsBatch()) == "gridpoints: ctx is NULL"


def test_gridscan_refuses_a_radius_beyond_max_range():
    """GridScan's own checks come before anything touches a device."""
    from lidar_slam_amd import mapping

    class FakeGrid(mapping.OccupancyGrid):
        def __init__(self):
            from lidar_slam_amd import _lib
            self.p, self.ctx, self.R, self.W = _lib.grid_params(), None, 1, 512

    with pytest.raises(ValueError, match="max_range"):
        mapping.GridScan(FakeGrid(), radius=8000.5)
    with pytest.raises(ValueError, match="OccupancyGrid"):
        mapping.GridScan(object())
