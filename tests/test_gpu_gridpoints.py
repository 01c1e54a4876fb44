"""GPU parity of a map read as a revolution (lslam_grid_points; mapping.GridScan, mapping.align_maps)
against its NumPy definition, tests/gridpoints_ref.py, and of the device chain against the references'.

The definition is FP64 in a written operation order, then integers, and the anchor's (cos, sin) are the
caller's bits, so xy (as uint64 patterns), pt_off, counts and flags are compared EXACTLY, as whole arrays.
Every output buffer holds junk before every call, the scratch too; xy lies inside a larger buffer, 24
bytes from its start (8-byte aligned, not 16), and the junk on both sides of xy[0 .. R * cap) must keep its
bytes.

grid_w 16, 24, 72 and 520 are multiples of 8 and take the 16-byte path when the grids' address allows; the
same grids one int16 further into their buffer take the lane-per-cell path.  The bands: one wave owns
ceil(W / bands) rows, with bands = min(256, ceil(32 CUs / R)): a row for the small widths, 3 or 5 rows at 520,
8 at 2048, and 12 to 15 rows for the small widths in the fleets of thousands.  The runs of
tests/test_gridpoints_plan.py's seam_map end at row ends that are band seams for each of those heights."""
import numpy as np
import pytest

import gridpoints_ref as gp
from test_gridpoints_plan import seam_map

pytestmark = pytest.mark.gpu
CELL = 20.0
PAD = 3  # doubles of canary before and behind xy


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def call(ctx, L, origin, anchor, rng, shift=0, bufs=None, **kw):
    """One lslam_grid_points through the C ABI on junk-filled buffers, held to the reference.  shift: int16s
    between the grids' buffer and the grids (1: the lane-per-cell path).  Returns (result, reference, bufs)."""
    from lidar_slam_amd import _lib
    p = dict(gp.DEFAULTS, cell=CELL, **kw)
    R, W, cap = len(L), L.shape[1], int(p["cap"])
    L = np.ascontiguousarray(L, np.int16)
    origin = np.ascontiguousarray(np.broadcast_to(origin, (R, 2)), np.float64)
    anchor = np.ascontiguousarray(np.broadcast_to(anchor, (R, 4)), np.float64)
    junk = rng.integers(1, 2 ** 62, 2 * R * cap + 2 * PAD).astype(np.uint64).view(np.float64)
    if bufs is None:
        bufs = {"xy": ctx.empty(junk.size, np.float64), "pt_off": ctx.empty(R + 1, np.int32), "counts": ctx.empty((R, 4), np.int32),
                "flags": ctx.empty(R, np.int32), "bands": ctx.empty((R, _lib.GRIDPOINTS_BANDS, 2), np.int32)}
    bufs["xy"].upload(junk)
    for k in ("pt_off", "counts", "flags", "bands"):
        bufs[k].upload(rng.integers(-2 ** 31, 2 ** 31, bufs[k].shape).astype(np.int32))
    dl = ctx.empty(L.size + 8, np.int16)
    dl.upload(np.concatenate([np.full(shift, 300, np.int16), L.ravel(), np.full(8 - shift, 300, np.int16)]))
    do, da = ctx.to_device(origin), ctx.to_device(anchor)
    b = _lib.GridPointsBatch()
    b.n_robots = R
    b.logodds, b.origin, b.anchor = dl.addr + 2 * shift, do.addr, da.addr
    b.xy, b.pt_off, b.counts, b.flags, b.band_counts = (bufs["xy"].addr + 8 * PAD, bufs["pt_off"].addr, bufs["counts"].addr,
                                                        bufs["flags"].addr, bufs["bands"].addr)
    g = _lib.grid_params(grid_w=W, cell=CELL)
    q = _lib.gridpoints_params(radius=float(p["radius"]), occ_min=int(p["occ_min"]), cap=cap)
    _lib.call("lslam_grid_points", ctx, b, g, q)
    ctx.sync()
    raw = bufs["xy"].download()
    res = {"xy": raw[PAD:-PAD].reshape(R, cap, 2), "pt_off": bufs["pt_off"].download(), "counts": bufs["counts"].download(),
           "flags": bufs["flags"].download()}
    ref = gp.points_batch(L, origin, anchor, **p)
    assert np.array_equal(bits(raw[:PAD]), bits(junk[:PAD])) and np.array_equal(bits(raw[-PAD:]), bits(junk[-PAD:])), "canary"
    assert np.array_equal(res["pt_off"], ref["pt_off"])
    assert np.array_equal(res["flags"], ref["flags"]), (res["flags"][:8].tolist(), ref["flags"][:8].tolist())
    assert np.array_equal(res["counts"], ref["counts"]), (np.argwhere(res["counts"] != ref["counts"])[:4].tolist(), res["counts"][:3].tolist(),
                                                          ref["counts"][:3].tolist())
    bad = np.argwhere(bits(res["xy"]) != bits(ref["xy"]))
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    assert np.array_equal(dl.download()[shift:shift + L.size], L.ravel())  # read only
    return res, ref, bufs


def fleet(rng, R, W):
    """R maps at 1 %, 30 % and 100 % occupancy in turn, every fourth with the seam runs; anchors on and off the
    grid at any heading, every fifth robot (between good ones) with a component that is not finite."""
    L = np.empty((R, W, W), np.int16)
    for r in range(R):
        occ = (0.01, 0.30, 1.00)[r % 3]
        L[r] = np.where(rng.random((W, W)) < occ, rng.integers(85, 351, (W, W)), rng.integers(-200, 85, (W, W)))
        if r % 4 == 3:
            L[r] = np.maximum(L[r], seam_map(W, rng))
    half = 0.5 * W * CELL
    origin = -half + rng.uniform(-300.0, 300.0, (R, 2))
    th = rng.uniform(-np.pi, np.pi, R)
    anchor = np.stack([rng.uniform(-1.2 * half, 1.2 * half, R), rng.uniform(-1.2 * half, 1.2 * half, R), np.cos(th), np.sin(th)], -1)
    for r in range(1, R - 1, 5):
        k = rng.integers(0, 6)
        (origin[r] if k < 2 else anchor[r])[k if k < 2 else k - 2] = (np.nan, np.inf, -np.inf)[r % 3]
    return L, origin, anchor


@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("W", [16, 24, 72, 520])
def test_fleets_of_every_width(ctx, W, R):
    """Default cap 1024: the 100 % map of 72 cells has 5184 cells in range and a stride of 6."""
    rng = np.random.default_rng(1000 * W + R)
    L, origin, anchor = fleet(rng, R, W)
    if W == 72 and R == 3:
        anchor[2, :2] = (1.0, 2.0)
    res, ref, _ = call(ctx, L, origin, anchor, rng)
    if W == 72 and R == 3:
        assert ref["counts"][2].tolist()[1:] == [5184, 6, 864] and ref["flags"][2] == gp.DECIMATED
    if R >= 3:
        assert ref["flags"][1] == gp.BAD_ANCHOR and ref["flags"][0] != gp.BAD_ANCHOR != ref["flags"][2]
    if W * W * 2 * R <= 2 ** 20:
        call(ctx, L, origin, anchor, rng, shift=1)             # the lane-per-cell path
        call(ctx, L, origin, anchor, rng, radius=0.3 * W * CELL, cap=37)  # a radius inside the grid, an odd cap


@pytest.mark.parametrize("W,R", [(24, 4500), (72, 2000)])
def test_bands_of_many_rows_in_a_large_fleet(ctx, W, R):
    """Thousands of robots: a wave owns many rows of a small grid (on 256 CUs 12 rows of 24 cells, 15 of 72)."""
    rng = np.random.default_rng(W)
    L8, origin, anchor = fleet(rng, 8, W)
    pick = rng.integers(0, 8, R)
    L, origin, anchor = L8[pick], origin[pick], anchor[pick]
    L[:, 0, 0] = rng.integers(-200, 351, R)
    call(ctx, L, origin, anchor, rng, cap=64)


def test_grid_2048(ctx):
    rng = np.random.default_rng(2048)
    W = 2048
    L = np.where(rng.random((1, W, W)) < 0.01, 120, -40).astype(np.int16)
    L[0, W - 1, W - 65:] = 200
    res, ref, _ = call(ctx, L, (-0.5 * W * CELL, -0.5 * W * CELL), (1234.5, -987.0, np.cos(2.5), np.sin(2.5)), rng, radius=0.45 * W * CELL)
    print("2048 cells: counts", res["counts"][0].tolist(), "flags", int(res["flags"][0]))
    assert ref["flags"][0] == gp.DECIMATED and ref["counts"][0, 1] > 20000


def test_radius_edge_anchor_cell_and_the_caps(ctx):
    """The hand-made cases of tests/test_gridpoints_ref.py on the device."""
    from test_gridpoints_ref import grid16
    rng = np.random.default_rng(7)
    L = grid16([(5, 5), (10, 5), (8, 9), (9, 9)])[None]
    res, ref, _ = call(ctx, L, (0.0, 0.0), (110.0, 110.0, 1.0, 0.0), rng, radius=5 * CELL, cap=8)
    assert res["counts"][0].tolist() == [4, 2, 1, 2] and res["xy"][0, :2].tolist() == [[100.0, 0.0], [60.0, 80.0]]
    res, _, _ = call(ctx, L, (0.0, 0.0), (110.0, 110.0, 1.0, 0.0), rng, radius=float(np.nextafter(100.0, 0.0)), cap=8)
    assert res["counts"][0].tolist() == [4, 0, 1, 0] and res["flags"][0] == gp.EMPTY
    cells = [(x, y) for y in (2, 7, 11) for x in (1, 4, 6, 9, 13)][:13]
    L = np.stack([grid16(cells), np.zeros((16, 16), np.int16), grid16(cells[:5])])
    for cap, counts in ((64, [13, 13, 1, 13]), (13, [13, 13, 1, 13]), (12, [13, 13, 2, 7]), (1, [13, 13, 13, 1]), (5, [13, 13, 3, 5])):
        res, _, _ = call(ctx, L, (0.0, 0.0), (163.0, 150.0, 1.0, 0.0), rng, cap=cap)
        assert res["counts"][0].tolist() == counts and res["flags"][1] == gp.EMPTY and res["counts"][2, 1] == 5
    # a quarter turn, exactly
    call(ctx, L, (-160.0, -160.0), (0.0, 0.0, 0.0, 1.0), rng, cap=16)


def test_a_second_call_zeroes_the_first_calls_tail(ctx):
    rng = np.random.default_rng(11)
    W = 72
    L, origin, anchor = fleet(rng, 3, W)
    _, ref1, bufs = call(ctx, L, origin, anchor, rng, cap=512)
    L2 = np.where(rng.random((3, W, W)) < 0.004, 100, 0).astype(np.int16)
    _, ref2, _ = call(ctx, L2, origin, anchor, rng, cap=512, bufs=bufs)
    assert (ref2["counts"][[0, 2], 3] < ref1["counts"][[0, 2], 3]).all() and (ref2["counts"][[0, 2], 3] > 0).all()


# ---- GridScan, align_maps and the chain ----

def room_grids(ctx, R=1):
    from lidar_slam_amd.mapping import OccupancyGrid
    from test_gridmerge_ref import origin_b, room_maps
    from test_reloc_ref import SCENE_ORIGIN
    A, B = room_maps()
    ga = OccupancyGrid(ctx, R, origin=SCENE_ORIGIN)
    gb = OccupancyGrid(ctx, R, origin=origin_b())
    ga.upload(np.stack([A] * R))
    gb.upload(np.stack([B] + [np.zeros_like(B)] * (R - 1)))
    return ga, gb, A, B


RELOC_KEYS = ("pose", "flags", "result", "n_occ", "n_used", "cand", "cand_pose", "fine_pose", "fine_best", "fine_flags")


def test_unsynced_scan_then_unsynced_relocalize(ctx):
    """GridScan.step and relocalize enqueued back to back with sync=False, then one sync: the synced pair's results."""
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import GridScan
    from test_gridpoints_ref import ANCHORS
    ga, gb, _, B = room_grids(ctx)
    pose = ANCHORS["off_centre_1rad"]()
    out = []
    for sync in (False, True):
        scan, rel = GridScan(gb, cap=256), GridRelocalizer(ctx, 1)
        scan.step(anchor=pose, sync=sync)
        rel.relocalize(scan.input, grid=ga, sync=sync)
        ctx.sync()
        out.append((scan.results(), rel.results()))
    for k in ("xy", "counts", "flags"):
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    for k in RELOC_KEYS:
        a, b = out[0][1][k], out[1][1][k]
        assert np.array_equal(a, b) if a.dtype.kind == "i" else np.array_equal(bits(a), bits(b)), k
    assert out[0][1]["flags"][0] == 0 and out[0][0]["counts"][0].tolist() == [827, 827, 4, 207]
    from test_gridmerge_ref import origin_b
    ref = gp.points(B, origin_b(), gp.anchor_of(pose), cap=256)
    assert np.array_equal(bits(out[0][0]["xy"][0]), bits(ref["xy"]))


def test_room_chain_on_the_device(ctx):
    """GridScan(B).step(), align_maps(A, B, GridRelocalizer), A.merge(B, xform) for two pairs: B into A, and
    an empty map into A.  Pair 0's pose, merge statistics and flags are the reference chain's of
    tests/test_gridpoints_ref.py bit for bit (the reference is fed the (cos, sin) that the device wrote for
    the candidate poses, as in tests/test_gpu_reloc.py, where those are not NumPy's); pair 1 is RELOC_LOST,
    then MERGE_BAD_XFORM, and its destination keeps every bit."""
    import gridmerge_ref as gm
    import reloc_ref as rr
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import GridScan, align_maps, merge_transform
    from test_gridmerge_ref import origin_b
    from test_gridpoints_ref import ANCHORS, room_chain
    from test_reloc_ref import SCENE_ORIGIN
    ga, gb, A, B = room_grids(ctx, 2)
    scan = GridScan(gb)
    scan.step()
    pose_b = ANCHORS["centre"]()
    assert np.array_equal(scan.anchor_pose, np.stack([pose_b, pose_b]))
    sr = scan.results()
    q = gp.points(B, origin_b(), gp.anchor_of(pose_b))
    assert np.array_equal(bits(sr["xy"][0]), bits(q["xy"])) and np.array_equal(sr["counts"][0], q["counts"])
    assert sr["flags"].tolist() == [0, gp.EMPTY] and not sr["xy"][1].any() and scan.pt_off.download().tolist() == [0, 1024, 2048]
    rel = GridRelocalizer(ctx, 2)
    out = align_maps(ga, gb, rel, scan=scan)
    res = rel.results()
    _, ref, xf, _ = room_chain("centre", 4096)  # (the same 827 points; the zeros behind them are invalid points)
    if not np.array_equal(bits(ref["fine_rot0"]), bits(res["fine_rot0"][:, 0])):
        ref = rr.relocalize(A, SCENE_ORIGIN, q["xy"], fine_rot0=res["fine_rot0"][:, 0])
        xf = merge_transform(ref["pose_out"], pose_b)
    assert out["flags"].tolist() == [0, rr.LOST] and ref["flags"] == 0
    assert np.array_equal(bits(out["pose"][0]), bits(ref["pose_out"])) and np.array_equal(res["result"][0], ref["result"])
    assert np.array_equal(bits(out["xform"][0]), bits(xf)) and np.isnan(out["pose"][1]).all() and np.isnan(out["xform"][1]).all()
    assert np.array_equal(out["counts"], sr["counts"])
    ga.merge(gb, out["xform"])
    m = ga.merge_results()
    mref = gm.merge(B, origin_b(), A, SCENE_ORIGIN, xf)
    assert m["flags"].tolist() == [gm.MERGED, gm.BAD_XFORM] and mref["flags"] == gm.MERGED
    assert np.array_equal(m["stats"][0], mref["stats"]) and not m["stats"][1].any()
    assert mref["stats"][2] >= 640 and 1000 * mref["stats"][3] <= 25 * (mref["stats"][2] + mref["stats"][3])
    print("scan counts %s; pose in A %s (flags %s); xform %s; merge stats %s flags %s" % (
        sr["counts"].tolist(), out["pose"][0].tolist(), out["flags"].tolist(), out["xform"][0].tolist(), m["stats"][0].tolist(), m["flags"].tolist()))
    after = ga.logodds.download()
    assert np.array_equal(after[0], mref["dst"]) and np.array_equal(after[1], A)
