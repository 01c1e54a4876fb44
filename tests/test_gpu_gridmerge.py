"""GPU parity of the map merge (lslam_grid_merge; OccupancyGrid.merge) against its NumPy definition,
tests/gridmerge_ref.py.

The definition is FP64 in a written operation order, then integers, and the transform's bits are the
caller's, so dst, stats and flags are compared EXACTLY, as whole arrays.  The maps hold sparse signed
values like a map's, with occupied cells in the corners, along the borders and on both sides of every
tile seam (the kernel's tiles are 64 columns by 32 rows), so the 3 x 3 block of N is read across seams
and clipped at the map's edge.  stats and flags hold junk before every call.

grid_w 16, 24 and 64 take the 16-byte path (8 cells a thread), 52 the lane-per-cell path; a gate set
between the pairs' figures leaves some pairs of every batch merged and some gated, so one comparison
holds both."""
import numpy as np
import pytest

import gridmerge_ref as gm

pytestmark = pytest.mark.gpu
CELL = 20.0
QUARTER = (0.0, 1.0)  # an exact quarter turn


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def map_like(rng, n, W, frac=0.35):
    """Sparse signed values (beyond the clamps too) with occupied cells in the corners, on the borders and
    on both sides of the tile seams."""
    L = np.where(rng.random((n, W, W)) < frac, rng.integers(-400, 401, (n, W, W)), 0).astype(np.int16)
    L[:, [0, 0, W - 1, W - 1], [0, W - 1, 0, W - 1]] = 120
    L[:, 0, 5::7] = 90
    L[:, 3::5, W - 1] = 85
    for s in (31, 32, 63, 64):
        if s < W:
            L[:, s, 1::6] = 100
            L[:, 2::9, s] = 100
    return L


def centred(W):
    return (-0.5 * W * CELL, -0.5 * W * CELL)


def grids(ctx, src, so, dst, do):
    from lidar_slam_amd.mapping import OccupancyGrid
    gs = OccupancyGrid(ctx, len(src), origin=so, grid_w=src.shape[1], cell=CELL)
    gs.upload(src)
    gd = OccupancyGrid(ctx, len(dst), origin=do, grid_w=dst.shape[1], cell=CELL)
    gd.upload(dst)
    return gs, gd


def junk_outputs(ctx, gd, rng):
    """stats and flags hold junk before the call (the buffers that merge() would allocate itself)."""
    n = gd.R
    gd._merge = (ctx.to_device(rng.integers(-2 ** 31, 2 ** 31, (n, 8)).astype(np.int32)),
                 ctx.to_device(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)))


def check(ctx, rng, src, so, dst, do, xf, src_index=None, what="", **kw):
    """One merge on fresh grids against the reference; returns the reference's result."""
    gs, gd = grids(ctx, src, so, dst, do)
    junk_outputs(ctx, gd, rng)
    gd.merge(gs, xf, src_index=src_index, **kw)
    res = gd.merge_results()
    ref = gm.merge_batch(src, np.broadcast_to(so, (len(src), 2)), dst, np.broadcast_to(do, (len(dst), 2)),
                         np.broadcast_to(xf, (len(dst), 4)), src_index=src_index, cell=CELL, **kw)
    assert np.array_equal(res["flags"], ref["flags"]), (what, res["flags"].tolist(), ref["flags"].tolist())
    assert np.array_equal(res["stats"], ref["stats"]), (what, np.argwhere(res["stats"] != ref["stats"])[:5].tolist(),
                                                        res["stats"][:3].tolist(), ref["stats"][:3].tolist())
    bad = np.argwhere(gd.logodds.download() != ref["dst"])
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())
    assert np.array_equal(gs.logodds.download(), src)  # read only
    return ref


def transforms(W, Sw):
    """Rotations 0, an exact quarter turn, 0.4, 3.1 and -2 about the grids' common centre, each with the
    source on the destination, shifted half off it, and wholly off it."""
    out = []
    for th in (0.0, QUARTER, 0.4, 3.1, -2.0):
        c, s = th if isinstance(th, tuple) else (np.cos(th), np.sin(th))
        for t in ((0.0, 0.0), (0.5 * Sw * CELL + 7.0, -13.0), (-3.3, 0.45 * (W + Sw) * CELL), ((W + Sw) * CELL, 0.0)):
            out.append((c, s, t[0], t[1]))
    return np.array(out)


@pytest.mark.parametrize("mode", [gm.ADD, gm.FILL])
@pytest.mark.parametrize("Sw", [16, 40, 80])
@pytest.mark.parametrize("W", [16, 24, 52, 64])
def test_widths_rotations_and_translations(ctx, W, Sw, mode):
    rng = np.random.default_rng(W * 100 + Sw + mode)
    xf = transforms(W, Sw)
    n = len(xf)
    src, dst = map_like(rng, n, Sw), map_like(rng, n, W)
    # a dry run with no gate gives the figures; the gates are then set between them
    open_kw = dict(min_support=0, max_contra_permille=1000)
    st = gm.merge_batch(src, np.tile(centred(Sw), (n, 1)), dst, np.tile(centred(W), (n, 1)), xf, cell=CELL, dry_run=True, **open_kw)["stats"]
    sup = np.sort(st[:, 2])
    kw = dict(min_support=int(sup[n // 3]) + 1, max_contra_permille=500, mode=mode)
    ref = check(ctx, rng, src, centred(Sw), dst, centred(W), xf, what=(W, Sw, mode), **kw)
    f = ref["flags"]
    print("W %d Sw %d mode %d: flags %s; cells on the source %s" % (W, Sw, mode, f.tolist(), ref["stats"][:, 0].tolist()))
    assert (f == gm.MERGED).sum() >= 3 and (f & gm.WEAK).sum() >= 5                # merged and gated pairs side by side
    assert (ref["stats"][:, 0] == 0).sum() >= 5 and (ref["stats"][:, 0] == W * W).sum() >= (1 if Sw >= 2 * W else 0)
    assert ((ref["stats"][:, 0] > 0) & (ref["stats"][:, 0] < min(W, Sw) ** 2)).sum() >= 5  # partly off
    assert ref["stats"][f == gm.MERGED, 7].min() > 0 and not ref["stats"][f != gm.MERGED, 7].any()
    check(ctx, rng, src, centred(Sw), dst, centred(W), xf, what=(W, Sw, mode, "open"), mode=mode, **open_kw)


def test_conflict_gate_side_by_side(ctx):
    """max_contra_permille between the pairs' shares: CONFLICT and MERGED in one batch, dst of the former bit for bit."""
    rng = np.random.default_rng(11)
    W = 52
    xf = transforms(W, W)[::2]
    n = len(xf)
    src, dst = map_like(rng, n, W), map_like(rng, n, W)
    dst[dst == 0] = -41  # known free where nothing else: contradictions are possible everywhere
    st = gm.merge_batch(src, np.tile(centred(W), (n, 1)), dst, np.tile(centred(W), (n, 1)), xf, cell=CELL, dry_run=True, min_support=0,
                        max_contra_permille=1000)["stats"]
    share = np.sort(1000 * st[:, 3] // np.maximum(st[:, 2] + st[:, 3], 1))
    ref = check(ctx, rng, src, centred(W), dst, centred(W), xf, min_support=0, max_contra_permille=int(share[n // 2]))
    assert (ref["flags"] == gm.MERGED).sum() >= 2 and (ref["flags"] == gm.CONFLICT).sum() >= 2, ref["flags"].tolist()


@pytest.mark.parametrize("n", [1, 3, 130])
def test_pairs_and_a_permuted_index(ctx, n):
    rng = np.random.default_rng(n)
    W, Sw, n_src = 24, 16, max(2, n // 2)
    src, dst = map_like(rng, n_src, Sw), map_like(rng, n, W)
    idx = rng.permutation(np.arange(n) % (n_src + 2) - 1).astype(np.int32)  # -1 .. n_src: both ends are outside
    if n == 1:
        idx[:] = 1
    th = rng.uniform(-3.2, 3.2, n)
    xf = np.stack([np.cos(th), np.sin(th), rng.uniform(-100, 100, n), rng.uniform(-100, 100, n)], -1)
    so, do = CELL * rng.integers(-20, 0, (n_src, 2)).astype(np.float64), CELL * rng.integers(-20, 0, (n, 2)).astype(np.float64)
    gs, gd = grids(ctx, src, so, dst, do)
    junk_outputs(ctx, gd, rng)
    kw = dict(min_support=2, max_contra_permille=600)
    gd.merge(gs, xf, src_index=idx, **kw)
    res = gd.merge_results()
    ref = gm.merge_batch(src, so, dst, do, xf, src_index=idx, cell=CELL, **kw)
    assert np.array_equal(res["flags"], ref["flags"]) and np.array_equal(res["stats"], ref["stats"])
    assert np.array_equal(gd.logodds.download(), ref["dst"])
    if n > 1:
        assert (ref["flags"] == gm.SKIPPED).sum() >= 1 and (ref["flags"] == gm.MERGED).sum() >= 1
    # without an index pair m reads source m, and the pairs beyond the sources are skipped
    gd.upload(dst)
    junk_outputs(ctx, gd, rng)
    gd.merge(gs, xf, **kw)
    ref = gm.merge_batch(src, so, dst, do, xf, cell=CELL, **kw)
    res = gd.merge_results()
    assert np.array_equal(res["flags"], ref["flags"]) and np.array_equal(res["stats"], ref["stats"])
    assert np.array_equal(gd.logodds.download(), ref["dst"])
    assert (ref["flags"] == gm.SKIPPED).sum() == max(0, n - n_src)
    # every pair skipped: nothing moves
    gd.upload(dst)
    gd.merge(gs, xf, src_index=np.full(n, -7, np.int32), **kw)
    res = gd.merge_results()
    assert (res["flags"] == gm.SKIPPED).all() and not res["stats"].any() and np.array_equal(gd.logodds.download(), dst)


def test_dry_run_and_transforms_that_are_not_finite(ctx):
    rng = np.random.default_rng(3)
    W = 40
    bad = [(np.nan, 0.0, 0.0, 0.0), (1.0, np.inf, 0.0, 0.0), (1.0, 0.0, -np.inf, 0.0), (1.0, 0.0, 0.0, np.nan),
           (1.0, 0.0, 1e300, -1e300), (1e300, 1e300, 1e300, 1e300), (-1e300, 1e300, 0.0, 0.0), (1.0, 0.0, 1e18, 0.0),
           (np.cos(0.4), np.sin(0.4), 20.0, 30.0), (1.0, 0.0, 0.0, 0.0)]
    xf = np.array(bad)
    n = len(xf)
    src, dst = map_like(rng, n, W), map_like(rng, n, W)
    open_kw = dict(min_support=0, max_contra_permille=1000)
    ref = check(ctx, rng, src, centred(W), dst, centred(W), xf, **open_kw)
    assert ref["flags"].tolist() == [gm.BAD_XFORM] * 4 + [gm.MERGED] * 6 and not ref["stats"][:8].any()
    assert np.array_equal(ref["dst"][:8], dst[:8]) and ref["stats"][8:, 7].min() > 0
    dry = check(ctx, rng, src, centred(W), dst, centred(W), xf, dry_run=True, **open_kw)
    assert dry["flags"].tolist() == [gm.BAD_XFORM] * 4 + [0] * 6 and np.array_equal(dry["dst"], dst)
    assert np.array_equal(dry["stats"][:, :7], ref["stats"][:, :7]) and not dry["stats"][:, 7].any()
    # origins that are not finite: the source's, then the destination's
    so = np.tile(centred(W), (n, 1))
    so[1, 0], so[2, 1] = np.nan, np.inf
    do = np.tile(centred(W), (n, 1))
    do[3, 1], do[9, 0] = -np.inf, np.nan
    good = np.tile(np.array(bad[8]), (n, 1))
    idx = np.arange(n, dtype=np.int32)
    ref = check(ctx, rng, src, so, dst, do, good, src_index=idx, **open_kw)
    assert [int(f) for f in ref["flags"]] == [gm.BAD_XFORM if m in (1, 2, 3, 9) else gm.MERGED for m in range(n)]


@pytest.mark.parametrize("n", [1, 6])
def test_grid_512(ctx, n):
    """The default width: 128 tiles a pair; one pair is a workgroup a tile, six pairs two tiles a workgroup."""
    rng = np.random.default_rng(512 + n)
    W = 512
    th = np.array([0.4, -2.0, 3.1, 0.0, 1.0, 0.4])[:n]
    xf = np.stack([np.cos(th), np.sin(th), np.linspace(300.0, -900.0, 6)[:n], np.linspace(-200.0, 5000.0, 6)[:n]], -1)
    src, dst = map_like(rng, n, W, frac=0.1), map_like(rng, n, W, frac=0.1)
    ref = check(ctx, rng, src, centred(W), dst, centred(W), xf, min_support=0, max_contra_permille=1000)
    assert (ref["flags"] == gm.MERGED).all() and ref["stats"][:, 7].min() > 1000


def test_world_canvas_as_the_source(ctx):
    """A 1024-cell world() canvas of one grid is the source of another grid's merge."""
    from lidar_slam_amd.mapping import OccupancyGrid
    rng = np.random.default_rng(1024)
    W, Cw = 64, 1024
    ga = OccupancyGrid(ctx, 1, origin=centred(W), canvas_w=Cw, grid_w=W, cell=CELL)
    win, canvas = map_like(rng, 1, W), map_like(rng, 1, Cw, frac=0.05)
    ga.upload(win)
    ga.canvas.upload(canvas)
    view = ga.world()
    assert view.W == Cw
    world = view.logodds.download()
    mid = (Cw - W) // 2 // 8 * 8
    assert np.array_equal(world[0, mid:mid + W, mid:mid + W], win[0])  # the flush laid the window over the canvas
    dst = map_like(rng, 1, 80)
    gd = OccupancyGrid(ctx, 1, origin=(-2000.0, 1500.0), grid_w=80, cell=CELL)
    gd.upload(dst)
    junk_outputs(ctx, gd, rng)
    xf = np.array([np.cos(0.4), np.sin(0.4), 300.0, -200.0])
    kw = dict(min_support=0, max_contra_permille=1000)
    gd.merge(view, xf, **kw)
    ref = gm.merge(world[0], view.origin_host[0], dst[0], (-2000.0, 1500.0), xf, cell=CELL, **kw)
    res = gd.merge_results()
    assert res["flags"][0] == ref["flags"] == gm.MERGED and np.array_equal(res["stats"][0], ref["stats"])
    assert ref["stats"][0] == 80 * 80 and np.array_equal(gd.logodds.download()[0], ref["dst"])
    # and the canvas is a destination too: the small grid merged into the world view
    junk_outputs(ctx, view, rng)
    inv = np.array([np.cos(-0.4), np.sin(-0.4), 0.0, 0.0])
    small = gd.logodds.download()
    view.merge(gd, inv, **kw)
    ref = gm.merge(small[0], (-2000.0, 1500.0), world[0], view.origin_host[0], inv, cell=CELL, **kw)
    assert view.merge_results()["flags"][0] == ref["flags"] and np.array_equal(view.merge_results()["stats"][0], ref["stats"])
    assert np.array_equal(ga.canvas.download()[0], ref["dst"])
    with pytest.raises(ValueError, match="same cell"):
        gd.merge(OccupancyGrid(ctx, 1, grid_w=16, cell=25.0), xf)


def test_same_buffer_goes_through_the_snapshot(ctx):
    """A grid merged into itself under a transform: the sources are the grids as they stood before the call."""
    rng = np.random.default_rng(8)
    n, W = 3, 52
    dst = map_like(rng, n, W)
    th = np.array([0.4, np.pi / 2, -1.0])
    xf = np.stack([np.cos(th), np.sin(th), [10.0, 0.0, -55.0], [0.0, 20.0, 5.0]], -1)
    _, gd = grids(ctx, dst[:1], centred(W), dst, centred(W))
    junk_outputs(ctx, gd, rng)
    idx = np.array([1, 2, 0], np.int32)
    kw = dict(min_support=0, max_contra_permille=1000)
    for _ in range(2):  # (the second call reuses the snapshot's buffer)
        before = gd.logodds.download()
        gd.merge(gd, xf, src_index=idx, **kw)
        ref = gm.merge_batch(before, np.tile(centred(W), (n, 1)), before, np.tile(centred(W), (n, 1)), xf, src_index=idx, cell=CELL, **kw)
        res = gd.merge_results()
        assert np.array_equal(res["flags"], ref["flags"]) and np.array_equal(res["stats"], ref["stats"])
        assert np.array_equal(gd.logodds.download(), ref["dst"]) and (ref["stats"][:, 7] > 0).all()
    assert gd._merge_snap is not None and gd._merge_snap.nbytes == 2 * n * W * W


def room_revolutions():
    from test_reloc_ref import L_OUTLINE, L_POSES, revolution
    return [revolution(L_OUTLINE, p, 900 + i) for i, p in enumerate(L_POSES)]


def step_one(grid, rev, pose, sync=True):
    grid.step(rev, np.array([0, 1]), np.array([0, len(rev)]), pose=np.asarray(pose, np.float64).reshape(1, 3), sync=sync)


def test_unsynced_after_an_unsynced_step(ctx):
    """grid.step and merge enqueued back to back with sync=False equal the same calls synced one by one."""
    from lidar_slam_amd.mapping import OccupancyGrid
    from test_gridmerge_ref import origin_b, to_frame_b
    from test_reloc_ref import L_POSES, SCENE_ORIGIN
    revs = room_revolutions()
    xf = np.array([np.cos(0.4), np.sin(0.4), 300.0, -200.0])
    out = []
    for sync in (False, True):
        ga = OccupancyGrid(ctx, 1, origin=SCENE_ORIGIN)
        gb = OccupancyGrid(ctx, 1, origin=origin_b())
        for i in range(3):
            step_one(ga, revs[i], L_POSES[i], sync=sync)
            step_one(gb, revs[4 + i], to_frame_b(L_POSES[4 + i]), sync=sync)
        ga.merge(gb, xf, sync=sync)
        step_one(ga, revs[3], L_POSES[3], sync=sync)  # a reader and writer of the merged grid behind it
        ctx.sync()
        out.append((ga.logodds.download(), ga.merge_results()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1]["stats"], out[1][1]["stats"]) and out[0][1]["flags"].tolist() == out[1][1]["flags"].tolist() == [gm.MERGED]
    assert out[0][1]["stats"][0, 7] > 1000


def test_room_end_to_end(ctx):
    """Two one-robot grids mapped on the device in the two frames of tests/test_gridmerge_ref.py; robot 4's
    revolution, B's, is relocalised in A's grid; merge_transform; merge.  Under the half-turn twin of that
    transform the merge is refused with CONFLICT and A keeps every bit.  The poses, the margins and the
    quality of the merged map are tests/test_gridmerge_ref.py's (test_room_end_to_end there)."""
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import MERGE_CONFLICT, MERGE_MERGED, OccupancyGrid, merge_transform
    from test_gridmerge_ref import origin_b, share, to_frame_b
    from test_reloc_ref import CAP_MM, CAP_RAD, L_POSES, SCENE_ORIGIN, pose_error
    revs = room_revolutions()
    ga = OccupancyGrid(ctx, 1, origin=SCENE_ORIGIN)
    gb = OccupancyGrid(ctx, 1, origin=origin_b())
    for i in range(4):
        step_one(ga, revs[i], L_POSES[i])
        step_one(gb, revs[4 + i], to_frame_b(L_POSES[4 + i]))
    A0, B0 = ga.logodds.download(), gb.logodds.download()
    rel = GridRelocalizer(ctx, 1)
    rel.relocalize(revs[4], np.array([0, 1]), np.array([0, len(revs[4])]), grid=ga)
    r = rel.results()
    assert r["flags"][0] == 0
    pose_a = r["pose"][0]
    dpos, dth = pose_error(pose_a, L_POSES[4])
    assert dpos <= CAP_MM and dth <= CAP_RAD
    pose_b = to_frame_b(L_POSES[4])
    # the twin first: refused, nothing changes
    mid = to_frame_b((2000.0, 1500.0, 0.0))
    twin = merge_transform(pose_a, [2 * mid[0] - pose_b[0], 2 * mid[1] - pose_b[1], pose_b[2] + np.pi])
    ga.merge(gb, twin)
    res = ga.merge_results()
    ref = gm.merge(B0[0], origin_b(), A0[0], SCENE_ORIGIN, twin)
    assert res["flags"][0] == ref["flags"] == MERGE_CONFLICT and np.array_equal(res["stats"][0], ref["stats"])
    assert np.array_equal(ga.logodds.download(), A0)
    twin_share = share(ref["stats"])
    # the transform itself
    xf = merge_transform(pose_a, pose_b)
    ga.merge(gb, xf)
    res = ga.merge_results()
    ref = gm.merge(B0[0], origin_b(), A0[0], SCENE_ORIGIN, xf)
    print("placed to %.1f mm %.4f rad; stats %s (%.1f permille); the twin's share %.1f" % (dpos, dth, ref["stats"].tolist(), share(ref["stats"]), twin_share))
    assert res["flags"][0] == ref["flags"] == MERGE_MERGED and np.array_equal(res["stats"][0], ref["stats"])
    assert np.array_equal(ga.logodds.download()[0], ref["dst"]) and np.array_equal(gb.logodds.download(), B0)
    assert ref["stats"][7] > 4000 and (ref["dst"] != 0).sum() >= (A0 != 0).sum() + 4000
