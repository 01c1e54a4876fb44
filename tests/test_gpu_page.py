"""GPU parity of the paged rolling grid (lslam_grid_recentre_paged, lslam_grid_page_flush,
lslam_grid_page_load; OccupancyGrid(canvas_w=...)) against its NumPy definition, tests/page_ref.py.

Everything is integers and 16-bit patterns (the origin: two rounded operations), so logodds, canvas,
win, moved, the page flags and the recentre batch's shift, flags and origin are compared EXACTLY, as
whole arrays: the windows and canvases hold random int16 values, so a stray write, or a cell copied
from the wrong place, differs from the reference.

The kernel copies a strip on one of two paths per robot: 16-byte groups where grid_w, canvas_w, sx and
wx are multiples of 8, a lane per cell otherwise.  With margin = W / 2 the pose chooses the shift, so a
batch holds both paths side by side: shifts of both signs, diagonal, zero, a whole window and more;
windows inside the canvas, with a wx that is no multiple of 8, half off each edge and wholly off."""
import numpy as np
import pytest

import dist_ref as dr
import page_ref as pr
import recentre_ref as rr
from test_page_ref import CELL, WALKS, bits, kw_for, make_walk, pose_for, rnd16, run_walk_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def make_grid(ctx, L0, canvas0, win, origin, W, Cw):
    from lidar_slam_amd.mapping import OccupancyGrid
    g = OccupancyGrid(ctx, len(L0), origin=origin, canvas_w=Cw, win=win, grid_w=W, cell=CELL)
    g.upload(L0)
    g.canvas.upload(canvas0)
    return g


def state(g):
    res = g.recentre_results()
    res["logodds"], res["canvas"] = g.logodds.download(), g.canvas.download()
    return res


def assert_same(res, ref, what=""):
    for key, rkey in (("shift", "shift"), ("flags", "flags"), ("win", "win"), ("moved", "moved"), ("page_flags", "page_flags")):
        assert np.array_equal(res[key], ref[rkey]), (what, key, np.argwhere(res[key] != ref[rkey])[:5].tolist())
    assert np.array_equal(bits(res["origin"]), bits(ref["origin"])), what
    for key, rkey in (("logodds", "L"), ("canvas", "canvas")):
        bad = np.argwhere(res[key] != ref[rkey])
        assert bad.size == 0, (what, key, len(bad), bad[:5].tolist(), ref["shift"][np.unique(bad[:, 0])[:8]].tolist(),
                               ref["win"][np.unique(bad[:, 0])[:8]].tolist())


def run(ctx, rng, W, Cw, quantum, shifts, wins):
    """One paged recentre of freshly uploaded windows and canvases against the reference."""
    R = len(shifts)
    origin = CELL * rng.integers(-50, 50, (R, 2)).astype(np.float64)
    pose = np.stack([pose_for(origin[r], W, *shifts[r]) for r in range(R)])
    L0, canvas0 = rnd16(rng, (R, W, W)), rnd16(rng, (R, Cw, Cw))
    wins = np.asarray(wins, np.int32).reshape(R, 2)
    g = make_grid(ctx, L0, canvas0, wins, origin, W, Cw)
    g.recentre(pose, margin=W // 2, quantum=quantum)
    res = state(g)
    ref = pr.recentre_paged_batch(L0, canvas0, wins, pose, origin, **kw_for(W, quantum))
    assert np.array_equal(ref["shift"], np.asarray(shifts)), "the pose chose the shift"
    assert_same(res, ref, (W, Cw, quantum))
    assert np.array_equal(bits(g.origin.download()), bits(ref["origin"]))
    return g, res, ref, (L0, canvas0, wins, pose, origin)


def shifts_for(W, quantum):
    if quantum == 8:
        Wr = (W + 7) // 8 * 8  # a whole window, in multiples of the quantum
        return [(0, 0), (8, 0), (0, -8), (8, -8), (-16, 8), (-8, -16), (Wr, 0), (0, -Wr), (Wr + 8, -8), (-8, Wr - 16)]
    return [(0, 0), (3, 0), (0, -5), (8, 1), (-8, 8), (-3, 7), (5, -9), (W - 1, 1), (W, 0), (0, -W), (W + 3, -2), (-1, W + 1)]


def wins_for(W, Cw):
    """Inside on a group, inside with a wx off the groups, half off each edge, two corners, wholly off."""
    mid = (Cw - W) // 2 // 8 * 8
    return [(mid, mid), (mid + 3, mid), (mid, mid + 5), (0, 0), (Cw - W, Cw - W), (-(W // 2), 8), (Cw - W // 2, 8), (8, -(W // 2)),
            (8, Cw - W // 2), (-(W // 2), Cw - W // 2), (-W - 8, 0), (0, Cw + 16), (-5 * Cw, 3)]


@pytest.mark.parametrize("quantum", [1, 8])
@pytest.mark.parametrize("W,Cw", [(16, 40), (24, 64), (64, 128), (20, 44)])
def test_every_shift_and_window(ctx, W, Cw, quantum):
    rng = np.random.default_rng(W * 1000 + Cw + quantum)
    cases = [(s, w) for s in shifts_for(W, quantum) for w in wins_for(W, Cw)]
    shifts, wins = [c[0] for c in cases], [c[1] for c in cases]
    g, res, ref, _ = run(ctx, rng, W, Cw, quantum, shifts, wins)
    s, w = np.array(shifts), np.array(wins)
    groups = s.any(1) & (s[:, 0] % 8 == 0) & (w[:, 0] % 8 == 0) & (W % 8 == 0) & (Cw % 8 == 0)
    print("W %d Cw %d quantum %d: %d robots, %d on 16-byte groups, %d a lane per cell, %d lost cells, %d loaded some"
          % (W, Cw, quantum, len(s), groups.sum(), (s.any(1) & ~groups).sum(), ref["page_flags"].sum(), (ref["moved"][:, 1] > 0).sum()))
    assert (groups.sum() > 0) == (W % 8 == 0) and (s.any(1) & ~groups).sum() > 0  # both paths in one launch
    assert ref["page_flags"].sum() > 10 and (ref["moved"][:, 1] > 0).sum() > 10 and (ref["flags"] & rr.CLEARED).sum() > 10
    # a second recentre with the same poses finds every robot in the middle: nothing changes
    before = state(g)
    g.recentre(np.stack([pose_for(before["origin"][r], W, 0, 0) for r in range(len(s))]), margin=W // 2, quantum=quantum)
    again = state(g)
    assert not again["shift"].any() and not again["flags"].any() and not again["moved"].any() and not again["page_flags"].any()
    for key in ("logodds", "canvas", "win"):
        assert np.array_equal(again[key], before[key]), key
    assert np.array_equal(bits(again["origin"]), bits(before["origin"]))


def test_band_seams(ctx):
    """grid_w 256: the in-place shift goes in bands of 64 rows, and the strips meet it at their seams."""
    from lidar_slam_amd.mapping import recentre_band_rows
    W, Cw = 256, 512
    B = recentre_band_rows(W)
    assert B == 64
    rng = np.random.default_rng(77)
    for quantum, shifts in ((1, [(1, B - 1), (-8, B), (9, -(B + 1)), (0, 2 * B), (-(B + 1), -1), (B, B)]),
                            (8, [(8, B), (-B, -B), (0, B + 8), (B - 8, -8), (-2 * B, 3 * B)])):
        wins = [(128, 128), (131, 120), (-40, 300), (300, -40), (128, 128), (8, 8)][:len(shifts)]
        run(ctx, rng, W, Cw, quantum, shifts, wins)


@pytest.mark.parametrize("R", [1, 9, 130])
def test_fleets(ctx, R):
    """9 robots: a launch padded to 16 workgroups; 130: more than one group of 64 in the block permutation.
    One robot alone computes what it computes in the fleet."""
    W, Cw, quantum = 16, 40, 8
    rng = np.random.default_rng(R)
    all_s, all_w = shifts_for(W, quantum), wins_for(W, Cw)
    shifts = [all_s[i] for i in rng.integers(0, len(all_s), R)]
    wins = [all_w[i] for i in rng.integers(0, len(all_w), R)]
    shifts[-1], wins[-1] = (8, -8), (11, 8)  # the last robot moves, a lane per cell
    g, res, ref, (L0, canvas0, wins, pose, origin) = run(ctx, rng, W, Cw, quantum, shifts, wins)
    for r in sorted({0, R // 2, R - 1}):
        g1 = make_grid(ctx, L0[r:r + 1], canvas0[r:r + 1], wins[r:r + 1], origin[r:r + 1], W, Cw)
        g1.recentre(pose[r:r + 1], margin=W // 2, quantum=quantum)
        one = state(g1)
        for key in res:
            assert one[key].tobytes() == res[key][r:r + 1].tobytes(), (r, key)


def test_one_in_sixteen_moves(ctx):
    W, Cw, quantum, R = 64, 128, 8, 64
    rng = np.random.default_rng(16)
    moving = np.arange(R) % 16 == 5
    shifts = [(16, -8) if m else (0, 0) for m in moving]
    g, res, ref, (L0, canvas0, wins, pose, origin) = run(ctx, rng, W, Cw, quantum, shifts, [(32, 32)] * R)
    still = ~moving
    assert np.array_equal(res["logodds"][still], L0[still]) and np.array_equal(res["canvas"][still], canvas0[still])
    assert np.array_equal(res["win"][still], wins[still]) and np.array_equal(bits(res["origin"][still]), bits(origin[still]))
    assert not res["moved"][still].any() and np.all(res["moved"][moving] == [16 * 64 + 8 * 48] * 2)
    assert res["flags"].tolist() == [rr.MOVED if m else 0 for m in moving]


def write_rows(ctx, g, staged, y0, y1, x0, x1):
    """Rows of a staged [W, W] device array into robot 0's window, on the stream."""
    W = g.W
    for y in range(y0, y1):
        off = (y * W + x0) * 2
        ctx.copy(g.logodds.addr + off, staged.addr + off, (x1 - x0) * 2)


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_unsynced(ctx, name):
    """The 12-step walk of tests/test_page_ref.py with sync=False throughout and one sync at the end; the
    same poses and writes through the plain recentre on a second grid."""
    from lidar_slam_amd.mapping import OccupancyGrid
    w = WALKS[name]
    W, Cw, q = w["W"], w["Cw"], w["quantum"]
    L, canvas, win, origin, model, log = run_walk_ref(name)
    origin0 = np.array([[-400.0, 260.0]])
    paged = OccupancyGrid(ctx, 1, origin=origin0, canvas_w=Cw, win=w["win"], grid_w=W, cell=CELL)
    plain = OccupancyGrid(ctx, 1, origin=origin0, grid_w=W, cell=CELL)
    assert plain.canvas is None and not hasattr(plain, "win")
    steps = make_walk(name)
    # the poses follow the origins, which the reference gives; the writes are staged on the device beforehand
    o, poses, staged = origin0[0], [], []
    for (s, (y0, y1, x0, x1, v)), ref in zip(steps, log):
        poses.append(ctx.to_device(pose_for(o, W, *s)[None]))
        o = ref["origin"]
        full = np.zeros((W, W), np.int16)
        full[y0:y1, x0:x1] = v
        staged.append(ctx.to_device(full))
    ctx.sync()
    for (s, (y0, y1, x0, x1, v)), pose, st in zip(steps, poses, staged):
        for g in (paged, plain):
            g.recentre(pose, margin=W // 2, quantum=q, sync=False)
            write_rows(ctx, g, st, y0, y1, x0, x1)
    paged.flush(sync=False)
    ctx.sync()
    res = state(paged)
    assert np.array_equal(res["logodds"][0], L) and np.array_equal(res["win"][0], win) and np.array_equal(bits(res["origin"][0]), bits(origin))
    assert np.array_equal(res["canvas"][0], model)  # flushed: the canvas is the world
    assert np.array_equal(res["shift"][0], log[-1]["shift"]) and res["moved"][0].tolist() == [W * W, 0]
    Lp = plain.logodds.download()[0]
    assert np.array_equal(Lp, run_walk_ref(name, plain=True)[0])
    assert np.any((Lp == 0) & (L != 0)) and "moved" not in plain.recentre_results()


@pytest.mark.parametrize("W,s,q", [(16, (8, 0), 8), (64, (-8, 16), 8), (24, (5, -3), 1)])
def test_out_and_back(ctx, W, s, q):
    """The old cells return; the plain call holds zeros there."""
    from lidar_slam_amd.mapping import OccupancyGrid
    Cw = 128
    rng = np.random.default_rng(W)
    L0 = rnd16(rng, (1, W, W)) | 1
    origin0 = np.array([[200.0, -40.0]])
    paged = OccupancyGrid(ctx, 1, origin=origin0, canvas_w=Cw, grid_w=W, cell=CELL)
    plain = OccupancyGrid(ctx, 1, origin=origin0, grid_w=W, cell=CELL)
    win0 = paged.win.download()
    assert win0.tolist() == [[(Cw - W) // 2 // 8 * 8] * 2]
    for g in (paged, plain):
        g.upload(L0)
        for sx, sy in (s, (-s[0], -s[1])):
            g.recentre(pose_for(g.origin_host[0], W, sx, sy)[None], margin=W // 2, quantum=q)
            assert g.recentre_results()["shift"].tolist() == [[sx, sy]]
    assert np.array_equal(paged.logodds.download(), L0) and np.array_equal(paged.win.download(), win0)
    assert np.array_equal(bits(paged.origin_host), bits(origin0))
    gone = pr.leaving(W, *s)
    Lp = plain.logodds.download()[0]
    assert gone.any() and not Lp[gone].any() and np.array_equal(Lp[~gone], L0[0][~gone])


@pytest.mark.parametrize("W,Cw", [(16, 40), (20, 44), (64, 128)])
def test_flush_and_load(ctx, W, Cw):
    rng = np.random.default_rng(W + Cw)
    wins = np.array(wins_for(W, Cw), np.int32)
    R = len(wins)
    L0, canvas0 = rnd16(rng, (R, W, W)) | 1, rnd16(rng, (R, Cw, Cw)) | 1
    g = make_grid(ctx, L0, canvas0, wins, np.zeros((R, 2)), W, Cw)
    g.flush()
    flushed = np.stack([pr.flush(L0[r], canvas0[r], wins[r])[0] for r in range(R)])
    stored = np.array([pr.flush(L0[r], canvas0[r], wins[r])[1] for r in range(R)])
    assert np.array_equal(g.canvas.download(), flushed) and np.array_equal(g.moved.download(), stored)
    assert np.array_equal(g.logodds.download(), L0) and np.array_equal(g.win.download(), wins)
    g.clear()
    g.load()
    back = g.logodds.download()
    want = np.stack([pr.load(flushed[r], wins[r], W)[0] for r in range(R)])
    assert np.array_equal(back, want) and np.array_equal(g.moved.download(), stored[:, ::-1])
    assert np.array_equal(g.canvas.download(), flushed)
    inside = [r for r in range(R) if stored[r, 0] == W * W]
    assert len(inside) >= 4 and np.array_equal(back[inside], L0[inside])  # restored bit for bit
    half = int(np.flatnonzero((wins[:, 0] == -(W // 2)) & (wins[:, 1] == 8))[0])
    assert not back[half][:, :W // 2].any() and np.array_equal(back[half][:, W // 2:], L0[half][:, W // 2:])
    # a load into a window that held other values: every cell is written
    g.upload(rnd16(rng, (R, W, W)) | 1)
    g.load(sync=False)
    g.ctx.sync()
    assert np.array_equal(g.logodds.download(), want)


def test_world_view_is_a_grid(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import DistanceField, GridRayCaster, OccupancyGrid
    W, Cw, R = 16, 64, 3
    rng = np.random.default_rng(4)
    L0 = rng.choice(np.array([-41, 0, 0, 85, 350], np.int16), (R, W, W))
    canvas0 = rng.choice(np.array([-41, 0, 0, 0, 85], np.int16), (R, Cw, Cw))
    wins = np.array([(24, 24), (-8, 40), (51, 3)], np.int32)
    origin = np.array([[0.0, 0.0], [400.0, -200.0], [-60.0, 20.0]])
    g = make_grid(ctx, L0, canvas0, wins, origin, W, Cw)
    world = g.world()
    ref = np.stack([pr.world_view(L0[r], canvas0[r], wins[r]) for r in range(R)])
    assert world.W == Cw and world.p.grid_w == Cw and g.p.grid_w == W and world.logodds is g.canvas
    assert np.array_equal(world.logodds.download(), ref)
    assert np.array_equal(world.origin_host, origin - wins * CELL)
    field = DistanceField(world, d_max=20)
    field.step()
    got = field.results()
    d2, n_src, flags = dr.field_batch(ref, d_max=20)
    assert np.array_equal(got["d2"], d2) and np.array_equal(got["n_src"], n_src) and np.array_equal(got["flags"], flags)
    GridRayCaster(world)  # (its parameters are checked against the view's geometry)
    # a canvas that overlaps the window's grids is refused
    pg = g._page_batch()
    pg.canvas = g.logodds.addr + 2
    b = _lib.RecentreBatch()
    b.n_robots = R
    b.pose = b.origin = b.shift = b.flags = g.moved.addr  # (never read: the call is refused first)
    b.logodds = g.logodds.addr
    with pytest.raises(ValueError, match="overlaps"):
        _lib.call("lslam_grid_recentre_paged", ctx, b, pg, g.p, _lib.recentre_params(margin=W // 2), g.pp)
    with pytest.raises(ValueError, match="overlaps"):
        _lib.call("lslam_grid_page_flush", ctx, pg, g.logodds.addr, g.p, g.pp)


def test_timing_slot_and_arguments(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import OccupancyGrid
    W, Cw = 16, 40
    g = OccupancyGrid(ctx, 2, grid_w=W, cell=CELL, canvas_w=Cw)
    pose = np.stack([pose_for(g.origin_host[r], W, 8, 0) for r in range(2)])
    ctx.set_timing(True, kernels=[_lib.K_RECENTRE])
    ctx.timing_reset()
    try:
        g.recentre(pose, margin=W // 2, quantum=8)
        ms, n = ctx.timing(_lib.K_RECENTRE)
        assert n == 1 and ms > 0.0  # a whole recentre: no slot of its own
    finally:
        ctx.set_timing(False)
    assert g.recentre_results()["moved"].tolist() == [[8 * W, 8 * W]] * 2
    for bad in (15, 2049):
        with pytest.raises(ValueError, match="canvas_w"):
            OccupancyGrid(ctx, 1, grid_w=W, canvas_w=bad)
    with pytest.raises(ValueError):
        OccupancyGrid(ctx, 1, grid_w=W, win=(0, 0))
    with pytest.raises(ValueError):
        OccupancyGrid(ctx, 1, grid_w=W).flush()
