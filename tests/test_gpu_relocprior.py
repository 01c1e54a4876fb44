"""GPU parity of relocalisation with priors (lslam_map_relocalize_prior, GridRelocalizer.relocalize with
field= and window=) against its NumPy definition, tests/relocprior_ref.py.

Everything is compared EXACTLY, as in test_gpu_reloc.py and with its means: the masked coarse volume,
n_admit, cand, the fine matcher's outputs per rank, fine_clear2, result, flags, pose_out and P_out, the
reference being fed the (cos, sin) that the device wrote to fine_rot0.  The shapes are that file's
smallest, chosen for the paths of the three new kernels: coarse widths that are no multiple of 32 (a
partial span), a map width that is no multiple of 8 (the field read cell by cell), a single admissible
bit at either end of a span, the widest bitmap with the bits and the task list beside it in LDS, point
counts around the fill of the planes and the staged tile, robots with nothing and with everything
admissible in one chunked batch, heading windows that wrap and that hold one heading, a prior call on
the scratch a plain call left, and calls that are not synced.  The field of the hand-made cases is
written straight into a DistanceField's buffer: any uint16 field is a valid input of the definition.
"""
import numpy as np
import pytest

import dist_ref as dr
import reloc_ref as rr
import relocprior_ref as rp
from test_gpu_occgrid import csr
from test_gpu_reloc import BIT_KEYS, INT_KEYS, assert_equal, fine_kw, points, random_map
from test_mapmatch_ref import pose_bits
from test_reloc_ref import L_OUTLINE, L_POSES, RECT_OUTLINE, RECT_POSES, SCENE_ORIGIN, draw_walls, scene
from test_relocprior_ref import WINDOW_OFF, inside_outline

pytestmark = pytest.mark.gpu

PRIOR_KEYS = ("n_admit", "fine_clear2")


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


class Rig:
    """A grid, a NOT_FREE field whose buffer the test fills, and a relocaliser, for R robots."""

    def __init__(self, ctx, L, origin, gkw, mkw, qkw, pkw):
        from lidar_slam_amd import _lib
        from lidar_slam_amd.localize import GridRelocalizer
        from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
        self.ctx, self.L, self.R = ctx, L, len(L)
        self.gkw, self.mkw, self.qkw, self.pkw = gkw, mkw, qkw, pkw
        self.grid = OccupancyGrid(ctx, self.R, origin=origin, **gkw)
        self.grid.upload(L)
        self.field = DistanceField(self.grid, mode=_lib.DIST_NOT_FREE, d_max=255)
        self.rel = GridRelocalizer(ctx, self.R, **mkw, **qkw, **pkw)

    def put_field(self, d2):
        self.field.d2.upload(np.ascontiguousarray(d2, np.uint16))
        self.field.steps = 1  # (the buffer holds a field)

    def call(self, arrays, d2=None, win=None, want_coarse=True, budget=None, sync=True, prior=False):
        xy, sco, cpo = csr(arrays)
        if d2 is not None:
            self.put_field(d2)
        if budget is not None:
            self.rel.set_budget(budget)
        try:
            self.rel.relocalize(xy, sco, cpo, grid=self.grid, want_coarse=want_coarse, sync=sync,
                                field=None if d2 is None else self.field, window=win, prior=prior)
        finally:
            self.rel.set_budget(0)
        return xy, cpo

    def check(self, arrays, d2=None, win=None, want_coarse=True, budget=None, what=""):
        """One call compared with the reference; returns (device results, reference)."""
        xy, cpo = self.call(arrays, d2, win, want_coarse, budget)
        res = self.rel.results()
        ref = rp.relocalize_batch(self.L, self.grid.origin_host, xy, cpo, clear_d2=d2, win_pose=win, fine_rot0=res["fine_rot0"],
                                  rot=self.rel.rot_host, head_rot=self.rel.head_rot_host, **self.gkw, **self.mkw, **self.qkw,
                                  **self.pkw)
        if not want_coarse:
            res = dict(res, coarse_scores=ref["coarse_scores"])
        assert_equal(res, ref, what)
        for key in PRIOR_KEYS:
            assert res[key].shape == ref[key].shape and np.array_equal(res[key], ref[key]), (what, key, res[key], ref[key])
        assert np.array_equal(self.grid.logodds.download(), self.L)  # read only
        if d2 is not None:
            assert np.array_equal(self.field.d2.download(), d2)
        return res, ref


def patchy_field(rng, R, W, lo=12, hi=21):
    """Values around clear_min2 = 16 in patches of 5 x 3 cells, zero elsewhere: blocks with no, one and
    several admissible fine cells."""
    d2 = np.zeros((R, W, W), np.uint16)
    for r in range(R):
        for _ in range(max(4, W * W // 60)):
            y, x = rng.integers(0, W, 2)
            d2[r, y:y + 3, x:x + 5] = rng.integers(lo, hi)
    return d2


@pytest.mark.parametrize("W,f,n_head", [(40, 2, 4), (72, 8, 5), (64, 4, 12), (36, 4, 4)])
def test_odd_widths(ctx, W, f, n_head):
    """Wc = 20, 9, 16 and 9: a partial span of 32 cells; W = 36: no 16-byte groups, the field and the map
    are read cell by cell.  The windows: in the middle, over the grid's corner, edges on cell centres."""
    rng = np.random.default_rng(W + n_head)
    R, cell = 3, 50.0
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.2)
    origin = np.array([[0.0, 0.0], [-1234.5, 777.25], [-W * cell / 2, -W * cell / 2]])
    cellc, Wc = cell * f, W // f
    half = 3.0 * cellc
    win = np.array([[origin[0, 0] + 0.52 * W * cell, origin[0, 1] + 0.47 * W * cell, 0.3],
                    [origin[1, 0] + 0.3 * cellc, origin[1, 1] + W * cell, 4.0],
                    [origin[2, 0] + 4.5 * cellc, origin[2, 1] + 3.5 * cellc, 6.2]])
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=6), dict(half_xy=half, half_theta=2.0))
    arrays = [points(rng, 40 + 25 * r, 0.45 * W * cell) for r in range(R)]
    d2 = patchy_field(rng, R, W)
    d2[:, 0, 0] = d2[:, W - 1, W - 1] = 16
    res, ref = rig.check(arrays, d2, win, what="field and window")
    assert res["n_admit"][2, 0] > 0 and 0 < res["n_admit"][0, 1] < n_head and res["coarse_scores"].any()
    only_field, _ = rig.check(arrays, d2, None, what="field")
    assert np.all(only_field["n_admit"][:, 1] == n_head) and np.all(only_field["n_admit"][:, 0] < Wc * Wc)
    assert np.all(only_field["cand"][0, :, 3] > 0)
    only_win, _ = rig.check(arrays, None, win, what="window")
    assert not only_win["fine_clear2"].any() and only_win["n_admit"][2].tolist()[0] == 49  # 7 x 7 centres, the edges inclusive


def test_single_bit_spans(ctx):
    """Wc = 64, two spans a row: one admissible cell at bit 0 and at bit 31 of either span, and the same
    by the window alone (a box of half side 0 on the cell's centre)."""
    rng = np.random.default_rng(31)
    W, f, cell, n_head = 128, 2, 50.0, 4
    cells = [(5, 0), (17, 31), (40, 32), (63, 63)]
    R = len(cells)
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.3)
    origin = np.tile([-3200.0, -3200.0], (R, 1))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=3), dict(half_xy=0.0, half_theta=np.inf))
    arrays = [points(rng, 120, 2500.0) for _ in range(R)]
    d2 = np.zeros((R, W, W), np.uint16)
    win = np.zeros((R, 3))
    for r, (ty, tx) in enumerate(cells):
        d2[r, f * ty + 1, f * tx] = 16
        win[r] = (origin[r, 0] + (tx + 0.5) * cell * f, origin[r, 1] + (ty + 0.5) * cell * f, 1.0)
    for what, a, b in (("field", d2, None), ("window", None, win)):
        res, _ = rig.check(arrays, a, b, what=what)
        assert res["n_admit"].tolist() == [[1, n_head]] * R
        for r, (ty, tx) in enumerate(cells):
            on = np.argwhere(res["coarse_scores"][r].any(0)).tolist()
            assert on == [[ty, tx]], (what, r, on)


def test_widest_bitmap(ctx):
    """Wc = 256: eight spans a row, 2048 tasks, the largest LDS (the bitmap, the bits and the list)."""
    rng = np.random.default_rng(256)
    W, cell = 512, 20.0
    mkw, qkw = fine_kw(4)
    L = random_map(rng, 1, W, 0.01)
    rig = Rig(ctx, L, np.array([[-5120.0, -5120.0]]), dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=2),
              dict(half_xy=3000.0, half_theta=2.0))
    arrays = [points(rng, 100, 0.3 * W * cell)]
    d2 = patchy_field(rng, 1, W)
    d2[0, 0, 0] = d2[0, W - 1, W - 1] = d2[0, 300, 511] = 16
    res, _ = rig.check(arrays, d2, np.array([[-3000.0, 2500.0, 0.5]]))
    assert res["coarse_scores"].shape == (1, 4, 256, 256) and res["cand"][0, 0, 3] > 0 and 0 < res["n_admit"][0, 0] < 65536
    res, _ = rig.check(arrays, d2, None, what="field alone")  # the corners' cells are in the set
    assert res["cand"][0, 0, 3] > 1


def test_point_counts(ctx):
    """Revolutions of 0, 1, 63, 65, 248, 250 and 2049 points: shorter and longer than a wave, around a fill
    of the planes and a staged tile."""
    sizes = (0, 1, 63, 65, 248, 250, 2049)
    rng = np.random.default_rng(sum(sizes))
    W, f, cell, R = 64, 4, 50.0, len(sizes)
    mkw, qkw = fine_kw(8)
    L = random_map(rng, R, W, 0.15)
    arrays = [points(rng, n, 0.5 * W * cell, junk=0.08) for n in sizes]
    arrays[1] = np.array([[120.0, -260.0]])
    origin = np.tile([-1600.0, -1600.0], (R, 1))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell, max_range=4000.0), mkw, dict(qkw, factor=f),
              dict(half_xy=1100.0, half_theta=1.7))
    win = np.column_stack([rng.uniform(-600.0, 600.0, (R, 2)), rng.uniform(0.0, 6.28, R)])
    res, _ = rig.check(arrays, patchy_field(rng, R, W), win)
    assert res["n_used"].tolist() == [len(rr.used_points(a, 4000.0)) for a in arrays]
    assert res["flags"][0] == rr.LOST and not res["coarse_scores"][0].any() and np.all(res["cand"][:, 0, 0] == -1)
    assert res["coarse_scores"][-1].any() and np.all(res["n_admit"] > 0)


def test_mixed_batch_in_chunks(ctx):
    """130 robots through a budget of three volumes (44 chunks).  First robot 77 alone has any admissible
    cell; then, on the scratch and the buffers that call left, a batch in which robot 5 has none
    and robot 9 has them all."""
    rng = np.random.default_rng(130)
    W, f, cell, n_head, R = 48, 4, 50.0, 6, 130
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.12)
    arrays = [points(rng, 30 + r % 7, 0.5 * W * cell, junk=0.05) for r in range(R)]
    origin = rng.uniform(-2000.0, 0.0, (R, 2))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=2), dict())
    one = n_head * (W // f) ** 2 * 4
    d2 = np.zeros((R, W, W), np.uint16)
    d2[77, 10:30, 8:40] = 100
    res, _ = rig.check(arrays, d2, None, budget=3 * one, what="robot 77 alone")
    assert np.nonzero(res["n_admit"][:, 0])[0].tolist() == [77] and res["cand"][0, 77, 3] > 0
    lost = np.arange(R) != 77
    assert np.all(res["flags"][lost] == rr.LOST) and np.all(res["cand"][:, lost, 0] == -1) and not res["coarse_scores"][lost].any()
    d2 = patchy_field(rng, R, W)
    d2[5], d2[9] = 0, 100
    res, _ = rig.check(arrays, d2, None, budget=3 * one, what="none and all")
    assert res["n_admit"][5, 0] == 0 and res["flags"][5] == rr.LOST and np.all(res["cand"][:, 5, 0] == -1)
    assert res["n_admit"][9, 0] == (W // f) ** 2 and res["cand"][0, 9, 3] > 0
    whole, _ = rig.check(arrays, d2, None, what="default budget")  # no result depends on the chunking
    for key in INT_KEYS + BIT_KEYS + PRIOR_KEYS + ("pose", "fine_rot0"):
        a, b = (pose_bits(v[key]) if v[key].dtype == np.float64 else v[key] for v in (whole, res))
        assert np.array_equal(a, b), key


def test_null_priors_equal_the_plain_call(ctx):
    """Neither pointer given: every output of the embedded batch is lslam_map_relocalize's, byte for byte,
    the coarse volume included, in one chunk and in chunks."""
    rng = np.random.default_rng(7)
    W, f, cell, n_head, R = 72, 4, 50.0, 5, 5
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.12)
    arrays = [points(rng, n, 0.5 * W * cell, junk=0.05) for n in (90, 0, 33, 300, 64)]
    origin = rng.uniform(-2000.0, 0.0, (R, 2))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=5), dict())
    rig.call(arrays)
    plain = rig.rel.results()
    assert "n_admit" not in plain and plain["cand"][0, 0, 3] > 0
    for key in ("cand", "fine_best", "result", "flags", "coarse_scores"):  # (the buffers are the same: clear them)
        buf = rig.rel.coarse if key == "coarse_scores" else rig.rel.ranks.get(key, getattr(rig.rel, key, None))
        buf.fill_zero()
    for budget in (None, 2 * n_head * (W // f) ** 2 * 4):
        rig.call(arrays, budget=budget, prior=True)
        res = rig.rel.results()
        for key in plain:
            a, b = (v[key].view(np.uint64) if v[key].dtype == np.float64 else v[key] for v in (plain, res))
            assert np.array_equal(a, b), (budget, key)
        assert res["n_admit"].tolist() == [[(W // f) ** 2, n_head]] * R and not res["fine_clear2"].any()


def test_stale_scratch_and_moving_masks(ctx):
    """The coarse volume in the context's scratch: a plain call fills it, a prior call with a small set
    follows, then one with another set.  Skipped cells read 0 to the peak pass, or stale peaks would
    be candidates."""
    rng = np.random.default_rng(17)
    W, f, cell, n_head, R = 64, 4, 50.0, 12, 4
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.25)
    arrays = [points(rng, 150, 0.5 * W * cell) for _ in range(R)]
    origin = np.tile([-1600.0, -1600.0], (R, 1))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=8), dict(half_xy=450.0, half_theta=0.6))
    rig.call(arrays, want_coarse=False)
    plain = rig.rel.results()
    win = np.array([[-900.0, -800.0, 6.2], [700.0, 900.0, 0.05], [0.0, 0.0, 3.0], [900.0, -900.0, 1.5]])
    first, _ = rig.check(arrays, None, win, want_coarse=False, what="after the plain call")
    assert np.all(plain["cand"][0, :, 0] >= 0) and not np.array_equal(first["cand"], plain["cand"])
    # the plain call's best peak lies outside the set for some robot: left in the scratch, it would be a candidate
    assert any(first["coarse_scores"][r, k, ty, tx] == 0 for r, (k, ty, tx, _) in enumerate(plain["cand"][0]))
    moved = win[::-1].copy()
    rig.check(arrays, patchy_field(rng, R, W), moved, want_coarse=False, what="after another set")


@pytest.mark.parametrize("half_theta,thetas,want", [
    (0.6, [6.2, 0.05, 3.0, -0.5], [[0, 11], [0, 1, 11], [5, 6], [0, 10, 11]]),          # n_head 12: a step of 0.5236 rad
    (0.0, [0.0, 7 * (2 * np.pi / 12), 11 * (2 * np.pi / 12), 0.1], [[0], [7], [11], []])])
def test_heading_windows(ctx, half_theta, thetas, want):
    """Windows that wrap across k = 0 and windows of one heading (half_theta 0 on a heading's own bits), and a
    robot with no heading at all: the slices divide the admissible headings, not all n_head."""
    rng = np.random.default_rng(12)
    W, f, cell, n_head, R = 64, 4, 50.0, 12, len(thetas)
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W, 0.25)
    arrays = [points(rng, 90, 0.5 * W * cell) for _ in range(R)]
    origin = np.tile([-1600.0, -1600.0], (R, 1))
    rig = Rig(ctx, L, origin, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=4), dict(half_xy=np.inf, half_theta=half_theta))
    win = np.column_stack([np.zeros((R, 2)), thetas])
    res, ref = rig.check(arrays, None, win)
    for r in range(R):
        assert np.nonzero(res["coarse_scores"][r].any((1, 2)))[0].tolist() == want[r], r
        assert res["n_admit"][r].tolist() == [256, len(want[r])]
    assert res["flags"][-1] == rr.LOST or want[-1]


@pytest.fixture(scope="module")
def rooms():
    """Eight robots at W 256 (cells of 40 mm, the rooms of test_reloc_ref at their size): four poses of the
    L-shaped room and the two of the plain room twice, unknown space outside the walls."""
    picks = [("L", 0), ("L", 6), ("rect", 0), ("rect", 1), ("L", 3), ("rect", 0), ("L", 5), ("rect", 1)]
    maps = {}
    for which, outline in (("L", L_OUTLINE), ("rect", RECT_OUTLINE)):
        walls = draw_walls(outline, grid_w=256, cell=40.0)
        maps[which] = np.where((walls < 85) & ~inside_outline(outline, 256, 40.0), 0, walls).astype(np.int16)
    L = np.stack([maps[w] for w, _ in picks])
    arrays = [scene(w)[2][i] for w, i in picks]
    truth = np.array([(L_POSES if w == "L" else RECT_POSES)[i] for w, i in picks])
    return L, arrays, truth


def test_rooms_with_field_and_window_unsynced(ctx, rooms):
    """The rooms through GridRelocalizer with field= and window=, the filter's stale mean as the window and
    as the output, nothing synced between the field's step, the relocalisation and a scan-to-map match
    from the re-seated mean: the chain equals the reference, and the synced calls."""
    from lidar_slam_amd import _lib
    from lidar_slam_amd.localize import GridLocalizer, GridRelocalizer
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    from lidar_slam_amd.slam import LandmarkMap
    L, arrays, truth = rooms
    R = len(L)
    xy, sco, cpo = csr(arrays)
    gkw = dict(grid_w=256, cell=40.0)
    stale = truth + WINDOW_OFF
    P0 = np.arange(9.0 * R).reshape(R, 3, 3) + 1.0
    d2_ref = dr.field_batch(L, mode=dr.NOT_FREE)[0]
    runs = []
    for sync in (False, True):
        grid = OccupancyGrid(ctx, R, origin=SCENE_ORIGIN, **gkw)
        grid.upload(L)
        lm = LandmarkMap(ctx, R, seeds=list(range(R)), x0=stale, P0=P0)
        field = DistanceField(grid, mode=_lib.DIST_NOT_FREE)
        rel, loc = GridRelocalizer(ctx, R, win_w=256), GridLocalizer(ctx, R, win_w=256)
        field.step(sync=sync)
        rel.relocalize(xy, sco, cpo, grid=grid, lm=lm, field=field, window=lm, want_coarse=True, sync=sync)
        loc.step(xy, sco, cpo, grid=grid, pose=lm, sync=sync)  # reads the mean the relocalisation wrote
        ctx.sync()
        runs.append((rel.results(), loc.results(), field.d2.download()))
    (res, after, d2), (res_s, after_s, _) = runs
    assert np.array_equal(d2, d2_ref)
    ref = rp.relocalize_batch(L, np.tile(SCENE_ORIGIN, (R, 1)), xy, cpo, clear_d2=d2_ref, win_pose=stale, pose_in=stale, P_in=P0,
                              fine_rot0=res["fine_rot0"], win_w=256, **gkw)
    assert_equal(res, ref)
    for key in PRIOR_KEYS:
        assert np.array_equal(res[key], ref[key]), key
    for a, b in ((res, res_s), (after, after_s)):
        for key in a:
            assert np.array_equal(pose_bits(a[key]) if a[key].dtype == np.float64 else a[key],
                                  pose_bits(b[key]) if b[key].dtype == np.float64 else b[key]), key
    print("flags", res["flags"].tolist(), "n_admit", res["n_admit"].tolist(), "winner's clear2",
          [int(res["fine_clear2"][max(w, 0), r]) for r, w in enumerate(res["result"][:, 0])])
    found = res["flags"] == 0
    assert found.all()  # (measured with the reference: all eight, 21 mm off at worst, the plain rooms without a rival)
    err = np.array([np.hypot(*(res["pose"][r, :2] - truth[r, :2])) for r in np.nonzero(found)[0]])
    assert err.max() <= 60.0  # 1.5 cells of 40 mm, the cap of test_reloc_ref in cells
    keep = ~found
    assert np.array_equal(pose_bits(res["pose"][keep]), pose_bits(stale[keep]))
    with pytest.raises(ValueError):
        rel.relocalize(xy, sco, cpo, grid=grid, field=DistanceField(grid))  # an OCC field
    with pytest.raises(ValueError):
        GridRelocalizer(ctx, R, clear_min2=4097).relocalize(xy, sco, cpo, grid=grid, field=field)  # d_max 64 saturates below
    with pytest.raises(ValueError):
        GridRelocalizer(ctx, R, half_xy=-1.0)
