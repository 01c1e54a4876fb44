"""GPU parity of global relocalisation (lslam_map_relocalize, lidar_slam_amd/localize.py) against its
NumPy definition, tests/reloc_ref.py.

Scores are integers and every double operation of the definition is rounded on its own, so every
output is compared EXACTLY: the coarse volume, n_occ, n_used, cand, cand_pose, the fine matcher's six
outputs per rank, result, flags, pose_out and P_out, the reference being fed the (cos, sin) that the
device wrote to fine_rot0 for the candidate poses: those bits are the fine definition's input.
fine_rot0 itself is held to 1e-15 as in test_gpu_mapmatch.  The shapes are the smallest that reach
each path of the kernels: coarse widths that are no multiple of 32, one and several spans of 32 cells,
more tasks than threads (Wc = 256), point counts around the fill of the bit-sliced planes (248) and
the staged tile (2048), robots in chunks.
"""
import numpy as np
import pytest

import mapmatch_ref as mmr
import reloc_ref as rr
from test_gpu_occgrid import assert_rot, csr
from test_mapmatch_ref import pose_bits
from test_reloc_ref import CAP_MM, CAP_RAD, L_POSES, SCENE_ORIGIN, pose_error, scene, scene_case

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_occ", "n_used", "coarse_scores", "cand", "fine_best", "fine_nvalid", "fine_flags", "result", "flags")
BIT_KEYS = ("cand_pose", "fine_pose", "fine_delta")


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def assert_equal(res, ref, what=""):
    for key in INT_KEYS:
        assert res[key].shape == ref[key].shape, (what, key, res[key].shape, ref[key].shape)
        bad = np.argwhere(res[key] != ref[key])
        assert bad.size == 0, (what, key, len(bad), bad[:5])
    for key in BIT_KEYS + ("pose",):
        want = ref["pose_out" if key == "pose" else key]
        bad = np.argwhere(pose_bits(res[key]) != pose_bits(want))
        assert bad.size == 0, (what, key, len(bad), bad[:5])
    if "P" in res:
        bad = np.argwhere(pose_bits(res["P"].reshape(-1, 9)) != pose_bits(ref["P_out"]))
        assert bad.size == 0, (what, "P", bad[:5])
    assert_rot(res["fine_rot0"].reshape(-1, 2), res["cand_pose"].reshape(-1, 3))


def fine_kw(n_head, **kw):
    """The smallest fine matcher that covers one coarse quantum of n_head headings and factor <= 8."""
    head_step = 2 * np.pi / n_head
    m = dict(win_w=16, k_trans=4, k_theta=2, theta_step=head_step / 3.9, smear=1, occ_min=85, min_permille=60)
    m.update(kw)
    return m, dict(n_head=n_head, head_step=head_step)


def check(ctx, L, origin, arrays, gkw, mkw, qkw, budget=None, what=""):
    """One call on fresh objects, compared with the reference; returns (device results, reference)."""
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    R = len(arrays)
    xy, sco, cpo = csr(arrays)
    grid = OccupancyGrid(ctx, R, origin=origin, **gkw)
    grid.upload(L)
    rel = GridRelocalizer(ctx, R, **mkw, **qkw)
    if budget is not None:
        rel.set_budget(budget)
    try:
        rel.relocalize(xy, sco, cpo, grid=grid, want_coarse=True)
    finally:
        rel.set_budget(0)
    res = rel.results()
    ref = rr.relocalize_batch(L, grid.origin_host, xy, cpo, fine_rot0=res["fine_rot0"], rot=rel.rot_host,
                              head_rot=rel.head_rot_host, **gkw, **mkw, **qkw)
    assert_equal(res, ref, what)
    assert np.array_equal(grid.logodds.download(), L)  # read only
    return res, ref


def random_map(rng, R, W, frac=0.1):
    """Values around occ_min on a fraction of the cells, free space elsewhere, and occupied cells in
    the first and the last row and column."""
    L = np.full((R, W, W), -41, np.int16)
    on = rng.random((R, W, W)) < frac
    L[on] = (85 + rng.integers(-1, 2, int(on.sum()))).astype(np.int16)
    L[:, [0, W - 1], ::3] = 90
    L[:, 1::4, [0, W - 1]] = 200
    return L


JUNK = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0], [-np.inf, np.nan], [1e300, 1e300], [-1e300, 3.0]])


def points(rng, n, reach, junk=0.0):
    a = rng.uniform(-reach, reach, (n, 2))
    bad = rng.random(n) < junk
    a[bad] = JUNK[rng.integers(0, len(JUNK), int(bad.sum()))]
    return a


@pytest.mark.parametrize("W,f,n_head", [(40, 2, 4), (72, 8, 5), (64, 4, 12)])
def test_odd_widths_and_border_cells(ctx, W, f, n_head):
    """Wc = 20, 9 and 16: a partial span of 32 cells, occupied cells in row and column 0 and Wc - 1."""
    rng = np.random.default_rng(W + n_head)
    R, cell = 3, 50.0
    mkw, qkw = fine_kw(n_head)
    L = random_map(rng, R, W)
    origin = np.array([[0.0, 0.0], [-1234.5, 777.25], [-W * cell / 2, -W * cell / 2]])
    arrays = [points(rng, 40 + 25 * r, 0.45 * W * cell) for r in range(R)]
    res, _ = check(ctx, L, origin, arrays, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=f, n_cand=6))
    Wc = W // f
    C = np.stack([rr.coarse_map(L[r], W, f, 85) for r in range(R)])
    assert C[:, 0].any() and C[:, Wc - 1].any() and C[:, :, 0].any() and C[:, :, Wc - 1].any()
    assert res["coarse_scores"].shape == (R, n_head, Wc, Wc) and np.all(res["cand"][0, :, 3] > 0)


def test_widest_bitmap(ctx):
    """Wc = 256: eight spans a row, four tasks per thread, the largest LDS (above 64 KiB)."""
    rng = np.random.default_rng(256)
    W, cell = 512, 20.0
    mkw, qkw = fine_kw(4)
    L = random_map(rng, 1, W, 0.01)
    arrays = [points(rng, 100, 0.3 * W * cell)]
    res, _ = check(ctx, L, np.array([[-5120.0, -5120.0]]), arrays, dict(grid_w=W, cell=cell), mkw, dict(qkw, factor=2))
    assert res["coarse_scores"].shape == (1, 4, 256, 256) and res["cand"][0, 0, 3] > 1


@pytest.mark.parametrize("sizes", [(0, 1, 63, 65, 130), (248, 250, 2049, 2100)])
def test_point_counts(ctx, sizes):
    """Revolutions shorter and longer than a wave, a fill of the planes (248) and a staged tile (2048),
    with NaN, inf, (0, 0) and huge points, points beyond max_range, and points whose rotated offsets
    fall at and beyond +-Wc (Wc = 16, cellc = 200 mm: +-3100 mm at heading 0)."""
    rng = np.random.default_rng(sum(sizes))
    W, f, cell, R = 64, 4, 50.0, len(sizes)
    mkw, qkw = fine_kw(8)
    L = random_map(rng, R, W, 0.15)
    edge = np.array([[3100.0, 0.0], [3099.9, 10.0], [-3100.0, 5.0], [-3100.1, 0.0], [0.0, 3100.0], [20.0, -3100.1],
                     [2200.0, 2200.0], [3999.0, 0.0], [4000.0, 0.0], [4000.1, 0.0], [2900.0, 2900.0], [5000.0, -100.0]])
    arrays = []
    for n in sizes:
        a = points(rng, n, 0.5 * W * cell, junk=0.08)
        sel = rng.random(n) < 0.15
        a[sel] = edge[rng.integers(0, len(edge), int(sel.sum()))]
        arrays.append(a)
    if sizes[1] == 1:
        arrays[1] = np.array([[120.0, -260.0]])
    origin = np.tile([-1600.0, -1600.0], (R, 1))
    res, ref = check(ctx, L, origin, arrays, dict(grid_w=W, cell=cell, max_range=4000.0), mkw, dict(qkw, factor=f))
    assert res["n_used"].tolist() == [len(rr.used_points(a, 4000.0)) for a in arrays]
    if sizes[0] == 0:
        assert res["flags"][0] == rr.LOST and not res["coarse_scores"][0].any() and np.all(res["cand"][:, 0, 0] == -1)
        assert np.all(np.isnan(res["pose"][0])) and np.all(res["fine_flags"][:, 0] == mmr.BAD_POSE)


def test_mixed_batch_in_chunks(ctx):
    """Five robots with different point counts, one of them empty: the default budget, a budget of
    two robots' volumes (chunks of 2, 2 and 1) and one below a single volume (chunks of one robot)."""
    rng = np.random.default_rng(5)
    W, f, cell, n_head, R = 48, 4, 50.0, 6, 5
    mkw, qkw = fine_kw(n_head)
    qkw = dict(qkw, factor=f, n_cand=5)
    L = random_map(rng, R, W, 0.12)
    arrays = [points(rng, n, 0.5 * W * cell, junk=0.05) for n in (90, 0, 33, 300, 64)]
    origin = rng.uniform(-2000.0, 0.0, (R, 2))
    gkw = dict(grid_w=W, cell=cell)
    one = n_head * (W // f) ** 2 * 4
    whole, _ = check(ctx, L, origin, arrays, gkw, mkw, qkw, what="default budget")
    for budget in (2 * one, one - 1):
        part, _ = check(ctx, L, origin, arrays, gkw, mkw, qkw, budget=budget, what="budget %d" % budget)
        for key in INT_KEYS + BIT_KEYS + ("pose", "fine_rot0"):
            a, b = (pose_bits(v[key]) if v[key].dtype == np.float64 else v[key] for v in (whole, part))
            assert np.array_equal(a, b), (budget, key)
    assert whole["flags"][1] == rr.LOST and np.all(whole["cand"][0, [0, 2, 3, 4], 3] > 0)


@pytest.mark.parametrize("K", [1, 16])
def test_selection_rules(ctx, K):
    """A map that is its own image under quarter turns about the grid's centre, seen by points that
    are too: ties among the coarse peaks and the fine scores (the order decides, and a tie is an
    ambiguity); a map of one cell seen by one point: fewer peaks than K; 70 robots: two workgroups of
    the selection kernel."""
    rng = np.random.default_rng(16)
    W, f, cell, n_head, R = 32, 4, 100.0, 4, 70
    mkw, qkw = fine_kw(n_head, smear=0, min_permille=0)  # (no gate: every rank with a score is eligible)
    L = np.full((R, W, W), -41, np.int16)
    base = np.zeros((W, W), bool)
    base[rng.integers(0, W, 12), rng.integers(0, W, 12)] = True
    sym = base | np.rot90(base, 1) | np.rot90(base, 2) | np.rot90(base, 3)
    quarter = rng.uniform(-900.0, 900.0, (9, 2))
    ring = np.concatenate([quarter @ np.array([[c, s], [-s, c]]) for c, s in ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))])
    arrays = []
    for r in range(R):
        if r % 3 == 0:
            L[r][sym] = 100
            arrays.append(ring)
        elif r % 3 == 1:
            L[r, 5 + r % 7, 9 + r % 5] = 100
            arrays.append(np.array([[310.0 + r, -120.0]]))
        else:
            L[r] = random_map(rng, 1, W, 0.1)[0]
            arrays.append(points(rng, 30 + r, 1200.0))
    res, ref = check(ctx, L, np.tile([-1600.0, -1600.0], (R, 1)), arrays, dict(grid_w=W, cell=cell), mkw,
                     dict(qkw, factor=f, n_cand=K))
    assert res["cand"].shape == (K, R, 4)
    if K == 16:
        assert np.all(res["cand"][-1, 1::3, 0] == -1) and np.all(res["cand"][0, 1::3, 3] == 1)  # fewer peaks than K
        tied = res["cand"][:4, 0::3, 3]
        assert np.all(tied == tied[0]) and np.all(res["flags"][0::3] == rr.AMBIGUOUS)
    else:
        assert not np.any(res["flags"] & rr.AMBIGUOUS) and np.all(res["result"][:, 6] == -1)


def test_rooms_through_the_filter(ctx):
    """The L-shaped room (found) and the plain room (ambiguous) of test_reloc_ref at the defaults, two
    robots each, through GridRelocalizer.relocalize(..., lm=lm): the found robots' lm.x and lm.P are
    replaced, the ambiguous ones keep their bits; everything equals the reference."""
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    from lidar_slam_amd.slam import LandmarkMap
    picks = [("L", 0), ("rect", 0), ("L", 4), ("rect", 1)]
    R = len(picks)
    L = np.stack([scene(w)[0] for w, _ in picks])
    arrays = [scene(w)[2][i] for w, i in picks]
    xy, sco, cpo = csr(arrays)
    x0 = np.array([[0.0, 0.0, 0.0], [1.5, -2.5, 0.25], [np.nan, 3.0, 1.0], [7.0, 8.0, 9.0]])
    P0 = np.arange(9.0 * R).reshape(R, 3, 3) + 1.0
    lm = LandmarkMap(ctx, R, seeds=list(range(R)), x0=x0, P0=P0)
    grid = OccupancyGrid(ctx, R, origin=SCENE_ORIGIN)
    grid.upload(L)
    rel = GridRelocalizer(ctx, R)
    rel.relocalize(xy, sco, cpo, grid=grid, lm=lm, want_coarse=True)
    res = rel.results()
    cached = [scene_case(w, i) for w, i in picks]
    same = all(np.array_equal(pose_bits(c["fine_rot0"]), pose_bits(res["fine_rot0"][:, r])) for r, c in enumerate(cached))
    print("the device's (cos, sin) of the candidate headings are NumPy's:", same)
    if same:  # the CPU test's results, with the filter's state in the place of the NaNs
        ref = {k: np.stack([c[k] for c in cached], axis=1) for k in rr.PER_RANK}
        ref.update({k: np.stack([c[k] for c in cached]) for k in rr.PER_ROBOT})
        found = ref["flags"] == 0
        ref["pose_out"] = np.where(found[:, None], ref["pose_out"], x0)
        ref["P_out"] = np.where(found[:, None], ref["P_out"], P0.reshape(R, 9))
    else:
        ref = rr.relocalize_batch(L, grid.origin_host, xy, cpo, pose_in=x0, P_in=P0, fine_rot0=res["fine_rot0"])
    assert_equal(res, ref)
    x, P = lm.x.download(), lm.P.download().reshape(R, 9)
    assert np.array_equal(pose_bits(x), pose_bits(res["pose"])) and np.array_equal(pose_bits(P), pose_bits(res["P"].reshape(R, 9)))
    assert res["flags"].tolist() == [0, rr.AMBIGUOUS, 0, rr.AMBIGUOUS]
    assert np.array_equal(pose_bits(x[[1, 3]]), pose_bits(x0[[1, 3]]))
    assert np.array_equal(pose_bits(P[[1, 3]]), pose_bits(P0.reshape(R, 9)[[1, 3]]))
    assert np.array_equal(P[0], np.diag([2500.0, 2500.0, 0.05 * 0.05]).ravel()) and np.array_equal(P[0], P[2])
    for r, i in ((0, 0), (2, 4)):
        dpos, dth = pose_error(x[r], L_POSES[i])
        print("L-room pose", i, "found within", dpos, "mm", dth, "rad; result", res["result"][r].tolist())
        assert dpos <= CAP_MM and dth <= CAP_RAD
    for r in (1, 3):
        assert 1000 * int(res["result"][r, 7]) >= 900 * int(res["result"][r, 5])


def test_timing_id(ctx):
    """LSLAM_K_RELOC brackets the whole call; the fine stage inside it is not a map-match call."""
    from lidar_slam_amd import _lib
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    rng = np.random.default_rng(13)
    W, cell, R = 32, 100.0, 2
    mkw, qkw = fine_kw(4)
    grid = OccupancyGrid(ctx, R, origin=(-1600.0, -1600.0), grid_w=W, cell=cell)
    grid.upload(random_map(rng, R, W))
    xy, sco, cpo = csr([points(rng, 50, 1200.0) for _ in range(R)])
    rel = GridRelocalizer(ctx, R, factor=4, n_cand=3, **mkw, **qkw)
    ctx.set_timing(True, kernels=[_lib.K_MAPMATCH, _lib.K_RELOC])
    ctx.timing_reset()
    try:
        rel.relocalize(xy, sco, cpo, grid=grid)
        assert ctx.timing(_lib.K_RELOC)[1] == 1 and ctx.timing(_lib.K_MAPMATCH)[1] == 0
        rel.relocalize(xy, sco, cpo, grid=grid)
        ms, n = ctx.timing(_lib.K_RELOC)
        assert n == 2 and ms > 0.0
    finally:
        ctx.set_timing(False)
    assert "coarse_scores" not in rel.results() and "P" not in rel.results()
    with pytest.raises(ValueError):
        GridRelocalizer(ctx, R, n_cand=17)
    with pytest.raises(ValueError):
        GridRelocalizer(ctx, R, k_trans=1)  # the fine window would not cover a coarse cell
