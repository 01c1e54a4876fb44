"""GPU parity of the correlative scan matcher (lslam_scan_match, lidar_slam_amd/odometry.py)
against its NumPy definition, tests/scanmatch_ref.py.

The scores are integers and every double operation of the definition is rounded on its own, so
scores, best, flags and n_valid are compared EXACTLY; delta within 1e-9 mm and 1e-12 rad (the
refinement is one division of small integers).  The reference is given the matcher's own rotation
table: the caller's bits are the definition.

The wheel-speed round trip runs the filter with alpha = 1 and a tiny P0: the predicted mean is then
fx of the mean to rounding (the default alpha = 1e-4 has sigma weights of ~1.7e7, which turn the
half-ulp roundings of the sigma points at 40 mm into ~1e-7 mm of the mean: the filter's noise, not
the matcher's), so the 1e-9 mm / 1e-12 rad check is of u against fx alone.
"""
import numpy as np
import pytest

import scanmatch_ref as smr
from lidar_slam_amd import synth
from oracle import cpu as orc
from oracle import slam as osl
from oracle import ukf_exact
from test_scanmatch_ref import motion_pair, motions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def csr(arrays):
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int32)
    xy = np.concatenate([np.asarray(a, np.float64).reshape(-1, 2) for a in arrays] + [np.zeros((0, 2))])
    return xy, off


def device_match(ctx, pairs, ukf=None, **kw):
    from lidar_slam_amd.odometry import ScanMatcher
    ref_xy, ref_off = csr([p[0] for p in pairs])
    cur_xy, cur_off = csr([p[1] for p in pairs])
    m = ScanMatcher(ctx, len(pairs), **kw)
    m.match(ref_xy, ref_off, cur_xy, cur_off, ukf=ukf, want_scores=True)
    return m, m.results()


def assert_same(res, ref, rows=None):
    """Device results (all robots, or `rows` of them) against the reference's."""
    sel = slice(None) if rows is None else rows
    assert np.array_equal(res["scores"][sel], ref["scores"])
    assert np.array_equal(res["best"][sel], ref["best"])
    assert np.array_equal(res["flags"][sel], ref["flags"])
    assert np.array_equal(res["n_valid"][sel], ref["n_valid"])
    d = np.abs(res["delta"][sel] - ref["delta"])
    print("delta diff", d.max(axis=0))
    assert d[:, :2].max() <= 1e-9 and d[:, 2].max() <= 1e-12


def check(ctx, pairs, **kw):
    m, res = device_match(ctx, pairs, **kw)
    ref_xy, ref_off = csr([p[0] for p in pairs])
    cur_xy, cur_off = csr([p[1] for p in pairs])
    ref = smr.match_batch(ref_xy, ref_off, cur_xy, cur_off, rot=m.rot_host, **kw)
    assert_same(res, ref)
    return res, ref


def nasty_points(rng, n, grid_w, cell, k):
    """Inside the grid, outside it, within k cells of its border on either side, and exactly on cell
    boundaries (negative ones included)."""
    half = grid_w // 2 * cell
    kinds = rng.integers(0, 4, n)
    xy = rng.uniform(-half, half, (n, 2))
    out = rng.uniform(half + (k + 1) * cell, 3 * half, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    edge = (half + rng.uniform(-(k + 0.5) * cell, (k + 0.5) * cell, (n, 2))) * rng.choice([-1.0, 1.0], (n, 2))
    edge[:, 1] = np.where(rng.random(n) < 0.5, edge[:, 1], rng.uniform(-half, half, n))
    onb = rng.integers(-grid_w // 2 - k - 1, grid_w // 2 + k + 2, (n, 2)) * cell
    xy = np.where((kinds == 1)[:, None], out, xy)
    xy = np.where((kinds == 2)[:, None], edge, xy)
    xy = np.where((kinds == 3)[:, None], onb, xy)
    return xy


def test_small_and_nasty(ctx):
    kw = dict(grid_w=64, cell=100.0, smear=1, k_trans=2, k_theta=2)
    rng = np.random.default_rng(11)
    sizes = [37, 64, 65, 200, 0, 3, 50]
    pairs = []
    for i, n in enumerate(sizes):
        ref = nasty_points(rng, 150, 64, 100.0, 2)
        cur = nasty_points(rng, n, 64, 100.0, 2)
        if i < 4:  # some structure to find: part of the current scan is the reference, moved a little
            t = min(n, 30)
            cur[:t] = ref[:t] + rng.uniform(-150, 150, 2)
        if i == 5:
            cur = np.array([[np.nan, 100.0], [np.inf, -50.0], [0.0, 0.0]])
        if i == 6:
            ref = np.zeros((0, 2))
        pairs.append((ref, cur))
    res, ref = check(ctx, pairs, **kw)
    assert ref["scores"].max() > 0
    for r in (4, 5, 6):
        assert res["flags"][r] == smr.EMPTY
        assert not res["delta"][r].any() and res["best"][r].tolist() == [2, 2, 2, 0]
    assert res["n_valid"][5].tolist() == [150, 0] and res["n_valid"][6].tolist() == [0, 50]


@pytest.mark.parametrize("smear", [0, 1, 2])
def test_every_smear_mid_grid(ctx, smear):
    rng = np.random.default_rng(20 + smear)
    pairs = []
    for _ in range(2):
        ref = nasty_points(rng, 100, 130, 20.0, 3)
        cur = nasty_points(rng, 100, 130, 20.0, 3)
        cur[:60] = ref[:60] + rng.uniform(-40, 40, 2)
        pairs.append((ref, cur))
    check(ctx, pairs, grid_w=130, smear=smear, k_trans=3, k_theta=2)


def test_widest_translation_window(ctx):
    """k_trans = 15: 31 translations a row (two 16-wide tasks per row), an apron wider than a dword,
    border points in both tasks."""
    rng = np.random.default_rng(31)
    pairs = []
    for n in (90, 33):
        ref = nasty_points(rng, 120, 64, 100.0, 15)
        cur = nasty_points(rng, n, 64, 100.0, 15)
        cur[:25] = ref[:25] + rng.uniform(-900, 900, 2)
        pairs.append((ref, cur))
    check(ctx, pairs, grid_w=64, cell=100.0, smear=2, k_trans=15, k_theta=1)


@pytest.fixture(scope="module")
def default_pairs():
    """Pairs r = 0, 6, 17 of test_scanmatch_ref's list (windows near +, - and mid rotation) and
    their reference results at the default parameters, computed once."""
    ms = motions()
    rs = [0, 6, 17]
    pairs = [motion_pair(r, ms[r]) for r in rs]
    ref_xy, ref_off = csr([p[0] for p in pairs])
    cur_xy, cur_off = csr([p[1] for p in pairs])
    ukf = dict(dt=0.005, wheel_radius=50.0, wheel_base=200.0)
    ref = smr.match_batch(ref_xy, ref_off, cur_xy, cur_off, rot=smr.rot_table(20, np.pi / 360), ukf=ukf)
    return pairs, ref


def test_default_window(ctx, default_pairs):
    pairs, ref = default_pairs
    m, res = device_match(ctx, pairs)
    assert np.array_equal(m.rot_host, smr.rot_table(20, np.pi / 360))
    assert_same(res, ref)
    assert not res["flags"].any()


def test_rotation_slices(ctx, default_pairs):
    """One robot (a slice per rotation) and the same robot 40 times (fewer, longer slices) give the
    reference's volume, whatever slicing the host chose."""
    pairs, ref = default_pairs
    one = {k: v[:1] for k, v in ref.items()}
    _, res = device_match(ctx, pairs[:1])
    assert_same(res, one)
    _, res = device_match(ctx, pairs[:1] * 40)
    for r in (0, 17, 39):
        assert_same(res, one, rows=slice(r, r + 1))
    assert np.array_equal(res["scores"], np.broadcast_to(ref["scores"][:1], res["scores"].shape))


def test_long_scan_tiles(ctx):
    p0 = synth.scan_polar(500)[2]
    p1 = smr.compose(p0, [30.0, -20.0, 0.01])
    ref = synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 7, n_beams=4096))
    cur = synth.polar_to_xy_ref(*synth.scan_polar_at(p1, 8, n_beams=4096))
    res, _ = check(ctx, [(ref, cur)], k_trans=4, k_theta=2)
    assert res["n_valid"][0].tolist() == [4096, 4096]


def test_edge_flag(ctx):
    p0 = synth.scan_polar(503)[2]
    p1 = smr.compose(p0, [260.0, 0.0, 0.0])  # past the default 200 mm window
    ref = synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 30))
    cur = synth.polar_to_xy_ref(*synth.scan_polar_at(p1, 31))
    res, rf = check(ctx, [(ref, cur)], k_theta=2)
    assert rf["flags"][0] & smr.EDGE and res["flags"][0] & smr.EDGE


def test_identity(ctx):
    from lidar_slam_amd.odometry import ScanMatcher
    xy = synth.polar_to_xy_ref(*synth.scan_polar_at(synth.scan_polar(504)[2], 40))
    kw = dict(k_trans=3, k_theta=2)
    res, _ = check(ctx, [(xy, xy)], **kw)
    assert res["best"][0, :3].tolist() == [2, 3, 3]
    p = smr.params(**kw)
    G = smr.lookup_grid(xy, p)
    c = np.floor(smr.valid_points(xy) * (1.0 / p["cell"])).astype(np.int64) + p["grid_w"] // 2
    ins = np.all((c >= 0) & (c < p["grid_w"]), axis=1)
    assert res["best"][0, 3] == G[c[ins, 1], c[ins, 0]].sum()
    # two calls: identical bytes
    off = np.array([0, len(xy)], np.int32)
    m = ScanMatcher(ctx, 1, **kw)
    outs = []
    for _ in range(2):
        m.match(xy, off, xy, off, want_scores=True)
        r = m.results()
        outs.append(b"".join(r[k].tobytes() for k in ("scores", "delta", "best", "flags", "n_valid")))
    assert outs[0] == outs[1]


def test_wheel_speeds_formula(ctx, default_pairs):
    from lidar_slam_amd import _lib
    pairs, ref = default_pairs
    up = _lib.ukf_params(8)
    _, res = device_match(ctx, pairs, ukf=up)
    assert_same(res, ref)
    for r in range(len(pairs)):
        want = smr.wheel_speeds(res["delta"][r], up.dt, up.wheel_radius, up.wheel_base)
        assert np.all(np.abs(res["u"][r] - want) <= 1e-12 * np.abs(want)), (res["u"][r], want)
        assert np.all(np.abs(res["u"][r] - ref["u"][r]) <= 1e-9 * np.abs(ref["u"][r]))


def test_wheel_speeds_round_trip_through_the_filter(ctx, default_pairs):
    """u is the exact inverse of the filter's fx: a predict-only map step over empty revolutions
    moves x by (tx cos th, tx sin th, dth).  (alpha = 1, tiny P0: see the module docstring.)"""
    from lidar_slam_amd.odometry import ScanMatcher
    from lidar_slam_amd.slam import LandmarkMap
    pairs, ref = default_pairs
    R = len(pairs)
    x0 = np.array([[1500.0, 900.0, 0.7], [2500.0, 2000.0, -2.1], [1000.0, 1200.0, 3.0]])
    P0 = np.diag([1e-10, 1e-10, 1e-14])
    lm = LandmarkMap(ctx, R, x0=x0, P0=P0, predict=True, update=False, alpha=1.0)
    ref_xy, ref_off = csr([p[0] for p in pairs])
    cur_xy, cur_off = csr([p[1] for p in pairs])
    m = ScanMatcher(ctx, R)
    m.match(ref_xy, ref_off, cur_xy, cur_off, u_out=lm.u, ukf=lm.up)
    d = m.results()["delta"]
    # one chunk of two points per robot: nothing to fit, the step is the predict alone
    lm.step(np.ones((2 * R, 2)), np.arange(R + 1), 2 * np.arange(R + 1))
    x = lm.results()["x"]
    want = x0 + np.stack([d[:, 0] * np.cos(x0[:, 2]), d[:, 0] * np.sin(x0[:, 2]), d[:, 2]], -1)
    err = np.abs(x - want)
    print("round trip", err.max(axis=0))
    assert err[:, :2].max() <= 1e-9 and err[:, 2].max() <= 1e-12


def test_odometry_keeps_its_own_copy_of_a_device_revolution(ctx):
    """LidarOdometry.step from a device array that the caller overwrites afterwards (an express
    ring), from a staged MapInput and from host arrays: the same deltas, the reference's."""
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = [300, 301]
    poses = synth.trajectory(robots, 2, u=(146.0, 174.0))
    revs = [synth.revolutions_at(poses[k], k, robots) for k in range(3)]
    kw = dict(k_trans=3, k_theta=6)
    host, dev, staged = (LidarOdometry(ctx, 2, **kw) for _ in range(3))
    lm = LandmarkMap(ctx, 2)
    ring = ctx.empty(revs[0]["xy"].shape, np.float64)
    assert host.results() is None
    for k, rev in enumerate(revs):
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        host.step(rev["xy"], sco, cpo)
        ring.upload(rev["xy"])
        dev.step(ring, sco, cpo)
        ring.upload(np.full(rev["xy"].shape, 7.0))  # the ring moves on
        staged.step(lm.upload(rev["xy"], sco, cpo))
        if k == 0:
            continue
        a, b, c = host.results(), dev.results(), staged.results()
        for key in ("delta", "best", "flags", "n_valid"):
            assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), (k, key)
        for i in range(2):
            p0, p1 = cpo[sco[i]], cpo[sco[i + 1]]
            ref = smr.match(revs[k - 1]["xy"][p0:p1], rev["xy"][p0:p1], rot=host.matcher.rot_host, **kw)
            assert np.array_equal(a["best"][i], ref["best"]) and a["flags"][i] == ref["flags"]
            assert np.max(np.abs(a["delta"][i] - ref["delta"])) <= 1e-9
            assert abs(a["delta"][i][0] - 40.0) <= 20.0 and abs(a["delta"][i][2] - 0.035) <= np.pi / 360


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end_without_odometry(ctx, loose):
    """Revolutions only: LidarOdometry writes lm.u on the device, lm.step runs without u.  Each
    step against oracle/slam.py's map_step given u from scanmatch_ref, restarted from the device's
    filter state (as test_gpu_map.py); then the pose stays within half a cell and half a rotation
    step of the truth (the reference composition, on the CPU: 3.5 mm, 0.0024 rad), and >= 100 chunks
    match (reference 137; with u = 0: 108, and 170 mm / 0.137 rad off by the last step)."""
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = list(range(200, 208))
    R = len(robots)
    poses = synth.trajectory(robots, 4, u=(146.0, 174.0))
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    rs = [osl.RobotState(seed=s, x0=poses[0][i], P0=P0, cap=256) for i, s in enumerate(robots)]
    p = smr.params()
    ukf = dict(dt=lm.up.dt, wheel_radius=lm.up.wheel_radius, wheel_base=lm.up.wheel_base)
    prev = None
    n_match = 0
    for step in range(5):  # step 0: the warm-up revolution at poses[0], u = 0
        k = step - 1
        rev = synth.revolutions_at(poses[step], step, robots)
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm)
        lm.step(rev["xy"], sco, cpo)
        res = lm.results()
        u_dev = lm.u.download()
        for i in range(R):
            c0, c1 = sco[i], sco[i + 1]
            xy = rev["xy"][cpo[c0]:cpo[c1]]
            if prev is None:
                u = np.zeros(2)
            else:
                u = smr.match(prev[i], xy, rot=odo.matcher.rot_host, ukf=ukf)["u"]
            assert np.all(np.abs(u_dev[i] - u) <= 1e-9 * np.maximum(np.abs(u), 1e-300)), (step, i, u_dev[i], u)
            mask, models = osl.map_step(rs[i], xy, cpo[c0:c1 + 1] - cpo[c0], (float(u[0]), float(u[1])), Rd)
            assert np.array_equal(res["mask"][cpo[c0]:cpo[c1]], mask), (step, i)
            dm = res["models"][c0:c1]
            assert list(dm["flags"]) == [m["flags"] for m in models], (step, i)
            assert list(dm["match_index"]) == [m["match_index"] for m in models], (step, i)
            assert list(dm["landmark_id"]) == [m["landmark_id"] for m in models]
            if k >= 0:
                n_match += int(np.sum((dm["flags"] & orc.FLAG_MATCHED) != 0))
            lst = res["landmarks"][i, :res["lmk_count"][i]]
            assert list(lst["id"]) == [L["id"] for L in rs[i].lst], (step, i)
            assert list(lst["life"]) == [L["life"] for L in rs[i].lst], (step, i)
            refl = np.array([[L["pos"][0], L["pos"][1], L["end"][0], L["end"][1]] for L in rs[i].lst])
            got = np.stack([lst["pos_x"], lst["pos_y"], lst["end_x"], lst["end_y"]], -1)
            assert np.max(np.abs(got - refl)) <= 1e-3, (step, i)
            err = ukf_exact.component_errors(res["x"][i:i + 1], res["P"][i:i + 1], rs[i].x[None], rs[i].P[None])
            assert max(err.values()) <= 1e-5, (step, i, err)
            assert np.array_equal(res["mt_state"][i, :624], rs[i].st.key), (step, i)
            assert res["mt_state"][i, 624] == rs[i].st.pos.value
            rs[i].x, rs[i].P = res["x"][i].copy(), res["P"][i].copy()
        if k >= 0:
            dpos = np.hypot(res["x"][:, 0] - poses[step][:, 0], res["x"][:, 1] - poses[step][:, 1])
            dth = np.abs((res["x"][:, 2] - poses[step][:, 2] + np.pi) % (2 * np.pi) - np.pi)
            print("step", k, "pose error", dpos.max(), dth.max())
            assert dpos.max() <= p["cell"] / 2, (k, dpos)
            assert dth.max() <= p["theta_step"] / 2, (k, dth)
        prev = [rev["xy"][cpo[sco[i]]:cpo[sco[i + 1]]] for i in range(R)]
    print("matched chunks", n_match)
    assert n_match >= 100, n_match
