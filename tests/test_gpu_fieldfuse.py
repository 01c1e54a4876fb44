"""GPU parity of the field fusion (lslam_field_fuse, DistanceField.fuse) against its NumPy definition,
tests/fieldfuse_ref.py, over fields that the device made.

Every double operation of the definition is rounded on its own and the sums are integers, so every
output (pose_out, P_out, z, info, info_f, s2, nis, trace, normal, n_used, iters, flags) is compared
EXACTLY, the doubles as bit patterns, the reference being fed the (cos, sin) that the device wrote to
trace (held to 1e-15 against NumPy's by test_gpu_fieldalign).  The end-to-end case repeats the caps of
tests/test_fieldfuse_ref.py on the device's own grid, fused into a LandmarkMap in place.
"""
import ctypes as C

import numpy as np
import pytest

import dist_ref as dr
import fieldalign_ref as far
import fieldfuse_ref as ffr
from oracle import cpu as orc
from test_fieldalign_ref import ROOM_CAP_MM, ROOM_CAP_RAD, ROOM_DISPLACEMENTS
from test_fieldfuse_ref import P_ROOM
from test_fieldscore_ref import ROOM_DIST
from test_gpu_fieldalign import assert_trace_rot, same_bits
from test_gpu_fieldscore import field_of
from test_gpu_occgrid import csr, nasty_points
from test_gpu_raycast import random_map
from test_mapfuse_ref import CORR, nan_payload
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, room_run

pytestmark = pytest.mark.gpu

ALIGN_KEYS = tuple(far.DEFAULTS)
FUSE_KEYS = tuple(ffr.DEFAULTS)
OUT_KEYS = ("flags", "iters", "n_used", "normal", "trace", "z", "s2", "info", "info_f", "nis", "pose_out", "P_out")


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, grid_kw, write_back=False, x=None, Pd=None):
    """One fuse compared with the reference; returns the device's results.  x, Pd: the device arrays to
    fuse into (default: fresh uploads of poses and P)."""
    R = len(poses)
    x = ctx.to_device(np.ascontiguousarray(poses, np.float64)) if x is None else x
    Pd = ctx.to_device(np.ascontiguousarray(P, np.float64).reshape(R, 9)) if Pd is None else Pd
    f.fuse(xy, sco, cpo, x=x, P=Pd, write_back=write_back)
    res = f.fuse_results()
    q = {k: getattr(f.a, k) for k in ALIGN_KEYS}
    q.update({k: getattr(f.f, k) for k in FUSE_KEYS})
    want = ffr.fuse_batch(d2, xy, cpo[sco], poses, P, res["trace"], f.grid.origin_host, grid_kw, **q)
    for k in OUT_KEYS:
        got, w = np.asarray(res[k]), np.asarray(want[k]).astype(res[k].dtype)
        assert same_bits(got, w), (k, np.argwhere(got.view(np.int64 if got.dtype == np.float64 else got.dtype)
                                                  != w.view(np.int64 if w.dtype == np.float64 else w.dtype))[:5], got, w)
    assert_trace_rot(res["trace"], res["iters"], res["flags"])
    if write_back:
        assert same_bits(x.download(), res["pose_out"]) and same_bits(Pd.download().reshape(R, 3, 3), res["P_out"])
    else:
        assert same_bits(x.download(), np.ascontiguousarray(poses, np.float64))
        assert same_bits(Pd.download().reshape(R, 3, 3), np.ascontiguousarray(P, np.float64).reshape(R, 3, 3))
    return res


def random_priors(rng, R):
    """[R, 3, 3]: correlated, standard deviations of 3 .. 300 mm and 1 .. 100 mrad."""
    P = np.empty((R, 3, 3))
    for r in range(R):
        d = np.array([10.0 ** rng.uniform(0.5, 2.5), 10.0 ** rng.uniform(0.5, 2.5), 10.0 ** rng.uniform(-3.0, -1.0)])
        P[r] = (CORR if r % 2 else np.eye(3)) * d[:, None] * d[None, :]
    return P


def shape_case(W, R, seed):
    """The map spans -4000 .. 4000 mm whatever W is (at W 24 the cell, 1000 / 3, and its inverse are no
    binary fractions).  One map for all robots but the last, whose field is EMPTY; 40 .. 200 points each."""
    cell = 8000.0 / W
    kw = dict(grid_w=W, cell=cell, max_range=3500.0)
    rng = np.random.default_rng(seed)
    L0 = np.repeat(random_map(rng, 1, W, occupied=0.08), R, 0)
    if R > 1:
        L0[-1] = 0
    dist_kw = dict(d_max=max(4, W // 4), trunc=float(max(4, W // 4)), min_points=3, min_permille=0, max_shift=np.inf,
                   max_turn=np.inf)
    poses = np.stack([rng.uniform(-1500, 1500, R), rng.uniform(-1500, 1500, R), rng.uniform(-3, 3, R)], -1)
    arrays = [nasty_points(rng, int(rng.integers(40, 201)), W, cell, 3500.0) for _ in range(R)]
    return kw, L0, dist_kw, poses, arrays, random_priors(rng, R)


@pytest.mark.parametrize("W", [16, 24])
@pytest.mark.parametrize("R", [1, 5, 65, 257])
def test_shapes(ctx, W, R):
    """1, 5, 65 and 257 robots: partly filled workgroups in both kernels (four robots to the alignment's,
    64 to the fusion's)."""
    kw, L0, dist_kw, poses, arrays, P = shape_case(W, R, 500 + 10 * W + R)
    g, f, d2 = field_of(ctx, L0, dist_kw=dist_kw, **kw)
    xy, sco, cpo = csr(arrays)
    res = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, kw)
    ok = (res["flags"] & ffr.REJECTED) == 0
    print("W", W, "R", R, "updated", int(ok.sum()), "outliers", int((res["flags"] & ffr.OUTLIER != 0).sum()),
          "rejected by the alignment", int((res["flags"] & far.KEEP != 0).sum()))
    if R >= 5:
        moved = ok[:-1]  # (the last robot's field is EMPTY: it is accepted and stays where it was)
        assert moved.any() or R < 65
        assert not same_bits(res["pose_out"][:-1][moved], poses[:-1][moved]) or R < 65
        assert np.all(res["info"][:-1][moved][:, 2, 2] > 0)
        assert not res["info"][-1].any() and not res["info_f"][-1].any() and res["s2"][-1] > 0  # the EMPTY field: no information
    check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, kw, write_back=True)


def test_long_revolution(ctx):
    """4096 points on one robot."""
    kw = dict(grid_w=64, cell=100.0, max_range=3000.0)
    rng = np.random.default_rng(581)
    L0 = random_map(rng, 1, 64, occupied=0.05)
    g, f, d2 = field_of(ctx, L0, dist_kw=dict(d_max=12, trunc=12.0, nis_max=np.inf, max_shift=np.inf, max_turn=np.inf), **kw)
    xy, sco, cpo = csr([nasty_points(rng, 4096, 64, 100.0, 3000.0)])
    res = check_fuse(ctx, f, d2, xy, sco, cpo, np.array([[310.0, -420.0, 0.7]]), np.diag([900.0, 900.0, 1e-3])[None], kw,
                     write_back=True)
    assert res["n_used"][0, 0] > 1500 and not res["flags"][0] & ffr.REJECTED and res["nis"][0] > 0


# ---- one robot for every flag ----

FLAG_KW = dict(grid_w=32, cell=100.0, max_range=3000.0)
BOX = [(x, y) for x in range(4, 28) for y in (6, 25)] + [(x, y) for x in (4, 27) for y in range(7, 25)]


def box_map():
    L = np.full((32, 32), -100, np.int16)
    for x, y in BOX:
        L[y, x] = 200
    return L


def corridor_map():
    L = np.full((32, 32), -100, np.int16)
    L[6, :] = L[25, :] = 200
    return L


def seen_from(cells, pose):
    """The centres of cells in the frame of pose."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    w = (np.array(cells, np.float64) + 0.5) * 100.0 - np.array(pose[:2])
    return np.stack([c * w[:, 0] + s * w[:, 1], -s * w[:, 0] + c * w[:, 1]], -1)


FLAG_ROBOTS = ("fine", "bad pose", "few", "corridor", "diverged", "weak", "outlier", "inf", "payload", "negative", "zero", "empty",
               "fine too")


def flag_case():
    """One batch, a robot for every flag: (L0 [R, 32, 32], arrays, poses, P)."""
    truth = np.array([1590.0, 1620.0, 0.02])
    box = seen_from(BOX[::2], truth)
    R = len(FLAG_ROBOTS)
    L0 = np.stack([box_map()] * R)
    arrays = [box.copy() for _ in range(R)]
    poses = np.tile(truth + np.array([12.0, -9.0, 0.004]), (R, 1))
    P = np.tile(np.diag([30.0 ** 2, 30.0 ** 2, 0.02 ** 2]), (R, 1, 1))
    i = FLAG_ROBOTS.index
    poses[i("bad pose")] = [1600.0, nan_payload(), 0.0]
    arrays[i("few")] = box[:7]
    L0[i("corridor")] = corridor_map()
    arrays[i("corridor")] = seen_from([(x, y) for x in range(6, 26, 2) for y in (6, 25)], truth)
    poses[i("diverged")] = truth + np.array([70.0, 0.0, 0.0])
    outside = seen_from([(x, y) for x in range(-8, -3) for y in range(8, 24)], truth)  # valid and in range, but off the map
    arrays[i("weak")] = np.concatenate([box[:30], outside])
    poses[i("outlier")] = truth + np.array([12.0, -9.0, 0.07])  # a filter that claims 0.1 mrad and is 70 mrad off
    P[i("outlier")] = np.diag([1.0, 1.0, 1e-8])
    P[i("inf"), 1, 1] = np.inf
    P[i("payload"), 0, 2] = nan_payload()
    P[i("negative"), 2, 2] = -1.0
    P[i("zero")] = 0.0
    L0[i("empty")] = -100
    P[i("fine too")] = CORR * np.array([40.0, 25.0, 0.03])[:, None] * np.array([40.0, 25.0, 0.03])[None, :]
    return L0, arrays, poses, P


FLAG_DIST = dict(d_max=4, trunc=4.0, min_points=8, max_shift=40.0)


def expected_flags(damped):
    i = FLAG_ROBOTS.index
    want = {r: 0 for r in range(len(FLAG_ROBOTS))}
    want[i("bad pose")] = far.BAD_POSE
    want[i("few")] = far.FEW
    want[i("diverged")] = far.DIVERGED
    want[i("weak")] = far.WEAK
    want[i("outlier")] = ffr.OUTLIER
    for n in ("inf", "payload", "negative", "zero"):
        want[i(n)] = ffr.BAD_COV
    if not damped:  # without damping the corridor's x and the EMPTY field have no pivot
        want[i("corridor")] = want[i("empty")] = far.SINGULAR
    return want


def assert_flag_case(res, poses, P, damped):
    mask = ffr.REJECTED
    want = expected_flags(damped)
    got = {r: int(res["flags"][r]) & mask for r in want}
    assert got == want, (got, want)
    for r, w in want.items():
        if w:
            assert same_bits(res["pose_out"][r], poses[r]) and same_bits(res["P_out"][r], P[r]), FLAG_ROBOTS[r]
        else:
            assert not same_bits(res["P_out"][r], P[r]), FLAG_ROBOTS[r]
        if w & far.KEEP:
            assert not res["info"][r].any() and not res["info_f"][r].any() and res["s2"][r] == 0.0 and res["nis"][r] == 0.0
            assert same_bits(res["z"][r], poses[r])
        elif w:
            assert res["info"][r, 1, 1] > 0 and res["info_f"][r, 1, 1] > 0 and res["s2"][r] > 0 and not same_bits(res["z"][r], poses[r])
            assert (res["nis"][r] > 16.27) if w == ffr.OUTLIER else (res["nis"][r] == 0.0)


def assert_corridor_and_empty(res, poses, P):
    c, e = FLAG_ROBOTS.index("corridor"), FLAG_ROBOTS.index("empty")
    assert not res["info"][c, 0].any() and not res["info_f"][c, 0].any() and res["pose_out"][c, 0] == poses[c, 0]
    assert abs(res["P_out"][c, 0, 0] - P[c, 0, 0]) <= 1e-12 * P[c, 0, 0] and res["P_out"][c, 1, 1] < P[c, 1, 1]
    assert not res["info"][e].any() and same_bits(res["pose_out"][e], poses[e]) and np.allclose(res["P_out"][e], P[e], rtol=1e-13, atol=0)


def test_flags(ctx):
    L0, arrays, poses, P = flag_case()
    g, f, d2 = field_of(ctx, L0, origin=(0.0, 0.0), dist_kw=FLAG_DIST, **FLAG_KW)
    assert (f.results()["flags"] == dr.EMPTY).sum() == 1
    xy, sco, cpo = csr(arrays)
    for damped in (True, False):
        if not damped:
            f.a.damp_t = f.a.damp_r = 0.0
        for write_back in (False, True):
            res = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW, write_back=write_back)
            assert_flag_case(res, poses, P, damped)
    # damped again: the corridor does not move along its walls, the EMPTY field adds nothing
    f.a.damp_t, f.a.damp_r = 1.0, 100.0
    res = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW)
    assert_corridor_and_empty(res, poses, P)
    # nis exactly at the gate is accepted; one ulp below it is not
    nis = float(res["nis"][0])
    f.f.nis_max = nis
    assert not check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW)["flags"][0] & ffr.REJECTED
    f.f.nis_max = float(np.nextafter(nis, 0.0))
    assert check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW)["flags"][0] & ffr.REJECTED == ffr.OUTLIER


def test_aliasing_stale_buffers_and_chaining(ctx):
    """pose_out on pose and P_out on P give what separate outputs give; outputs pre-filled with garbage
    keep none of it; a second call chains from the fused state."""
    L0, arrays, poses, P = flag_case()
    g, f, d2 = field_of(ctx, L0, origin=(0.0, 0.0), dist_kw=FLAG_DIST, **FLAG_KW)
    xy, sco, cpo = csr(arrays)
    R = len(poses)
    apart = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW)
    for a in list(f._align.values()) + list(f._fuse.values()):
        a.upload(np.frombuffer(b"\xa5" * a.nbytes, np.uint8).view(a.dtype).reshape(a.shape))
    again = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW)
    x, Pd = ctx.to_device(poses), ctx.to_device(P.reshape(R, 9))
    for a in list(f._align.values()) + list(f._fuse.values()):
        a.upload(np.frombuffer(b"\x5a" * a.nbytes, np.uint8).view(a.dtype).reshape(a.shape))
    place = check_fuse(ctx, f, d2, xy, sco, cpo, poses, P, FLAG_KW, write_back=True, x=x, Pd=Pd)
    for k in OUT_KEYS:
        assert same_bits(apart[k], again[k]) and same_bits(apart[k], place[k]), k
    # the second call reads what the first wrote, in place
    x1, P1 = place["pose_out"], place["P_out"]
    second = check_fuse(ctx, f, d2, xy, sco, cpo, x1, P1, FLAG_KW, write_back=True, x=x, Pd=Pd)
    assert second["P_out"][0, 0, 0] < P1[0, 0, 0] < P[0, 0, 0] and second["nis"][0] < place["nis"][0]
    # an alignment after a fusion reads the same buffers and leaves fuse_results to the fusion
    f.align(xy, sco, cpo, pose=poses)
    with pytest.raises(ValueError):
        f.fuse_results()


def test_refusals(ctx):
    from lidar_slam_amd import _lib
    from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
    from lidar_slam_amd.slam import LandmarkMap
    g = OccupancyGrid(ctx, 2, grid_w=32, cell=100.0, max_range=3000.0)
    for bad in (dict(sigma_min=0.0), dict(r_scale=-1.0), dict(floor_t=np.inf), dict(floor_r=np.nan), dict(nis_max=0.0),
                dict(sigma_min=np.nan), dict(n_iter=0), dict(nis=1.0)):
        with pytest.raises((ValueError, TypeError)):
            DistanceField(g, **bad)
    f = DistanceField(g, nis_max=np.inf, r_scale=2.0)
    assert f.f.nis_max == np.inf and f.f.r_scale == 2.0
    xy, sco, cpo = csr([np.ones((5, 2)), np.ones((5, 2))])
    x, P = ctx.to_device(np.zeros((2, 3))), ctx.to_device(np.tile(np.eye(3).reshape(9), (2, 1)))
    with pytest.raises(ValueError):
        f.fuse(xy, sco, cpo, x=x, P=P)  # no field yet
    with pytest.raises(ValueError):
        f.fuse_results()
    f.step()
    for kw in (dict(x=np.zeros((2, 3)), P=P), dict(x=x), dict(x=x, P=ctx.empty((1, 9), np.float64)), dict(x=ctx.empty((2, 3), np.float32), P=P),
               dict(lm=LandmarkMap(ctx, 2, lmk_capacity=16, seeds=[1, 2]), x=x, P=P), dict(lm=x), dict()):
        with pytest.raises(ValueError):
            f.fuse(xy, sco, cpo, **kw)
    L = _lib.load()
    b = _lib.FieldFuseBatch()  # n_robots 0 does nothing, whatever the pointers
    assert L.lslam_field_fuse(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a), C.byref(f.f)) == 0
    b.a.n_robots = 2
    b.a.xy = f.d2.addr
    assert L.lslam_field_fuse(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a), C.byref(f.f)) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    f.fuse(xy, sco, cpo, x=x, P=P)  # fills a whole batch; then z on the mean is refused and nothing is written
    before = x.download()
    o, fo = f._align, f._fuse
    b.a.xy, b.a.pt_off, b.a.pose, b.a.origin, b.a.d2 = f._stage.xy.buf.addr, f._stage.off.addr, x.addr, g.origin.addr, f.d2.addr
    b.a.pose_out, b.a.trace, b.a.normal = x.addr, o["trace"].addr, o["normal"].addr
    b.a.n_used, b.a.iters, b.a.flags = o["n_used"].addr, o["iters"].addr, o["flags"].addr
    b.P, b.P_out, b.z = P.addr, P.addr, x.addr + 24
    b.info, b.info_f, b.s2, b.nis = fo["info"].addr, fo["info_f"].addr, fo["s2"].addr, fo["nis"].addr
    assert L.lslam_field_fuse(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a), C.byref(f.f)) == _lib.LSLAM_ERR_ARG
    assert b"z must not overlap" in L.lslam_last_error()
    b.z = fo["z"].addr
    assert L.lslam_field_fuse(ctx.handle, C.byref(b), C.byref(g.p), C.byref(f.a), C.byref(f.f)) == 0
    ctx.sync()
    assert same_bits(x.download(), before)  # the field is EMPTY at d_max 64, beyond trunc: FEW, the filter stays
    assert f.fuse_results()["flags"].tolist() == [far.FEW | far.WEAK] * 2


@pytest.fixture
def loose():
    orc.set_tolerances(0.1, 100.0, 1000.0)
    yield dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
    orc.set_tolerances()


def test_end_to_end(ctx, loose):
    """The five-revolution device chain of test_gpu_fieldalign.test_end_to_end; then lm.x is set to the
    true poses displaced by each of ROOM_DISPLACEMENTS and lm.P to diag(50^2, 50^2, 0.05^2) on the device,
    and the fifth revolution is fused into the filter in place: exact against the reference fed the
    device grid's field, and the caps of tests/test_fieldfuse_ref.py."""
    from lidar_slam_amd.mapping import FIELDFUSE_REJECTED, DistanceField, OccupancyGrid
    from lidar_slam_amd.odometry import LidarOdometry
    from lidar_slam_amd.slam import LandmarkMap
    robots = ROOM_ROBOTS
    R = len(robots)
    poses, revs = room_run()
    P0, Rd = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
    lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=robots, x0=poses[0], P0=P0, R_diag=Rd, **loose)
    odo = LidarOdometry(ctx, R)
    grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
    field = DistanceField(grid, **ROOM_DIST)
    for rev in revs:
        sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
        odo.step(rev["xy"], sco, cpo, lm, sync=False)
        lm.step(rev["xy"], sco, cpo, sync=False)
        grid.step(rev["xy"], sco, cpo, pose=lm, sync=False)
    rev = revs[4]
    sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
    field.step(sync=False)
    d2 = dr.field_batch(grid.results()["logodds"], **ROOM_DIST)[0]
    assert np.array_equal(field.results()["d2"], d2)
    P = np.tile(P_ROOM, (R, 1, 1))
    for disp in ROOM_DISPLACEMENTS:
        guess = poses[4] + np.array(disp)
        lm.x.upload(guess)
        lm.P.upload(P.reshape(R, 9))
        field.fuse(rev["xy"], sco, cpo, lm=lm)
        res = field.fuse_results()
        want = ffr.fuse_batch(d2, rev["xy"], cpo[sco], guess, P, res["trace"], grid.origin_host, ROOM_KW, **ROOM_DIST)
        for k in OUT_KEYS:
            assert same_bits(np.asarray(res[k]), np.asarray(want[k]).astype(res[k].dtype)), k
        x1, P1 = lm.x.download(), lm.P.download().reshape(R, 3, 3)
        assert same_bits(x1, res["pose_out"]) and same_bits(P1, res["P_out"])
        err = x1 - poses[4]
        mm, rad = np.hypot(err[:, 0], err[:, 1]), np.abs(err[:, 2])
        print("displaced by", disp, "error mm", mm.round(2), "mrad", (1e3 * rad).round(3), "nis", res["nis"].round(3), "sigma",
              np.sqrt(np.diagonal(P1, axis1=1, axis2=2)).max(0).round(4), "flags", res["flags"])
        assert not (res["flags"] & FIELDFUSE_REJECTED).any()
        assert np.all(mm <= ROOM_CAP_MM) and np.all(rad <= ROOM_CAP_RAD) and np.all(res["nis"] <= 16.27)
        assert np.all(np.diagonal(P1, axis1=1, axis2=2) < np.diag(P_ROOM)) and same_bits(P1, P1.transpose(0, 2, 1))
        assert np.all(np.linalg.eigvalsh(P1)[:, 0] > 0)
