"""The field fusion (include/lidarslam.h, lslam_field_fuse) on the CPU: tests/fieldfuse_ref.py in the
five-revolution room of test_fieldalign_ref, its consistency against the true poses, the corridor, steps
6-11 against mpmath at 50 digits, a hand-made case per rule, and the ABI checks that need no device.
tests/test_gpu_fieldfuse.py holds the kernels to the reference bit for bit.

The room.  The fixture of test_fieldalign_ref (robots 200-207, the map built at the true poses), the
fifth revolution, both ROOM_DISPLACEMENTS, P = diag(50^2, 50^2, 0.05^2), the defaults.  Measured on the
reference: no rejecting flag, the fused pose within 0.66 mm of the aligned pose (a prior of 50 mm against a
measurement of 5.8 mm keeps 1.3 % of the 39 mm displacement) and at most 4.6 mm from the truth (the caps are
test_fieldalign_ref's, which rest on the alignment's own error), nis at most 1.20.

Consistency.  Revolutions 1-4 x both displacements x 8 robots.  If P_out is an honest covariance of the
error e = pose_out - truth, e^T inverse(P_out) e has the mean of chi-square with 3 degrees of freedom, 3;
a mean at or below 3 makes the estimate conservative.  Measured: 0.53 mean, 1.88 max.  The control, floors
of 0.01 cell and 1e-5 rad (next to none), claims more than the alignment delivers: 8.86.

Exactness.  Steps 6-11 against mpmath at 50 digits, written there in the covariance form
(inverse(Lambda) + diag(ft, ft, fr), P + R, K = P inverse(P + R)), which is NOT the order of the
definition; the cap is 1e-10, the project's own for lslam_map_fuse, in test_mapfuse_ref's norms.  Measured
worst: 2.3e-13 mm, 2.2e-16 rad, 6.1e-16 for P', 6.2e-16 for nis.  The control, P - P G P with
G = Lambda_f - Lambda_f inverse(inverse(P) + Lambda_f) Lambda_f in float64, subtracts nearly equal matrices
and misses the cap from the 150^2 scale on (2.8e-6), by 12 at the 1e8 scale.
"""
import ctypes as C
import math
import re

import mpmath as mp
import numpy as np
import pytest

import fieldalign_ref as far
import fieldfuse_ref as ffr
import occgrid_ref as ogr
from lidar_slam_amd import _lib
from test_fieldalign_ref import KW, ROOM_CAP_MM, ROOM_CAP_RAD, ROOM_DISPLACEMENTS, corridor_field, room  # noqa: F401
from test_mapfuse_ref import CORR, SCALES, nan_payload
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS

P_ROOM = np.diag([50.0 ** 2, 50.0 ** 2, 0.05 ** 2])
TIGHT = dict(floor_t=0.01, floor_r=1e-5)
CELL = float(ogr.params(**ROOM_KW)["cell"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def room_aligns(room, step, disp):
    """fieldalign_ref.align for the eight robots at revolution step, from the true poses displaced by disp."""
    poses, revs, L, d2 = room
    rev = revs[step]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    guess = poses[step] + np.array(disp)
    return guess, [far.align(d2[r], rev["xy"][off[r]:off[r + 1]], guess[r], None, ROOM_ORIGIN, ROOM_KW)
                   for r in range(len(ROOM_ROBOTS))]


@pytest.fixture(scope="module")
def room_cases(room):
    """(step, disp) -> (guesses, alignments), revolutions 1-4 x both displacements."""
    return {(step, disp): room_aligns(room, step, disp) for step in (1, 2, 3, 4) for disp in ROOM_DISPLACEMENTS}


def test_room(room, room_cases):
    poses = room[0]
    fp = dict(ffr.DEFAULTS)
    for disp in ROOM_DISPLACEMENTS:
        guess, als = room_cases[4, disp]
        for r, al in enumerate(als):
            f = ffr.fuse_steps(al, guess[r], P_ROOM, CELL, fp)
            assert not f["flags"] & ffr.REJECTED, f["flags"]
            err = f["pose_out"] - poses[4][r]
            mm, rad = math.hypot(err[0], err[1]), abs(err[2])
            dz = f["pose_out"] - f["z"]
            print("displaced by", disp, "robot", r, "error mm %.2f mrad %.3f" % (mm, 1e3 * rad), "from z mm %.4f" % math.hypot(dz[0], dz[1]),
                  "nis %.3f" % f["nis"], "s2 %.3f" % f["s2"], "sigma", np.sqrt(np.diag(f["P_out"])).round(4))
            assert mm <= ROOM_CAP_MM and rad <= ROOM_CAP_RAD
            assert f["nis"] <= fp["nis_max"]
            Po = f["P_out"]
            assert np.array_equal(bits(Po), bits(Po.T)) and np.linalg.eigvalsh(Po)[0] > 0
            assert np.all(np.diag(Po) < np.diag(P_ROOM))
            assert np.array_equal(bits(f["z"]), bits(al["pose_out"])) and np.array_equal(bits(f["info"]), bits(f["info"].T))


def test_room_through_fuse(room):
    """fuse and fuse_batch are fuse_steps on align's output."""
    poses, revs, L, d2 = room
    rev = revs[4]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    guess = poses[4][:2] + np.array(ROOM_DISPLACEMENTS[0])
    out = ffr.fuse_batch(d2[:2], rev["xy"], off[:3], guess, np.stack([P_ROOM, P_ROOM]), None, np.tile(ROOM_ORIGIN, (2, 1)), ROOM_KW)
    for r in range(2):
        al = far.align(d2[r], rev["xy"][off[r]:off[r + 1]], guess[r], None, ROOM_ORIGIN, ROOM_KW)
        f = ffr.fuse_steps(al, guess[r], P_ROOM, CELL, dict(ffr.DEFAULTS))
        for k in ("pose_out", "P_out", "z", "info", "info_f", "s2", "nis", "normal", "flags"):
            assert np.array_equal(np.asarray(out[k][r]), np.asarray(f[k])), k


def test_consistency(room, room_cases):
    poses = room[0]
    stats = {}
    for name, over in (("default", {}), ("control", TIGHT)):
        fp = dict(ffr.DEFAULTS, **over)
        vals = []
        for (step, disp), (guess, als) in room_cases.items():
            for r, al in enumerate(als):
                f = ffr.fuse_steps(al, guess[r], P_ROOM, CELL, fp)
                assert not f["flags"] & (far.KEEP | ffr.BAD_COV), (step, disp, r, f["flags"])
                e = f["pose_out"] - poses[step][r]
                vals.append(float(e @ np.linalg.solve(f["P_out"], e)))
        assert len(vals) == 64
        stats[name] = (np.mean(vals), np.max(vals))
    print("mean, max of e^T inverse(P_out) e: default %.3f %.3f; control (floors 0.01 cell, 1e-5 rad) %.3f %.3f"
          % (stats["default"] + stats["control"]))
    assert stats["default"][0] <= 3.0
    assert stats["control"][0] > 3.0


# ---- the corridor ----

CORRIDOR_PTS = np.array([[dx, wy] for dx in np.arange(-900.0, 901.0, 150.0) for wy in (650.0 - 1600.0, 2550.0 - 1600.0)])
CORRIDOR_POSE = np.array([1600.0, 1660.0, 0.0])
P_CORRIDOR = np.diag([150.0 ** 2, 150.0 ** 2, 0.12 ** 2])


def M(a):
    return mp.matrix([[mp.mpf(float(v)) for v in rw] for rw in np.atleast_2d(a)])


def exact_inputs(al, cell, fp):
    """(Lambda, F = diag(ft, ft, fr)) at 50 digits from the alignment's integers."""
    mp.mp.dps = 50
    N, n = [int(v) for v in al["normal"]], int(al["n_used"][1])
    sc = mp.mpf(2) ** -20
    smin = mp.mpf(float(fp["sigma_min"]))
    mean = N[9] * sc / n if n else mp.mpf(0)
    s2 = max(mean, smin * smin) * mp.mpf(float(fp["r_scale"]))
    u = [1 / mp.mpf(float(cell)), 1 / mp.mpf(float(cell)), mp.mpf(1)]
    lam = mp.zeros(3, 3)
    for k, (i, j) in enumerate(ffr.PAIRS):
        lam[i, j] = lam[j, i] = N[k] * sc * u[i] * u[j] / s2
    ft = (mp.mpf(float(fp["floor_t"])) * mp.mpf(float(cell))) ** 2
    fr = mp.mpf(float(fp["floor_r"])) ** 2
    return lam, mp.diag([ft, ft, fr])


def exact_update(x, z, P, lam_f):
    """(x', P', nis) from the floored information, in information form (Lambda_f may be singular)."""
    Pm, y = M(P), M(z).T - M(x).T
    P1 = mp.inverse(mp.inverse(Pm) + lam_f)
    c = P1 * lam_f * y
    return M(x).T + c, P1, (y.T * mp.inverse(Pm) * c)[0]


def test_corridor():
    d2 = corridor_field()
    for P in (P_CORRIDOR, CORR * np.sqrt(np.diag(P_CORRIDOR))[:, None] * np.sqrt(np.diag(P_CORRIDOR))[None, :]):
        f = ffr.fuse(d2, CORRIDOR_PTS, CORRIDOR_POSE, P, None, (0.0, 0.0), KW)
        assert not f["flags"] & ffr.REJECTED and f["nis"] <= 16.27
        assert not f["info"][0].any() and not f["info_f"][0].any() and not f["info"][:, 0].any() and not f["info_f"][:, 0].any()
        assert f["info"][1, 1] > 0 and f["info_f"][1, 1] > 0 and f["info_f"][1, 1] < f["info"][1, 1]
        assert f["P_out"][1, 1] < P[1, 1] and f["P_out"][2, 2] < P[2, 2]
        # 50 digits: Lambda is singular, so its floored form is the definition's product, taken exactly
        lam, F = exact_inputs(f, KW["cell"], ffr.DEFAULTS)
        W = mp.inverse(F)
        x1, P1, nis = exact_update(CORRIDOR_POSE, f["z"], P, lam * mp.inverse(lam + W) * W)
        if P is P_CORRIDOR:
            assert f["pose_out"][0] == CORRIDOR_POSE[0]
            assert abs(f["P_out"][0, 0] - P[0, 0]) <= 1e-12 * P[0, 0]
            print("corridor: P_out[0][0] / P[0][0] - 1 =", f["P_out"][0, 0] / P[0, 0] - 1.0, "sigma y", math.sqrt(f["P_out"][1, 1]))
        else:  # x and y are correlated in the prior: what y learns moves x
            assert abs(f["pose_out"][0] - CORRIDOR_POSE[0]) > 1.0
            print("corridor, correlated prior: x moves by", f["pose_out"][0] - CORRIDOR_POSE[0])
        assert abs(mp.mpf(float(f["pose_out"][0])) - x1[0]) <= 1e-10 and abs(mp.mpf(float(f["pose_out"][1])) - x1[1]) <= 1e-10
        assert abs(mp.mpf(float(f["P_out"][0, 0])) - P1[0, 0]) <= 1e-10 * P1[0, 0]


# ---- exactness of steps 6-11 against 50 digits ----

def exact_steps(al, x, P, cell, fp):
    """Steps 6-11 in the covariance form: R = inverse(Lambda) + F, S = P + R, K = P inverse(S)."""
    lam, F = exact_inputs(al, cell, fp)
    R = mp.inverse(lam) + F
    Pm, y = M(P), M(al["pose_out"]).T - M(x).T
    Si = mp.inverse(Pm + R)
    K = Pm * Si
    return M(x).T + K * y, (mp.eye(3) - K) * Pm, (y.T * Si * y)[0], mp.inverse(R)


def exact_errors(f_x, f_P, f_nis, ex):
    """test_mapfuse_ref.exact_errors' norms: (mm, rad, P' relative to sqrt(P'ii P'jj), nis relative)."""
    x1, P1, nis = ex[:3]
    ex_ = [abs(mp.mpf(float(f_x[i])) - x1[i]) for i in range(3)]
    eP = max(abs(mp.mpf(float(f_P[i, j])) - P1[i, j]) / mp.sqrt(P1[i, i] * P1[j, j]) for i in range(3) for j in range(3))
    en = abs(mp.mpf(float(f_nis)) - nis) / nis
    return float(max(ex_[0], ex_[1])), float(ex_[2]), float(eP), float(en)


def test_steps_6_to_11_against_50_digits(room_cases):
    cap = 1e-10
    worst = np.zeros(4)
    ctl = {}
    for disp in ROOM_DISPLACEMENTS:
        guess, als = room_cases[4, disp]
        for r, al in enumerate(als):
            for scale in [tuple(np.diag(P_ROOM))] + SCALES:
                d = np.sqrt(np.array(scale))
                P = CORR * d[:, None] * d[None, :]
                for over in ({}, TIGHT):
                    fp = dict(ffr.DEFAULTS, nis_max=np.inf, **over)
                    f = ffr.fuse_steps(al, guess[r], P, CELL, fp)
                    assert f["flags"] & ffr.REJECTED == 0 and f["nis"] > 0
                    ex = exact_steps(al, guess[r], P, CELL, fp)
                    worst = np.maximum(worst, exact_errors(f["pose_out"], f["P_out"], f["nis"], ex))
                    # the control: the subtractive form in float64 from the reference's own Lambda_f
                    lf = f["info_f"]
                    G = lf - lf @ np.linalg.inv(np.linalg.inv(P) + lf) @ lf
                    e = exact_errors(f["pose_out"], P - P @ G @ P, f["nis"], ex)[2]
                    ctl[scale[0]] = max(ctl.get(scale[0], 0.0), e)
    print("worst against 50 digits: x'", worst[0], "mm", worst[1], "rad; P'", worst[2], "; nis", worst[3],
          "; control P - P G P by prior scale:", {k: float("%.3g" % v) for k, v in ctl.items()})
    assert np.all(worst <= cap), worst
    assert max(ctl.values()) > cap


# ---- rules ----

def corridor_fuse(P=P_CORRIDOR, pose=CORRIDOR_POSE, pts=CORRIDOR_PTS, **kw):
    return ffr.fuse(corridor_field(), pts, pose, P, None, (0.0, 0.0), KW, **kw)


def assert_untouched(f, pose, P, zeros=True):
    assert np.array_equal(bits(f["pose_out"]), bits(pose)) and np.array_equal(bits(f["P_out"]), bits(P))
    if zeros:
        assert not f["info"].any() and not f["info_f"].any() and f["s2"] == 0.0 and f["nis"] == 0.0
        assert np.array_equal(bits(f["z"]), bits(pose))


def test_align_rejections_leave_the_filter_alone():
    P = np.array(P_CORRIDOR)
    P[0, 1] = nan_payload()  # P is not looked at: the payload survives
    far_pts = np.concatenate([CORRIDOR_PTS, [[0.0, -150.0], [100.0, -150.0]]])
    cases = [(far.FEW, dict(min_points=27)), (far.SINGULAR, dict(damp_t=0.0, damp_r=0.0)), (far.DIVERGED, dict(max_shift=20.0)),
             (far.WEAK, dict(pts=far_pts, trunc=5.0, min_permille=1000)),
             (far.BAD_POSE, dict(pose=np.array([1600.0, nan_payload(), 0.0]))), (far.BAD_POSE, dict(pose=np.array([1e9, 0.0, 0.0])))]
    for flag, kw in cases:
        f = corridor_fuse(P, **kw)
        assert f["flags"] & flag and not f["flags"] & (ffr.OUTLIER | ffr.BAD_COV), (flag, f["flags"])
        assert_untouched(f, kw.get("pose", CORRIDOR_POSE), P)
    assert bits(corridor_fuse(P, pose=cases[4][1]["pose"])["pose_out"])[1] == bits(nan_payload())


def test_outlier_gate(room, room_cases):
    """A filter that claims 5 mm and 1 mrad while it is 39 mm and 10 mrad off: nis 30 .. 43."""
    P = np.diag([25.0, 25.0, 1e-6])
    guess, als = room_cases[4, ROOM_DISPLACEMENTS[0]]
    for r, al in enumerate(als):
        f = ffr.fuse_steps(al, guess[r], P, CELL, dict(ffr.DEFAULTS))
        print("robot", r, "nis", f["nis"])
        assert f["flags"] & (ffr.REJECTED) == ffr.OUTLIER and 16.27 < f["nis"] < 60.0
        assert_untouched(f, guess[r], P, zeros=False)
        assert np.array_equal(bits(f["z"]), bits(al["pose_out"])) and f["info"][0, 0] > 0 and f["info_f"][2, 2] > 0 and f["s2"] > 0
        assert not ffr.fuse_steps(al, guess[r], P, CELL, dict(ffr.DEFAULTS, nis_max=np.inf))["flags"] & ffr.REJECTED


def test_nis_at_the_gate_is_accepted():
    nis = corridor_fuse()["nis"]
    assert 0.0 < nis < 16.27
    assert not corridor_fuse(nis_max=float(nis))["flags"] & ffr.REJECTED
    f = corridor_fuse(nis_max=float(np.nextafter(nis, 0.0)))
    assert f["flags"] & ffr.REJECTED == ffr.OUTLIER and f["nis"] == nis
    assert_untouched(f, CORRIDOR_POSE, P_CORRIDOR, zeros=False)
    assert corridor_fuse(nis_max=5e-324)["flags"] & ffr.OUTLIER


BAD_COVS = [("nan", (0, 1), np.nan), ("payload", (2, 2), nan_payload()), ("inf", (1, 1), np.inf), ("-inf", (0, 2), -np.inf),
            ("negative x", (0, 0), -1e4), ("negative y", (1, 1), -1e4), ("negative theta", (2, 2), -1.0)]


@pytest.mark.parametrize("what,at,value", BAD_COVS)
def test_bad_cov(what, at, value):
    P = np.array(P_CORRIDOR)
    P[at] = value
    f = corridor_fuse(P)
    assert f["flags"] & ffr.REJECTED == ffr.BAD_COV and f["nis"] == 0.0 and not np.signbit(f["nis"])
    assert_untouched(f, CORRIDOR_POSE, P, zeros=False)
    assert f["info"][1, 1] > 0 and f["info_f"][1, 1] > 0 and f["s2"] > 0 and f["z"][1] != CORRIDOR_POSE[1]  # reported


def test_bad_cov_of_a_zero_matrix_and_of_floors_that_overflow():
    f = corridor_fuse(np.zeros((3, 3)))
    assert f["flags"] & ffr.REJECTED == ffr.BAD_COV and not f["P_out"].any() and f["info_f"][1, 1] > 0
    # 1 / ft overflows: B has no inverse, info_f is zeros
    f = corridor_fuse(floor_t=1e-160)
    assert f["flags"] & ffr.REJECTED == ffr.BAD_COV and not f["info_f"].any() and f["info"][1, 1] > 0
    assert_untouched(f, CORRIDOR_POSE, P_CORRIDOR, zeros=False)


def test_r_scale_scales_the_information_by_powers_of_two():
    a, b, c = corridor_fuse(), corridor_fuse(r_scale=4.0), corridor_fuse(r_scale=0.25)
    assert np.array_equal(b["info"], a["info"] / 4.0) and np.array_equal(c["info"], a["info"] * 4.0) and a["info"][1, 1] > 0
    assert b["s2"] == 4.0 * a["s2"] and np.array_equal(a["normal"], b["normal"])
    assert b["P_out"][1, 1] > a["P_out"][1, 1] > c["P_out"][1, 1]


def test_sigma_min_floors_the_noise():
    """Step 6 on hand-made sums: r^2 = 3 over two points is a mean of 1.5 squared cells."""
    al = dict(flags=far.CONVERGED, pose_out=np.array([10.0, -5.0, 0.01]), n_used=np.array([2, 2, 2], np.int32),
              normal=np.array([4 << 20, 1 << 20, 0, 6 << 20, 0, 900 << 20, 0, 0, 0, 3 << 20], np.int64))
    run = lambda **kw: ffr.fuse_steps(al, np.zeros(3), P_ROOM, 20.0, dict(ffr.DEFAULTS, **kw))  # noqa: E731
    a = run()
    assert a["s2"] == 1.5 and not a["flags"] & ffr.REJECTED
    inv = 1.0 / 20.0  # in the definition's order: ((N sc) inv) inv / s2
    xx, xy, yy = 4.0 * inv * inv / 1.5, 1.0 * inv * inv / 1.5, 6.0 * inv * inv / 1.5
    assert a["info"].tolist() == [[xx, xy, 0.0], [xy, yy, 0.0], [0.0, 0.0, 600.0]]
    assert run(sigma_min=3.0)["s2"] == 9.0 and run(sigma_min=1.0)["s2"] == 1.5 and run(sigma_min=2.0, r_scale=0.5)["s2"] == 2.0
    assert corridor_fuse()["s2"] == 0.25  # the corridor's points end on the walls' centres: the floor alone


def test_no_point_used_at_all():
    """n_last = 0 with min_points 0: mean 0, zero information, a zero innovation; the update is the prior's."""
    d2 = np.full((32, 32), 256, np.int64)
    a = 0.1 + 2.0 * np.pi * np.arange(40) / 40
    pts = np.stack([800.0 * np.cos(a), 800.0 * np.sin(a)], -1)
    pose = np.array([1600.0, 1500.0, 0.3])
    f = ffr.fuse(d2, pts, pose, P_CORRIDOR, None, (0.0, 0.0), KW, trunc=15.0, min_points=0, min_permille=0)
    assert f["flags"] == far.CONVERGED and f["n_used"].tolist() == [0, 0, 40]
    assert f["s2"] == 0.25 and not f["info"].any() and not f["info_f"].any() and f["nis"] == 0.0
    assert np.array_equal(f["pose_out"], pose) and np.allclose(f["P_out"], P_CORRIDOR, rtol=1e-14, atol=0.0)


# ---- the ABI checks that need no device ----

def test_params_default_and_struct_sizes():
    p = _lib.fieldfuse_params()
    got = {k: getattr(p, k) for k in ffr.DEFAULTS}
    assert got == ffr.DEFAULTS and p.reserved == 0
    assert p.nis_max == _lib.mapfuse_params().nis_max
    sizes = (C.c_int64 * 2)()
    assert _lib.load().lslam_fieldfuse_abi_sizes(sizes, 2) == 2
    assert list(sizes) == [C.sizeof(_lib.FieldFuseParams), C.sizeof(_lib.FieldFuseBatch)] == [48, 152]
    assert _lib.FieldFuseBatch.P.offset == C.sizeof(_lib.FieldAlignBatch) == 96
    assert (_lib.FIELDFUSE_OUTLIER, _lib.FIELDFUSE_BAD_COV) == (ffr.OUTLIER, ffr.BAD_COV) == (64, 128)
    from lidar_slam_amd import mapping
    assert mapping.FIELDFUSE_REJECTED == ffr.REJECTED == mapping.FIELDALIGN_REJECTED | 64 | 128


def call(b, g, p, f):
    L = _lib.load()
    st = L.lslam_field_fuse(None, None if b is None else C.byref(b), C.byref(g), None if p is None else C.byref(p),
                            None if f is None else C.byref(f))
    return st, L.lslam_last_error()


BAD_FIELDS = [(k, v) for k in ("sigma_min", "r_scale", "floor_t", "floor_r") for v in (0.0, -1.0, float("inf"), float("nan"))] + \
             [("nis_max", 0.0), ("nis_max", -1.0), ("nis_max", float("nan"))]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_validation_needs_no_device(field, value):
    st, msg = call(_lib.FieldFuseBatch(), _lib.grid_params(), _lib.fieldalign_params(), _lib.fieldfuse_params(**{field: value}))
    assert st == _lib.LSLAM_ERR_ARG and field in msg.decode() and b"fieldfuse" in msg


@pytest.mark.parametrize("field,value", [("trunc", -1.0), ("trunc", 255.5), ("damp_t", -1.0), ("eps_r", float("inf")), ("n_iter", 0),
                                         ("n_iter", 33), ("min_points", -1), ("min_permille", 1001), ("max_turn", -0.1)])
def test_checks_the_align_params_as_the_align_does(field, value):
    p, g, L = _lib.fieldalign_params(**{field: value}), _lib.grid_params(), _lib.load()
    st, msg = call(_lib.FieldFuseBatch(), g, p, _lib.fieldfuse_params())
    assert L.lslam_field_align(None, C.byref(_lib.FieldAlignBatch()), C.byref(g), C.byref(p)) == _lib.LSLAM_ERR_ARG
    assert st == _lib.LSLAM_ERR_ARG and msg == L.lslam_last_error() and field.encode() in msg


def test_accepts_the_ends_of_the_ranges():
    g, p = _lib.grid_params(), _lib.fieldalign_params()
    for kw in (dict(sigma_min=5e-324, r_scale=5e-324, floor_t=5e-324, floor_r=5e-324, nis_max=5e-324),
               dict(sigma_min=1.7e308, r_scale=1.7e308, floor_t=1.7e308, floor_r=1.7e308, nis_max=float("inf"))):
        st, msg = call(_lib.FieldFuseBatch(), g, p, _lib.fieldfuse_params(**kw))  # (an empty batch: then the context is named)
        assert st == _lib.LSLAM_ERR_ARG and b"ctx is NULL" in msg
    ends = _lib.fieldalign_params(trunc=0.0, damp_t=0.0, damp_r=0.0, eps_t=0.0, eps_r=0.0, max_shift=float("inf"),
                                  max_turn=float("inf"), n_iter=32, min_points=0, min_permille=1000)
    assert b"ctx is NULL" in call(_lib.FieldFuseBatch(), g, ends, _lib.fieldfuse_params())[1]


NAMES_A = ("xy", "pt_off", "pose", "origin", "d2", "pose_out", "trace", "normal", "n_used", "iters", "flags")
NAMES_F = ("P", "P_out", "z", "info", "info_f", "s2", "nis")


def full_batch(n_robots=1):
    """Every pointer set to an address of its own, 4096 bytes apart: nothing overlaps for one robot."""
    b = _lib.FieldFuseBatch()
    b.a.n_robots = n_robots
    for i, n in enumerate(NAMES_A):
        setattr(b.a, n, 4096 * (i + 1))
    for i, n in enumerate(NAMES_F):
        setattr(b, n, 4096 * (i + 1 + len(NAMES_A)))
    return b


def test_missing_pointers_and_nulls():
    g, p, f = _lib.grid_params(), _lib.fieldalign_params(), _lib.fieldfuse_params()
    assert b"batch is NULL" in call(None, g, p, f)[1]
    assert b"fieldalign: params is NULL" in call(_lib.FieldFuseBatch(), g, None, f)[1]
    assert b"fieldfuse: params is NULL" in call(_lib.FieldFuseBatch(), g, p, None)[1]
    b = _lib.FieldFuseBatch()
    b.a.n_robots = -1
    assert b"negative" in call(b, g, p, f)[1]
    st, msg = call(full_batch(), g, p, f)
    assert st == _lib.LSLAM_ERR_ARG and b"ctx is NULL" in msg
    for missing in NAMES_A + NAMES_F:
        b = full_batch()
        setattr(b.a if missing in NAMES_A else b, missing, None)
        st, msg = call(b, g, p, f)
        assert st == _lib.LSLAM_ERR_ARG and b"missing" in msg and missing.encode() in re.findall(rb"\w+", msg), missing
    st, msg = call(_lib.FieldFuseBatch(), _lib.grid_params(cell=0.0), p, f)
    assert st == _lib.LSLAM_ERR_ARG and b"cell" in msg


def test_z_must_not_overlap_the_filter():
    g, p, f = _lib.grid_params(), _lib.fieldalign_params(), _lib.fieldfuse_params()
    for other, owner in (("pose", "a"), ("pose_out", "a"), ("P", None), ("P_out", None)):
        for n_robots, shift in ((1, 0), (1, 16), (1, -16), (3, 64), (3, -64)):
            b = full_batch(n_robots)
            at = getattr(b.a if owner else b, other)
            b.z = at + shift
            st, msg = call(b, g, p, f)
            assert st == _lib.LSLAM_ERR_ARG and b"z must not overlap" in msg, (other, n_robots, shift)
        b = full_batch(3)
        at = getattr(b.a if owner else b, other)
        b.z = at - 72  # ends where the other begins
        assert b"ctx is NULL" in call(b, g, p, f)[1]
    b = full_batch(2)  # the pairs that may alias
    b.a.pose_out, b.P_out = b.a.pose, b.P
    assert b"ctx is NULL" in call(b, g, p, f)[1]
