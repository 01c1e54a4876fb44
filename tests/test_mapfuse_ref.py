"""The match-fusion definition (include/lidarslam.h, lslam_map_fuse) on the CPU: how the fused pose
and covariance behave in the synthetic room and in a corridor, hand-made moments, the gates, the
exactness of steps 6-8 against a 50-digit evaluation, and the ABI checks that need no device.
tests/mapfuse_ref.py is the NumPy form of the definition; tests/test_gpu_mapfuse.py holds the kernel
to it bit for bit.

Room.  test_mapmatch_ref's room_case("good", d), the prior P = diag(150^2, 150^2, 0.12^2) that the
guesses were drawn from, default parameters.  Caps (the match's own): every fused pose within 20 mm
and pi/360 rad of the truth, no flag, nis <= nis_max; P' symmetric bit for bit, positive definite,
each diagonal entry below P's.  Measured here: 4.53 mm and 0.0051 rad at worst, nis <= 1.76; match
standard deviations 6.4-14.6 mm and 0.0073-0.0095 rad against match errors of at most 4.6 mm and
0.0047 rad, normalised match errors e' Rm^-1 e <= 0.50: the covariance is conservative.  At
cut_permille 500 the fused pose reaches 22.7 mm, which is why the default is not lower.

Exactness.  Steps 6-8 against mpmath at 50 digits over the room cases and four prior scales, cap
1e-10 (absolute in mm and rad for x', relative to sqrt(P'ii P'jj) for P', relative for nis).
Measured worst: 2.3e-13 mm, 2.3e-16 rad, 4.4e-16 for P', 5.5e-16 for nis; the two controls (K
transposed: 3.9e4, the quantum floor left out: 6.6) miss the cap by orders of magnitude.
"""
import ctypes as C
import functools

import mpmath as mp
import numpy as np
import pytest

import mapfuse_ref as mfr
import mapmatch_ref as mmr
from lidar_slam_amd import _lib
from test_mapmatch_ref import KW, at_cell, cells, grid_with, pose_bits, room_case, room_setup
from test_occgrid_ref import ROOM_KW

P_ROOM = np.diag([150.0 ** 2, 150.0 ** 2, 0.12 ** 2])
ROOM_P = mmr.params(**ROOM_KW)


def row(res, r):
    """Robot r of a stacked mapmatch_ref.match_batch result, as mapmatch_ref.match returns it."""
    return {k: res[k][r] for k in ("delta", "best", "n_valid", "rot0", "scores", "flags", "pose_out")}


def room_fuse(which, draw, P, **fkw):
    """fuse_steps on every robot of a room case: [(guess, result)]."""
    _, g, res = room_case(which, draw) if which in ("good", "one") else room_case(which)
    fp = dict(mfr.DEFAULTS, **fkw)
    return [(g[r], mfr.fuse_steps(row(res, r), g[r], P, ROOM_P, fp)) for r in range(len(g))]


def test_room():
    truth = room_setup()[0]
    worst_d = worst_t = worst_nis = worst_ne = 0.0
    sd = []
    for draw in range(4):
        _, _, res = room_case("good", draw)
        for r, (g, f) in enumerate(room_fuse("good", draw, P_ROOM)):
            assert f["flags"] == res["flags"][r] == 0
            d = np.hypot(f["pose_out"][0] - truth[r, 0], f["pose_out"][1] - truth[r, 1])
            t = abs(f["pose_out"][2] - truth[r, 2])
            assert d <= 20.0 and t <= np.pi / 360, (draw, r, d, t)
            assert f["nis"] <= mfr.DEFAULTS["nis_max"]
            P1 = f["P_out"]
            assert np.array_equal(pose_bits(P1), pose_bits(P1.T))
            assert np.all(np.linalg.eigvalsh(P1) > 0) and np.all(np.diag(P1) < np.diag(P_ROOM)), P1
            assert np.array_equal(f["z"], g + f["delta"]) and f["moments"][0] >= 1
            e = f["z"] - truth[r]
            worst_ne = max(worst_ne, float(e @ np.linalg.solve(f["Rm"], e)))
            sd.append(np.sqrt(np.diag(f["Rm"])))
            worst_d, worst_t, worst_nis = max(worst_d, d), max(worst_t, t), max(worst_nis, float(f["nis"]))
    sd = np.array(sd)
    print("fused: worst", worst_d, "mm", worst_t, "rad, nis", worst_nis, "; match sd", sd.min(0), sd.max(0),
          "; normalised match error", worst_ne)
    assert worst_ne <= 3.0  # conservative: far inside one sigma^2 per degree of freedom


def test_room_lower_cut_is_why_the_default_is_900():
    """Reported, not capped: a cut of 500 lets far candidates pull the covariance wide."""
    truth = room_setup()[0]
    worst = 0.0
    for draw in range(4):
        for r, (g, f) in enumerate(room_fuse("good", draw, P_ROOM, cut_permille=500)):
            worst = max(worst, np.hypot(f["pose_out"][0] - truth[r, 0], f["pose_out"][1] - truth[r, 1]))
    print("cut 500: fused pose off by", worst, "mm at worst")


# ---- corridor: two full-width walls, the score row along them is flat ----

def corridor():
    L = np.zeros((32, 32), np.int16)
    L[13, :] = 100
    L[19, :] = 100
    pts = cells(*[(i, -3) for i in range(-3, 4)], *[(i, 3) for i in range(-3, 4)])
    return L, at_cell(16, 16), pts


def test_corridor():
    L, pose, pts = corridor()
    f = mfr.fuse(L, (0.0, 0.0), pose, np.diag([1e4, 1e4, 1e-2]), pts, **KW)
    # 14 points score on every shift along x and under every rotation, on no other row: 27 ties, the
    # centre wins; cut = 12, w = 2 each: sum w a^2 = 2 * 3 * 60, sum w c^2 = 2 * 9 * 2
    assert f["best"].tolist() == [1, 4, 4, 14] and f["flags"] == 0
    assert f["moments"].tolist() == [54, 0, 0, 0, 360, 0, 0, 0, 0, 36]
    Rm = f["Rm"]
    assert Rm[1, 1] == (100.0 * 100.0) / 12.0  # across: the quantum alone, exactly
    assert Rm[0, 0] == ((360.0 / 54.0) * 100.0) * 100.0 + (100.0 * 100.0) / 12.0
    print("corridor: variance along / across", Rm[0, 0] / Rm[1, 1])
    assert Rm[0, 0] >= 10.0 * Rm[1, 1]
    assert not Rm[0, 1] and not Rm[0, 2] and not Rm[1, 2] and np.array_equal(Rm, Rm.T)
    # the update trusts the match across the corridor far more than along it
    P1 = f["P_out"]
    assert P1[1, 1] < 0.1 * 1e4 and P1[0, 0] > 0.8 * 1e4


# ---- hand-made moments ----

def winner(S, kt, kth):
    from scanmatch_ref import pick
    return pick(S, dict(k_trans=kt, k_theta=kth, cell=1.0, theta_step=1.0))[1]


def test_moments_one_candidate():
    f = mfr.fuse(grid_with(32, [(17, 16)]), (0.0, 0.0), at_cell(16, 16), np.eye(3), cells((1, 0)),
                 **dict(KW, k_trans=0, k_theta=0))
    assert f["scores"].shape == (1, 1, 1) and f["best"].tolist() == [0, 0, 0, 1] and f["flags"] == mfr.EDGE
    assert f["moments"].tolist() == [1] + [0] * 9
    q, qt = (100.0 * 100.0) / 12.0, (KW.get("theta_step", np.pi / 360) ** 2) / 12.0
    assert np.array_equal(f["Rm"], np.diag([q, q, qt]))
    assert np.array_equal(f["z"], at_cell(16, 16)) and np.array_equal(f["pose_out"], at_cell(16, 16)) and f["nis"] == 0.0
    assert mfr.moments(np.full((1, 1, 1), 1000, np.int32), (0, 0, 0, 1000), 900) == [100] + [0] * 9


def test_moments_winner_in_a_corner():
    S = np.zeros((3, 9, 9), np.int32)
    S[2, 8, 8], S[0, 0, 0], S[1, 4, 4] = 100, 95, 90  # cut = 90: the centre weighs nothing
    best = winner(S, 4, 1)
    assert best.tolist() == [2, 8, 8, 100]
    assert mfr.moments(S, best, 900) == [15, -40, -40, -10, 320, 320, 80, 320, 80, 20]
    assert mfr.moments(S, best, 0) == [285, -760 - 360, -760 - 360, -190 - 90, 6080 + 1440, 6080 + 1440, 1520 + 360,
                                       6080 + 1440, 1520 + 360, 380 + 90]
    # the largest window: |a|, |b| = 30, |c| = 62
    S = np.zeros((63, 31, 31), np.int32)
    S[62, 30, 30], S[0, 0, 0] = 1000, 950
    best = winner(S, 15, 31)
    assert best.tolist() == [62, 30, 30, 1000]
    assert mfr.moments(S, best, 900) == [150, -1500, -1500, -3100, 45000, 45000, 93000, 45000, 93000, 192200]


def test_moments_of_a_tie_follow_the_winner_of_step_3():
    S = np.zeros((3, 9, 9), np.int32)
    S[1, 4, 3] = S[1, 4, 5] = S[0, 4, 4] = 7  # d2 = 1 each: the smallest flat index wins
    best = winner(S, 4, 1)
    assert best.tolist() == [0, 4, 4, 7]
    assert mfr.moments(S, best, 900) == [3, 0, 0, 2, 2, 0, 0, 0, 0, 2]
    # through the matcher: test_mapmatch_ref.test_tie_break_order's map; the nearer cell wins, the
    # other weighs in at a = -4, both under all three rotations
    f = mfr.fuse(grid_with(32, [(17, 16), (13, 16)]), (0.0, 0.0), at_cell(16, 16), np.eye(3) * 1e4, cells((0, 0)), **KW)
    assert f["best"].tolist() == [1, 4, 5, 1]
    assert f["moments"].tolist() == [6, -12, 0, 0, 48, 0, 0, 0, 0, 4]
    assert f["Rm"][0, 0] == ((48.0 / 6.0 - (-12.0 / 6.0) * (-12.0 / 6.0)) * 100.0) * 100.0 + (100.0 * 100.0) / 12.0


def test_moment_bound():
    """The largest sums a volume can hold stay below 5e17, inside int64."""
    S = np.full((63, 31, 31), 2 ** 31 - 1, np.int32)
    S[62, 30, 30] = 0  # any winner: the moments about the far corner are the largest
    mo = mfr.moments(S, (62, 30, 30, 0), 0)
    assert max(abs(v) for v in mo) < 5 * 10 ** 17 < 2 ** 63
    assert mo[9] == (2 ** 31 - 1) * 31 * 31 * sum(c * c for c in range(63))


# ---- gates ----

HAND = dict(L=grid_with(32, [(18, 17), (19, 17), (18, 19)]), origin=(0.0, 0.0), pose=at_cell(16, 16),
            xy=cells((1, 1), (2, 1), (1, 3)))


def hand(P, **kw):
    return mfr.fuse(HAND["L"], HAND["origin"], HAND["pose"], P, HAND["xy"], **dict(KW, **kw))


@functools.lru_cache(maxsize=None)
def room_off_by_100():
    """The room matched from 100 mm beside the truth: (guesses, match results)."""
    truth, rev5, off, L5, _, origin, _ = room_setup()
    g = truth + [100.0, 0.0, 0.0]
    return g, mmr.match_batch(L5, origin, g, rev5["xy"], off, **ROOM_KW)


def test_outlier_gate():
    g, res = room_off_by_100()
    P = np.diag([1.0, 1.0, 1e-6])
    for r in range(len(g)):
        assert res["flags"][r] == 0
        f = mfr.fuse_steps(row(res, r), g[r], P, ROOM_P, dict(mfr.DEFAULTS))
        assert f["flags"] == mfr.OUTLIER and f["nis"] > 16.27, (r, f["nis"])
        assert np.array_equal(pose_bits(f["pose_out"]), pose_bits(g[r])) and np.array_equal(pose_bits(f["P_out"]), pose_bits(P))
        assert np.array_equal(f["z"], g[r] + f["delta"]) and f["Rm"][0, 0] > 0 and f["moments"][0] > 0  # reported
        # without a gate the same match updates
        f = mfr.fuse_steps(row(res, r), g[r], P, ROOM_P, dict(mfr.DEFAULTS, nis_max=np.inf))
        assert f["flags"] == 0 and np.any(f["pose_out"] != g[r]) and np.all(np.diag(f["P_out"]) < np.diag(P))


def test_nis_at_the_gate_is_accepted():
    P = np.diag([1e4, 1e4, 1e-2])
    nis = hand(P)["nis"]
    assert 0.0 < nis < 16.27
    assert hand(P, nis_max=float(nis))["flags"] == 0
    f = hand(P, nis_max=float(np.nextafter(nis, 0.0)))
    assert f["flags"] == mfr.OUTLIER and f["nis"] == nis
    assert hand(P, nis_max=np.inf)["flags"] == 0 and hand(P, nis_max=5e-324)["flags"] == mfr.OUTLIER


def nan_payload():
    return np.frombuffer(np.uint64(0x7FF80000DEADBEEF).tobytes(), np.float64)[0]


BAD_COVS = [("nan", (0, 1), np.nan), ("payload", (2, 2), nan_payload()), ("inf", (1, 1), np.inf), ("-inf", (0, 2), -np.inf),
            ("negative x", (0, 0), -1e4), ("negative theta", (2, 2), -1.0), ("negative y", (1, 1), -1e4)]


@pytest.mark.parametrize("what,at,value", BAD_COVS)
def test_bad_cov(what, at, value):
    P = np.diag([1e4, 1e4, 1e-2])
    P[at] = value
    f = hand(P)
    assert f["flags"] == mfr.BAD_COV and f["nis"] == 0.0 and not np.signbit(f["nis"])
    assert np.array_equal(pose_bits(f["pose_out"]), pose_bits(HAND["pose"]))
    assert np.array_equal(pose_bits(f["P_out"]), pose_bits(P))
    assert f["moments"][0] > 0 and f["Rm"][0, 0] > 0 and f["z"][0] == HAND["pose"][0] + 100.0  # reported


def test_weak_and_empty_leave_the_filter_alone():
    _, g, res = room_case("bad")
    P = np.array(P_ROOM)
    P[0, 1] = nan_payload()  # (the gate on P is still evaluated for a WEAK robot, and reported)
    for r, (_, f) in enumerate(room_fuse("bad", 0, P_ROOM)):
        assert f["flags"] & mfr.WEAK and not f["flags"] & (mfr.EMPTY | mfr.BAD_POSE)
        assert np.array_equal(pose_bits(f["pose_out"]), pose_bits(g[r])) and np.array_equal(pose_bits(f["P_out"]), pose_bits(P_ROOM))
        assert f["moments"][0] > 0 and np.all(np.diag(f["Rm"]) > 0) and np.array_equal(f["z"], g[r] + f["delta"])
        assert f["nis"] > 0.0
    f = mfr.fuse_steps(row(res, 0), g[0], P, ROOM_P, dict(mfr.DEFAULTS))
    assert f["flags"] & mfr.WEAK and f["flags"] & mfr.BAD_COV and f["nis"] == 0.0
    assert np.array_equal(pose_bits(f["P_out"]), pose_bits(P))
    # EMPTY (the window off the map) and BAD_POSE: zeros, z = pose, and P is not looked at
    L = np.full((32, 32), 300, np.int16)
    for pose, flag in ((at_cell(60, 8, 0.1), mfr.EMPTY), (np.array([np.nan, 1650.0, 0.1]), mfr.BAD_POSE),
                       (np.array([1650.0, 1650.0, nan_payload()]), mfr.BAD_POSE)):
        f = mfr.fuse(L, (0.0, 0.0), pose, P, cells((1, 1)), **KW)
        assert f["flags"] == flag
        assert not f["moments"].any() and not f["Rm"].any() and f["nis"] == 0.0 and not f["delta"].any()
        for key in ("pose_out", "z"):
            assert np.array_equal(pose_bits(f[key]), pose_bits(pose)), key
        assert np.array_equal(pose_bits(f["P_out"]), pose_bits(P))


def test_edge_alone_still_updates():
    _, g, res = room_case("edge")
    for r, (_, f) in enumerate(room_fuse("edge", 0, np.diag([250.0 ** 2, 250.0 ** 2, 0.12 ** 2]))):
        assert f["flags"] == mfr.EDGE and f["pose_out"][0] > g[r, 0] + 100.0 and f["P_out"][0, 0] < 250.0 ** 2


def test_r_scale_scales_the_match_covariance():
    P = np.diag([1e4, 1e4, 1e-2])
    a, b = hand(P), hand(P, r_scale=4.0)
    assert np.array_equal(b["Rm"], a["Rm"] * 4.0) and np.array_equal(a["moments"], b["moments"])
    assert b["nis"] < a["nis"] and np.all(np.diag(b["P_out"]) > np.diag(a["P_out"]))


# ---- exactness of steps 6-8 against 50 digits ----

def exact_steps(mo, y, x, P, sc, r_scale, transpose_K=False, floor=True):
    """Steps 6-8 in mpmath from the same inputs: (x', P', nis)."""
    mp.mp.dps = 50
    M = lambda a: mp.matrix([[mp.mpf(float(v)) for v in rw] for rw in np.atleast_2d(a)])  # noqa: E731
    W = mp.mpf(int(mo[0]))
    mean = [mp.mpf(int(mo[1 + i])) / W for i in range(3)]
    m2 = {(0, 0): mo[4], (0, 1): mo[5], (0, 2): mo[6], (1, 1): mo[7], (1, 2): mo[8], (2, 2): mo[9]}
    Rm = mp.zeros(3, 3)
    s = [mp.mpf(float(v)) for v in sc]
    for i in range(3):
        for j in range(i, 3):
            v = (mp.mpf(int(m2[i, j])) / W - mean[i] * mean[j]) * s[i] * s[j]
            if i == j and floor:
                v += s[i] * s[i] / 12
            Rm[i, j] = Rm[j, i] = v * mp.mpf(float(r_scale))
    Pm, ym = M(P), M(y).T
    Si = mp.inverse(Pm + Rm)
    nis = (ym.T * Si * ym)[0]
    K = Pm * Si
    if transpose_K:
        K = K.T
    x1 = M(x).T + K * ym
    A = mp.eye(3) - K
    P1 = A * Pm * A.T + K * Rm * K.T
    return x1, P1, nis


def exact_errors(f_x, f_P, f_nis, ex):
    x1, P1, nis = ex
    ex_ = [abs(mp.mpf(float(f_x[i])) - x1[i]) for i in range(3)]
    eP = max(abs(mp.mpf(float(f_P[i, j])) - P1[i, j]) / mp.sqrt(P1[i, i] * P1[j, j]) for i in range(3) for j in range(3))
    en = abs(mp.mpf(float(f_nis)) - nis) / nis
    return float(max(ex_[0], ex_[1])), float(ex_[2]), float(eP), float(en)


CORR = np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.1], [-0.2, 0.1, 1.0]])
SCALES = [(150.0 ** 2, 150.0 ** 2, 0.12 ** 2), (1e6, 1e-2, 1e-8), (4.0, 4.0, 1e-6), (1e8, 1e8, 10.0)]


def test_steps_6_to_8_against_50_digits():
    cap = 1e-10
    worst = np.zeros(4)
    ctl_K = ctl_floor = 0.0
    sc = (ROOM_P["cell"], ROOM_P["cell"], ROOM_P["theta_step"])
    for draw in range(4):
        _, g, res = room_case("good", draw)
        for r in range(len(g)):
            m = row(res, r)
            mo = mfr.moments(m["scores"], m["best"], 900)
            Rm = mfr.match_cov(mo, sc[0], sc[2], 1.0)
            y = np.array(m["delta"])
            if not y.any():
                continue  # (nis is 0: no relative error)
            for scale in SCALES:
                d = np.sqrt(np.array(scale))
                P = CORR * d[:, None] * d[None, :]
                Si, nis = mfr.gate(P, Rm, y)
                assert Si is not None
                x1, P1 = mfr.update(g[r], P, Rm, Si, y)
                worst = np.maximum(worst, exact_errors(x1, P1, nis, exact_steps(mo, y, g[r], P, sc, 1.0)))
                e = exact_errors(x1, P1, nis, exact_steps(mo, y, g[r], P, sc, 1.0, transpose_K=True))
                ctl_K = max(ctl_K, e[0], e[1], e[2])
                e = exact_errors(x1, P1, nis, exact_steps(mo, y, g[r], P, sc, 1.0, floor=False))
                ctl_floor = max(ctl_floor, *e)
    print("worst against 50 digits: x'", worst[0], "mm", worst[1], "rad; P'", worst[2], "; nis", worst[3],
          "; controls: K transposed", ctl_K, ", no quantum floor", ctl_floor)
    assert np.all(worst <= cap), worst
    assert ctl_K > cap and ctl_floor > cap


# ---- ABI, no device ----

def test_mapfuse_params_default_and_constants():
    p = _lib.mapfuse_params()
    assert (p.r_scale, p.nis_max, p.cut_permille, p.reserved) == (1.0, 16.27, 900, 0)
    assert mfr.DEFAULTS == dict(r_scale=1.0, nis_max=16.27, cut_permille=900)
    assert (_lib.MAPFUSE_OUTLIER, _lib.MAPFUSE_BAD_COV) == (16, 32) == (mfr.OUTLIER, mfr.BAD_COV)
    assert (mfr.EMPTY, mfr.EDGE, mfr.BAD_POSE, mfr.WEAK) == (1, 2, 4, 8)
    assert _lib.K_MAPFUSE == 12 and _lib.K_MAPMATCH == 11 and _lib.ABI_VERSION == 6
    assert _lib.load().lslam_mapfuse_params_default(None) == _lib.LSLAM_ERR_ARG


def test_mapfuse_struct_sizes():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_mapfuse_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.MapFuseParams) == 24
    assert got[1] == C.sizeof(_lib.MapFuseBatch) == 160
    assert _lib.MapFuseBatch.m.offset == 0 and _lib.MapFuseBatch.P.offset == 112 and _lib.MapFuseBatch.moments.offset == 152
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_mapfuse_abi_sizes(one, 1) == 2 and list(one) == [24, -1]
    assert L.lslam_mapfuse_abi_sizes(None, 2) == 2
    two, nine = (C.c_int64 * 2)(), (C.c_int64 * 9)()
    assert L.lslam_mapmatch_abi_sizes(two, 2) == 2 and list(two) == [32, 112]  # the earlier tables are as they were
    assert L.lslam_grid_abi_sizes(two, 2) == 2 and list(two) == [40, 72]
    assert L.lslam_abi_sizes(nine, 9) == 9 and list(nine) == [112, 56, 56, 128, 232, 48, 48, 32, 96]


def call(b, g, m, f):
    L = _lib.load()
    ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
    st = L.lslam_map_fuse(None, ref(b), ref(g), ref(m), ref(f))
    return st, L.lslam_last_error()


BAD_FIELDS = [("r_scale", 0.0), ("r_scale", -1.0), ("r_scale", float("nan")), ("r_scale", float("inf")),
              ("nis_max", 0.0), ("nis_max", -1.0), ("nis_max", float("nan")), ("nis_max", float("-inf")),
              ("cut_permille", -1), ("cut_permille", 1000)]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_mapfuse_validation_needs_no_device(field, value):
    b = _lib.MapFuseBatch()
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(), _lib.mapfuse_params())
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg  # valid parameters, an empty batch: only the context is missing
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(), _lib.mapfuse_params(**{field: value}))
    assert st == _lib.LSLAM_ERR_ARG and field.encode() in msg and b"mapfuse" in msg


@pytest.mark.parametrize("field,value", [("win_w", 14), ("k_trans", 16), ("k_theta", 32), ("theta_step", 0.0),
                                         ("min_permille", 1001)])
def test_mapfuse_checks_the_match_params_as_the_match_does(field, value):
    st, msg = call(_lib.MapFuseBatch(), _lib.grid_params(), _lib.mapmatch_params(**{field: value}), _lib.mapfuse_params())
    assert st == _lib.LSLAM_ERR_ARG and field.encode() in msg
    st, msg = call(_lib.MapFuseBatch(), _lib.grid_params(grid_w=15), _lib.mapmatch_params(), _lib.mapfuse_params())
    assert st == _lib.LSLAM_ERR_ARG and b"grid_w" in msg


def test_mapfuse_accepts_the_ends_of_the_ranges():
    b = _lib.MapFuseBatch()
    for kw in (dict(r_scale=5e-324, nis_max=5e-324, cut_permille=0),
               dict(r_scale=1.7976931348623157e308, nis_max=float("inf"), cut_permille=999)):
        st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(), _lib.mapfuse_params(**kw))
        assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg, kw


INPUTS = ("xy", "pt_off", "pose", "origin", "logodds", "rot")
OUTPUTS = ("pose_out", "delta", "best", "n_valid", "rot0", "flags")
FUSE_OUTPUTS = ("P_out", "z", "Rm", "nis")


def test_mapfuse_missing_pointers():
    g, m, f = _lib.grid_params(), _lib.mapmatch_params(), _lib.mapfuse_params()

    def batch(without=None):
        b = _lib.MapFuseBatch()
        b.m.n_robots = 1
        for name in INPUTS + OUTPUTS:
            if name != without:
                setattr(b.m, name, 4096)
        for name in ("P",) + FUSE_OUTPUTS:
            if name != without:
                setattr(b, name, 4096)
        return b

    for name in INPUTS + ("P",):
        st, msg = call(batch(name), g, m, f)
        assert st == _lib.LSLAM_ERR_ARG and b"missing input" in msg and name.encode() in msg, name
    for name in OUTPUTS + FUSE_OUTPUTS:
        st, msg = call(batch(name), g, m, f)
        assert st == _lib.LSLAM_ERR_ARG and b"missing output" in msg and name.encode() in msg, name
    b = batch()
    assert not b.moments and not b.m.scores  # both optional: only the context is missing
    st, msg = call(b, g, m, f)
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg
    b.m.n_robots = -1
    assert call(b, g, m, f)[0] == _lib.LSLAM_ERR_ARG
    for args in ((None, g, m, f), (batch(), None, m, f), (batch(), g, None, f), (batch(), g, m, None)):
        assert call(*args)[0] == _lib.LSLAM_ERR_ARG
    empty = _lib.MapFuseBatch()  # n_robots == 0 with no pointer at all: nothing but the context is asked for
    st, msg = call(empty, g, m, f)
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg
