"""The relocalisation definition (include/lidarslam.h, lslam_map_relocalize) on the CPU: the NumPy
reference held against a second, loop-by-loop form of its coarse stage, hand-made cases for each
rule, the two room scenes, and the ABI checks that need no device.  tests/reloc_ref.py is the NumPy
form of the definition; tests/test_gpu_reloc.py holds the kernels to it bit for bit.

L-shaped room (unique).  Outline (0,0)-(4000,0)-(4000,2000)-(3000,2000)-(3000,3000)-(0,3000) mm, the
walls drawn one cell thick into a 512-cell grid of 20 mm; revolutions of 720 beams ray-cast from
eight fixed poses with synth.scan_polar_at's noise model (sigma 5 mm, 3 % outliers); defaults
throughout.  Caps: 30 mm (1.5 cells) and 0.0131 rad (1.5 theta_step); every pose found, neither flag
set, the winner at coarse rank 0.  Measured with this reference: 7.9 mm and 0.0079 rad at worst
(two thirds of the caps are 20 mm and 0.0087 rad), the best rival at 0.863 of the winner's fine
score at most.

Plain room (symmetric under a half turn).  The 4000 x 3000 room of synth.py, two poses: AMBIGUOUS,
the rival at 0.9 of the winner's fine score or more, pose_out untouched.  Measured: the two
candidates' coarse scores (702, 702 and 628, 628) and fine scores (1825, 1825 and 1821, 1821) are
equal.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mapmatch_ref as mmr
import reloc_ref as rr
from lidar_slam_amd import _lib, synth
from test_mapmatch_ref import pose_bits

L_OUTLINE = [(0.0, 0.0), (4000.0, 0.0), (4000.0, 2000.0), (3000.0, 2000.0), (3000.0, 3000.0), (0.0, 3000.0)]
RECT_OUTLINE = [(0.0, 0.0), (synth.ROOM_W, 0.0), (synth.ROOM_W, synth.ROOM_H), (0.0, synth.ROOM_H)]
SCENE_ORIGIN = (-3110.0, -3610.0)  # the room in the middle of the 10.24 m grid, its walls through cell centres
L_POSES = np.array([[800.0, 700.0, 0.3], [2000.0, 1000.0, 5.1], [3400.0, 1200.0, 2.5], [1500.0, 2400.0, 1.0],
                    [600.0, 2500.0, 3.5], [2600.0, 1500.0, 0.05], [3500.0, 500.0, 4.0], [2400.0, 2550.0, 6.0]])
RECT_POSES = np.array([[1200.0, 900.0, 0.7], [2900.0, 1800.0, 4.4]])
CAP_MM, CAP_RAD = 30.0, 0.0131


def draw_walls(outline, grid_w=512, cell=20.0, origin=SCENE_ORIGIN):
    """A map of free space (-41) with the outline's walls occupied (350), one cell thick."""
    L = np.full((grid_w, grid_w), -41, np.int16)
    pts = np.array(outline)
    for a, b in zip(pts, np.roll(pts, -1, axis=0)):
        n = int(np.hypot(*(b - a)) / 2.0) + 1
        t = np.linspace(0.0, 1.0, n)[:, None]
        p = a + t * (b - a)
        ix = np.floor((p[:, 0] - origin[0]) / cell).astype(int)
        iy = np.floor((p[:, 1] - origin[1]) / cell).astype(int)
        L[iy, ix] = 350
    return L


def ray_outline(outline, px, py, ang):
    """Distance from (px, py) along each direction ang to the nearest wall of the outline."""
    pts = np.array(outline)
    d = np.stack([np.cos(ang), np.sin(ang)], -1)
    best = np.full(ang.shape, np.inf)
    for a, b in zip(pts, np.roll(pts, -1, axis=0)):
        e = b - a
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a[0] - px) * e[1] - (a[1] - py) * e[0]) / den
            u = ((a[0] - px) * d[:, 1] - (a[1] - py) * d[:, 0]) / den
        ok = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(ok & (t < best), t, best)
    return best


def revolution(outline, pose, scan_id, n_beams=720):
    """One revolution seen from pose in the outline's room: synth.scan_polar_at's beam model, noise
    and outliers, with the outline's walls in the place of the rectangle's."""
    rng = np.random.default_rng(1_000_003 * int(scan_id) + 0x5A17)
    px, py, heading = (float(v) for v in pose)
    theta = np.arange(n_beams, dtype=np.float64) * (360.0 / n_beams)
    world = heading + (np.pi / 2 - np.deg2rad(theta))
    dist = ray_outline(outline, px, py, world) + rng.normal(0.0, synth.NOISE_MM, n_beams)
    out = rng.random(n_beams) < synth.OUTLIER_FRAC
    dist = np.where(out, rng.uniform(150.0, 5000.0, n_beams), dist)
    return synth.polar_to_xy_ref(theta, dist)


@functools.lru_cache(maxsize=None)
def scene(which):
    """(map [512][512], poses [n, 3], revolutions: a list of [720, 2]); which = "L" or "rect"."""
    outline, poses = (L_OUTLINE, L_POSES) if which == "L" else (RECT_OUTLINE, RECT_POSES)
    return draw_walls(outline), poses, [revolution(outline, p, 900 + i) for i, p in enumerate(poses)]


@functools.lru_cache(maxsize=None)
def scene_case(which, i):
    """The reference's result for pose i of a scene (NumPy's cos and sin for the fine stage)."""
    L, poses, revs = scene(which)
    return rr.relocalize(L, SCENE_ORIGIN, revs[i])


def pose_error(pose, truth):
    dth = np.abs(pose[2] - truth[2]) % (2 * np.pi)
    return np.hypot(pose[0] - truth[0], pose[1] - truth[1]), min(dth, 2 * np.pi - dth)


def test_rectangle_scans_are_synth_scans():
    """The ray-caster on the plain room's outline is synth.scan_polar_at."""
    th, d = synth.scan_polar_at(RECT_POSES[0], 900)
    assert np.allclose(synth.polar_to_xy_ref(th, d), revolution(RECT_OUTLINE, RECT_POSES[0], 900), atol=1e-6)


@pytest.mark.parametrize("i", range(len(L_POSES)))
def test_l_room_is_found(i):
    res = scene_case("L", i)
    dpos, dth = pose_error(res["pose_out"], L_POSES[i])
    sw, sr = int(res["result"][5]), int(res["result"][7])
    print("pose", i, "flags", res["flags"], "result", res["result"].tolist(), "error", dpos, "mm", dth, "rad; rival ratio",
          sr / max(sw, 1), "n_occ", res["n_occ"], "n_used", res["n_used"])
    assert res["flags"] == 0 and res["result"][0] == 0
    assert dpos <= CAP_MM and dth <= CAP_RAD
    assert dpos <= CAP_MM * 2 / 3 and dth <= CAP_RAD * 2 / 3  # the margin these poses were chosen with
    assert 1000 * sr < 900 * sw
    sxy, sth = rr.DEFAULTS["reset_sigma_xy"], rr.DEFAULTS["reset_sigma_theta"]
    assert np.array_equal(res["P_out"], np.diag([sxy * sxy, sxy * sxy, sth * sth]).ravel())


@pytest.mark.parametrize("i", range(len(RECT_POSES)))
def test_plain_room_is_ambiguous(i):
    res = scene_case("rect", i)
    sw, sr = int(res["result"][5]), int(res["result"][7])
    print("pose", i, "result", res["result"].tolist(), "cand", res["cand"][:2].tolist(), "rival ratio", sr / max(sw, 1))
    assert res["flags"] == rr.AMBIGUOUS and res["result"][6] >= 0
    assert 1000 * sr >= 900 * sw
    assert np.all(np.isnan(res["pose_out"])) and not res["P_out"].any()  # untouched
    # the winner or its rival is the true pose, the other its image under the half turn about the room's centre
    truth = RECT_POSES[i]
    image = np.array([synth.ROOM_W - truth[0], synth.ROOM_H - truth[1], truth[2] + np.pi])
    pair = [res["fine_pose"][res["result"][0]], res["fine_pose"][res["result"][6]]]
    for want in (truth, image):
        assert min(max(pose_error(p, want)[0] / CAP_MM, pose_error(p, want)[1] / CAP_RAD) for p in pair) <= 1.0


# ---- the coarse stage against a loop-by-loop form ----

def loops_scores(C, pts, head_rot, cellc):
    Wc = C.shape[0]
    invc = 1.0 / cellc
    Sc = np.zeros((len(head_rot), Wc, Wc), np.int32)
    for k, (c, s) in enumerate(head_rot):
        for x, y in pts:
            ax = np.floor((c * x - s * y) * invc + 0.5)
            ay = np.floor((s * x + c * y) * invc + 0.5)
            if not (-Wc < ax < Wc and -Wc < ay < Wc):
                continue
            for ty in range(Wc):
                for tx in range(Wc):
                    yy, xx = ty + int(ay), tx + int(ax)
                    if 0 <= yy < Wc and 0 <= xx < Wc and C[yy, xx]:
                        Sc[k, ty, tx] += 1
    return Sc


def loops_peaks(Sc, K):
    nh, Wc, _ = Sc.shape

    def before(a, b):  # candidate a comes before candidate b
        sa, sb = Sc[a], Sc[b]
        fa, fb = (a[0] * Wc + a[1]) * Wc + a[2], (b[0] * Wc + b[1]) * Wc + b[2]
        return sa > sb or (sa == sb and fa < fb)

    found = []
    for k in range(nh):
        for ty in range(Wc):
            for tx in range(Wc):
                if Sc[k, ty, tx] <= 0:
                    continue
                nb = {((k + dk) % nh, ty + dy, tx + dx) for dk in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                      if 0 <= ty + dy < Wc and 0 <= tx + dx < Wc} - {(k, ty, tx)}
                if all(before((k, ty, tx), n) for n in nb):
                    found.append((-int(Sc[k, ty, tx]), (k * Wc + ty) * Wc + tx))
    return [f for _, f in sorted(found)][:K]


@pytest.mark.parametrize("Wc,n_head,f", [(5, 4, 2), (9, 5, 4), (9, 4, 8)])
def test_coarse_stage_against_loops(Wc, n_head, f):
    rng = np.random.default_rng(10 * Wc + n_head)
    cell, gw = 50.0, Wc * f
    L = np.full((gw, gw), -10, np.int16)
    # hand-placed cells: the corners of the grid, one cell exactly at occ_min, one just below, a few inside
    for y, x in [(0, 0), (gw - 1, gw - 1), (0, gw - 1), (gw // 2, gw // 2), (f, 2 * f + 1), (3 * f - 1, f)]:
        L[y, x] = 85
    L[gw // 2 + 1, 1] = 84
    C = rr.coarse_map(L, gw, f, 85)
    assert C[0, 0] and C[-1, -1] and C[0, -1] and not C[(gw // 2 + 1) // f, 0] and C.sum() == 6
    pts = rng.uniform(-Wc * cell * f * 0.8, Wc * cell * f * 0.8, (25, 2))
    pts = np.concatenate([pts, [[np.nan, 1.0], [0.0, 0.0], [np.inf, 3.0], [1e5, 0.0], [cell * f * (Wc - 0.5), 0.0],
                                [cell * f * (Wc - 0.5001), 0.0], [-cell * f * (Wc - 0.5), 10.0]]])
    used = rr.used_points(pts, 8000.0)
    assert len(used) == len(pts) - 4  # NaN, (0, 0), inf and the point beyond max_range
    head = rr.head_table(n_head, 2 * np.pi / n_head)
    Sc = rr.coarse_scores(C, used, head, cell * f)
    assert np.array_equal(Sc, loops_scores(C, used, head, cell * f)) and Sc.any()
    for K in (1, 3, 16):
        assert list(rr.peaks(Sc, K)) == loops_peaks(Sc, K), K
    # a random volume with many ties: the peak rule alone
    S = rng.integers(0, 3, (n_head, Wc, Wc)).astype(np.int32)
    assert list(rr.peaks(S, 16)) == loops_peaks(S, 16)


# ---- hand-made cases for the rules ----

def flat_of(Sc, k, ty, tx):
    return (k * Sc.shape[1] + ty) * Sc.shape[1] + tx


def test_tie_break_by_flat_index():
    S = np.zeros((4, 6, 6), np.int32)
    S[2, 3, 3] = S[0, 1, 1] = S[2, 0, 0] = 7   # three equal, separated peaks: flat order
    S[0, 1, 2] = 7                              # a neighbour of (0, 1, 1) with the same score: the smaller index wins
    assert list(rr.peaks(S, 8)) == [flat_of(S, 0, 1, 1), flat_of(S, 2, 0, 0), flat_of(S, 2, 3, 3)]
    S[2, 3, 3] = 8
    assert list(rr.peaks(S, 2)) == [flat_of(S, 2, 3, 3), flat_of(S, 0, 1, 1)]


def test_peak_across_the_heading_wrap():
    S = np.zeros((5, 6, 6), np.int32)
    S[0, 2, 2], S[4, 2, 3] = 5, 6   # neighbours through the wrap: only the higher one is a peak
    assert list(rr.peaks(S, 8)) == [flat_of(S, 4, 2, 3)]
    S[4, 2, 3] = 5                  # equal: the smaller flat index, k = 0
    assert list(rr.peaks(S, 8)) == [flat_of(S, 0, 2, 2)]
    S[2, 2, 2] = 1                  # not a neighbour of either
    assert list(rr.peaks(S, 8)) == [flat_of(S, 0, 2, 2), flat_of(S, 2, 2, 2)]


def test_peak_on_the_border_and_fewer_peaks_than_k():
    S = np.zeros((4, 5, 5), np.int32)
    S[1, 0, 0], S[1, 4, 4], S[3, 0, 4] = 3, 2, 9   # translations do not wrap: (0, 0) and (4, 4) are apart
    assert list(rr.peaks(S, 16)) == [flat_of(S, 3, 0, 4), flat_of(S, 1, 0, 0), flat_of(S, 1, 4, 4)]
    cand, pose = rr.candidates(S, 5, (100.0, -50.0), 80.0, 0.5)
    assert cand.tolist() == [[3, 0, 4, 9], [1, 0, 0, 3], [1, 4, 4, 2], [-1, -1, -1, 0], [-1, -1, -1, 0]]
    assert pose[0].tolist() == [100.0 + 4.5 * 80.0, -50.0 + 0.5 * 80.0, 1.5] and np.all(np.isnan(pose[3:]))
    assert np.array_equal(pose_bits(pose[3:]), np.full((2, 3), 0x7FF8000000000000, np.uint64))  # quiet NaNs


def test_selection_and_the_duplicate_rule():
    q = dict(rr.DEFAULTS)
    cand = np.array([[k, k + 1, k + 2, 100 - k] for k in range(5)], np.int32)
    pose = np.array([[0.0, 0.0, 0.01], [60.0, -100.0, 6.2831], [0.0, 100.0001, 0.0], [5000.0, 0.0, 3.0], [1.0, 1.0, 0.0]])
    best = np.zeros((5, 4), np.int32)
    best[:, 3] = [1000, 990, 800, 899, 2000]
    flags = np.array([0, mmr.EDGE, 0, 0, mmr.WEAK], np.int32)
    # rank 4 is WEAK; rank 0 wins; rank 1 is a duplicate (dt = 0.0102 through two_pi, |dy| = dup_mm exactly);
    # rank 2 is 0.0001 mm past dup_mm: the best rival at 0.8; rank 3 at 0.899
    res, fl = rr.select(pose, best, flags, cand, q)
    assert res.tolist() == [0, 0, 1, 2, 100, 1000, 3, 899] and fl == 0
    best[3, 3] = 900
    res, fl = rr.select(pose, best, flags, cand, q)
    assert res.tolist()[5:] == [1000, 3, 900] and fl == rr.AMBIGUOUS
    pose[1, 2] = 6.2831 - 0.09   # dt = 0.1002 > dup_rad: rank 1 becomes the rival
    res, fl = rr.select(pose, best, flags, cand, q)
    assert res.tolist()[5:] == [1000, 1, 990] and fl == rr.AMBIGUOUS
    best[1, 3] = 1000            # a tie in the fine score: the lower rank wins, the other is its rival
    res, fl = rr.select(pose, best, flags, cand, q)
    assert res.tolist()[0] == 0 and res.tolist()[5:] == [1000, 1, 1000]
    res, fl = rr.select(pose, best, np.full(5, mmr.EMPTY, np.int32), cand, q)
    assert res.tolist() == [-1, -1, -1, -1, 0, 0, -1, 0] and fl == rr.LOST
    one = np.array([mmr.WEAK, mmr.BAD_POSE, 0, mmr.EMPTY, mmr.WEAK], np.int32)
    res, fl = rr.select(pose, best, one, cand, q)   # a single eligible rank has no rival
    assert res.tolist() == [2, 2, 3, 4, 98, 800, -1, 0] and fl == 0
    res, fl = rr.select(pose, best, flags, cand, dict(q, ambig_permille=0))  # any rival is an ambiguity
    assert fl == rr.AMBIGUOUS


SMALL = dict(cell=100.0, grid_w=32, factor=4, n_head=4, head_step=np.pi / 2, n_cand=3, win_w=16, k_trans=4, k_theta=4,
             theta_step=np.pi / 16, smear=0, min_permille=300)


def test_lost_on_an_empty_map_and_on_zero_points():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-800.0, 800.0, (30, 2))
    L = np.where(rng.random((32, 32)) < 0.2, 100, -41).astype(np.int16)
    keep = np.array([7.0, 8.0, 9.0])
    for Lm, xy in ((np.full((32, 32), 84, np.int16), pts), (L, np.zeros((0, 2))), (L, np.full((5, 2), np.nan))):
        res = rr.relocalize(Lm, (0.0, 0.0), xy, pose_in=keep, P_in=np.arange(9.0), **SMALL)
        assert res["flags"] == rr.LOST and res["result"].tolist() == [-1, -1, -1, -1, 0, 0, -1, 0]
        assert not res["coarse_scores"].any() and np.all(res["cand"] == [-1, -1, -1, 0])
        assert np.all(res["fine_flags"] == mmr.BAD_POSE) and np.all(np.isnan(res["fine_pose"]))
        assert np.array_equal(res["pose_out"], keep) and np.array_equal(res["P_out"], np.arange(9.0))
    res = rr.relocalize(L, (0.0, 0.0), pts, **SMALL)  # (the same map with points: something is found or refused)
    assert res["n_occ"] > 0 and res["n_used"] == 30 and res["coarse_scores"].any() and res["cand"][0, 3] > 0


# ---- ABI, no device ----

def test_reloc_params_default():
    p = _lib.reloc_params()
    got = {k: getattr(p, k) for k in rr.DEFAULTS}
    assert got == dict(head_step=2 * np.pi / 180, n_head=180, factor=4, n_cand=8, ambig_permille=900, dup_mm=100.0,
                       dup_rad=0.0873, reset_sigma_xy=50.0, reset_sigma_theta=0.05)
    assert got == rr.DEFAULTS
    assert (_lib.RELOC_LOST, _lib.RELOC_AMBIGUOUS) == (rr.LOST, rr.AMBIGUOUS) == (1, 2)
    assert _lib.K_RELOC == 13 and _lib.ABI_VERSION == 6


def test_reloc_struct_sizes():
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_reloc_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.RelocParams) == 56
    assert got[1] == C.sizeof(_lib.RelocBatch) == 176
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_reloc_abi_sizes(one, 1) == 2 and list(one) == [56, -1]
    assert L.lslam_reloc_abi_sizes(None, 2) == 2
    two, nine = (C.c_int64 * 2)(), (C.c_int64 * 9)()  # the earlier tables are as they were
    assert L.lslam_grid_abi_sizes(two, 2) == 2 and list(two) == [40, 72]
    assert L.lslam_mapmatch_abi_sizes(two, 2) == 2 and list(two) == [32, 112]
    assert L.lslam_mapfuse_abi_sizes(two, 2) == 2 and list(two) == [24, 160]
    assert L.lslam_abi_sizes(nine, 9) == 9 and list(nine) == [112, 56, 56, 128, 232, 48, 48, 32, 96]


def call(b, g, m, q):
    L = _lib.load()
    ref = lambda s: None if s is None else C.byref(s)
    st = L.lslam_map_relocalize(None, ref(b), ref(g), ref(m), ref(q))
    return st, L.lslam_last_error()


BAD_FIELDS = [("head_step", 0.0), ("head_step", -1.0), ("head_step", float("nan")), ("head_step", float("inf")),
              ("n_head", 3), ("n_head", 1025), ("factor", 1), ("factor", 3), ("factor", 16), ("n_cand", 0), ("n_cand", 17),
              ("ambig_permille", -1), ("ambig_permille", 1001), ("dup_mm", -1.0), ("dup_mm", float("nan")),
              ("dup_rad", -0.1), ("reset_sigma_xy", 0.0), ("reset_sigma_xy", float("inf")), ("reset_sigma_theta", -1.0),
              ("reset_sigma_theta", float("nan"))]


@pytest.mark.parametrize("field,value", BAD_FIELDS)
def test_reloc_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    b = _lib.RelocBatch()
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params())
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg  # valid parameters, an empty batch: only the context is missing
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params(**{field: value}))
    assert st == _lib.LSLAM_ERR_ARG and field.encode() in msg


def test_reloc_factor_and_grid_width():
    b, m = _lib.RelocBatch(), _lib.mapmatch_params()
    for gw, f, ok in ((2048, 8, True), (2048, 4, False), (20, 2, True), (20, 8, False), (16, 4, True), (16, 8, False),
                      (36, 8, False), (512, 2, True)):
        st, msg = call(b, _lib.grid_params(grid_w=gw), m, _lib.reloc_params(factor=f))
        assert st == _lib.LSLAM_ERR_ARG and ((b"ctx" in msg) if ok else (b"factor" in msg and b"grid_w" in msg)), (gw, f)


def test_reloc_fine_window_must_cover_a_coarse_quantum():
    b, g = _lib.RelocBatch(), _lib.grid_params()
    for mkw, qkw, word in ((dict(k_trans=1), dict(), b"k_trans"), (dict(k_trans=3), dict(factor=8), b"k_trans"),
                           (dict(k_theta=1), dict(), b"k_theta"), (dict(), dict(head_step=0.4, n_head=16), b"k_theta"),
                           (dict(k_theta=0), dict(), b"k_theta")):
        st, msg = call(b, g, _lib.mapmatch_params(**mkw), _lib.reloc_params(**qkw))
        assert st == _lib.LSLAM_ERR_ARG and word in msg, (mkw, qkw, msg)
    for mkw, qkw in ((dict(k_trans=2), dict()), (dict(k_trans=4), dict(factor=8)), (dict(k_theta=2), dict()),
                     (dict(k_trans=1, k_theta=31, theta_step=0.1), dict(factor=2, head_step=6.2, n_head=4))):
        st, msg = call(b, g, _lib.mapmatch_params(**mkw), _lib.reloc_params(**qkw))
        assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg, (mkw, qkw, msg)


def test_reloc_checks_the_other_params_as_the_matcher_does():
    b = _lib.RelocBatch()
    st, msg = call(b, _lib.grid_params(cell=0.0), _lib.mapmatch_params(), _lib.reloc_params())
    assert st == _lib.LSLAM_ERR_ARG and b"cell" in msg
    st, msg = call(b, _lib.grid_params(), _lib.mapmatch_params(win_w=15), _lib.reloc_params())
    assert st == _lib.LSLAM_ERR_ARG and b"win_w" in msg


INPUTS = ("xy", "pt_off", "origin", "logodds", "rot", "head_rot")
OUTPUTS = ("n_occ", "n_used", "cand", "cand_pose", "fine_pose", "fine_delta", "fine_best", "fine_nvalid", "fine_rot0",
           "fine_flags", "result", "flags", "pose_out")


def test_reloc_missing_pointers():
    g, m, q = _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params()

    def batch(without=None):
        b = _lib.RelocBatch()
        b.n_robots = 1
        for f in INPUTS + OUTPUTS:
            if f != without:
                setattr(b, f, 4096)
        return b

    for f in INPUTS:
        st, msg = call(batch(f), g, m, q)
        assert st == _lib.LSLAM_ERR_ARG and b"missing input" in msg and f.encode() in msg, f
    for f in OUTPUTS:
        st, msg = call(batch(f), g, m, q)
        assert st == _lib.LSLAM_ERR_ARG and b"missing output" in msg and f.encode() in msg, f
    st, msg = call(batch(), g, m, q)  # P_out and coarse_scores are optional: only the context is missing
    assert st == _lib.LSLAM_ERR_ARG and b"ctx" in msg
    b = batch()
    b.n_robots = -1
    assert call(b, g, m, q)[0] == _lib.LSLAM_ERR_ARG
    for args in ((None, g, m, q), (batch(), None, m, q), (batch(), g, None, q), (batch(), g, m, None)):
        assert call(*args)[0] == _lib.LSLAM_ERR_ARG
