"""Relocalisation with priors (include/lidarslam.h, lslam_map_relocalize_prior) on the CPU: the NumPy
reference tests/relocprior_ref.py against reloc_ref where no prior is given, a hand-made case for each
rule of the admissible set, the two room scenes of test_reloc_ref.py, and the ABI checks that need no
device.  tests/test_gpu_relocprior.py holds the kernels to the reference bit for bit.

The rooms' maps here are the maps a robot would have drawn: test_reloc_ref's walls and free space, with
the cells outside the outline unknown (0) as a grid that was never seen there holds them.  The occupied
cells are the same, so lslam_map_relocalize's results are those of test_reloc_ref.  The free-space field
is lslam_grid_distance's NOT_FREE field of that map at its defaults (free_max -1, d_max 64).

Free-space value, L-shaped room, eight poses, defaults (clear_min2 16).  Measured with this reference:
1620 of 16384 coarse cells are admissible; the plain call's eight candidates include one in an
inadmissible cell for poses 0 and 6 (rank 6 both times); the prior call has none, finds all eight poses
within the plain call's caps, and the true poses' clear2 is 484 at least.

Window value, plain room (AMBIGUOUS to the plain call): a window of +-1000 mm and +-0.5 rad around a
pose 600 mm and 0.3 rad off the truth leaves 625 cells and 28 or 29 headings of the 16384 and 180; both
poses are found, with no rival at 0.9 of the winner.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dist_ref as dr
import mapmatch_ref as mmr
import reloc_ref as rr
import relocprior_ref as rp
from lidar_slam_amd import _lib
from test_reloc_ref import (CAP_MM, CAP_RAD, L_OUTLINE, L_POSES, RECT_OUTLINE, RECT_POSES, SCENE_ORIGIN, SMALL, pose_error,
                            scene, scene_case)

WINDOW_OFF = np.array([360.0, 480.0, 0.3])  # 600 mm and 0.3 rad


def inside_outline(outline, grid_w=512, cell=20.0, origin=SCENE_ORIGIN):
    """bool [grid_w][grid_w]: the cell's centre lies inside the outline (even-odd rule)."""
    c = (np.arange(grid_w) + 0.5) * cell
    X, Y = origin[0] + c[None, :], origin[1] + c[:, None]
    pts = np.array(outline)
    ins = np.zeros((grid_w, grid_w), bool)
    for a, b in zip(pts, np.roll(pts, -1, axis=0)):
        if a[1] == b[1]:
            continue
        xi = a[0] + (Y - a[1]) * (b[0] - a[0]) / (b[1] - a[1])
        ins ^= ((a[1] > Y) != (b[1] > Y)) & (X < xi)
    return ins


@functools.lru_cache(maxsize=None)
def seen_scene(which):
    """(map with unknown space outside the room, its NOT_FREE field, poses, revolutions)."""
    L, poses, revs = scene(which)
    ins = inside_outline(L_OUTLINE if which == "L" else RECT_OUTLINE)
    Ls = np.where((L < 85) & ~ins, 0, L).astype(np.int16)
    assert np.array_equal(Ls >= 85, L >= 85)
    return Ls, dr.field(Ls, mode=dr.NOT_FREE)[0], poses, revs


@functools.lru_cache(maxsize=None)
def prior_case(which, i, field, window):
    Ls, d2, poses, revs = seen_scene(which)
    return rp.relocalize(Ls, SCENE_ORIGIN, revs[i], clear_d2=d2 if field else None,
                         win_pose=poses[i] + WINDOW_OFF if window else None)


def same(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), k


# ---- no prior ----

def test_null_priors_are_the_plain_call():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-800.0, 800.0, (30, 2))
    L = np.where(rng.random((32, 32)) < 0.2, 100, -41).astype(np.int16)
    plain = rr.relocalize(L, (0.0, 0.0), pts, pose_in=[1.0, 2.0, 3.0], **SMALL)
    prior = rp.relocalize(L, (0.0, 0.0), pts, pose_in=[1.0, 2.0, 3.0], **SMALL)
    same(prior, plain, plain.keys())
    assert prior["n_admit"].tolist() == [64, 4] and not prior["fine_clear2"].any() and prior["admissible"].all()
    assert plain["cand"][0, 3] > 0
    # the room, one pose: every key of the plain call
    Ls, _, _, revs = seen_scene("L")
    same(rp.relocalize(Ls, SCENE_ORIGIN, revs[3]), scene_case("L", 3), scene_case("L", 3).keys())


# ---- a hand-made case per rule ----

@pytest.mark.parametrize("f", [2, 4, 8])
def test_field_block_rule(f):
    """Af: one fine cell of the block at clear_min2 admits the coarse cell, one below does not."""
    Wc = 5
    gw = Wc * f
    d2 = np.zeros((gw, gw), np.uint16)
    d2[0, 0] = 16                       # the block's first cell
    d2[2 * f - 1, 3 * f - 1] = 17       # the last cell of block (1, 2)
    d2[3 * f, 4 * f] = 15               # below: not admissible
    d2[gw - 1, gw - 1] = 65025          # the grid's last cell
    Af = rp.field_admissible(d2, gw, f, 16)
    assert np.argwhere(Af).tolist() == [[0, 0], [1, 2], [Wc - 1, Wc - 1]]
    assert rp.field_admissible(d2, gw, f, 0).all()                         # 0: every cell passes
    assert np.argwhere(rp.field_admissible(d2, gw, f, 65025)).tolist() == [[Wc - 1, Wc - 1]]
    assert rp.field_admissible(None, gw, f, 65025).all()


def test_window_box():
    """Aw: cell centres at 200, 600, .. mm (cellc 400, origin 0): <= is inclusive, the box may leave the grid."""
    Wc, cellc, o = 8, 400.0, (0.0, 0.0)
    Aw = rp.window_admissible([600.0, 1400.0, 0.0], o, Wc, cellc, 400.0)  # the edges fall on centres
    assert np.argwhere(Aw.any(0)).ravel().tolist() == [0, 1, 2] and np.argwhere(Aw.any(1)).ravel().tolist() == [2, 3, 4]
    assert Aw.sum() == 9
    Aw = rp.window_admissible([600.0, 1400.0, 0.0], o, Wc, cellc, np.nextafter(400.0, 0.0))
    assert np.argwhere(Aw).tolist() == [[3, 1]]
    assert rp.window_admissible([600.0, 1400.0, 0.0], o, Wc, cellc, 0.0).sum() == 1      # the centre itself
    assert rp.window_admissible([601.0, 1400.0, 0.0], o, Wc, cellc, 0.0).sum() == 0
    Aw = rp.window_admissible([-300.0, 3100.0, 0.0], o, Wc, cellc, 600.0)  # partly off the grid: x <= 300, y >= 2500
    assert np.argwhere(Aw).tolist() == [[6, 0], [7, 0]]
    assert not rp.window_admissible([-5000.0, 200.0, 0.0], o, Wc, cellc, 600.0).any()    # wholly off
    assert rp.window_admissible([1.0, 2.0, 0.0], o, Wc, cellc, np.inf).all()
    assert rp.window_admissible(None, o, Wc, cellc, 0.0).all()
    for bad in ([np.nan, 200.0, 0.0], [200.0, np.nan, 0.0]):
        assert not rp.window_admissible(bad, o, Wc, cellc, np.inf).any()
    # an origin that is no multiple of the cell: the expression is cand_pose's
    cand_x = -1234.5 + (np.arange(Wc) + 0.5) * cellc
    Aw = rp.window_admissible([cand_x[5], 0.0, 0.0], (-1234.5, -200.0), Wc, cellc, 0.0)
    assert np.argwhere(Aw).tolist() == [[0, 5]]


def test_heading_window():
    step = 2.0 * np.pi / 180
    H = rp.heading_admissible([0.0, 0.0, 0.01], 180, step, 0.1)  # wraps across k = 0
    assert np.nonzero(H)[0].tolist() == [0, 1, 2, 3, 178, 179]
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, 10 * step], 180, step, 0.0))[0].tolist() == [10]  # one heading
    assert not rp.heading_admissible([0.0, 0.0, 0.01], 180, step, 0.0).any()
    assert rp.heading_admissible([0.0, 0.0, 0.01], 180, step, np.inf).all()
    assert rp.heading_admissible(None, 180, step, 0.0).all()
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, 0.01 + 4 * np.pi], 180, step, 0.1))[0].tolist() == [0, 1, 2, 3, 178, 179]
    for bad in (np.nan, np.inf, -np.inf):
        assert not rp.heading_admissible([0.0, 0.0, bad], 180, step, np.inf).any()
    # k head_step - theta = +pi and -pi exactly: the remainder is +-pi (the tie goes to the even quotient, 0)
    q = np.pi / 2
    assert 2.0 * q == rr.PI and 2.0 * rr.PI == rp.TWO_PI
    assert math.remainder(rr.PI, rp.TWO_PI) == rr.PI and math.remainder(-rr.PI, rp.TWO_PI) == -rr.PI
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, 0.0], 4, q, rr.PI))[0].tolist() == [0, 1, 2, 3]
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, 0.0], 4, q, np.nextafter(rr.PI, 0.0)))[0].tolist() == [0, 1, 3]
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, rp.TWO_PI], 4, q, np.nextafter(rr.PI, 0.0)))[0].tolist() == [0, 1, 3]
    assert np.nonzero(rp.heading_admissible([0.0, 0.0, rp.TWO_PI], 4, q, rr.PI))[0].tolist() == [0, 1, 2, 3]


def small_case():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-800.0, 800.0, (30, 2))
    L = np.where(rng.random((32, 32)) < 0.2, 100, -41).astype(np.int16)
    return L, pts


def test_masked_volume_counts_and_candidates():
    """Step 2': the volume is the plain one under the set, the candidates are its peaks, n_admit counts."""
    L, pts = small_case()
    plain = rr.relocalize(L, (0.0, 0.0), pts, **SMALL)
    d2 = np.zeros((32, 32), np.uint16)
    d2[4:20, 8:30] = 40
    win = [1700.0, 1500.0, np.pi / 2 + 0.2]
    res = rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, win_pose=win, half_xy=900.0, half_theta=1.0, clear_min2=40, **SMALL)
    adm = res["admissible"]
    # cells: Af rows 1..4, columns 2..7; the box 800..2600 x 600..2400 holds centres 1000 .. 2600 (tx 2..6), 600 .. 2200 (ty 1..5)
    assert np.argwhere(adm.any(0)).tolist() == [[ty, tx] for ty in range(1, 5) for tx in range(2, 7)]
    assert np.nonzero(adm.any((1, 2)))[0].tolist() == [1] and res["n_admit"].tolist() == [20, 1]
    assert np.array_equal(res["coarse_scores"], np.where(adm, plain["coarse_scores"], 0)) and res["coarse_scores"].any()
    assert all(adm[k, ty, tx] for k, ty, tx, s in res["cand"] if k >= 0) and res["cand"][0, 3] > 0
    assert list(rr.peaks(res["coarse_scores"], 3)) == [(k * 8 + ty) * 8 + tx for k, ty, tx, s in res["cand"] if k >= 0]


@pytest.mark.parametrize("win", [[np.nan, 100.0, 0.0], [100.0, 100.0, np.nan], [-9000.0, 0.0, 0.0]])
def test_nothing_admissible_is_lost(win):
    L, pts = small_case()
    keep = np.array([7.0, 8.0, 9.0])
    res = rp.relocalize(L, (0.0, 0.0), pts, win_pose=win, pose_in=keep, P_in=np.arange(9.0), **SMALL)
    assert res["flags"] == rr.LOST and res["result"].tolist() == [-1, -1, -1, -1, 0, 0, -1, 0]
    assert not res["coarse_scores"].any() and np.all(res["cand"] == [-1, -1, -1, 0]) and 0 in res["n_admit"].tolist()
    assert np.all(res["fine_flags"] == mmr.BAD_POSE) and not res["fine_clear2"].any()  # (no field: zeros)
    assert np.array_equal(res["pose_out"], keep) and np.array_equal(res["P_out"], np.arange(9.0))
    assert res["n_occ"] > 0 and res["n_used"] == 30  # steps 0 and 1 are the plain call's


def test_clear_min2_extremes():
    L, pts = small_case()
    plain = rr.relocalize(L, (0.0, 0.0), pts, **SMALL)
    d2 = np.full((32, 32), 65024, np.uint16)
    zero = rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, clear_min2=0, **SMALL)
    same(zero, plain, plain.keys())
    assert zero["n_admit"].tolist() == [64, 4]
    top = rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, clear_min2=65025, **SMALL)
    assert top["flags"] == rr.LOST and top["n_admit"].tolist() == [0, 4] and np.all(top["fine_clear2"] == -1)
    d2[:] = 65025
    same(rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, clear_min2=65025, **SMALL), plain, plain.keys())


def test_fine_clearance_rejects_a_rank():
    """Step 5': the coarse cell is admissible by another of its fine cells, the refined pose stands on a
    cell without clearance: the rank is reported and not eligible."""
    L, pts = small_case()
    kw = dict(SMALL, min_permille=0)  # (no gate of the matcher's: every rank with a pose is eligible)
    d2 = np.full((32, 32), 100, np.uint16)
    first = rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, **kw)
    assert first["flags"] in (0, rr.AMBIGUOUS) and np.all(first["fine_clear2"][first["cand"][:, 0] >= 0] == 100)
    w = int(first["result"][0])
    X0, Y0 = (int(np.floor(first["fine_pose"][w][i] / 100.0)) for i in (0, 1))
    d2[Y0, X0] = 15
    res = rp.relocalize(L, (0.0, 0.0), pts, clear_d2=d2, **kw)
    same(res, first, ("coarse_scores", "cand", "fine_pose", "fine_best", "fine_flags"))  # the block stays admissible
    assert res["fine_clear2"][w] == 15 and res["result"][0] != w and res["result"][6] != w
    others = [j for j in range(3) if j != w and first["cand"][j, 0] >= 0 and res["fine_clear2"][j] >= 16]
    assert (res["flags"] == rr.LOST) == (not others)
    if others:
        assert res["result"][0] == min(others, key=lambda j: (-int(res["fine_best"][j][3]), j))
    # off the map: a pose left of the grid reads -1
    assert rp.fine_clear(d2, np.array([[-1.0, 50.0, 0.0], [50.0, 3200.0, 0.0], [np.nan, 0.0, 0.0], [3199.0, 0.0, 0.0]]),
                         np.zeros(2), 32, 100.0).tolist() == [-1, -1, -1, 100]


# ---- the rooms ----

def test_plain_call_refines_inadmissible_candidates():
    """The premise of the free-space prior, on the reference: the plain call spends refinement slots on
    coarse cells where no robot can stand."""
    _, d2, poses, _ = seen_scene("L")
    Af = rp.field_admissible(d2, 512, 4, rp.DEFAULTS["clear_min2"])
    print("admissible coarse cells", int(Af.sum()), "of", Af.size)
    spent = {i: [j for j, (k, ty, tx, s) in enumerate(scene_case("L", i)["cand"]) if k >= 0 and not Af[ty, tx]]
             for i in range(len(poses))}
    print("ranks in inadmissible cells, per pose:", spent)
    assert any(spent.values())
    # the true poses stand in free space at the default
    for which in ("L", "rect"):
        _, f2, ps, _ = seen_scene(which)
        cells = np.floor((ps[:, :2] - np.array(SCENE_ORIGIN)) / 20.0).astype(int)
        clear = f2[cells[:, 1], cells[:, 0]]
        print(which, "clear2 of the true poses", clear.tolist())
        assert np.all(clear >= rp.DEFAULTS["clear_min2"])


@pytest.mark.parametrize("i", range(len(L_POSES)))
def test_free_space_prior_in_the_l_room(i):
    plain, res = scene_case("L", i), prior_case("L", i, True, False)
    adm = res["admissible"]
    assert all(adm[k, ty, tx] for k, ty, tx, s in res["cand"] if k >= 0) and np.all(res["cand"][:, 0] >= 0)
    assert np.array_equal(res["coarse_scores"], np.where(adm, plain["coarse_scores"], 0))
    dpos, dth = pose_error(res["pose_out"], L_POSES[i])
    print("pose", i, "n_admit", res["n_admit"].tolist(), "result", res["result"].tolist(), "fine_clear2", res["fine_clear2"].tolist(),
          "error", dpos, "mm", dth, "rad")
    assert plain["flags"] == 0 and res["flags"] == 0  # every robot the plain call finds
    assert dpos <= CAP_MM and dth <= CAP_RAD
    assert res["fine_clear2"][res["result"][0]] >= rp.DEFAULTS["clear_min2"] and res["n_admit"].tolist() == [int(adm[0].sum()), 180]


@pytest.mark.parametrize("i", range(len(RECT_POSES)))
def test_window_resolves_the_half_turn(i):
    plain, res = scene_case("rect", i), prior_case("rect", i, False, True)
    assert plain["flags"] == rr.AMBIGUOUS
    dpos, dth = pose_error(res["pose_out"], RECT_POSES[i])
    sw, sr = int(res["result"][5]), int(res["result"][7])
    print("pose", i, "n_admit", res["n_admit"].tolist(), "result", res["result"].tolist(), "error", dpos, "mm", dth, "rad")
    assert res["flags"] == 0 and 1000 * sr < 900 * sw
    assert dpos <= CAP_MM and dth <= CAP_RAD
    # 2000 mm hold 25 or 26 centres of 80 mm cells a side, 1 rad holds 28 or 29 headings of 2 degrees
    assert res["n_admit"][0] in (625, 650, 676) and res["n_admit"][1] in (28, 29)
    both = prior_case("rect", i, True, True)  # with the field as well: the same pose
    assert both["flags"] == 0 and np.array_equal(both["pose_out"], res["pose_out"]) and both["n_admit"][0] <= res["n_admit"][0]


# ---- ABI, no device ----

def test_relocprior_params_default_and_sizes():
    p = _lib.relocprior_params()
    assert {k: getattr(p, k) for k in rp.DEFAULTS} == rp.DEFAULTS == dict(half_xy=1000.0, half_theta=0.5, clear_min2=16)
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_relocprior_abi_sizes(got, 2) == 2
    assert got[0] == C.sizeof(_lib.RelocPriorParams) == 24
    assert got[1] == C.sizeof(_lib.RelocPriorBatch) == 208
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_relocprior_abi_sizes(one, 1) == 2 and list(one) == [24, -1]
    assert L.lslam_relocprior_abi_sizes(None, 2) == 2
    assert L.lslam_reloc_abi_sizes(got, 2) == 2 and list(got) == [56, 176]  # the embedded batch is as it was
    assert _lib.ABI_VERSION == 6 and _lib.RelocPriorBatch.r.offset == 0 and _lib.RelocPriorBatch.clear_d2.offset == 176
    assert L.lslam_relocprior_params_default(None) == _lib.LSLAM_ERR_ARG


def call(b, g, m, q, pp):
    L = _lib.load()
    ref = lambda s: None if s is None else C.byref(s)
    st = L.lslam_map_relocalize_prior(None, ref(b), ref(g), ref(m), ref(q), ref(pp))
    return st, L.lslam_last_error()


@pytest.mark.parametrize("field,value", [("half_xy", -1.0), ("half_xy", float("nan")), ("half_theta", -0.1),
                                         ("half_theta", float("nan")), ("clear_min2", -1), ("clear_min2", 65026)])
def test_relocprior_validation_needs_no_device(field, value):
    b, g, m, q = _lib.RelocPriorBatch(), _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params()
    for ok in (dict(), dict(half_xy=float("inf"), half_theta=float("inf")), dict(half_xy=0.0, half_theta=0.0, clear_min2=0),
               dict(clear_min2=65025)):
        st, msg = call(b, g, m, q, _lib.relocprior_params(**ok))
        assert st == _lib.LSLAM_ERR_ARG and msg == b"relocprior: ctx is NULL", ok
    st, msg = call(b, g, m, q, _lib.relocprior_params(**{field: value}))
    assert st == _lib.LSLAM_ERR_ARG and msg.startswith(b"relocprior: " + field.encode())


def test_relocprior_checks_the_other_params_as_the_plain_call_does():
    b, g, m, q, pp = _lib.RelocPriorBatch(), _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params(), _lib.relocprior_params()
    assert b"cell" in call(b, _lib.grid_params(cell=0.0), m, q, pp)[1]
    assert b"win_w" in call(b, g, _lib.mapmatch_params(win_w=15), q, pp)[1]
    assert b"n_cand" in call(b, g, m, _lib.reloc_params(n_cand=17), pp)[1]
    assert b"k_trans" in call(b, g, _lib.mapmatch_params(k_trans=1), q, pp)[1]
    assert call(b, g, m, q, None)[1] == b"relocprior: params is NULL"
    for args in ((None, g, m, q, pp), (b, None, m, q, pp), (b, g, None, q, pp), (b, g, m, None, pp)):
        assert call(*args)[0] == _lib.LSLAM_ERR_ARG
    assert call(None, g, m, q, pp)[1] == b"relocprior: batch is NULL"


INPUTS = ("xy", "pt_off", "origin", "logodds", "rot", "head_rot")
OUTPUTS = ("n_occ", "n_used", "cand", "cand_pose", "fine_pose", "fine_delta", "fine_best", "fine_nvalid", "fine_rot0",
           "fine_flags", "result", "flags", "pose_out")
OWN_OUTPUTS = ("n_admit", "fine_clear2")


def full_batch(n=1):
    """Every pointer a dummy address of its own, 4 GiB apart (nothing is dereferenced without a context)."""
    b = _lib.RelocPriorBatch()
    b.r.n_robots = n
    for i, f in enumerate(INPUTS + OUTPUTS + ("P_out", "coarse_scores")):
        setattr(b.r, f, (i + 1) << 32)
    for i, f in enumerate(OWN_OUTPUTS + ("clear_d2", "win_pose")):
        setattr(b, f, (i + 40) << 32)
    return b


def test_relocprior_missing_pointers():
    g, m, q, pp = _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params(), _lib.relocprior_params()
    missing_in = b"relocprior: missing input (xy, pt_off, origin, logodds, rot, head_rot)"
    missing_out = (b"relocprior: missing output (n_occ, n_used, cand, cand_pose, fine_pose, fine_delta, fine_best, "
                   b"fine_nvalid, fine_rot0, fine_flags, result, flags, pose_out, n_admit, fine_clear2)")
    for f in INPUTS + OUTPUTS:
        b = full_batch()
        setattr(b.r, f, None)
        assert call(b, g, m, q, pp) == (_lib.LSLAM_ERR_ARG, missing_in if f in INPUTS else missing_out), f
    for f in OWN_OUTPUTS:
        b = full_batch()
        setattr(b, f, None)
        assert call(b, g, m, q, pp) == (_lib.LSLAM_ERR_ARG, missing_out), f
    for owner, f in (("r", "P_out"), ("r", "coarse_scores"), (None, "clear_d2"), (None, "win_pose")):  # optional
        b = full_batch()
        setattr(getattr(b, owner) if owner else b, f, None)
        assert call(b, g, m, q, pp)[1] == b"relocprior: ctx is NULL", f
    assert call(full_batch(-1), g, m, q, pp)[1] == b"relocprior: negative n_robots"
    assert call(_lib.RelocPriorBatch(), g, m, q, pp)[1] == b"relocprior: ctx is NULL"  # an empty batch needs no pointer


def test_relocprior_field_must_not_overlap_an_output():
    g, m, q, pp = _lib.grid_params(), _lib.mapmatch_params(), _lib.reloc_params(), _lib.relocprior_params()
    field_bytes = 512 * 512 * 2
    for owner, f in [("r", n) for n in OUTPUTS + ("P_out", "coarse_scores")] + [(None, n) for n in OWN_OUTPUTS]:
        b = full_batch()
        setattr(getattr(b, owner) if owner else b, f, b.clear_d2 + field_bytes - 4)  # the output begins in the field's last bytes
        assert call(b, g, m, q, pp) == (_lib.LSLAM_ERR_ARG, b"relocprior: clear_d2 overlaps an output"), f
        setattr(getattr(b, owner) if owner else b, f, b.clear_d2 + field_bytes)      # right behind it: no overlap
        assert call(b, g, m, q, pp)[1] == b"relocprior: ctx is NULL", f
    b = full_batch()
    b.r.logodds = b.clear_d2  # (an input may: the call only reads both)
    assert call(b, g, m, q, pp)[1] == b"relocprior: ctx is NULL"
