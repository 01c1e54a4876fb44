"""The NumPy form of lslam_pose_graph_gate (tests/posegate_ref.py) against what it must mean: the statistic and the
covariance against a dense np.linalg form, true closures accepted and false ones rejected on the circle loops,
the calibration of d2, its independence of z and of a rigid motion, the appended graph's solve, every flag.  CPU
only; the reference alone (the kernel is held to it bit for bit in tests/test_gpu_posegate.py, the core header in
tests/test_posegate_core.py).

Figures measured here (printed by the tests), on posegraph_ref.circle_loop(N, seed) with default parameters, the
trusted graph its N - 1 odometry edges at ``init``, seeds 1000 + N, 1001 + N, 1002 + N:
  d2 and cov against np.linalg, worst relative difference of either over the table's 45 cases: 1.3e-13
  (N = 4: 2.0e-15, N = 24: 2.5e-14, N = 48: 1.3e-13); DENSE_BOUND is ten times that.
  d2 (smallest - largest over the seeds):
    N   true N-1->0   same, x + 500 mm   N/2->0 x + 500 mm, odometry's weight   true N/2->0   N-1->0, heading + 0.3
    4   0.16 - 0.47   589 - 595          606 - 619                              0.12 - 0.70   466 - 476
    24  2.2 - 3.5     84 - 94            143 - 151                              2.3 - 3.0     76 - 82
    48  8.0 - 9.8     54 - 61            75 - 78                                5.2 - 7.1     58 - 64
  the strong false closure of circle_loop(N, false_closure=500.0) (5 mm, 0.005 rad): d2 589, 84, 54 at N = 4, 24,
  48 (seed 1000 + N), OUTLIER, while after a solve that was given it its edge_chi2 (34.7, 0.9, 0.2) is below the
  largest odometry edge's (209.4, 4.9, 1.7).
  calibration, 200 draws of circle_loop(N, seed, bias=0, noise=(10, 0.01)) with the closure's z perturbed by
  N(0, (5, 5, 0.005)): mean d2 3.02, 2.87, 3.33 at N = 4, 24, 48 (3 for a calibrated 3-dof statistic); 0.5 %, 0 %
  and 0.5 % of the draws above 16.27."""
import math

import numpy as np
import pytest

import posegate_ref as gr
import posegraph_ref as pg
from lidar_slam_amd import posegraph

LOOPS = (4, 24, 48)
DENSE_BOUND = 1.3e-12  # ten times the worst relative difference measured (the docstring)
NIS_MAX = 16.27
assert hasattr(posegraph.PoseGraph, "gate")  # (the feature's module: the reference tests belong to it)


def table_cases(N, seed):
    """The trusted graph (the odometry at init) and the table's five candidates: (init, ij, z, info, cij, cz, cinfo,
    truth of each candidate: True for a true closure)."""
    truth, init, ij, z, info = pg.circle_loop(N, seed)
    half = pg.relative_pose(truth[N // 2], truth[0])
    zf, hf, zr = z[-1].copy(), half.copy(), z[-1].copy()
    zf[0] += 500.0
    hf[0] += 500.0
    zr[2] += 0.3
    cij = np.array([[N - 1, 0], [N - 1, 0], [N // 2, 0], [N // 2, 0], [N - 1, 0]])
    cz = np.array([z[-1], zf, hf, half, zr])
    cinfo = np.array([info[-1], info[-1], info[0], info[-1], info[-1]])
    return init, ij[:-1], z[:-1], info[:-1], cij, cz, cinfo, (True, False, False, True, False)


def test_d2_and_cov_against_the_dense_form():
    worst = {}
    for N in LOOPS:
        w = 0.0
        for seed in (1000 + N, 1001 + N, 1002 + N):
            init, ij, z, info, cij, cz, cinfo, _ = table_cases(N, seed)
            r = gr.gate(init, ij, z, info, cij, cz, cinfo)
            assert r["flags"] == 0
            for c in range(len(cij)):
                d2, M = gr.dense(init, ij, z, info, cij[c, 0], cij[c, 1], cz[c], cinfo[c])
                cov = np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])
                w = max(w, abs(r["cand_nis"][c] - d2) / d2, float(np.abs(r["cand_cov"][c] - cov).max() / np.abs(cov).max()))
        print("N = %d: worst relative difference %.2e" % (N, w))
        worst[N] = w
    print("worst %.2e, bound %.2e" % (max(worst.values()), DENSE_BOUND))
    assert max(worst.values()) <= DENSE_BOUND


@pytest.mark.parametrize("N", LOOPS)
def test_the_table_true_closures_pass_and_false_ones_do_not(N):
    for seed in (1000 + N, 1001 + N, 1002 + N):
        init, ij, z, info, cij, cz, cinfo, true = table_cases(N, seed)
        r = gr.gate(init, ij, z, info, cij, cz, cinfo, nis_max=NIS_MAX)
        closed = pg.solve(init, np.vstack([ij, cij[:1]]), np.vstack([z, cz[:1]]), np.vstack([info, cinfo[:1]]), n_iter=0)
        print("N = %d seed %d: d2 %s, the true closure's edge chi %.0f" % (N, seed, np.round(r["cand_nis"], 2), closed["edge_chi2"][-1]))
        assert r["flags"] == 0
        for c, t in enumerate(true):
            assert r["cand_flags"][c] == (gr.ACCEPTED if t else gr.OUTLIER), (c, r["cand_nis"][c])
        # the issue's separation: every true closure below 16.27, every false one far above
        assert r["cand_nis"][[0, 3]].max() < 10.0 and r["cand_nis"][[1, 2, 4]].min() > 50.0


@pytest.mark.parametrize("N", LOOPS)
def test_the_strong_false_closure_is_an_outlier_although_its_edge_chi2_is_not_the_largest(N):
    """tests/test_posegraph_ref.py's limit case: the loop's one closure wrong by 500 mm at 5 mm, stronger than the
    odometry.  After a solve that was given it, its edge_chi2 is not the largest; the gate, asked before, rejects it."""
    _, init, ij, z, info = pg.circle_loop(N, seed=1000 + N, false_closure=500.0)
    solved = pg.solve(init, ij, z, info)
    ec = solved["edge_chi2"]
    assert not solved["flags"] & pg.REJECTED and int(np.argmax(ec)) != len(ij) - 1
    r = gr.gate(init, ij[:-1], z[:-1], info[:-1], ij[-1:], z[-1:], info[-1:], nis_max=NIS_MAX)
    print("N = %d: d2 %.1f; after a solve its edge_chi2 %.1f, the largest other %.1f" % (N, r["cand_nis"][0], ec[-1], ec[:-1].max()))
    assert r["flags"] == 0 and r["cand_flags"][0] == gr.OUTLIER and r["cand_nis"][0] > 50.0


def test_calibration_200_draws():
    for N in LOOPS:
        d2 = []
        for seed in range(200):
            truth, init, ij, z, info = pg.circle_loop(N, seed, bias=(0, 0, 0), noise=(10.0, 0.01))
            zc = z[-1] + np.random.default_rng(9000 + seed).normal(0.0, (5.0, 5.0, 0.005))
            r = gr.gate(init, ij[:-1], z[:-1], info[:-1], ij[-1:], zc[None], info[-1:])
            d2.append(r["cand_nis"][0])
        d2 = np.array(d2)
        print("N = %d: mean d2 %.2f, %.1f %% above %.2f" % (N, d2.mean(), 100.0 * (d2 > NIS_MAX).mean(), NIS_MAX))
        assert 2.0 <= d2.mean() <= 4.0


def test_cov_does_not_depend_on_z_bit_for_bit():
    init, ij, z, info, cij, cz, cinfo, _ = table_cases(24, 1024)
    a = gr.gate(init, ij, z, info, cij[:2], cz[:2], cinfo[:2])
    far = cz[:2] + [[1e4, -3e3, 2.5], [-7.0, 1e5, -3.0]]
    b = gr.gate(init, ij, z, info, cij[:2], far, cinfo[:2])
    assert np.array_equal(a["cand_cov"].view(np.uint64), b["cand_cov"].view(np.uint64)) and a["cand_cov"].any()
    assert not np.array_equal(a["cand_nis"], b["cand_nis"])
    # nor on Omega
    c = gr.gate(init, ij, z, info, cij[:2], cz[:2], 7.0 * cinfo[:2])
    assert np.array_equal(a["cand_cov"].view(np.uint64), c["cand_cov"].view(np.uint64))


@pytest.mark.parametrize("N", LOOPS)
def test_a_rigid_motion_of_the_graph_leaves_d2(N):
    init, ij, z, info, cij, cz, cinfo, _ = table_cases(N, 1000 + N)
    th, t = 0.7, np.array([-350.0, 1200.0])
    c, s = math.cos(th), math.sin(th)
    moved = np.concatenate([init[:, :2] @ np.array([[c, -s], [s, c]]).T + t, init[:, 2:] + th], 1)
    a, b = gr.gate(init, ij, z, info, cij, cz, cinfo), gr.gate(moved, ij, z, info, cij, cz, cinfo)
    rel = np.abs(b["cand_nis"] - a["cand_nis"]) / a["cand_nis"]
    print("N = %d: worst relative difference of d2 under a rigid motion %.2e" % (N, rel.max()))
    assert np.array_equal(a["cand_flags"], b["cand_flags"]) and rel.max() <= DENSE_BOUND


@pytest.mark.parametrize("N", LOOPS)
def test_the_appended_graph_solves_to_the_poses_of_the_true_closure_alone(N):
    init, ij, z, info, cij, cz, cinfo, true = table_cases(N, 1000 + N)
    pad = lambda a: np.concatenate([a, np.zeros((4,) + a.shape[1:], a.dtype)])  # noqa: E731
    r = gr.gate(init, pad(ij), pad(z), pad(info), cij, cz, cinfo, n_edges=N - 1, append=1)
    assert r["n_edges"] == N + 1 and [bool(f & gr.APPENDED) for f in r["cand_flags"]] == list(true)
    got = pg.solve(init, r["edge_ij"], r["edge_z"], r["edge_info"], n_edges=r["n_edges"])
    keep = [c for c, t in enumerate(true) if t]
    want = pg.solve(init, np.vstack([ij, cij[keep]]), np.vstack([z, cz[keep]]), np.vstack([info, cinfo[keep]]))
    assert got["flags"] == want["flags"] == pg.CONVERGED
    assert np.array_equal(got["pose_out"].view(np.uint64), want["pose_out"].view(np.uint64))


def unit_info(n):
    return np.tile([1e-2, 0.0, 0.0, 1e-2, 0.0, 1e2], (n, 1))


def test_every_flag():
    pose = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.1], [1000.0, 1000.0, 1.6], [5.0, 6.0, 7.0]])
    ij = np.array([[0, 1], [1, 2], [0, 0], [0, 0]])
    z = np.zeros((4, 3))
    z[:2] = pg.relative_pose(pose[ij[:2, 0]], pose[ij[:2, 1]]) + 3.0 * np.array([[1.0, -1.0, 0.001]])
    info = unit_info(4)
    cij = np.array([[2, 0], [2, 0]])
    cz = np.tile(pg.relative_pose(pose[2], pose[0]), (2, 1))
    cinfo = unit_info(2)
    kw = dict(n_nodes=3, n_edges=2, append=1)
    untouched = lambda r, E=2: (r["n_edges"] == E and not r["cand_flags"].any() and not r["cand_nis"].any()  # noqa: E731
                           and not r["cand_err"].any() and not r["cand_cov"].any())
    zero = lambda r, E=2: untouched(r, E) and not r["trace"].any() and r["chi2"] == 0.0  # noqa: E731
    good = gr.gate(pose, ij, z, info, cij, cz, cinfo, **kw)
    assert good["flags"] == 0 and (good["cand_flags"] == gr.ACCEPTED | gr.APPENDED).all() and good["n_edges"] == 4
    assert np.array_equal(good["cand_nis"][:1], good["cand_nis"][1:]) and good["chi2"] > 0  # two equal candidates
    assert np.array_equal(good["edge_ij"][2:], cij) and np.array_equal(good["edge_z"][2:], cz)
    # UNJUDGED under EMPTY, BAD_GRAPH and SINGULAR: zero outputs, nothing appended
    for over in (dict(n_nodes=1), dict(n_nodes=0, n_edges=0), dict(n_edges=0)):
        r = gr.gate(pose, ij, z, info, cij, cz, cinfo, **dict(kw, **over))
        assert r["flags"] == gr.EMPTY and zero(r, over.get("n_edges", 2)), over
    for over in (dict(n_nodes=5), dict(n_edges=5), dict(n_nodes=-1), dict(n_edges=-1), dict(n_cand=3), dict(n_cand=-1)):
        r = gr.gate(pose, ij, z, info, cij, cz, cinfo, **dict(kw, **over))
        assert r["flags"] == gr.BAD_GRAPH and zero(r, over.get("n_edges", 2)), over
    bad = ij.copy()
    bad[1] = [1, 3]
    assert gr.gate(pose, bad, z, info, cij, cz, cinfo, **kw)["flags"] == gr.BAD_GRAPH
    nanz = z.copy()
    nanz[0, 1] = np.nan
    assert zero(gr.gate(pose, ij, nanz, info, cij, cz, cinfo, **kw))
    r = gr.gate(pose, ij[:1], z[:1], info[:1], cij, cz, cinfo, n_nodes=3, max_edges=4, damp_t=0.0, damp_r=0.0, append=1)
    assert r["flags"] == gr.SINGULAR and r["n_edges"] == 1 and not r["cand_flags"].any() and not r["cand_nis"].any()
    assert r["chi2"] > 0 and r["trace"][:3].any()  # (the evaluation was made)
    # n_cand = 0: the graph is evaluated, nothing is judged
    r = gr.gate(pose, ij, z, info, cij, cz, cinfo, **dict(kw, n_cand=0))
    assert r["flags"] == 0 and untouched(r) and r["chi2"] == good["chi2"]
    # BAD_EDGE: on itself, on a node that is not there, a value that is not finite; the others are still judged
    for at, (arr, val) in enumerate((("ij", [1, 1]), ("ij", [0, 3]), ("ij", [-1, 2]), ("z", np.inf), ("info", np.nan))):
        c2, z2, o2 = cij.copy(), cz.copy(), cinfo.copy()
        if arr == "ij":
            c2[0] = val
        elif arr == "z":
            z2[0, 2] = val
        else:
            o2[0, 4] = val
        r = gr.gate(pose, ij, z, info, c2, z2, o2, **kw)
        assert r["flags"] == 0 and r["cand_flags"][0] == gr.BAD_EDGE and r["cand_flags"][1] == gr.ACCEPTED | gr.APPENDED, at
        assert not r["cand_nis"][0] and not r["cand_err"][0].any() and not r["cand_cov"][0].any() and r["n_edges"] == 3
        assert r["cand_nis"][1] == good["cand_nis"][1]
    # BAD_INFO from a negative and from a singular Omega: nis 0, no verdict, not appended
    for om in (-cinfo[0], [1e-2, 1e-2, 0.0, 1e-2, 0.0, 1e2], np.zeros(6)):
        o2 = cinfo.copy()
        o2[0] = om
        r = gr.gate(pose, ij, z, info, cij, cz, o2, **kw)
        assert r["cand_flags"][0] == gr.BAD_INFO and r["cand_nis"][0] == 0.0 and r["n_edges"] == 3, om
        assert np.array_equal(r["cand_cov"][0], good["cand_cov"][0])
    # a NaN d2 is an OUTLIER, under an infinite gate too: e of 1e200 and 1e300 with a positive xy term in S
    # (e0 w0 = -inf, e1 w1 = +inf)
    z2, o2 = cz.copy(), cinfo.copy()
    z2[0, :2] = [-1e200, -1e300]
    o2[0] = [1e-2, -5e-3, 0.0, 1e-2, 0.0, 1e2]
    for nis_max in (NIS_MAX, np.inf):
        r = gr.gate(pose, ij, z, info, cij, z2, o2, **dict(kw, nis_max=nis_max))
        assert np.isnan(r["cand_nis"][0]) and r["cand_flags"][0] == gr.OUTLIER
    # nis_max = +inf accepts what 16.27 rejects
    z2 = cz.copy()
    z2[0, 0] += 5000.0
    r = gr.gate(pose, ij, z, info, cij, z2, cinfo, **kw)
    assert r["cand_flags"][0] == gr.OUTLIER and r["cand_nis"][0] > NIS_MAX and r["n_edges"] == 3
    r = gr.gate(pose, ij, z, info, cij, z2, cinfo, **dict(kw, nis_max=np.inf))
    assert r["cand_flags"][0] == gr.ACCEPTED | gr.APPENDED
    # APPENDED and NO_ROOM at E = E_cap - 1 with two accepted candidates; without append neither, and the edges stay
    r = gr.gate(pose, ij[:3], z[:3], info[:3], cij, cz, cinfo, **kw)
    assert list(r["cand_flags"]) == [gr.ACCEPTED | gr.APPENDED, gr.ACCEPTED | gr.NO_ROOM] and r["n_edges"] == 3
    r = gr.gate(pose, ij[:3], z[:3], info[:3], cij, cz, cinfo, n_nodes=3, n_edges=2)
    assert list(r["cand_flags"]) == [gr.ACCEPTED, gr.ACCEPTED] and r["n_edges"] == 2 and np.array_equal(r["edge_ij"], ij[:3])
    # candidates into node 0 and out of it (i > j and i < j): the same pair read both ways has the same d2 up to rounding
    back = pg.relative_pose(pose[0], pose[2])
    r = gr.gate(pose, ij, z, info, [[2, 0], [0, 2], [1, 2], [2, 1]],
                [cz[0], back, pg.relative_pose(pose[1], pose[2]), pg.relative_pose(pose[2], pose[1])], unit_info(4), n_nodes=3, n_edges=2)
    assert (r["cand_flags"] == gr.ACCEPTED).all() and (r["cand_cov"][:, [0, 3, 5]] > 0).all()
    assert abs(r["cand_cov"][0, 5] - r["cand_cov"][1, 5]) <= 1e-12 * r["cand_cov"][0, 5]
    # (an edge already in the graph is better known than one across two edges)
    assert r["cand_cov"][2, 5] < r["cand_cov"][0, 5]


def test_closure_window():
    cov = np.array([[400.0, 0.0, 0.0, 100.0, 0.0, 0.0004], [250.0, 150.0, 0.0, 250.0, 0.0, 0.01]])
    xy, th = posegraph.closure_window(cov)
    assert np.allclose(xy, [60.0, 60.0]) and np.allclose(th, [0.06, 0.3])
    xy, th = posegraph.closure_window(cov[0], k=1.0)
    assert np.isclose(xy, 20.0) and np.isclose(th, 0.02)
    with pytest.raises(ValueError):
        posegraph.closure_window(np.zeros((2, 5)))
