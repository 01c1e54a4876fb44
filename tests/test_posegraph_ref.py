"""The NumPy form of lslam_pose_graph (tests/posegraph_ref.py) against what it must mean: its Jacobians
against central differences, its LDL^T step against np.linalg.solve, loops that close, the gauge, a false
closure, every flag, headings across +-pi.  CPU only; the reference alone (the kernel is held to it bit for
bit in tests/test_gpu_posegraph.py, the core header in tests/test_posegraph_core.py).

Figures measured here (printed by the tests; DESIGN.md 4.4 records them):
  the step against np.linalg.solve, worst |delta - delta_np| / max|delta_np| over the three loops: 5.3e-14
  (N = 4: 7.4e-15, N = 24: 4.7e-15, N = 48: 5.3e-14; cond(H) 1.4e7, 4.6e8, 1.9e9); STEP_BOUND is ten times that.
  loops, worst pose error against the truth before -> after, steps to CONVERGED, chi2 before -> after:
    N = 4:  7.7 mm 0.012 rad -> 4.7 mm 0.001 rad, 3 steps, 10.7 -> 0.47
    N = 24: 43.2 mm 0.078 rad -> 35.1 mm 0.008 rad, 4 steps, 289.7 -> 2.82
    N = 48: 128.0 mm 0.190 rad -> 59.4 mm 0.007 rad, 5 steps, 2095.0 -> 7.68"""
import math

import numpy as np
import pytest

import posegraph_ref as pg
from lidar_slam_amd import posegraph  # (the feature's module: the reference tests belong to it)

LOOPS = (4, 24, 48)
STEP_BOUND = 5.3e-13  # ten times the worst relative difference measured (the docstring)


def loop(N, **kw):
    return pg.circle_loop(N, seed=1000 + N, **kw)


def test_jacobians_against_central_differences():
    rng = np.random.default_rng(1)
    for _ in range(20):
        pose = np.concatenate([rng.uniform(-3000, 3000, (2, 2)), rng.uniform(-3.0, 3.0, (2, 1))], 1)
        z = np.concatenate([rng.uniform(-500, 500, 2), rng.uniform(-0.5, 0.5, 1)])[None]
        ij, info = np.array([[0, 1]]), np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]])

        def err(p):
            cs = np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], 1)
            return pg.edge_terms(p, ij, z, info, cs)["e"][0]
        t = pg.edge_terms(pose, ij, z, info, np.stack([np.cos(pose[:, 2]), np.sin(pose[:, 2])], 1))
        for node, J in ((0, t["A"][0]), (1, t["B"][0])):
            for c in range(3):
                h = 1e-3 if c < 2 else 1e-6
                hi, lo = pose.copy(), pose.copy()
                hi[node, c] += h
                lo[node, c] -= h
                num = (err(hi) - err(lo)) / (2 * h)
                # (e is linear in the positions; in theta_i the second derivative is ux, uy: h^2 of 6000 mm)
                assert np.allclose(num, J[:, c], rtol=0, atol=1e-4), (node, c, num, J[:, c])


def first_step(N, pose, ij, z, info):
    r = pg.solve(pose, ij, z, info, n_iter=1)
    Hr, gr, delta, _ = r["first"]
    full = np.tril(Hr) + np.tril(Hr, -1).T
    want = -np.linalg.solve(full, gr)
    return delta, want, np.linalg.cond(full)


def test_step_against_numpy_solve():
    worst = 0.0
    for N in LOOPS:
        _, init, ij, z, info = loop(N)
        delta, want, cond = first_step(N, init, ij, z, info)
        rel = float(np.abs(delta - want).max() / np.abs(want).max())
        print("N = %d: relative difference %.2e, cond(H) %.2e" % (N, rel, cond))
        worst = max(worst, rel)
    print("worst %.2e, bound %.2e" % (worst, STEP_BOUND))
    assert worst <= STEP_BOUND


@pytest.mark.parametrize("N", LOOPS)
def test_loop_closes(N):
    truth, init, ij, z, info = loop(N)
    r = pg.solve(init, ij, z, info)
    before, after = pg.pose_error(init, truth), pg.pose_error(r["pose_out"], truth)
    print("N = %d: %.1f mm %.3f rad -> %.1f mm %.3f rad, %d steps, chi2 %.1f -> %.2f"
          % (N, before[0], before[1], after[0], after[1], r["iters"], r["chi2"][0], r["chi2"][1]))
    assert r["flags"] == pg.CONVERGED and 1 <= r["iters"] <= 10
    assert r["chi2"][1] < r["chi2"][0]
    assert after[0] < before[0] and after[1] < before[1]
    assert np.array_equal(r["pose_out"][0], init[0])  # the gauge keeps its bits
    assert not r["trace"][r["iters"] + 1:].any() and r["trace"][r["iters"], :N].any()


@pytest.mark.parametrize("N", LOOPS)
def test_gauge_a_rigid_motion_of_the_graph_moves_the_solution(N):
    _, init, ij, z, info = loop(N)
    r0 = pg.solve(init, ij, z, info)
    th, t = 0.7, np.array([-350.0, 1200.0])
    c, s = math.cos(th), math.sin(th)
    R = np.array([[c, -s], [s, c]])

    def move(p):
        return np.concatenate([p[:, :2] @ R.T + t, p[:, 2:] + th], 1)
    r1 = pg.solve(move(init), ij, z, info)
    assert r1["flags"] == r0["flags"] == pg.CONVERGED and r1["iters"] == r0["iters"]
    want = move(r0["pose_out"])
    scale = np.abs(want).max()
    assert np.abs(r1["pose_out"] - want).max() <= STEP_BOUND * scale * r0["iters"]


def with_false_closure(N, sigma):
    """The loop with its true closure, plus a closure N / 2 -> 0 whose z is off by 500 mm, at ``sigma`` (mm, rad)."""
    truth, init, ij, z, info = loop(N)
    zf = pg.relative_pose(truth[N // 2], truth[0])
    zf[0] += 500.0
    om = [1.0 / sigma[0] ** 2, 0.0, 0.0, 1.0 / sigma[0] ** 2, 0.0, 1.0 / sigma[1] ** 2]
    return init, np.vstack([ij, [[N // 2, 0]]]), np.vstack([z, zf[None]]), np.vstack([info, [om]])


def test_a_false_closure_has_the_largest_edge_chi2():
    """A closure that is 500 mm wrong, weighted as the odometry it contradicts (10 mm, 0.01 rad): it carries the
    largest edge_chi2 by a factor of two and more (measured 627 against 328 at N = 4, 41.0 against 14.0 at N = 24,
    11.6 against 4.4 at N = 48), and the graph is not rejected: there is no robust kernel."""
    for N in LOOPS:
        init, ij, z, info = with_false_closure(N, (10.0, 0.01))
        r = pg.solve(init, ij, z, info)
        ec = r["edge_chi2"]
        print("N = %d: false closure %.1f, largest other %.1f" % (N, ec[-1], ec[:-1].max()))
        assert r["flags"] == pg.CONVERGED
        assert int(np.argmax(ec)) == len(ij) - 1 and ec[-1] > 1.5 * ec[:-1].max()
        good = pg.solve(*loop(N)[1:])
        assert r["chi2"][1] > 10 * good["chi2"][1]


def test_the_limit_of_edge_chi2_a_false_closure_stronger_than_the_odometry():
    """The known limit, held here so that the documents stay honest.  In a cycle the converged residual spreads in
    proportion to the edges' variances, so an edge's chi is proportional to its own variance: the weakest edges
    carry the largest.  A false closure given MORE weight than the odometry (5 mm against 10 mm) bends the
    odometry and does not stand out: the largest edge_chi2 is an odometry edge.  Before any step (n_iter = 0) it
    still does: the odometry edges are at rest."""
    for N in LOOPS:
        _, init, ij, z, info = loop(N, false_closure=500.0)  # the loop's one closure, wrong, at 5 mm
        r = pg.solve(init, ij, z, info)
        assert not r["flags"] & pg.REJECTED and int(np.argmax(r["edge_chi2"])) != len(ij) - 1
        r = pg.solve(init, ij, z, info, n_iter=0)
        assert int(np.argmax(r["edge_chi2"])) == len(ij) - 1


def unit_info(n):
    return np.tile([1e-2, 0.0, 0.0, 1e-2, 0.0, 1e2], (n, 1))


def test_every_flag():
    pose = np.array([[0.0, 0.0, 0.0], [1000.0, 0.0, 0.1], [1000.0, 1000.0, 1.6], [5.0, 6.0, 7.0]])
    ij = np.array([[0, 1], [1, 2], [2, 0]])
    z = pg.relative_pose(pose[ij[:, 0]], pose[ij[:, 1]]) + 3.0 * np.array([[1.0, -1.0, 0.001]])
    info = unit_info(3)
    same = lambda r: np.array_equal(r["pose_out"].view(np.uint64), pose.view(np.uint64))  # noqa: E731
    zero = lambda r: not (r["trace"].any() or r["chi2"].any() or r["edge_chi2"].any() or r["iters"])  # noqa: E731
    # EMPTY: fewer than two nodes, or no edge
    for kw in (dict(n_nodes=1, n_edges=3), dict(n_nodes=0, n_edges=0), dict(n_nodes=3, n_edges=0)):
        r = pg.solve(pose, ij, z, info, **kw)
        assert r["flags"] == pg.EMPTY and same(r) and zero(r), kw
    # BAD_GRAPH: counts out of range; an edge on itself, on a node that is not there; values that are not finite
    for kw in (dict(n_nodes=5), dict(n_edges=4), dict(n_nodes=-1), dict(n_edges=-1)):
        r = pg.solve(pose, ij, z, info, **dict(dict(n_nodes=3, n_edges=3), **kw))
        assert r["flags"] == pg.BAD_GRAPH and same(r) and zero(r), kw
    for bad_ij in ([1, 1], [0, 3], [-1, 2], [3, 0]):
        b = ij.copy()
        b[1] = bad_ij
        r = pg.solve(pose, b, z, info, n_nodes=3)
        assert r["flags"] == pg.BAD_GRAPH and same(r) and zero(r), bad_ij
    for arr, at in ((0, (2, 1)), (2, (0, 2)), (3, (1, 4))):
        args = [pose.copy(), ij, z.copy(), info.copy()]
        args[arr][at] = (np.nan, np.inf, -np.inf)[arr % 3]
        r = pg.solve(*args, n_nodes=3)
        assert r["flags"] == pg.BAD_GRAPH and zero(r), (arr, at)
        assert np.array_equal(r["pose_out"].view(np.uint64), args[0].view(np.uint64))
    # (a value that is not finite on a node or an edge that is not used does not count)
    p2 = pose.copy()
    p2[3] = np.nan
    r = pg.solve(p2, ij, z, info, n_nodes=3)
    assert r["flags"] == pg.CONVERGED and np.isnan(r["pose_out"][3]).all()
    # CONVERGED, and the slab of the unused node copied through
    r = pg.solve(pose, ij, z, info, n_nodes=3)
    assert r["flags"] == pg.CONVERGED and r["chi2"][1] < r["chi2"][0] and np.array_equal(r["pose_out"][3], pose[3])
    # n_iter = 0: one evaluation, no step
    r = pg.solve(pose, ij, z, info, n_nodes=3, n_iter=0)
    assert r["flags"] == 0 and r["iters"] == 0 and same(r) and r["chi2"][0] == r["chi2"][1] > 0 and r["trace"].shape[0] == 1
    # not converged within n_iter: no flag, the poses moved
    r = pg.solve(pose, ij, z, info, n_nodes=3, n_iter=1)
    assert r["flags"] == 0 and r["iters"] == 1 and not same(r)
    # SINGULAR: an isolated node with no damping; with the default damping it stays put bit for bit
    r = pg.solve(pose, ij[:1], z[:1], info[:1], n_nodes=3, damp_t=0.0, damp_r=0.0)
    assert r["flags"] == pg.SINGULAR and same(r) and r["iters"] == 0 and r["chi2"][0] == r["chi2"][1] > 0
    r = pg.solve(pose, ij[:1], z[:1], info[:1], n_nodes=3)
    assert r["flags"] == pg.CONVERGED and np.array_equal(r["pose_out"][2:].view(np.uint64), pose[2:].view(np.uint64))
    assert not np.array_equal(r["pose_out"][1], pose[1])
    # SINGULAR: an information matrix that is not positive (a negative pivot)
    r = pg.solve(pose, ij, z, -info, n_nodes=3)
    assert r["flags"] & pg.SINGULAR and same(r)
    # DIVERGED: measurements far from the poses (kilometres, radians) with anisotropic weights: the linear step
    # overshoots and chi2 of the last evaluation is above the first's (4.4e6 -> 1.5e9 after one step, 2.9e7
    # after ten); a NaN chi2 (an infinite chi of either sign) fails the gate too, before any step
    r = pg.diverging()
    for n_iter in (1, 10):
        d = pg.solve(*r, n_iter=n_iter)
        assert d["flags"] == pg.DIVERGED and d["iters"] == n_iter and d["chi2"][1] > d["chi2"][0]
        assert np.array_equal(d["pose_out"].view(np.uint64), r[0].view(np.uint64))
    big = info.copy()
    big[0], big[1] = 1.7e308, -1.7e308
    r = pg.solve(pose, ij, z, big, n_nodes=3, n_iter=0)
    assert r["flags"] == pg.DIVERGED and np.isnan(r["chi2"]).all() and same(r)


def test_heading_differences_across_pi():
    """Two nodes whose headings straddle +-pi, the measurement likewise: e2 is the wrapped difference, small, and
    the solution is the one a graph rotated away from the seam gives, rotated back."""
    base = np.array([[0.0, 0.0, 0.0], [800.0, 100.0, 0.05], [900.0, 700.0, 0.02]])
    ij = np.array([[0, 1], [1, 2], [2, 0]])
    info = unit_info(3)
    z = pg.relative_pose(base[ij[:, 0]], base[ij[:, 1]]) + np.array([[2.0, 1.0, 0.002]])
    r0 = pg.solve(base, ij, z, info)
    for turn in (math.pi - 0.03, -math.pi - 0.03):
        c, s = math.cos(turn), math.sin(turn)
        p = np.concatenate([base[:, :2] @ np.array([[c, -s], [s, c]]).T, base[:, 2:] + turn], 1)
        p[:, 2] = pg.ieee_remainder(p[:, 2])  # every heading written inside +-pi: the nodes lie on both sides of the seam
        assert (np.abs(p[:, 2]) <= math.pi).all() and np.ptp(p[:, 2]) > 6.0
        zz = z.copy()
        zz[0, 2] += 2.0 * math.pi  # the same measurement written a turn away
        r = pg.solve(p, ij, zz, info)
        assert r["flags"] == pg.CONVERGED and r["iters"] == r0["iters"]
        e = pg.edge_terms(p, ij, zz, info, np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], 1))["e"]
        assert np.abs(e[:, 2]).max() < 0.01
        back = r["pose_out"].copy()
        back[:, 2] = pg.ieee_remainder(back[:, 2] - turn)
        back[:, :2] = back[:, :2] @ np.array([[c, s], [-s, c]]).T
        assert np.abs(back - r0["pose_out"]).max() < 1e-6


def test_relative_pose_is_the_package_s():
    """``lidar_slam_amd.posegraph.relative_pose`` makes z's bits; the reference's twin agrees with it."""
    rng = np.random.default_rng(5)
    a, b = rng.uniform(-3, 3, (50, 3)) * [1000, 1000, 1], rng.uniform(-3, 3, (50, 3)) * [1000, 1000, 1]
    assert np.array_equal(posegraph.relative_pose(a, b), pg.relative_pose(a, b))
    assert np.array_equal(posegraph.relative_pose(a[3], b[3]), pg.relative_pose(a, b)[3])
    th = 0.4
    info_w = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, -0.2], [0.5, -0.2, 9.0]])
    z, om = posegraph.closure_edge(a[0], b[0], info_w, cell=20.0)
    assert np.array_equal(z, pg.relative_pose(a[0], b[0]))
    assert np.allclose(om, pg.rotate_information(info_w, a[0, 2], 20.0), rtol=1e-14, atol=0)
