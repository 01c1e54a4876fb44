"""NumPy form of lslam_pose_graph (the definition is the comment in include/lidarslam.h): one graph, FP64,
every operation rounded on its own, in the definition's order.  The kernel (lslam_posegraph.h) and the
core header's CPU program must match it bit for bit, given the (cos, sin) of every evaluation: ``solve``
takes them as ``trace`` (the device's, so that the library's cos and sin are the definition's input) or
makes them with NumPy's.

Per edge the terms are computed for all edges at once, elementwise (NumPy rounds each elementwise
operation on its own, as the C does); the sums over edges are a Python loop in ascending e."""
import math

import numpy as np

EMPTY, BAD_GRAPH, CONVERGED, SINGULAR, DIVERGED = 1, 2, 4, 8, 16
REJECTED = BAD_GRAPH | SINGULAR | DIVERGED
TWO_PI = 6.283185307179586
DEFAULTS = dict(n_iter=10, damp_t=1e-6, damp_r=1e-3, eps_t=0.01, eps_r=1e-5)


def relative_pose(a, b):
    """z of an edge a -> b: the pose b seen from a.  [3] and [3] -> [3]; [n, 3] and [n, 3] -> [n, 3]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, b[..., 2] - a[..., 2]], -1)


def dot3(a0, b0, a1, b1, a2, b2):
    t0, t1, t2 = a0 * b0, a1 * b1, a2 * b2
    return (t0 + t1) + t2


def ieee_remainder(v):
    return np.array([math.remainder(float(x), TWO_PI) for x in np.atleast_1d(v)], np.float64)


def edge_terms(pose, ij, z, info, cs):
    """All edges at one evaluation.  pose [N, 3], ij [E, 2], z [E, 3], info [E, 6], cs [N, 2] -> dict of
    e [E, 3], A, B, MA, MB [E, 3, 3], w [E, 3], chi [E]."""
    i, j = ij[:, 0], ij[:, 1]
    E = len(i)
    pi, pj = pose[i], pose[j]
    c, s = cs[i, 0], cs[i, 1]
    zero, one = np.zeros(E), np.ones(E)
    dx, dy = pj[:, 0] - pi[:, 0], pj[:, 1] - pi[:, 1]
    ux, uy = c * dx + s * dy, c * dy - s * dx
    e = np.stack([ux - z[:, 0], uy - z[:, 1], ieee_remainder((pj[:, 2] - pi[:, 2]) - z[:, 2])], 1)
    A = np.stack([np.stack([-c, -s, uy], 1), np.stack([s, -c, -ux], 1), np.stack([zero, zero, -one], 1)], 1)
    B = np.stack([np.stack([c, s, zero], 1), np.stack([-s, c, zero], 1), np.stack([zero, zero, one], 1)], 1)
    O = np.empty((E, 3, 3))
    for (r, k), q in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
        O[:, r, k] = O[:, k, r] = info[:, q]
    MA, MB, w = np.empty((E, 3, 3)), np.empty((E, 3, 3)), np.empty((E, 3))
    for r in range(3):
        for k in range(3):
            MA[:, r, k] = dot3(O[:, r, 0], A[:, 0, k], O[:, r, 1], A[:, 1, k], O[:, r, 2], A[:, 2, k])
            MB[:, r, k] = dot3(O[:, r, 0], B[:, 0, k], O[:, r, 1], B[:, 1, k], O[:, r, 2], B[:, 2, k])
        w[:, r] = dot3(O[:, r, 0], e[:, 0], O[:, r, 1], e[:, 1], O[:, r, 2], e[:, 2])
    chi = dot3(e[:, 0], w[:, 0], e[:, 1], w[:, 1], e[:, 2], w[:, 2])
    return dict(e=e, A=A, B=B, MA=MA, MB=MB, w=w, chi=chi)


def jt_m(J, M):
    """J^T M per edge, element (r, k) = (J[0][r] M[0][k] + J[1][r] M[1][k]) + J[2][r] M[2][k]."""
    out = np.empty_like(M)
    for r in range(3):
        for k in range(3):
            out[:, r, k] = dot3(J[:, 0, r], M[:, 0, k], J[:, 1, r], M[:, 1, k], J[:, 2, r], M[:, 2, k])
    return out


def jt_w(J, w):
    return np.stack([dot3(J[:, 0, r], w[:, 0], J[:, 1, r], w[:, 1], J[:, 2, r], w[:, 2]) for r in range(3)], 1)


def assemble(N, ij, t):
    """The full H [3N, 3N] (lower triangle and diagonal meaningful, the blocks above the diagonal are the
    definition's transposes) and g [3N], each element summed from +0.0 in ascending e; chi2."""
    H, g = np.zeros((3 * N, 3 * N)), np.zeros(3 * N)
    Hii, Hij, Hjj = jt_m(t["A"], t["MA"]), jt_m(t["A"], t["MB"]), jt_m(t["B"], t["MB"])
    gi, gj = jt_w(t["A"], t["w"]), jt_w(t["B"], t["w"])
    chi2 = 0.0
    for e in range(len(ij)):
        i, j = 3 * int(ij[e, 0]), 3 * int(ij[e, 1])
        H[i:i + 3, i:i + 3] += Hii[e]
        H[i:i + 3, j:j + 3] += Hij[e]
        H[j:j + 3, i:i + 3] += Hij[e].T
        H[j:j + 3, j:j + 3] += Hjj[e]
        g[i:i + 3] += gi[e]
        g[j:j + 3] += gj[e]
        chi2 = chi2 + float(t["chi"][e])
    return H, g, chi2


def pivot_ok(d):
    return d > 0.0 and d < math.inf


def ldlt_solve(H, g):
    """The definition's step 2 on the reduced, damped H (its lower triangle) and g: x with H x = g, or
    None at the first pivot that is not finite and > 0.  Column by column; the elementwise NumPy
    operations round as the C's one product and one subtraction."""
    H, n = H.copy(), len(g)
    with np.errstate(all="ignore"):
        for p in range(n):
            d = H[p, p]
            if not pivot_ok(d):
                return None
            u = H[p + 1:, p].copy()
            l = u / d
            H[p + 1:, p] = l
            H[p + 1:, p + 1:] = H[p + 1:, p + 1:] - l[:, None] * u[None, :]
        y = g.copy()
        for b in range(n):
            y[b + 1:] = y[b + 1:] - H[b + 1:, b] * y[b]
        x = y / np.diag(H)
        for b in range(n - 1, 0, -1):
            x[:b] = x[:b] - H[b, :b] * x[b]
    return x


def damped(H, g, N, damp_t, damp_r):
    """Node 0 dropped, the damping added after the sums."""
    Hr, gr = H[3:, 3:].copy(), g[3:].copy()
    for v in range(N - 1):
        Hr[3 * v, 3 * v] = Hr[3 * v, 3 * v] + damp_t
        Hr[3 * v + 1, 3 * v + 1] = Hr[3 * v + 1, 3 * v + 1] + damp_t
        Hr[3 * v + 2, 3 * v + 2] = Hr[3 * v + 2, 3 * v + 2] + damp_r
    return Hr, gr


def solve(pose, ij, z, info, n_nodes=None, n_edges=None, max_nodes=None, max_edges=None, trace=None, **kw):
    """One graph.  pose [N_cap, 3]; ij [E_cap, 2]; z [E_cap, 3]; info [E_cap, 6]; n_nodes, n_edges (default: all
    given); trace [n_iter + 1, N_cap, 2]: the (cos, sin) to use, or None for NumPy's.  Returns pose_out
    [N_cap, 3], trace (NumPy's own cos and sin of the poses it evaluated at, zeros beyond), chi2 [2], edge_chi2
    [E_cap], iters, flags, and ``first``: (H, g, delta or None, chi2) of evaluation 0's reduced damped system."""
    p = dict(DEFAULTS, **kw)
    pose = np.array(pose, np.float64).reshape(-1, 3)
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    z, info = np.asarray(z, np.float64).reshape(-1, 3), np.asarray(info, np.float64).reshape(-1, 6)
    Nc = len(pose) if max_nodes is None else int(max_nodes)
    Ec = len(ij) if max_edges is None else int(max_edges)
    N = len(pose) if n_nodes is None else int(n_nodes)
    E = len(ij) if n_edges is None else int(n_edges)
    n_iter = int(p["n_iter"])
    out = dict(pose_out=pose.copy(), trace=np.zeros((n_iter + 1, Nc, 2)), chi2=np.zeros(2), edge_chi2=np.zeros(Ec),
               iters=0, flags=0, first=None)
    if N < 0 or E < 0 or N > Nc or E > Ec:
        out["flags"] = BAD_GRAPH
        return out
    if N < 2 or E == 0:
        out["flags"] = EMPTY
        return out
    ij, z, info = ij[:E], z[:E], info[:E]
    bad = np.any(ij[:, 0] == ij[:, 1]) or np.any(ij < 0) or np.any(ij >= N)
    bad = bad or not (np.isfinite(pose[:N]).all() and np.isfinite(z).all() and np.isfinite(info).all())
    if bad:
        out["flags"] = BAD_GRAPH
        return out
    x = pose[:N].copy()
    flags, iters, chi_first, chi_last = 0, 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        for k in range(n_iter + 1):
            own = np.stack([np.cos(x[:, 2]), np.sin(x[:, 2])], 1)
            out["trace"][k, :N] = own
            cs = own if trace is None else np.asarray(trace, np.float64)[k, :N]
            t = edge_terms(x, ij, z, info, cs)
            H, g, chi2 = assemble(N, ij, t)
            out["edge_chi2"][:E] = t["chi"]
            chi_last = chi2
            if k == 0:
                chi_first = chi2
            if k == n_iter or flags & CONVERGED:
                break
            Hr, gr = damped(H, g, N, p["damp_t"], p["damp_r"])
            sol = ldlt_solve(Hr, gr)
            if k == 0:
                out["first"] = (Hr, gr, None if sol is None else -sol, chi2)
            if sol is None:
                flags |= SINGULAR
                break
            delta = (-sol).reshape(N - 1, 3)
            stepped = x.copy()
            stepped[1:] = x[1:] + delta
            if not np.isfinite(stepped).all():
                flags |= SINGULAR
                break
            x, iters = stepped, k + 1
            if np.all(np.abs(delta[:, :2]) < p["eps_t"]) and np.all(np.abs(delta[:, 2]) < p["eps_r"]):
                flags |= CONVERGED
    if not chi_last <= chi_first:
        flags |= DIVERGED
    if not flags & REJECTED:
        out["pose_out"][:N] = x
    out.update(chi2=np.array([chi_first, chi_last]), iters=iters, flags=flags)
    return out


def rotate_information(info_world, theta_i, unit_mm):
    """A world-frame 3 x 3 information matrix in (unit, unit, rad) -> the 6 values xx, xy, xt, yy, yt, tt of
    Omega in the frame of a node with heading theta_i, in (mm, mm, rad): T^T info T with
    T = diag(R(theta_i), 1) / diag(unit_mm, unit_mm, 1)."""
    c, s = math.cos(theta_i), math.sin(theta_i)
    T = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.diag([1.0 / unit_mm, 1.0 / unit_mm, 1.0])
    O = T.T @ np.asarray(info_world, np.float64) @ T
    O = 0.5 * (O + O.T)
    return np.array([O[0, 0], O[0, 1], O[0, 2], O[1, 1], O[1, 2], O[2, 2]])


def circle_loop(N, seed, radius=700.0, centre=(2000.0, 1500.0), bias=(3.0, -2.0, 0.004), noise=(2.0, 0.002),
                sig_odo=(10.0, 0.01), sig_loop=(5.0, 0.005), false_closure=0.0):
    """The loop of the tests: N keyframes on a circle, heading along it.  Returns truth [N, 3], the drifted
    initial poses [N, 3] (the biased, noisy odometry chained from the true first pose), ij [N, 2], z [N, 3] and
    info [N, 6]: N - 1 odometry edges k -> k + 1 and one closure N - 1 -> 0 (its z the truth's, x off by
    ``false_closure`` mm)."""
    rng = np.random.default_rng(seed)
    a = 2.0 * math.pi * np.arange(N) / N
    truth = np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a), a + 0.5 * math.pi], 1)
    z_odo = relative_pose(truth[:-1], truth[1:])
    z_odo[:, :2] += np.asarray(bias[:2]) + rng.normal(0.0, noise[0], (N - 1, 2))
    z_odo[:, 2] += bias[2] + rng.normal(0.0, noise[1], N - 1)
    init = np.empty((N, 3))
    init[0] = truth[0]
    for k in range(N - 1):
        c, s = math.cos(init[k, 2]), math.sin(init[k, 2])
        init[k + 1] = (init[k, 0] + c * z_odo[k, 0] - s * z_odo[k, 1], init[k, 1] + s * z_odo[k, 0] + c * z_odo[k, 1],
                       init[k, 2] + z_odo[k, 2])
    z_loop = relative_pose(truth[-1], truth[0])
    z_loop[0] += false_closure
    ij = np.array([[k, k + 1] for k in range(N - 1)] + [[N - 1, 0]], np.int32)
    z = np.vstack([z_odo, z_loop[None]])

    def diag(st, sr):
        return [1.0 / st ** 2, 0.0, 0.0, 1.0 / st ** 2, 0.0, 1.0 / sr ** 2]
    info = np.array([diag(*sig_odo)] * (N - 1) + [diag(*sig_loop)])
    return truth, init, ij, z, info


def pose_error(x, truth):
    """(worst position error in mm, worst heading error in rad, wrapped)."""
    d = np.asarray(x) - np.asarray(truth)
    return float(np.hypot(d[:, 0], d[:, 1]).max()), float(np.abs(ieee_remainder(d[:, 2])).max())


def random_graph(N, rng, extra):
    """A chain with noise, closures and ``extra`` random edges (i > j, into node 0, repeated pairs among them)."""
    pose = np.concatenate([rng.uniform(-4000, 4000, (N, 2)), rng.uniform(-3.2, 3.2, (N, 1))], 1)
    ij = [[k, k + 1] for k in range(N - 1)] + [[N - 1, 0]]
    for _ in range(extra):
        i, j = rng.choice(N, 2, replace=False) if N > 2 else (1, 0)
        ij.append([int(i), int(j)])
    if N > 2:
        ij += [[2, 1], [2, 1], [1, 2]]  # three edges on one pair, in both directions
    ij = np.array(ij, np.int32)
    z = relative_pose(pose[ij[:, 0]], pose[ij[:, 1]]) + rng.normal(0, 1, (len(ij), 3)) * [20.0, 20.0, 0.02]
    A = rng.normal(0, 1, (len(ij), 3, 3)) * [0.1, 0.1, 10.0]
    O = np.einsum("eij,ekj->eik", A, A) + np.diag([1e-3, 1e-3, 10.0])  # symmetric positive definite, with cross terms
    info = np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], 1)
    return pose, ij, z, info


def diverging():
    """(pose, ij, z, info) of a three-node graph whose Gauss-Newton steps raise chi2."""
    pose = np.array([[350.0, -150.0, -0.85], [680.0, -560.0, 2.83], [-480.0, 730.0, -2.2]])
    ij = np.array([[0, 1], [1, 2], [2, 0]])
    z = np.array([[3570.0, 525.0, -0.58], [367.0, 334.0, 0.76], [-3176.0, 2755.0, 0.85]])
    info = np.array([[0.16, 0, 0, 1.7e-5, 0, 5.7e-3], [0.36, 0, 0, 1.4e-3, 0, 2.6e-3], [1.7e-3, 0, 0, 0.99, 0, 2.8]])
    return pose, ij, z, info
