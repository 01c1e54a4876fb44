"""NumPy form of lslam_pose_graph_gate (the definition is the comment in include/lidarslam.h): one graph and its
closure candidates, FP64, every operation rounded on its own, in the definition's order.  The kernel
(lslam_posegate.h) and the core header's CPU program must match it bit for bit, given the (cos, sin) of the one
evaluation: ``gate`` takes them as ``trace`` (the device's) or makes them with NumPy's.

The edge terms, the assembly and the damping are posegraph_ref's, the 3 x 3 inverse is fieldfuse_ref's.  The
LDL^T is written here as factor once, solve many, with the element order of posegraph_ref.ldlt_solve."""
import numpy as np

import fieldfuse_ref as ffr
import posegraph_ref as pg

EMPTY, BAD_GRAPH, SINGULAR = pg.EMPTY, pg.BAD_GRAPH, pg.SINGULAR
UNJUDGED, ACCEPTED, OUTLIER, BAD_EDGE, BAD_INFO, APPENDED, NO_ROOM = 0, 1, 2, 4, 8, 16, 32
DEFAULTS = dict(damp_t=1e-6, damp_r=1e-3, nis_max=16.27, append=0)
f64 = np.float64


def ldlt_factor(H):
    """The definition's step 2 on the reduced, damped H (its lower triangle): the unit lower factor below the
    diagonal and d on it, or None at the first pivot that is not finite and > 0."""
    H, n = H.copy(), len(H)
    with np.errstate(all="ignore"):
        for p in range(n):
            d = H[p, p]
            if not pg.pivot_ok(d):
                return None
            u = H[p + 1:, p].copy()
            l = u / d
            H[p + 1:, p] = l
            H[p + 1:, p + 1:] = H[p + 1:, p + 1:] - l[:, None] * u[None, :]
    return H


def ldlt_apply(F, R):
    """X with H X = R, R [n, m]: every column forward, divided and back as posegraph_ref.ldlt_solve treats g."""
    n = len(F)
    with np.errstate(all="ignore"):
        Y = np.array(R, np.float64)
        for b in range(n):
            Y[b + 1:] = Y[b + 1:] - F[b + 1:, b][:, None] * Y[b][None, :]
        X = Y / np.diag(F)[:, None]
        for b in range(n - 1, 0, -1):
            X[:b] = X[:b] - F[b, :b][:, None] * X[b][None, :]
    return X


def full3(om):
    return np.array([[om[0], om[1], om[2]], [om[1], om[3], om[4]], [om[2], om[4], om[5]]], np.float64)


def judge(pose, cs, F, N, i, j, z, om, nis_max):
    """Step 3 for one candidate -> (flag, nis, e [3], cov [6])."""
    zero = (0.0, np.zeros(3), np.zeros(6))
    if i == j or not (0 <= i < N and 0 <= j < N) or not (np.isfinite(z).all() and np.isfinite(om).all()):
        return (BAD_EDGE,) + zero
    n = 3 * (N - 1)
    with np.errstate(all="ignore"):
        t = pg.edge_terms(pose, np.array([[i, j]]), z[None], om[None], cs)
        e, A, B = t["e"][0], t["A"][0], t["B"][0]
        R = np.zeros((n, 3))
        if i >= 1:
            R[3 * (i - 1):3 * i] = A.T
        if j >= 1:
            R[3 * (j - 1):3 * j] = B.T
        X = ldlt_apply(F, R)
        M = np.zeros((3, 3))
        for r in range(3):
            for k in range(3):
                m = f64(0.0)
                for node, J in ((i, A), (j, B)):
                    if node >= 1:
                        for q in range(3):
                            m = m + J[r, q] * X[3 * (node - 1) + q, k]
                M[r, k] = m
        Ms = 0.5 * (M + M.T)
        cov = np.array([Ms[0, 0], Ms[0, 1], Ms[0, 2], Ms[1, 1], Ms[1, 2], Ms[2, 2]])
        Sc = ffr.inverse(full3(om))
        if Sc is None:
            return BAD_INFO, 0.0, e, cov
        Si = ffr.inverse(Ms + Sc)
        if Si is None:
            return BAD_INFO, 0.0, e, cov
        w = ffr.mulv(Si, e)
        d2 = (e[0] * w[0] + e[1] * w[1]) + e[2] * w[2]
    return (ACCEPTED if d2 <= nis_max else OUTLIER), float(d2), e, cov


def gate(pose, ij, z, info, cand_ij, cand_z, cand_info, n_nodes=None, n_edges=None, n_cand=None, max_nodes=None,
         max_edges=None, max_cand=None, trace=None, **kw):
    """One graph.  pose [N_cap, 3]; ij [E_cap, 2], z [E_cap, 3], info [E_cap, 6]; cand_ij [C_cap, 2], cand_z [C_cap, 3],
    cand_info [C_cap, 6]; the counts default to all given; trace [N_cap, 2]: the (cos, sin) to use, or None for
    NumPy's.  Returns flags, chi2, trace (NumPy's own), cand_nis [C_cap], cand_err [C_cap, 3], cand_cov [C_cap, 6],
    cand_flags [C_cap], and the edge arrays and n_edges as they stand behind step 4."""
    p = dict(DEFAULTS, **kw)
    pose = np.array(pose, np.float64).reshape(-1, 3)
    ij = np.array(ij, np.int64).reshape(-1, 2)
    z, info = np.array(z, np.float64).reshape(-1, 3), np.array(info, np.float64).reshape(-1, 6)
    cij = np.asarray(cand_ij, np.int64).reshape(-1, 2)
    cz, cinfo = np.asarray(cand_z, np.float64).reshape(-1, 3), np.asarray(cand_info, np.float64).reshape(-1, 6)
    Nc = len(pose) if max_nodes is None else int(max_nodes)
    Ec = len(ij) if max_edges is None else int(max_edges)
    Cc = len(cij) if max_cand is None else int(max_cand)
    N = len(pose) if n_nodes is None else int(n_nodes)
    E = len(ij) if n_edges is None else int(n_edges)
    C = len(cij) if n_cand is None else int(n_cand)
    out = dict(flags=0, chi2=0.0, trace=np.zeros((Nc, 2)), cand_nis=np.zeros(Cc), cand_err=np.zeros((Cc, 3)),
               cand_cov=np.zeros((Cc, 6)), cand_flags=np.zeros(Cc, np.int32), edge_ij=ij, edge_z=z, edge_info=info, n_edges=E)
    if N < 0 or E < 0 or N > Nc or E > Ec or C < 0 or C > Cc:
        out["flags"] = BAD_GRAPH
        return out
    if N < 2 or E == 0:
        out["flags"] = EMPTY
        return out
    bad = np.any(ij[:E, 0] == ij[:E, 1]) or np.any(ij[:E] < 0) or np.any(ij[:E] >= N)
    bad = bad or not (np.isfinite(pose[:N]).all() and np.isfinite(z[:E]).all() and np.isfinite(info[:E]).all())
    if bad:
        out["flags"] = BAD_GRAPH
        return out
    x = pose[:N]
    with np.errstate(all="ignore"):
        own = np.stack([np.cos(x[:, 2]), np.sin(x[:, 2])], 1)
        out["trace"][:N] = own
        cs = own if trace is None else np.asarray(trace, np.float64)[:N]
        t = pg.edge_terms(x, ij[:E], z[:E], info[:E], cs)
        H, g, chi2 = pg.assemble(N, ij[:E], t)
        out["chi2"] = chi2
        Hr, _ = pg.damped(H, g, N, p["damp_t"], p["damp_r"])
        F = ldlt_factor(Hr)
    if F is None:
        out["flags"] = SINGULAR
        return out
    for c in range(C):
        fl, nis, e, cov = judge(x, cs, F, N, int(cij[c, 0]), int(cij[c, 1]), cz[c], cinfo[c], p["nis_max"])
        out["cand_flags"][c], out["cand_nis"][c], out["cand_err"][c], out["cand_cov"][c] = fl, nis, e, cov
    if p["append"]:
        for c in range(C):
            if out["cand_flags"][c] != ACCEPTED:
                continue
            if E < Ec:
                ij[E], z[E], info[E] = cij[c], cz[c], cinfo[c]
                E += 1
                out["cand_flags"][c] |= APPENDED
            else:
                out["cand_flags"][c] |= NO_ROOM
        out["n_edges"] = E
    return out


def dense(pose, ij, z, info, i, j, cz, cinfo, damp_t=1e-6, damp_r=1e-3):
    """The same statistic in dense np.linalg form, for the reference's own test: (d2, J Sigma J^T [3, 3])."""
    N = len(pose)
    cs = np.stack([np.cos(pose[:, 2]), np.sin(pose[:, 2])], 1)
    t = pg.edge_terms(pose, np.asarray(ij), np.asarray(z, np.float64), np.asarray(info, np.float64), cs)
    H, g, _ = pg.assemble(N, np.asarray(ij), t)
    Hr, _ = pg.damped(H, g, N, damp_t, damp_r)
    Hf = np.tril(Hr) + np.tril(Hr, -1).T
    c = pg.edge_terms(pose, np.array([[i, j]]), np.asarray(cz, np.float64)[None], np.asarray(cinfo, np.float64)[None], cs)
    J = np.zeros((3, 3 * N))
    J[:, 3 * i:3 * i + 3], J[:, 3 * j:3 * j + 3] = c["A"][0], c["B"][0]
    J = J[:, 3:]
    M = J @ np.linalg.solve(Hf, J.T)
    S = M + np.linalg.inv(full3(cinfo))
    e = c["e"][0]
    return float(e @ np.linalg.solve(S, e)), M
