"""NumPy reference of the match fusion (include/lidarslam.h, lslam_map_fuse), written straight from
the definition on top of mapmatch_ref.match: the tests hold the kernel to it bit for bit.

Steps 0-4 are mapmatch_ref.match's.  The moments of step 5 are Python ints (exact); steps 6-8 are
NumPy float64 scalars, one rounding per operation, in the order the comment fixes.
"""
import numpy as np

import mapmatch_ref as mmr

EMPTY, EDGE, BAD_POSE, WEAK, OUTLIER, BAD_COV = 1, 2, 4, 8, 16, 32

DEFAULTS = dict(r_scale=1.0, nis_max=16.27, cut_permille=900)

f64 = np.float64


def split(kw):
    """(the fusion's parameters, the rest: mapmatch_ref's)."""
    fp = dict(DEFAULTS)
    rest = {}
    for k, v in kw.items():
        (fp if k in DEFAULTS else rest)[k] = v
    return fp, rest


def moments(S, best, cut_permille):
    """Step 5: ten Python ints (W, a, b, c, aa, ab, ac, bb, bc, cc) about the winner best = (k, jy, jx, s0)."""
    ks, jys, jxs, s0 = (int(v) for v in best)
    cut = (s0 * int(cut_permille)) // 1000
    w = np.maximum(S.astype(np.int64) - cut, 0).astype(object)  # exact integers of any size
    Nth, Nt = S.shape[0], S.shape[1]
    c, b, a = np.meshgrid(np.arange(Nth) - ks, np.arange(Nt) - jys, np.arange(Nt) - jxs, indexing="ij")
    a, b, c = a.astype(object), b.astype(object), c.astype(object)
    return [int((w * t).sum()) for t in (1 + 0 * a, a, b, c, a * a, a * b, a * c, b * b, b * c, c * c)]


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def mul(A, B, tb=False):
    """A B, or A B^T: every element (t0 + t1) + t2."""
    C = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            col = B[j, :] if tb else B[:, j]
            C[i, j] = dot3(A[i, 0], col[0], A[i, 1], col[1], A[i, 2], col[2])
    return C


def mulv(M, v):
    return np.array([dot3(M[i, 0], v[0], M[i, 1], v[1], M[i, 2], v[2]) for i in range(3)])


def match_cov(mo, cell, theta_step, r_scale):
    """Step 6: Rm [3, 3]."""
    Wd = f64(mo[0])
    mean = [f64(mo[1]) / Wd, f64(mo[2]) / Wd, f64(mo[3]) / Wd]
    sc = [f64(cell), f64(cell), f64(theta_step)]
    m2 = {(0, 0): mo[4], (0, 1): mo[5], (0, 2): mo[6], (1, 1): mo[7], (1, 2): mo[8], (2, 2): mo[9]}
    Rm = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            c = f64(m2[i, j]) / Wd - mean[i] * mean[j]
            v = (c * sc[i]) * sc[j]
            if i == j:
                v = v + (sc[i] * sc[i]) / f64(12.0)
            v = v * f64(r_scale)
            Rm[i, j] = Rm[j, i] = v
    return Rm


def adjugate(S):
    """Step 7: the adjugate of S, entries p q - r s, and det."""
    A = np.zeros((3, 3))
    A[0, 0] = S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]
    A[0, 1] = S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]
    A[0, 2] = S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]
    A[1, 0] = S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]
    A[1, 1] = S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]
    A[1, 2] = S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]
    A[2, 0] = S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]
    A[2, 1] = S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]
    A[2, 2] = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    det = (S[0, 0] * A[0, 0] + S[0, 1] * A[1, 0]) + S[0, 2] * A[2, 0]
    return A, det


def gate(P, Rm, y):
    """Step 7: (Si or None when BAD_COV, nis)."""
    with np.errstate(all="ignore"):
        S = P + Rm
        A, det = adjugate(S)
        if not np.all(np.isfinite(P)) or not (S[0, 0] > 0 and A[2, 2] > 0 and det > 0 and np.isfinite(det)):
            return None, f64(0.0)
        Si = A / det
        v = mulv(Si, y)
        return Si, dot3(y[0], v[0], y[1], v[1], y[2], v[2])


def update(x, P, Rm, Si, y):
    """Step 8: (x', P'), Joseph form."""
    with np.errstate(all="ignore"):
        K = mul(P, Si)
        Ky = mulv(K, y)
        x1 = np.array([x[i] + Ky[i] for i in range(3)])
        IK = np.eye(3) - K
        U = mul(mul(IK, P), IK, tb=True)
        V = mul(mul(K, Rm), K, tb=True)
        T = U + V
        return x1, f64(0.5) * (T + T.T)


def fuse_steps(m, pose, P, p, fp):
    """Steps 5-8 on a match result m of mapmatch_ref.match (its flags, best, delta, scores)."""
    pose = np.array(pose, np.float64).reshape(3)
    P = np.array(P, np.float64).reshape(3, 3)
    flags = int(m["flags"])
    out = dict(m)
    if flags & (EMPTY | BAD_POSE):
        out.update(pose_out=pose.copy(), P_out=P.copy(), z=pose.copy(), Rm=np.zeros((3, 3)), nis=f64(0.0),
                   moments=np.zeros(10, np.int64), flags=flags)
        return out
    mo = moments(m["scores"], m["best"], fp["cut_permille"])
    Rm = match_cov(mo, p["cell"], p["theta_step"], fp["r_scale"])
    y = np.array(m["delta"], np.float64)
    z = np.array([pose[i] + y[i] for i in range(3)])
    Si, nis = gate(P, Rm, y)
    if Si is None:
        flags |= BAD_COV
    elif not (nis <= f64(fp["nis_max"])):
        flags |= OUTLIER
    if flags & (WEAK | BAD_COV | OUTLIER):
        x1, P1 = pose.copy(), P.copy()
    else:
        x1, P1 = update(pose, P, Rm, Si, y)
    out.update(pose_out=x1, P_out=P1, z=z, Rm=Rm, nis=f64(nis), moments=np.array(mo, np.int64), flags=flags)
    return out


def fuse(L, origin, pose, P, xy, rot0=None, rot=None, **kw):
    """One robot.  Returns mapmatch_ref.match's dict with pose_out and flags as the fusion defines them,
    plus P_out [3, 3], z [3], Rm [3, 3], nis, moments [10] (int64)."""
    fp, rest = split(kw)
    m = mmr.match(L, origin, pose, xy, rot0, rot, **rest)
    return fuse_steps(m, pose, P, mmr.params(**rest), fp)


def fuse_batch(L, origin, pose, P, xy, pt_off, rot0=None, rot=None, **kw):
    """The batch form of the C ABI; stacked results (without G)."""
    R = len(pt_off) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    P = np.asarray(P, np.float64).reshape(R, 3, 3)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    rs = [fuse(L[r], origin[r], pose[r], P[r], xy[pt_off[r]:pt_off[r + 1]], None if rot0 is None else rot0[r], rot, **kw)
          for r in range(R)]
    keys = ("pose_out", "P_out", "z", "Rm", "nis", "moments", "delta", "best", "n_valid", "rot0", "scores")
    out = {k: np.stack([r[k] for r in rs]) for k in keys}
    out["flags"] = np.array([r["flags"] for r in rs], np.int32)
    return out
