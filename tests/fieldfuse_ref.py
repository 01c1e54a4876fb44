"""NumPy reference of the field fusion (include/lidarslam.h, lslam_field_fuse), written straight from
the definition on top of fieldalign_ref.align: the tests hold the kernel to it bit for bit.

Steps 0-4 are fieldalign_ref.align's.  Steps 6-11 are NumPy float64 scalars, one rounding per operation,
in the order the comment fixes; the 3 x 3 products and the adjugate are mapfuse_ref's, the same text that
lslam_map_fuse's reference uses.
"""
import math

import numpy as np

import fieldalign_ref as far
import occgrid_ref as ogr
from mapfuse_ref import adjugate, dot3, mul, mulv

OUTLIER, BAD_COV = 64, 128
REJECTED = far.KEEP | OUTLIER | BAD_COV

DEFAULTS = dict(sigma_min=0.5, r_scale=1.0, floor_t=1.0 / math.sqrt(12.0), floor_r=(math.pi / 360.0) / math.sqrt(12.0),
                nis_max=16.27)

f64 = np.float64
SC = f64(1.0 / far.SCALE)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # normal[0..5]


def split(kw):
    """(the fusion's parameters, the rest: fieldalign_ref's)."""
    fp = dict(DEFAULTS)
    rest = {}
    for k, v in kw.items():
        (fp if k in DEFAULTS else rest)[k] = v
    return fp, rest


def inverse(S):
    """The adjugate/determinant inverse of lslam_map_fuse step 7 with its pass test: Si, or None."""
    with np.errstate(all="ignore"):
        A, det = adjugate(S)
        if not (S[0, 0] > 0 and A[2, 2] > 0 and det > 0 and np.isfinite(det)):
            return None
        return A / det


def noise(normal, n_last, fp):
    """Step 6: s2."""
    n = int(n_last)
    with np.errstate(all="ignore"):
        mean = (f64(int(normal[9])) * SC) / f64(n) if n else f64(0.0)
        smin = f64(fp["sigma_min"])
        return f64(max(mean, smin * smin)) * f64(fp["r_scale"])


def information(normal, s2, cell):
    """Step 7: the alignment's information in mm and rad, [3, 3]."""
    inv = f64(1.0) / f64(cell)
    u = (inv, inv, f64(1.0))
    lam = np.zeros((3, 3))
    with np.errstate(all="ignore"):
        for k, (i, j) in enumerate(PAIRS):
            lam[i, j] = lam[j, i] = (((f64(int(normal[k])) * SC) * u[i]) * u[j]) / s2
    return lam


def weights(cell, fp):
    """Step 8's w = (1 / ft, 1 / ft, 1 / fr)."""
    with np.errstate(all="ignore"):
        ft = (f64(fp["floor_t"]) * f64(cell)) * (f64(fp["floor_t"]) * f64(cell))
        fr = f64(fp["floor_r"]) * f64(fp["floor_r"])
        return np.array([f64(1.0) / ft, f64(1.0) / ft, f64(1.0) / fr])


def floored(lam, w):
    """Step 8: the floored information, or None if B has no inverse."""
    with np.errstate(all="ignore"):
        Bi = inverse(lam + np.diag(w))
        if Bi is None:
            return None
        T = mul(lam, Bi)
        E = T * w[None, :]
        return f64(0.5) * (E + E.T)


def posterior(P, lam_f):
    """Step 9: (Pi, Po), or None with BAD_COV."""
    with np.errstate(all="ignore"):
        if lam_f is None or not np.all(np.isfinite(P)):
            return None
        Pi = inverse(P)
        if Pi is None:
            return None
        Mi = inverse(Pi + lam_f)
        if Mi is None:
            return None
        Po = f64(0.5) * (Mi + Mi.T)
        d = np.diag(Po)
        if not (np.all(np.isfinite(d)) and np.all(d > 0)):
            return None
        return Pi, Po


def innovation(x, z, lam_f, Pi, Po):
    """Step 10: (c, nis)."""
    with np.errstate(all="ignore"):
        y = np.array([z[i] - x[i] for i in range(3)])
        c = mulv(Po, mulv(lam_f, y))
        e = mulv(Pi, c)
        return c, dot3(y[0], e[0], y[1], e[1], y[2], e[2])


def fuse_steps(al, pose, P, cell, fp):
    """Steps 5-11 on an alignment al of fieldalign_ref.align (its pose_out, normal, n_used, flags)."""
    pose = np.array(pose, np.float64).reshape(3)
    P = np.array(P, np.float64).reshape(3, 3)
    flags = int(al["flags"])
    out = dict(al)
    out.update(z=np.array(al["pose_out"], np.float64), pose_out=pose.copy(), P_out=P.copy(), info=np.zeros((3, 3)),
               info_f=np.zeros((3, 3)), s2=f64(0.0), nis=f64(0.0), flags=flags)
    if flags & far.KEEP:
        return out
    z = out["z"]
    s2 = noise(al["normal"], al["n_used"][1], fp)
    lam = information(al["normal"], s2, cell)
    lam_f = floored(lam, weights(cell, fp))
    out.update(s2=s2, info=lam, info_f=np.zeros((3, 3)) if lam_f is None else lam_f)
    post = posterior(P, lam_f)
    if post is None:
        out["flags"] = flags | BAD_COV
        return out
    Pi, Po = post
    c, nis = innovation(pose, z, lam_f, Pi, Po)
    out["nis"] = f64(nis)
    if not (nis <= f64(fp["nis_max"])):
        out["flags"] = flags | OUTLIER
        return out
    with np.errstate(all="ignore"):
        out.update(pose_out=np.array([pose[i] + c[i] for i in range(3)]), P_out=Po)
    return out


def fuse(d2, xy, pose, P, cs=None, origin=(0.0, 0.0), grid=None, **kw):
    """One robot.  Returns fieldalign_ref.align's dict with pose_out and flags as the fusion defines them,
    plus z [3], info [3, 3], info_f [3, 3], s2, nis, P_out [3, 3].  cs: the device's (cos, sin), as align's."""
    fp, rest = split(kw)
    al = far.align(d2, xy, pose, cs, origin, grid, **rest)
    return fuse_steps(al, pose, P, float(ogr.params(**(grid or {}))["cell"]), fp)


def fuse_batch(d2, xy, pt_off, pose, P, trace=None, origin=None, grid=None, **kw):
    """R robots -> dict of stacked arrays.  trace: the device's, for its (cos, sin)."""
    R = len(pt_off) - 1
    origin = np.zeros((R, 2)) if origin is None else np.asarray(origin, np.float64).reshape(R, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    P = np.asarray(P, np.float64).reshape(R, 3, 3)
    outs = [fuse(d2[r], xy[pt_off[r]:pt_off[r + 1]], pose[r], P[r], None if trace is None else trace[r][:, 3:5], origin[r],
                 grid, **kw) for r in range(R)]
    keys = ("pose_out", "P_out", "z", "info", "info_f", "s2", "nis", "trace", "normal", "n_used", "iters", "flags")
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in keys}
