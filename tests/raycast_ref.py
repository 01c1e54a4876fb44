"""NumPy reference of grid ray casting (include/lidarslam.h, lslam_grid_raycast), written straight
from the definition and independently of the kernel's header: the tests hold the kernel to it bit
for bit.

All arithmetic is float64, one rounding per operation (NumPy's elementwise ufuncs fuse nothing),
then integers.  One revolution, a pose and the robot's grid -> per beam where the map stops it:

0. pose, rotation (cos, sin: the device's bits when given, else NumPy's), robot cell, BAD_POSE;
1. valid points, beyond points, the measured step i_m;
2. the far cell of every beam, one division per point;
3. the walk: a plain loop over the steps i = 0, 1, ..., every beam that is still walking tested at
   its step i by the closed form of the offset (no carried remainder);
4. the class from (kind, i_h, i_m, tol), in integers;
5. counts.
"""
import numpy as np

BAD_POSE = 1
INVALID, MATCH, NOVEL, THROUGH, UNMAPPED = 0, 1, 2, 3, 4
NONE, UNKNOWN, OCC = 0, 1, 2
CLASS_NAMES = ("INVALID", "MATCH", "NOVEL", "THROUGH", "UNMAPPED")

DEFAULTS = dict(occ_min=1, free_max=-1, tol=3)
GRID_DEFAULTS = dict(cell=20.0, max_range=8000.0, grid_w=512)


def params(**kw):
    p = dict(GRID_DEFAULTS)
    p.update(DEFAULTS)
    p.update({k: v for k, v in kw.items() if k in p})
    return p


def _cells(px, py, c, s, ox, oy, inv, x, y):
    """lslam_grid_update step 1: the cell of robot-frame points, as doubles."""
    wx = px + (c * x - s * y)
    wy = py + (s * x + c * y)
    return np.floor((wx - ox) * inv), np.floor((wy - oy) * inv)


def cast(L, xy, pose, rot=None, origin=(0.0, 0.0), **kw):
    """One robot: L [W, W] int16 -> (cls uint8 [n], stop int32 [n, 3], counts int32 [8], flags).
    rot: the (cos, sin) the library wrote for this pose (the definition's input); None: NumPy's."""
    p = params(**kw)
    W = int(p["grid_w"])
    L = np.asarray(L, np.int16).reshape(W, W)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    N = len(xy)
    cls = np.zeros(N, np.uint8)
    stop = np.zeros((N, 3), np.int32)
    counts = np.zeros(8, np.int32)
    cell, max_range = float(p["cell"]), float(p["max_range"])
    occ_min, free_max, tol = int(p["occ_min"]), int(p["free_max"]), int(p["tol"])
    inv = 1.0 / cell
    px, py, th = (float(v) for v in pose)
    ox, oy = (float(v) for v in origin)
    if rot is None:
        with np.errstate(invalid="ignore"):
            rot = (np.cos(th), np.sin(th))
    c, s = (float(v) for v in rot)
    # ---- 0 ----
    with np.errstate(invalid="ignore", over="ignore"):
        X0d, Y0d = np.floor((px - ox) * inv), np.floor((py - oy) * inv)
        if not (np.all(np.isfinite([px, py, th, ox, oy])) and abs(X0d) < 2.0 ** 20 and abs(Y0d) < 2.0 ** 20):
            return cls, stop, counts, BAD_POSE
    X0, Y0 = int(X0d), int(Y0d)
    # ---- 1 ----
    x, y = xy[:, 0], xy[:, 1]
    valid = np.isfinite(x) & np.isfinite(y) & ~((x == 0.0) & (y == 0.0))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        beyond = valid & (x * x + y * y > max_range * max_range)
        # ---- 2 ----
        m = np.maximum(np.abs(x), np.abs(y))
        far = max_range + 2.0 * cell
        q = far / m
        XFd, YFd = _cells(px, py, c, s, ox, oy, inv, x * q, y * q)
        Dxd, Dyd = XFd - X0d, YFd - Y0d
        valid &= np.isfinite(Dxd) & np.isfinite(Dyd) & (np.abs(Dxd) <= 8192.0) & (np.abs(Dyd) <= 8192.0)
    beyond &= valid
    idx = np.flatnonzero(valid)
    if idx.size:
        Dx, Dy = Dxd[idx].astype(np.int64), Dyd[idx].astype(np.int64)
        adx, ady = np.abs(Dx), np.abs(Dy)
        n = np.maximum(adx, ady)
        # the measured step (beyond: +infinity)
        near = ~beyond[idx]
        i_m = np.full(idx.size, np.iinfo(np.int64).max // 4, np.int64)
        X1d, Y1d = _cells(px, py, c, s, ox, oy, inv, x[idx][near], y[idx][near])
        i_m[near] = np.maximum(np.abs(X1d.astype(np.int64) - X0), np.abs(Y1d.astype(np.int64) - Y0))
        # ---- 3 ----
        Rc = int(np.floor(max_range * inv))
        kind = np.full(idx.size, NONE, np.int64)
        i_h = n + 1
        sox, soy = np.zeros(idx.size, np.int64), np.zeros(idx.size, np.int64)
        walking = np.ones(idx.size, bool)
        n2 = np.maximum(2 * n, 1)
        for i in range(int(n.max()) + 1):
            w = np.flatnonzero(walking & (n >= i))
            if w.size == 0:
                break
            ofx = np.sign(Dx[w]) * ((2 * i * adx[w] + n[w]) // n2[w])
            ofy = np.sign(Dy[w]) * ((2 * i * ady[w] + n[w]) // n2[w])
            sox[w], soy[w] = ofx, ofy  # (a ray that nothing stops keeps the offset of step n)
            X, Y = X0 + ofx, Y0 + ofy
            on = (X >= 0) & (X < W) & (Y >= 0) & (Y < W)
            l = np.zeros(w.size, np.int64)
            l[on] = L[Y[on], X[on]]
            out = ofx * ofx + ofy * ofy > Rc * Rc
            occ = ~out & on & (l >= occ_min)
            unk = ~out & ~occ & ~(on & (l <= free_max))
            stopped = out | occ | unk
            kind[w[occ]] = OCC
            kind[w[unk]] = UNKNOWN
            i_h[w[stopped]] = i
            walking[w[stopped]] = False
        # ---- 4 ----
        early, late = i_m < i_h - tol, i_m > i_h + tol
        k_occ = np.where(early, NOVEL, np.where(late, THROUGH, MATCH))
        k_unk = np.where(early, NOVEL, UNMAPPED)
        k_none = np.where(early, NOVEL, MATCH)  # (a beyond point's i_m is never early)
        klass = np.where(kind == OCC, k_occ, np.where(kind == UNKNOWN, k_unk, k_none))
        cls[idx] = (klass | (kind << 4)).astype(np.uint8)
        stop[idx] = np.stack([sox, soy, i_h], -1).astype(np.int32)
        counts[6] = int(np.sum(kind == NONE))
    # ---- 5 ----
    for k in range(5):
        counts[k] = int(np.sum((cls & 15) == k))
    counts[5] = int(beyond.sum())
    return cls, stop, counts, 0


def cast_batch(L, xy, pt_off, pose, rot=None, origin=None, **kw):
    """R robots: L [R, W, W], robot r's points xy[pt_off[r]:pt_off[r+1]] -> (cls [P], stop [P, 3],
    counts [R, 8], flags [R])."""
    R = len(pt_off) - 1
    origin = np.zeros((R, 2)) if origin is None else np.asarray(origin, np.float64).reshape(R, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    outs = [cast(L[r], xy[pt_off[r]:pt_off[r + 1]], pose[r], None if rot is None else rot[r], origin[r], **kw)
            for r in range(R)]
    return (np.concatenate([o[0] for o in outs] + [np.zeros(0, np.uint8)]),
            np.concatenate([o[1] for o in outs] + [np.zeros((0, 3), np.int32)]),
            np.stack([o[2] for o in outs]), np.array([o[3] for o in outs], np.int32))


def expected_range(cls, stop, cell):
    """cell hypot(ox, oy) where the kind is OCC, inf elsewhere."""
    stop = np.asarray(stop, np.float64)
    return np.where((np.asarray(cls) >> 4) == OCC, cell * np.hypot(stop[:, 0], stop[:, 1]), np.inf)


def inconsistency(counts):
    """(NOVEL + THROUGH) / valid points that are not beyond, per robot; 0 where there are none."""
    counts = np.asarray(counts, np.int64).reshape(-1, 8)
    den = counts[:, 1:5].sum(1) - counts[:, 5]
    return np.where(den > 0, (counts[:, NOVEL] + counts[:, THROUGH]) / np.maximum(den, 1), 0.0)
