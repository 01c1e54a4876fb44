"""NumPy reference of the occupancy-grid update (include/lidarslam.h, lslam_grid_update), written
straight from the definition: the tests hold the kernel to it bit for bit.

All arithmetic is float64, one rounding per operation (NumPy's elementwise ufuncs fuse nothing),
then integers.  One revolution and a pose -> the robot's grid of clamped log-odds:

0. pose, rotation (cos, sin: the device's bits when given, else NumPy's), robot cell, BAD_POSE;
1. valid points within max_range -> hit cells;
2. the integer ray from the robot cell to each hit cell, in closed form per step;
3. the per-revolution sum D of l_miss over free cells and l_hit over hit cells, CLIPPED;
4. one clamped update per call, where D != 0.
"""
import numpy as np

BAD_POSE, CLIPPED = 1, 2

DEFAULTS = dict(cell=20.0, max_range=8000.0, grid_w=512, l_hit=85, l_miss=-41, l_min=-200, l_max=350)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def ray_cells(X0, Y0, X1, Y1):
    """The free cells [n, 2] (x, y) of the ray from the robot cell to the hit cell, and the hit cell."""
    dx, dy = int(X1) - int(X0), int(Y1) - int(Y0)
    n = max(abs(dx), abs(dy))
    i = np.arange(n, dtype=np.int64)
    if n == 0:
        return np.zeros((0, 2), np.int64), (int(X1), int(Y1))
    x = int(X0) + np.sign(dx) * ((2 * i * abs(dx) + n) // (2 * n))
    y = int(Y0) + np.sign(dy) * ((2 * i * abs(dy) + n) // (2 * n))
    return np.stack([x, y], -1), (int(X1), int(Y1))


def hit_cells(xy, pose, rot, origin, p):
    """Steps 0 and 1: (X0, Y0), hit cells [m, 2], n_used (2,); None for a bad pose."""
    inv = 1.0 / float(p["cell"])
    px, py, th = (float(v) for v in pose)
    ox, oy = (float(v) for v in origin)
    with np.errstate(invalid="ignore", over="ignore"):
        X0, Y0 = np.floor((px - ox) * inv), np.floor((py - oy) * inv)
        if not (np.all(np.isfinite([px, py, th, ox, oy])) and abs(X0) < 2.0 ** 20 and abs(Y0) < 2.0 ** 20):
            return None
    c, s = (float(v) for v in rot)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    ok = np.isfinite(x) & np.isfinite(y) & ~((x == 0.0) & (y == 0.0))
    x, y = x[ok], y[ok]
    with np.errstate(over="ignore"):
        far = x * x + y * y > float(p["max_range"]) * float(p["max_range"])
    x, y = x[~far], y[~far]
    wx = px + (c * x - s * y)
    wy = py + (s * x + c * y)
    X1 = np.floor((wx - ox) * inv).astype(np.int64)
    Y1 = np.floor((wy - oy) * inv).astype(np.int64)
    return (int(X0), int(Y0)), np.stack([X1, Y1], -1), np.array([x.size, int(far.sum())], np.int32)


def revolution_sum(X0, Y0, hits, W, l_hit, l_miss):
    """Steps 2 and 3: D [W, W] (int64) and whether some cell of some ray lies outside the grid."""
    D = np.zeros((W, W), np.int64)
    m = len(hits)
    if m == 0:
        return D, False
    dx, dy = hits[:, 0] - X0, hits[:, 1] - Y0
    ax, ay = np.abs(dx), np.abs(dy)
    n = np.maximum(ax, ay)
    ray = np.repeat(np.arange(m), n)                    # the ray of every free cell
    i = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    nn = n[ray]
    x = X0 + np.sign(dx)[ray] * ((2 * i * ax[ray] + nn) // (2 * nn))
    y = Y0 + np.sign(dy)[ray] * ((2 * i * ay[ray] + nn) // (2 * nn))
    ins = (x >= 0) & (x < W) & (y >= 0) & (y < W)
    np.add.at(D, (y[ins], x[ins]), l_miss)
    hin = (hits[:, 0] >= 0) & (hits[:, 0] < W) & (hits[:, 1] >= 0) & (hits[:, 1] < W)
    np.add.at(D, (hits[hin, 1], hits[hin, 0]), l_hit)
    return D, bool((~ins).any() or (~hin).any())


def update(L, xy, pose, rot=None, origin=(0.0, 0.0), **kw):
    """One robot, one call: L [W, W] int16 -> (L', n_used (2,), flags).  rot: the (cos, sin) the
    library wrote for this pose (the definition's input); None: NumPy's."""
    p = params(**kw)
    W = int(p["grid_w"])
    L = np.asarray(L, np.int16).reshape(W, W)
    if rot is None:
        with np.errstate(invalid="ignore"):
            rot = (np.cos(float(pose[2])), np.sin(float(pose[2])))
    h = hit_cells(xy, pose, rot, origin, p)
    if h is None:
        return L.copy(), np.zeros(2, np.int32), BAD_POSE
    (X0, Y0), hits, n_used = h
    D, clipped = revolution_sum(X0, Y0, hits, W, int(p["l_hit"]), int(p["l_miss"]))
    out = np.where(D != 0, np.clip(L.astype(np.int64) + D, int(p["l_min"]), int(p["l_max"])), L).astype(np.int16)
    return out, n_used, CLIPPED if clipped else 0


def update_batch(L, xy, pt_off, pose, rot=None, origin=None, **kw):
    """R robots: L [R, W, W], robot r's points xy[pt_off[r]:pt_off[r+1]]."""
    R = len(pt_off) - 1
    origin = np.zeros((R, 2)) if origin is None else np.asarray(origin, np.float64).reshape(R, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    outs = [update(L[r], xy[pt_off[r]:pt_off[r + 1]], pose[r], None if rot is None else rot[r], origin[r], **kw)
            for r in range(R)]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]),
            np.array([o[2] for o in outs], np.int32))
