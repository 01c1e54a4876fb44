"""NumPy form of the definition of a map read as a revolution (include/lidarslam.h, lslam_grid_points):
FP64 in the written operation order (no fused product: NumPy's element-wise operations round one by one),
then integers.  np.nonzero walks a [W, W] mask in row-major order, Y outer and X inner: the definition's
order.  The kernels (lidar_slam_amd/csrc/lslam_gridpoints.h) match it bit for bit in xy, pt_off, counts
and flags."""
import numpy as np

BAD_ANCHOR, EMPTY, DECIMATED = 1, 2, 4
DEFAULTS = dict(cell=20.0, radius=8000.0, occ_min=85, cap=1024)
COUNTS = ("n_occ", "n_in", "stride", "n_out")


def anchor_of(pose):
    """(ax, ay, cos theta, sin theta) of a pose (x, y, theta), or [n, 4] of [n, 3]: the caller's bits."""
    p = np.asarray(pose, np.float64)
    return np.stack([p[..., 0], p[..., 1], np.cos(p[..., 2]), np.sin(p[..., 2])], -1)


def points(L, origin, anchor, **kw):
    """One robot: {"xy" [cap, 2] float64, "counts" [4] int32, "flags"}."""
    p = dict(DEFAULTS, **kw)
    cap = int(p["cap"])
    L = np.asarray(L, np.int16)
    W = L.shape[0]
    xy = np.zeros((cap, 2), np.float64)
    counts = np.zeros(4, np.int32)
    ox, oy = (np.float64(v) for v in origin)
    ax, ay, c, s = (np.float64(v) for v in anchor)
    if not np.all(np.isfinite([ox, oy, ax, ay, c, s])):
        return {"xy": xy, "counts": counts, "flags": BAD_ANCHOR}
    cell, radius = np.float64(p["cell"]), np.float64(p["radius"])
    r2 = radius * radius
    Y, X = np.nonzero(L >= p["occ_min"])
    with np.errstate(over="ignore", invalid="ignore"):
        wx = ox + (X.astype(np.float64) + 0.5) * cell
        wy = oy + (Y.astype(np.float64) + 0.5) * cell
        dx, dy = wx - ax, wy - ay
        d2 = dx * dx + dy * dy
        inr = (d2 > 0.0) & (d2 <= r2)
        dx, dy = dx[inr], dy[inr]
        n_in = int(inr.sum())
        stride = max(1, (n_in + cap - 1) // cap)
        n_out = (n_in + stride - 1) // stride
        dx, dy = dx[::stride], dy[::stride]
        assert len(dx) == n_out <= cap
        xy[:n_out, 0] = (c * dx) + (s * dy)
        xy[:n_out, 1] = (c * dy) - (s * dx)
    counts[:] = [len(X), n_in, stride, n_out]
    return {"xy": xy, "counts": counts, "flags": (EMPTY if n_out == 0 else 0) | (DECIMATED if stride > 1 else 0)}


def points_batch(L, origin, anchor, **kw):
    """The batch form of the C ABI: L [R, W, W], origin [R, 2], anchor [R, 4] ->
    {"xy" [R, cap, 2], "pt_off" [R + 1] int32, "counts" [R, 4], "flags" [R]}."""
    R = len(L)
    cap = int(dict(DEFAULTS, **kw)["cap"])
    out = {"xy": np.zeros((R, cap, 2)), "pt_off": (np.arange(R + 1, dtype=np.int64) * cap).astype(np.int32),
           "counts": np.zeros((R, 4), np.int32), "flags": np.zeros(R, np.int32)}
    for r in range(R):
        q = points(L[r], origin[r], anchor[r], **kw)
        out["xy"][r], out["counts"][r], out["flags"][r] = q["xy"], q["counts"], q["flags"]
    return out


def as_revolution(q):
    """The valid points of one robot's result [n_out, 2]: what a host consumer is given as a revolution."""
    return q["xy"][:int(q["counts"][3])]
