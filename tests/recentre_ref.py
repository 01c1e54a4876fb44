"""NumPy reference of the grid recentre (include/lidarslam.h, lslam_grid_recentre), written straight
from the definition: the tests hold the kernel to it bit for bit.

All arithmetic is float64, one rounding per operation (NumPy scalars fuse nothing), then integers.
A pose and an origin -> a whole-cell shift, the new origin and the shifted grid:

0. robot cell (X0, Y0), BAD_POSE (the condition of occgrid_ref.hit_cells);
1. the shift: none while the robot cell keeps `margin` cells from every edge, else both axes go
   back to the middle in multiples of `quantum`;
2. a zero shift changes nothing;
3. origin' = origin + s * cell, two roundings; BAD_POSE when it is not finite;
4. L'[y][x] = L[y + sy][x + sx] on the map, 0 elsewhere, as 16-bit patterns; MOVED, CLEARED.
"""
import numpy as np

BAD_POSE, MOVED, CLEARED = 1, 2, 4

DEFAULTS = dict(margin=128, quantum=8)
GRID_DEFAULTS = dict(cell=20.0, grid_w=512)
BAND_CELLS = 16384  # lslam_recentre_plan.h RECENTRE_BAND_CELLS


def params(**kw):
    """margin, quantum and the two the call takes from the grid's parameters (cell, grid_w); the
    grid's other parameters are accepted and ignored."""
    p = dict(GRID_DEFAULTS)
    p.update(DEFAULTS)
    p.update({k: v for k, v in kw.items() if k in p})
    return p


def band_rows(grid_w):
    """lslam_recentre_plan.h recentre_band_rows."""
    return max(1, min(int(grid_w), BAND_CELLS // int(grid_w)))


def axis_shift(c, W, quantum):
    """Step 1 for one axis once the margin has triggered (Python's // rounds toward minus infinity)."""
    return int(quantum) * ((int(c) - int(W) // 2 + int(quantum) // 2) // int(quantum))


def shift_of(X0, Y0, W, margin, quantum):
    """Step 1: (sx, sy) of a robot cell."""
    if margin <= X0 < W - margin and margin <= Y0 < W - margin:
        return 0, 0
    return axis_shift(X0, W, quantum), axis_shift(Y0, W, quantum)


def shifted(L, sx, sy):
    """Step 4 for one grid, out of place."""
    L = np.asarray(L, np.int16)
    W = L.shape[0]
    out = np.zeros_like(L)
    if abs(sx) >= W or abs(sy) >= W:
        return out
    y0, y1 = max(0, -sy), min(W, W - sy)
    x0, x1 = max(0, -sx), min(W, W - sx)
    out[y0:y1, x0:x1] = L[y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def recentre(L, pose, origin, **kw):
    """One robot: L [W, W] int16 -> (L', origin' (2,) float64, shift (2,) int32, flags)."""
    p = params(**kw)
    W, margin, quantum = int(p["grid_w"]), int(p["margin"]), int(p["quantum"])
    cell = np.float64(p["cell"])
    inv = np.float64(1.0) / cell
    L = np.asarray(L, np.int16).reshape(W, W)
    pose = np.asarray(pose, np.float64).reshape(3)
    origin = np.asarray(origin, np.float64).reshape(2)
    bad = (L.copy(), origin.copy(), np.zeros(2, np.int32), BAD_POSE)
    with np.errstate(invalid="ignore", over="ignore"):
        X0 = np.floor((pose[0] - origin[0]) * inv)
        Y0 = np.floor((pose[1] - origin[1]) * inv)
        if not (np.all(np.isfinite(pose)) and np.all(np.isfinite(origin)) and abs(X0) < 2.0 ** 20 and abs(Y0) < 2.0 ** 20):
            return bad
        sx, sy = shift_of(int(X0), int(Y0), W, margin, quantum)
        if sx == 0 and sy == 0:
            return L.copy(), origin.copy(), np.zeros(2, np.int32), 0
        new = np.array([origin[0] + np.float64(sx) * cell, origin[1] + np.float64(sy) * cell], np.float64)
    if not np.all(np.isfinite(new)):
        return bad
    flags = MOVED | (CLEARED if abs(sx) >= W or abs(sy) >= W else 0)
    return shifted(L, sx, sy), new, np.array([sx, sy], np.int32), flags


def recentre_batch(L, pose, origin, **kw):
    """R robots: L [R, W, W], pose [R, 3], origin [R, 2] -> (L', origin', shift [R, 2], flags [R])."""
    pose = np.asarray(pose, np.float64).reshape(-1, 3)
    R = len(pose)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    outs = [recentre(L[r], pose[r], origin[r], **kw) for r in range(R)]
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs]),
            np.array([o[3] for o in outs], np.int32))


def pose_for_shift(origin, cell, W, sx, sy):
    """A pose (x, y) on the centre of the robot cell that, with margin = W / 2 and quantum = 1, gives
    exactly the shift (sx, sy) != (0, 0): the cell (W / 2 + sx, W / 2 + sy)."""
    origin = np.asarray(origin, np.float64)
    return origin + (np.array([W // 2 + sx, W // 2 + sy], np.float64) + 0.5) * cell
