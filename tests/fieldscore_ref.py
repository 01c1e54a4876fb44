"""NumPy reference of the field read under a revolution (include/lidarslam.h, lslam_field_score):
occgrid_ref.hit_cells (steps 0 and 1 of lslam_grid_update) plus a look-up in the distance field.  It
is fed the (cos, sin) that the library wrote to rot: those bits are the definition's input.
"""
import numpy as np

import occgrid_ref as ogr

BAD_POSE = 1

DEFAULTS = dict(trunc2=625, near2=4, off2=4096)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def score(d2, xy, pose, rot, origin=(0.0, 0.0), grid=None, **kw):
    """One robot: d2 [W, W] -> (stats (4,) int64, clear2, flags).  grid: the lslam_grid_params that
    differ from the defaults (cell, max_range, grid_w)."""
    q = params(**kw)
    p = ogr.params(**(grid or {}))
    W = int(p["grid_w"])
    d2 = np.asarray(d2).reshape(W, W).astype(np.int64)
    h = ogr.hit_cells(xy, pose, rot, origin, p)
    if h is None:
        return np.zeros(4, np.int64), 0, BAD_POSE
    (X0, Y0), hits, _ = h
    on0 = 0 <= X0 < W and 0 <= Y0 < W
    clear2 = int(d2[Y0, X0]) if on0 else int(q["off2"])
    on = (hits[:, 0] >= 0) & (hits[:, 0] < W) & (hits[:, 1] >= 0) & (hits[:, 1] < W)
    v = np.full(len(hits), int(q["off2"]), np.int64)
    v[on] = d2[hits[on, 1], hits[on, 0]]
    stats = np.array([np.minimum(v, int(q["trunc2"])).sum(), len(v), (v <= int(q["near2"])).sum(), (~on).sum()], np.int64)
    return stats, clear2, 0


def score_batch(d2, xy, pt_off, pose, rot, origin=None, grid=None, **kw):
    """R robots -> (stats [R, 4] int64, clear2 [R] int32, flags [R] int32)."""
    R = len(pt_off) - 1
    origin = np.zeros((R, 2)) if origin is None else np.asarray(origin, np.float64).reshape(R, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    outs = [score(d2[r], xy[pt_off[r]:pt_off[r + 1]], pose[r], rot[r], origin[r], grid, **kw) for r in range(R)]
    return (np.stack([o[0] for o in outs]), np.array([o[1] for o in outs], np.int32),
            np.array([o[2] for o in outs], np.int32))


def clearance_mm(clear2, cell):
    return float(cell) * np.sqrt(np.asarray(clear2, np.float64))


def near_share(stats):
    s = np.asarray(stats, np.int64)
    return np.where(s[:, 1] > 0, s[:, 2] / np.maximum(s[:, 1], 1), 0.0)


def mean_d2(stats):
    s = np.asarray(stats, np.int64)
    return np.where(s[:, 1] > 0, s[:, 0] / np.maximum(s[:, 1], 1), 0.0)
