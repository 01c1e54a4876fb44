"""NumPy reference of the distance field (include/lidarslam.h, lslam_grid_distance): the tests hold
the kernel to it bit for bit.  All integers.

``field`` is the separable form: a column pass (the distance to the column's nearest source, saturated
at d_max) and a row pass written as at most 2 d_max - 1 shifted whole-array minima.  ``brute`` is the
definition as written, the minimum over all source cells; tests/test_dist_ref.py holds the two
together.
"""
import numpy as np

OCC, NOT_FREE = 0, 1
EMPTY = 1

DEFAULTS = dict(mode=OCC, occ_min=85, free_max=-1, d_max=64)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def sources(L, p):
    """bool [W, W]: the source cells on the map."""
    L = np.asarray(L, np.int16).astype(np.int64)
    return L > int(p["free_max"]) if int(p["mode"]) == NOT_FREE else L >= int(p["occ_min"])


def border2(W):
    """[W, W]: b b, b = min(x + 1, W - x, y + 1, W - y): the squared distance to the nearest cell off the map."""
    i = np.arange(W, dtype=np.int64)
    b1 = np.minimum(i + 1, W - i)
    b = np.minimum(b1[None, :], b1[:, None])
    return b * b


def column_g(src, d_max):
    """[W, W] int64: the distance to the nearest source of the same column, saturated at d_max."""
    W = src.shape[0]
    y = np.arange(W, dtype=np.int64)[:, None]
    far = np.int64(4 * W + 4 * d_max)
    last = np.maximum.accumulate(np.where(src, y, -far), axis=0)            # nearest source at or above
    nxt = np.minimum.accumulate(np.where(src, y, far)[::-1], axis=0)[::-1]  # at or below
    return np.minimum(np.minimum(y - last, nxt - y), d_max)


def row_d2(g, d_max):
    """[W, W] int64: min over |x - x'| < d_max of (x - x')^2 + g[y][x']^2, saturated at d_max^2."""
    W = g.shape[1]
    cap = np.int64(d_max) * d_max
    g2 = np.where(g >= d_max, cap, g * g)
    out = g2.copy()
    for s in range(1, min(int(d_max), W)):
        np.minimum(out[:, s:], g2[:, :-s] + s * s, out=out[:, s:])
        np.minimum(out[:, :-s], g2[:, s:] + s * s, out=out[:, :-s])
    return np.minimum(out, cap)


def field(L, **kw):
    """One robot: L [W, W] int16 -> (d2 [W, W] uint16, n_src, flags)."""
    p = params(**kw)
    d_max = int(p["d_max"])
    src = sources(L, p)
    d2 = row_d2(column_g(src, d_max), d_max)
    if int(p["mode"]) == NOT_FREE:
        d2 = np.minimum(d2, border2(src.shape[0]))
    n = int(src.sum())
    return d2.astype(np.uint16), n, EMPTY if n == 0 else 0


def brute(L, rows=None, **kw):
    """The definition as written: per cell the minimum over all source cells (rows: only these rows of
    the field, for a large map).  Returns d2 [len(rows), W] int64."""
    p = params(**kw)
    d_max = int(p["d_max"])
    cap = d_max * d_max
    src = sources(L, p)
    W = src.shape[0]
    rows = np.arange(W) if rows is None else np.asarray(rows)
    sy, sx = np.nonzero(src)
    x = np.arange(W, dtype=np.int64)
    out = np.full((len(rows), W), cap, np.int64)
    if len(sx):
        for i, y in enumerate(rows):
            d = (x[:, None] - sx[None, :]) ** 2 + (int(y) - sy[None, :]) ** 2
            out[i] = np.minimum(d.min(1), cap)
    if int(p["mode"]) == NOT_FREE:
        out = np.minimum(out, border2(W)[rows])
    return out


def field_batch(L, **kw):
    """R robots: L [R, W, W] -> (d2 [R, W, W] uint16, n_src [R] int32, flags [R] int32)."""
    outs = [field(Lr, **kw) for Lr in L]
    return (np.stack([o[0] for o in outs]), np.array([o[1] for o in outs], np.int32),
            np.array([o[2] for o in outs], np.int32))
