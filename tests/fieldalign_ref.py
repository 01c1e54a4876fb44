"""NumPy reference of the Gauss-Newton alignment in the distance field (include/lidarslam.h,
lslam_field_align), written straight from the definition: float64 with one rounding per operation
(NumPy's elementwise ufuncs and Python's floats fuse nothing), math.isqrt for a corner's distance,
int64 for the sums.  It is fed the (cos, sin) that the library wrote to trace: those bits are the
definition's input; without them it takes NumPy's.
"""
import math

import numpy as np

import occgrid_ref as ogr

BAD_POSE, CONVERGED, SINGULAR, FEW, DIVERGED, WEAK = 1, 2, 4, 8, 16, 32
KEEP = BAD_POSE | SINGULAR | FEW | DIVERGED | WEAK
S = 20
SCALE = float(2 ** S)

DEFAULTS = dict(trunc=25.0, damp_t=1.0, damp_r=100.0, eps_t=0.01, eps_r=1e-4, max_shift=200.0, max_turn=0.1,
                n_iter=10, min_points=16, min_permille=500)

# dq(w) = isqrt(65536 w) / 256.0 for every uint16
DQ = np.array([math.isqrt(65536 * w) for w in range(65536)], np.float64) / 256.0


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def used_points(xy, max_range):
    """Steps 0-1 of lslam_grid_update: the valid points that are not beyond, (x, y)."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    ok = np.isfinite(x) & np.isfinite(y) & ~((x == 0.0) & (y == 0.0))
    x, y = x[ok], y[ok]
    with np.errstate(over="ignore"):
        far = x * x + y * y > float(max_range) * float(max_range)
    return x[~far], y[~far]


def point_terms(d2, x, y, px, py, c, s, ox, oy, inv, trunc):
    """One evaluation's points -> a dict of per-point arrays over the points whose four corners lie on the
    map: rx, ry, ix, iy, fu, fv, the corner values v00, v10, v01, v11, m, gx, gy, jt, used (m <= trunc)
    and terms [n, 10] int64 (zeros where not used)."""
    W = d2.shape[0]
    px, py, c, s, ox, oy, inv = (np.float64(v) for v in (px, py, c, s, ox, oy, inv))
    with np.errstate(invalid="ignore", over="ignore"):
        rx = c * x - s * y
        ry = s * x + c * y
        wx = px + rx
        wy = py + ry
        u = (wx - ox) * inv - 0.5
        v = (wy - oy) * inv - 0.5
        iu, iv = np.floor(u), np.floor(v)
        on = (iu >= 0.0) & (iu <= W - 2.0) & (iv >= 0.0) & (iv <= W - 2.0)
    rx, ry, u, v, iu, iv = (a[on] for a in (rx, ry, u, v, iu, iv))
    ix, iy = iu.astype(np.int64), iv.astype(np.int64)
    fu, fv = u - iu, v - iv
    v00, v10, v01, v11 = d2[iy, ix], d2[iy, ix + 1], d2[iy + 1, ix], d2[iy + 1, ix + 1]
    d00, d10, d01, d11 = DQ[v00], DQ[v10], DQ[v01], DQ[v11]
    e0, e1 = d10 - d00, d11 - d01
    a0, a1 = d00 + fu * e0, d01 + fu * e1
    gy = a1 - a0
    m = a0 + fv * gy
    gx = e0 + fv * (e1 - e0)
    jt = (gy * rx - gx * ry) * inv
    used = ~(m > np.float64(trunc))
    prods = np.stack([gx * gx, gx * gy, gx * jt, gy * gy, gy * jt, jt * jt, gx * m, gy * m, jt * m, m * m], -1)
    terms = np.rint(prods * SCALE).astype(np.int64)
    terms[~used] = 0
    return dict(rx=rx, ry=ry, ix=ix, iy=iy, fu=fu, fv=fv, v00=v00, v10=v10, v01=v01, v11=v11, m=m, gx=gx, gy=gy,
                jt=jt, used=used, terms=terms)


def evaluate(d2, x, y, px, py, c, s, ox, oy, inv, trunc):
    """-> (N: ten Python ints as int64 would hold them, points used)."""
    t = point_terms(d2, x, y, px, py, c, s, ox, oy, inv, trunc)
    with np.errstate(over="ignore"):
        N = t["terms"].sum(0, dtype=np.int64)
    return [int(v) for v in N], int(t["used"].sum())


def _good(d):
    return d > 0.0 and d < math.inf


def solve(N, damp_t, damp_r):
    """Step 2: -> ((dx, dy, dt), ok).  Python floats: one rounding per operation."""
    sc = 1.0 / SCALE
    h00, h01, h02 = float(N[0]) * sc + damp_t, float(N[1]) * sc, float(N[2]) * sc
    h11, h12, h22 = float(N[3]) * sc + damp_t, float(N[4]) * sc, float(N[5]) * sc + damp_r
    g0, g1, g2 = float(N[6]) * sc, float(N[7]) * sc, float(N[8]) * sc
    d0 = h00
    if not _good(d0):
        return (0.0, 0.0, 0.0), False
    l10, l20 = h01 / d0, h02 / d0
    d1 = h11 - l10 * h01
    if not _good(d1):
        return (0.0, 0.0, 0.0), False
    t21 = h12 - l20 * h01
    l21 = t21 / d1
    d2 = (h22 - l20 * h02) - l21 * t21
    if not _good(d2):
        return (0.0, 0.0, 0.0), False
    y0 = g0
    y1 = g1 - l10 * y0
    y2 = (g2 - l20 * y0) - l21 * y1
    z0, z1, z2 = y0 / d0, y1 / d1, y2 / d2
    x2 = z2
    x1 = z1 - l21 * x2
    x0 = (z0 - l10 * x1) - l20 * x2
    return (-x0, -x1, -x2), True


def align(d2, xy, pose, cs=None, origin=(0.0, 0.0), grid=None, **kw):
    """One robot: d2 [W, W] -> dict(pose_out (3,), trace [n_iter + 1, 5], normal (10,) int64, n_used (3,),
    iters, flags, deltas: the steps taken).  cs [n_iter + 1, 2]: the (cos, sin) of every evaluation as
    the device wrote them (rows beyond the last evaluation are ignored); None: NumPy's.  grid: the
    lslam_grid_params that differ from the defaults."""
    q = params(**kw)
    g = ogr.params(**(grid or {}))
    W, cell = int(g["grid_w"]), float(g["cell"])
    inv = 1.0 / cell
    d2 = np.asarray(d2).reshape(W, W).astype(np.int64)
    E = int(q["n_iter"]) + 1
    pose = np.array(pose, np.float64).reshape(3)
    out = dict(pose_out=pose.copy(), trace=np.zeros((E, 5)), normal=np.zeros(10, np.int64), n_used=np.zeros(3, np.int32),
               iters=0, flags=0, deltas=[])
    px, py, th = (float(v) for v in pose)
    ox, oy = (float(v) for v in origin)
    with np.errstate(invalid="ignore", over="ignore"):
        X0, Y0 = np.floor((px - ox) * inv), np.floor((py - oy) * inv)
        if not (np.all(np.isfinite([px, py, th, ox, oy])) and abs(X0) < 2.0 ** 20 and abs(Y0) < 2.0 ** 20):
            out["flags"] = BAD_POSE
            return out
    x, y = used_points(xy, g["max_range"])
    px0, py0, th0 = px, py, th
    flags = iters = n_first = n_last = 0
    N = [0] * 10
    for k in range(E):
        c, s = (float(np.cos(th)), float(np.sin(th))) if cs is None else (float(cs[k][0]), float(cs[k][1]))
        out["trace"][k] = (px, py, th, c, s)
        N, n_last = evaluate(d2, x, y, px, py, c, s, ox, oy, inv, q["trunc"])
        if k == 0:
            n_first = n_last
        if n_last < int(q["min_points"]):
            flags |= FEW
            break
        if k == E - 1 or flags & CONVERGED:
            break
        (dx, dy, dt), ok = solve(N, float(q["damp_t"]), float(q["damp_r"]))
        nx, ny, nt = px + dx * cell, py + dy * cell, th + dt
        if not (ok and math.isfinite(nx) and math.isfinite(ny) and math.isfinite(nt)):
            flags |= SINGULAR
            break
        px, py, th = nx, ny, nt
        iters = k + 1
        out["deltas"].append((dx, dy, dt))
        if max(abs(dx), abs(dy)) < q["eps_t"] and abs(dt) < q["eps_r"]:
            flags |= CONVERGED
    if abs(px - px0) > q["max_shift"] or abs(py - py0) > q["max_shift"] or abs(th - th0) > q["max_turn"]:
        flags |= DIVERGED
    if 1000 * n_last < int(q["min_permille"]) * len(x):
        flags |= WEAK
    if not flags & KEEP:
        out["pose_out"] = np.array([px, py, th])
    out.update(normal=np.array(N, np.int64), n_used=np.array([n_first, n_last, len(x)], np.int32), iters=iters, flags=flags)
    return out


def align_batch(d2, xy, pt_off, pose, trace=None, origin=None, grid=None, **kw):
    """R robots -> dict of stacked arrays (pose_out [R, 3], trace [R, E, 5], normal [R, 10], n_used [R, 3],
    iters [R], flags [R]).  trace: the device's, for its (cos, sin)."""
    R = len(pt_off) - 1
    origin = np.zeros((R, 2)) if origin is None else np.asarray(origin, np.float64).reshape(R, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    outs = [align(d2[r], xy[pt_off[r]:pt_off[r + 1]], pose[r], None if trace is None else trace[r][:, 3:5], origin[r],
                  grid, **kw) for r in range(R)]
    return {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("pose_out", "trace", "normal", "n_used", "iters", "flags")}


def information(normal):
    """normal [R, 10] -> (H [R, 3, 3], g [R, 3]) as float64, in cells and rad."""
    n = np.asarray(normal, np.int64).reshape(-1, 10).astype(np.float64) / SCALE
    H = np.empty((len(n), 3, 3))
    for (i, j), k in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
        H[:, i, j] = H[:, j, i] = n[:, k]
    return H, n[:, 6:9].copy()
