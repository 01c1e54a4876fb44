"""NumPy reference of the correlative scan matcher (include/lidarslam.h, lslam_scan_match),
written straight from the definition: the tests hold the kernels to it bit for bit.

All arithmetic is float64, one rounding per operation (NumPy's elementwise ufuncs fuse nothing).
A pair of scans -> the pose of the current frame in the previous one, q ~ R(theta) p + t:

1. look-up grid G from the previous scan: occupied cells, smeared by Chebyshev distance;
2. score volume S[k][jy][jx]: the sum of G under the current points rotated by rot[k] and shifted
   by whole cells;
3. winner: highest score, then smallest d^2 from "no motion", then smallest flat index;
4. one parabola per axis through the winner and its two neighbours;
5. delta, best, n_valid, flags; 6. the wheel speeds that the filter's fx turns back into delta.
"""
import numpy as np

EMPTY, EDGE = 1, 2

DEFAULTS = dict(cell=20.0, theta_step=np.pi / 360, grid_w=512, smear=2, k_trans=10, k_theta=20)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def rot_table(k_theta, theta_step):
    """(cos, sin) of (k - k_theta) * theta_step: the caller's table, whose bits are the definition."""
    a = (np.arange(2 * int(k_theta) + 1) - int(k_theta)) * float(theta_step)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))


def valid_points(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    ok = np.isfinite(xy[:, 0]) & np.isfinite(xy[:, 1]) & ~((xy[:, 0] == 0.0) & (xy[:, 1] == 0.0))
    return xy[ok]


def lookup_grid(ref_xy, p):
    """G [grid_w][grid_w], values 0..smear+1."""
    gw, s = int(p["grid_w"]), int(p["smear"])
    half, inv = gw // 2, 1.0 / float(p["cell"])
    v = valid_points(ref_xy)
    G = np.zeros((gw, gw), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = np.floor(v[:, 0] * inv), np.floor(v[:, 1] * inv)
        ins = (fx >= -half) & (fx < half) & (fy >= -half) & (fy < half)  # in doubles
    ix, iy = fx[ins].astype(np.int64) + half, fy[ins].astype(np.int64) + half
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            yy, xx = iy + dy, ix + dx
            m = (yy >= 0) & (yy < gw) & (xx >= 0) & (xx < gw)
            np.maximum.at(G, (yy[m], xx[m]), s + 1 - max(abs(dx), abs(dy)))
    return G


def score_volume(G, cur_xy, rot, p):
    """S [Ntheta][Nt][Nt] int32."""
    gw, kt, kth = int(p["grid_w"]), int(p["k_trans"]), int(p["k_theta"])
    half, inv = gw // 2, 1.0 / float(p["cell"])
    Nt, Nth = 2 * kt + 1, 2 * kth + 1
    v = valid_points(cur_xy)
    x, y = v[:, 0], v[:, 1]
    pad = 2 * kt  # a reachable point is at most k_trans cells out, and is shifted by as many
    Gp = np.pad(G, pad)
    S = np.zeros((Nth, Nt, Nt), np.int32)
    jx = np.arange(Nt)
    for k in range(Nth):
        c, s = float(rot[k][0]), float(rot[k][1])
        with np.errstate(invalid="ignore", over="ignore"):
            xr = c * x - s * y
            yr = s * x + c * y
            ax, ay = np.floor(xr * inv), np.floor(yr * inv)
            keep = (ax >= -half - kt) & (ax < half + kt) & (ay >= -half - kt) & (ay < half + kt)  # in doubles
        axi, ayi = ax[keep].astype(np.int64), ay[keep].astype(np.int64)
        if axi.size == 0:
            continue
        # one gather per rotation, in slabs of points: [points][jy][jx]
        for i0 in range(0, axi.size, 1024):
            cols = axi[i0:i0 + 1024, None, None] + (jx[None, None, :] - kt) + half + pad
            rows = ayi[i0:i0 + 1024, None, None] + (jx[None, :, None] - kt) + half + pad
            S[k] += Gp[rows, cols].sum(axis=0, dtype=np.int32)
    return S


def pick(S, p, ukf=None):
    """(delta[3], best[4], flags, u[2] or None) from the score volume."""
    kt, kth = int(p["k_trans"]), int(p["k_theta"])
    cell, step = float(p["cell"]), float(p["theta_step"])
    Nth, Nt = S.shape[0], S.shape[1]
    kk, yy, xx = np.meshgrid(np.arange(Nth), np.arange(Nt), np.arange(Nt), indexing="ij")
    d2 = ((kk - kth) ** 2 + (yy - kt) ** 2 + (xx - kt) ** 2).ravel()
    flat = np.arange(S.size)
    w = int(np.lexsort((flat, d2, -S.ravel().astype(np.int64)))[0])
    k, jy, jx = w // (Nt * Nt), (w // Nt) % Nt, w % Nt
    s0 = int(S[k, jy, jx])
    if s0 == 0:
        u = None if ukf is None else np.zeros(2)
        return np.zeros(3), np.array([kth, kt, kt, 0], np.int32), EMPTY, u

    def refine(i, n, sm, sp):
        if i == 0 or i == n - 1:
            return 0.0, True
        den = float(sm) - 2.0 * float(s0) + float(sp)
        if den < 0.0:
            return 0.5 * (float(sm) - float(sp)) / den, False
        return 0.0, False

    dx, ex = refine(jx, Nt, S[k, jy, jx - 1] if jx > 0 else 0, S[k, jy, jx + 1] if jx < Nt - 1 else 0)
    dy, ey = refine(jy, Nt, S[k, jy - 1, jx] if jy > 0 else 0, S[k, jy + 1, jx] if jy < Nt - 1 else 0)
    dt, et = refine(k, Nth, S[k - 1, jy, jx] if k > 0 else 0, S[k + 1, jy, jx] if k < Nth - 1 else 0)
    delta = np.array([(float(jx - kt) + dx) * cell, (float(jy - kt) + dy) * cell, (float(k - kth) + dt) * step])
    flags = EDGE if (ex or ey or et) else 0
    u = None
    if ukf is not None:
        u = wheel_speeds(delta, **ukf)
    return delta, np.array([k, jy, jx, s0], np.int32), flags, u


def wheel_speeds(delta, dt=0.005, wheel_radius=50.0, wheel_base=200.0):
    """The inverse of the filter's fx (x += dt B(theta) u) for a forward displacement delta[0] and a
    heading change delta[2]."""
    a = delta[0] / (wheel_radius * dt)
    b = delta[2] * wheel_base / (2.0 * wheel_radius * dt)
    return np.array([a - b, a + b])


def match(ref_xy, cur_xy, rot=None, ukf=None, **kw):
    """One robot.  Returns dict(delta, best, flags, n_valid, scores, G[, u])."""
    p = params(**kw)
    if rot is None:
        rot = rot_table(p["k_theta"], p["theta_step"])
    G = lookup_grid(ref_xy, p)
    S = score_volume(G, cur_xy, rot, p)
    delta, best, flags, u = pick(S, p, ukf)
    out = dict(delta=delta, best=best, flags=flags, scores=S, G=G,
               n_valid=np.array([len(valid_points(ref_xy)), len(valid_points(cur_xy))], np.int32))
    if ukf is not None:
        out["u"] = u
    return out


def match_batch(ref_xy, ref_off, cur_xy, cur_off, rot=None, ukf=None, **kw):
    """The batch form of the C ABI: CSR offsets per robot; stacked results."""
    ref_xy = np.asarray(ref_xy, np.float64).reshape(-1, 2)
    cur_xy = np.asarray(cur_xy, np.float64).reshape(-1, 2)
    rs = [match(ref_xy[ref_off[r]:ref_off[r + 1]], cur_xy[cur_off[r]:cur_off[r + 1]], rot=rot, ukf=ukf, **kw)
          for r in range(len(ref_off) - 1)]
    out = {k: np.stack([r[k] for r in rs]) for k in ("delta", "best", "n_valid", "scores")}
    out["flags"] = np.array([r["flags"] for r in rs], np.int32)
    if ukf is not None:
        out["u"] = np.stack([r["u"] for r in rs])
    return out


def compose(pose, d):
    """pose (x, y, th) composed with a motion d = (tx, ty, dth) given in pose's own frame."""
    x, y, th = pose
    c, s = np.cos(th), np.sin(th)
    return np.array([x + c * d[0] - s * d[1], y + s * d[0] + c * d[1], th + d[2]])
