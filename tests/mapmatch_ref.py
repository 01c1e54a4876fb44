"""NumPy reference of the scan-to-map matcher (include/lidarslam.h, lslam_map_match), written
straight from the definition: the tests hold the kernels to it bit for bit.

All arithmetic is float64, one rounding per operation (NumPy's elementwise ufuncs fuse nothing),
then integers.  A revolution, a pose guess and the robot's log-odds grid -> the corrected pose:

0. rotation (cos, sin: the device's bits when given, else NumPy's), robot cell, BAD_POSE;
1. look-up grid G of the window around the robot cell: occupied map cells (L >= occ_min), smeared by
   Chebyshev distance, clipped to the window;
2. score volume S[k][jy][jx]: the sum of G under the points, rotated by the guess's heading composed
   with rot[k], moved to the world frame, quantised in the map's grid and shifted by whole cells;
3. winner, parabola, best, EMPTY, EDGE: scanmatch_ref.pick;
4. the acceptance gate WEAK; 5. the output pose.
"""
import numpy as np

import occgrid_ref as ogr
from scanmatch_ref import pick, rot_table, valid_points

EMPTY, EDGE, BAD_POSE, WEAK = 1, 2, 4, 8

DEFAULTS = dict(cell=ogr.DEFAULTS["cell"], grid_w=ogr.DEFAULTS["grid_w"], theta_step=np.pi / 360, win_w=512, smear=2,
                k_trans=10, k_theta=20, occ_min=85, min_permille=500)


def params(**kw):
    """The matcher's parameters and the two it takes from the grid's (cell, grid_w); the grid's other
    parameters (occgrid_ref.DEFAULTS) are accepted and ignored."""
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in DEFAULTS and k not in ogr.DEFAULTS:
            raise TypeError("unknown parameter %r" % k)
        if k in DEFAULTS:
            p[k] = v
    return p


def robot_cell(pose, origin, p):
    """Step 0: (X0, Y0) as ints, or None for a bad pose (the condition of occgrid_ref.hit_cells)."""
    inv = 1.0 / float(p["cell"])
    px, py, th = (float(v) for v in pose)
    ox, oy = (float(v) for v in origin)
    with np.errstate(invalid="ignore", over="ignore"):
        X0, Y0 = np.floor((px - ox) * inv), np.floor((py - oy) * inv)
        if not (np.all(np.isfinite([px, py, th, ox, oy])) and abs(X0) < 2.0 ** 20 and abs(Y0) < 2.0 ** 20):
            return None
    return int(X0), int(Y0)


def lookup_grid(L, X0, Y0, p):
    """Step 1: (G [win_w][win_w] with values 0..smear+1, the number of occupied window cells)."""
    gw, ww, s = int(p["grid_w"]), int(p["win_w"]), int(p["smear"])
    half = ww // 2
    L = np.asarray(L, np.int16).reshape(gw, gw)
    my, mx = Y0 - half + np.arange(ww), X0 - half + np.arange(ww)
    oky, okx = (my >= 0) & (my < gw), (mx >= 0) & (mx < gw)
    occ = np.zeros((ww, ww), bool)
    if oky.any() and okx.any():
        occ[np.ix_(oky, okx)] = L[np.ix_(my[oky], mx[okx])].astype(np.int64) >= int(p["occ_min"])
    pad = np.pad(occ, s)
    G = np.zeros((ww, ww), np.int32)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            near = pad[s + dy:s + dy + ww, s + dx:s + dx + ww]  # the cell at (dy, dx) is occupied
            G = np.maximum(G, np.where(near, s + 1 - max(abs(dx), abs(dy)), 0).astype(np.int32))
    return G, int(occ.sum())


def score_volume(G, xy, pose, origin, rot0, rot, X0, Y0, p):
    """Step 2: S [Ntheta][Nt][Nt] int32."""
    ww, kt, kth = int(p["win_w"]), int(p["k_trans"]), int(p["k_theta"])
    half, inv = ww // 2, 1.0 / float(p["cell"])
    Nt, Nth = 2 * kt + 1, 2 * kth + 1
    px, py = float(pose[0]), float(pose[1])
    ox, oy = float(origin[0]), float(origin[1])
    c, s = float(rot0[0]), float(rot0[1])
    v = valid_points(xy)
    x, y = v[:, 0], v[:, 1]
    pad = 2 * kt  # a counted point is at most k_trans cells outside the window, and is shifted by as many
    Gp = np.pad(G, pad)
    Wp = Gp.shape[1]
    flatG = Gp.ravel()
    j = np.arange(Nt) - kt
    shifts = (j[:, None] * Wp + j[None, :]).ravel()  # [jy][jx]
    S = np.zeros((Nth, Nt, Nt), np.int32)
    for k in range(Nth):
        ck, sk = float(rot[k][0]), float(rot[k][1])
        cc = c * ck - s * sk
        ss = s * ck + c * sk
        with np.errstate(invalid="ignore", over="ignore"):
            wx = px + (cc * x - ss * y)
            wy = py + (ss * x + cc * y)
            ax = np.floor((wx - ox) * inv) - float(X0)
            ay = np.floor((wy - oy) * inv) - float(Y0)
            keep = (ax >= -half - kt) & (ax < half + kt) & (ay >= -half - kt) & (ay < half + kt)  # in doubles
        axi, ayi = ax[keep].astype(np.int64), ay[keep].astype(np.int64)
        if axi.size == 0:
            continue
        base = (ayi + half + pad) * Wp + (axi + half + pad)
        for i0 in range(0, base.size, 2048):
            S[k] += flatG.take(base[i0:i0 + 2048, None] + shifts[None, :]).sum(axis=0, dtype=np.int32).reshape(Nt, Nt)
    return S


def match(L, origin, pose, xy, rot0=None, rot=None, **kw):
    """One robot.  Returns dict(pose_out, delta, best, n_valid, rot0, flags, scores, G).  rot0: the
    (cos, sin) the library wrote for this pose (the definition's input); None: NumPy's."""
    p = params(**kw)
    kt, kth = int(p["k_trans"]), int(p["k_theta"])
    Nt, Nth, ww = 2 * kt + 1, 2 * kth + 1, int(p["win_w"])
    pose = np.array(pose, np.float64).reshape(3)
    origin = np.asarray(origin, np.float64).reshape(2)
    if rot is None:
        rot = rot_table(kth, p["theta_step"])
    if rot0 is None:
        with np.errstate(invalid="ignore"):
            rot0 = (np.cos(pose[2]), np.sin(pose[2]))
    rot0 = np.array(rot0, np.float64).reshape(2)
    cell = robot_cell(pose, origin, p)
    if cell is None:
        return dict(pose_out=pose.copy(), delta=np.zeros(3), best=np.array([kth, kt, kt, 0], np.int32),
                    n_valid=np.zeros(2, np.int32), rot0=rot0, flags=BAD_POSE, scores=np.zeros((Nth, Nt, Nt), np.int32),
                    G=np.zeros((ww, ww), np.int32))
    X0, Y0 = cell
    G, n_occ = lookup_grid(L, X0, Y0, p)
    S = score_volume(G, xy, pose, origin, rot0, rot, X0, Y0, p)
    delta, best, flags, _ = pick(S, p)  # (EMPTY and EDGE have scanmatch_ref's values)
    n_pts = len(valid_points(xy))
    if not (flags & EMPTY) and 1000 * int(best[3]) < int(p["min_permille"]) * (int(p["smear"]) + 1) * n_pts:
        flags |= WEAK
    if flags & (EMPTY | WEAK):
        pose_out = pose.copy()
    else:
        pose_out = np.array([pose[0] + delta[0], pose[1] + delta[1], pose[2] + delta[2]])
    return dict(pose_out=pose_out, delta=delta, best=best, n_valid=np.array([n_occ, n_pts], np.int32), rot0=rot0,
                flags=flags, scores=S, G=G)


def match_batch(L, origin, pose, xy, pt_off, rot0=None, rot=None, **kw):
    """The batch form of the C ABI: L [R, W, W], robot r's points xy[pt_off[r]:pt_off[r+1]]; stacked
    results (without G)."""
    R = len(pt_off) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    pose = np.asarray(pose, np.float64).reshape(R, 3)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    rs = [match(L[r], origin[r], pose[r], xy[pt_off[r]:pt_off[r + 1]], None if rot0 is None else rot0[r], rot, **kw)
          for r in range(R)]
    out = {k: np.stack([r[k] for r in rs]) for k in ("pose_out", "delta", "best", "n_valid", "rot0", "scores")}
    out["flags"] = np.array([r["flags"] for r in rs], np.int32)
    return out
