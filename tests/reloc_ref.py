"""NumPy reference of global relocalisation (include/lidarslam.h, lslam_map_relocalize), written
straight from the definition: the tests hold the kernels to it bit for bit.

All arithmetic is float64, one rounding per operation (NumPy's elementwise ufuncs fuse nothing),
then integers.  A revolution and the robot's log-odds grid, no pose guess -> the pose in the grid:

0. coarse map C: a coarse cell is set iff some fine cell of its f x f block holds L >= occ_min;
1. the used points: valid and within max_range;
2. coarse scores Sc[k][ty][tx]: the number of points that, rotated by head_rot[k] and quantised in
   coarse cells around the robot at the centre of cell (ty, tx), fall on a set cell;
3. peaks: the candidates that come before all their neighbours in the order (score, flat index),
   the first K of them, and their poses;
4. the fine stage: mapmatch_ref.match from each candidate pose;
5. selection: the best eligible rank, its rivals, LOST and AMBIGUOUS; 6. the outputs.
"""
import numpy as np

import mapmatch_ref as mmr
import occgrid_ref as ogr
from scanmatch_ref import valid_points

LOST, AMBIGUOUS = 1, 2
PI, TWO_PI = 3.141592653589793, 6.283185307179586

DEFAULTS = dict(head_step=2.0 * np.pi / 180, n_head=180, factor=4, n_cand=8, ambig_permille=900, dup_mm=100.0,
                dup_rad=0.0873, reset_sigma_xy=50.0, reset_sigma_theta=0.05)


def split_params(**kw):
    """(reloc parameters, the matcher's and the grid's keywords, max_range) from one keyword set."""
    q = dict(DEFAULTS)
    rest = {}
    for k, v in kw.items():
        if k in DEFAULTS:
            q[k] = v
        elif k in mmr.DEFAULTS or k in ogr.DEFAULTS:
            rest[k] = v
        else:
            raise TypeError("unknown parameter %r" % k)
    return q, rest, float(rest.get("max_range", ogr.DEFAULTS["max_range"]))


def head_table(n_head, head_step):
    """(cos, sin) of k * head_step: the caller's table, whose bits are the definition."""
    a = np.arange(int(n_head)).astype(np.float64) * float(head_step)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))


def coarse_map(L, grid_w, f, occ_min):
    """Step 0: C [Wc][Wc] bool."""
    gw, f = int(grid_w), int(f)
    Wc = gw // f
    occ = np.asarray(L, np.int16).reshape(gw, gw).astype(np.int64) >= int(occ_min)
    return occ.reshape(Wc, f, Wc, f).any(axis=(1, 3))


def used_points(xy, max_range):
    """Step 1."""
    v = valid_points(xy)
    with np.errstate(over="ignore"):
        r2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]
        return v[r2 <= float(max_range) * float(max_range)]


def point_offsets(pts, c, s, invc, Wc):
    """Step 2's (ay, ax) of the points that count, as int64 arrays."""
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        xr = c * x - s * y
        yr = s * x + c * y
        ax = np.floor(xr * invc + 0.5)
        ay = np.floor(yr * invc + 0.5)
        keep = (ax > -Wc) & (ax < Wc) & (ay > -Wc) & (ay < Wc)  # in doubles
    return ay[keep].astype(np.int64), ax[keep].astype(np.int64)


def coarse_scores(C, pts, head_rot, cellc):
    """Step 2: Sc [n_head][Wc][Wc] int32.  A point at offset (ay, ax) on the set cell (cy, cx) counts
    for the robot cell (cy - ay, cx - ax): one histogram per heading over (points x set cells)."""
    Wc = C.shape[0]
    invc = 1.0 / float(cellc)
    cy, cx = np.nonzero(C)
    Sc = np.zeros((len(head_rot), Wc, Wc), np.int32)
    for k in range(len(head_rot)):
        ay, ax = point_offsets(pts, float(head_rot[k][0]), float(head_rot[k][1]), invc, Wc)
        if ay.size == 0 or cy.size == 0:
            continue
        ty = cy[None, :] - ay[:, None]
        tx = cx[None, :] - ax[:, None]
        ok = (ty >= 0) & (ty < Wc) & (tx >= 0) & (tx < Wc)
        Sc[k] = np.bincount((ty[ok] * Wc + tx[ok]).ravel(), minlength=Wc * Wc).astype(np.int32).reshape(Wc, Wc)
    return Sc


def peaks(Sc, K):
    """Step 3: the flat indices of the first K peaks, in order."""
    nh, Wc, _ = Sc.shape
    S = Sc.astype(np.int64)
    flat = np.arange(S.size, dtype=np.int64).reshape(S.shape)
    is_peak = S > 0
    # neighbours: the heading wraps, translations outside the grid do not exist (-1 loses to every score > 0)
    Sp = np.pad(S, ((0, 0), (1, 1), (1, 1)), constant_values=-1)
    Fp = np.pad(flat, ((0, 0), (1, 1), (1, 1)), constant_values=0)
    for dk in (-1, 0, 1):
        Sk, Fk = np.roll(Sp, -dk, axis=0), np.roll(Fp, -dk, axis=0)  # Sk[k] = Sp[(k + dk) mod nh]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dk == 0 and dy == 0 and dx == 0:
                    continue
                Sn = Sk[:, 1 + dy:1 + dy + Wc, 1 + dx:1 + dx + Wc]
                Fn = Fk[:, 1 + dy:1 + dy + Wc, 1 + dx:1 + dx + Wc]
                is_peak &= (S > Sn) | ((S == Sn) & (flat < Fn))
    idx = np.nonzero(is_peak.ravel())[0]
    order = np.lexsort((idx, -S.ravel()[idx]))
    return idx[order][:int(K)]


def candidates(Sc, K, origin, cellc, head_step):
    """Step 3's outputs: cand [K][4] int32, cand_pose [K][3]."""
    nh, Wc, _ = Sc.shape
    cand = np.tile(np.array([-1, -1, -1, 0], np.int32), (int(K), 1))
    pose = np.full((int(K), 3), np.nan)
    for j, i in enumerate(peaks(Sc, K)):
        k, ty, tx = int(i) // (Wc * Wc), (int(i) // Wc) % Wc, int(i) % Wc
        cand[j] = (k, ty, tx, Sc[k, ty, tx])
        pose[j] = (float(origin[0]) + (float(tx) + 0.5) * cellc, float(origin[1]) + (float(ty) + 0.5) * cellc,
                   float(k) * float(head_step))
    return cand, pose


def select(fine_pose, fine_best, fine_flags, cand, q):
    """Step 5: (result [8] int32, flags)."""
    K = len(fine_flags)
    elig = [j for j in range(K) if not (int(fine_flags[j]) & (mmr.EMPTY | mmr.BAD_POSE | mmr.WEAK))]
    if not elig:
        return np.array([-1, -1, -1, -1, 0, 0, -1, 0], np.int32), LOST
    win = min(elig, key=lambda j: (-int(fine_best[j][3]), j))
    sw = int(fine_best[win][3])
    a = fine_pose[win]
    rivals = []
    for j in elig:
        if j == win:
            continue
        b = fine_pose[j]
        dt = np.abs(a[2] - b[2])
        if dt > PI:
            dt = TWO_PI - dt
        if np.abs(a[0] - b[0]) <= q["dup_mm"] and np.abs(a[1] - b[1]) <= q["dup_mm"] and dt <= q["dup_rad"]:
            continue
        rivals.append(j)
    riv, sr = -1, 0
    if rivals:
        riv = min(rivals, key=lambda j: (-int(fine_best[j][3]), j))
        sr = int(fine_best[riv][3])
    flags = AMBIGUOUS if riv >= 0 and 1000 * sr >= int(q["ambig_permille"]) * sw else 0
    return np.array([win, cand[win][0], cand[win][1], cand[win][2], cand[win][3], sw, riv, sr], np.int32), flags


def relocalize(L, origin, xy, pose_in=None, P_in=None, fine_rot0=None, rot=None, head_rot=None, **kw):
    """One robot.  pose_in [3] / P_in [9]: what pose_out and P_out held before the call (NaN and zeros
    if None).  fine_rot0 [K][2]: the (cos, sin) the library wrote for the candidate poses (None:
    NumPy's).  Returns a dict of every output of the definition."""
    q, rest, max_range = split_params(**kw)
    p = mmr.params(**rest)
    f, K, nh = int(q["factor"]), int(q["n_cand"]), int(q["n_head"])
    gw = int(p["grid_w"])
    Wc, cellc = gw // f, float(p["cell"]) * f
    origin = np.asarray(origin, np.float64).reshape(2)
    if head_rot is None:
        head_rot = head_table(nh, q["head_step"])
    C = coarse_map(L, gw, f, p["occ_min"])
    pts = used_points(xy, max_range)
    Sc = coarse_scores(C, pts, head_rot, cellc)
    cand, cand_pose = candidates(Sc, K, origin, cellc, q["head_step"])
    fine = [mmr.match(L, origin, cand_pose[j], xy, None if fine_rot0 is None else fine_rot0[j], rot, **rest)
            for j in range(K)]
    out = dict(n_occ=np.int32(C.sum()), n_used=np.int32(len(pts)), coarse_scores=Sc, cand=cand, cand_pose=cand_pose,
               fine_pose=np.stack([m["pose_out"] for m in fine]), fine_delta=np.stack([m["delta"] for m in fine]),
               fine_best=np.stack([m["best"] for m in fine]), fine_nvalid=np.stack([m["n_valid"] for m in fine]),
               fine_rot0=np.stack([m["rot0"] for m in fine]),
               fine_flags=np.array([m["flags"] for m in fine], np.int32))
    out["result"], out["flags"] = select(out["fine_pose"], out["fine_best"], out["fine_flags"], cand, q)
    out["flags"] = np.int32(out["flags"])
    pose_out = np.full(3, np.nan) if pose_in is None else np.array(pose_in, np.float64).reshape(3)
    P_out = np.zeros(9) if P_in is None else np.array(P_in, np.float64).reshape(9)
    if out["flags"] == 0:
        pose_out = out["fine_pose"][out["result"][0]].copy()
        sxy, sth = float(q["reset_sigma_xy"]), float(q["reset_sigma_theta"])
        P_out = np.diag([sxy * sxy, sxy * sxy, sth * sth]).reshape(9)
    out["pose_out"], out["P_out"] = pose_out, P_out
    return out


PER_RANK = ("cand", "cand_pose", "fine_pose", "fine_delta", "fine_best", "fine_nvalid", "fine_rot0", "fine_flags")
PER_ROBOT = ("n_occ", "n_used", "coarse_scores", "result", "flags", "pose_out", "P_out")


def relocalize_batch(L, origin, xy, pt_off, pose_in=None, P_in=None, fine_rot0=None, **kw):
    """The batch form of the C ABI: L [R, W, W], robot r's points xy[pt_off[r]:pt_off[r+1]];
    fine_rot0 [K][R][2].  Per-rank outputs are stacked [K][R][..], the others [R][..]."""
    R = len(pt_off) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    rs = [relocalize(L[r], origin[r], xy[pt_off[r]:pt_off[r + 1]], None if pose_in is None else pose_in[r],
                     None if P_in is None else np.asarray(P_in).reshape(R, 9)[r],
                     None if fine_rot0 is None else np.asarray(fine_rot0)[:, r], **kw) for r in range(R)]
    out = {k: np.stack([r[k] for r in rs], axis=1) for k in PER_RANK}
    out.update({k: np.stack([r[k] for r in rs]) for k in PER_ROBOT})
    return out
