"""NumPy reference of relocalisation with priors (include/lidarslam.h, lslam_map_relocalize_prior), on
top of reloc_ref: the definition is lslam_map_relocalize's but for the admissible set.

    Af[ty][tx]  some fine cell of the coarse cell's f x f block has clear_d2 >= clear_min2
    Aw[ty][tx]  the cell's centre (cand_pose's own expressions) lies in the box of half_xy around win_pose
    H[k]        fabs(remainder(k head_step - wtheta, two_pi)) <= half_theta, the IEEE remainder
    2'.         Sc' = Sc where Af & Aw & H[k], else 0; peaks and candidates from Sc'
    5'.         fine_clear2[j] = clear_d2 at the refined pose's cell; a rank below clear_min2 is not eligible

math.remainder is the IEEE operation (exact), np.remainder is another function.
"""
import math

import numpy as np

import mapmatch_ref as mmr
import reloc_ref as rr

DEFAULTS = dict(half_xy=1000.0, half_theta=0.5, clear_min2=16)
TWO_PI = 6.283185307179586


def split_params(**kw):
    """(the priors' parameters, the rest for reloc_ref)."""
    pp = dict(DEFAULTS)
    pp.update({k: kw.pop(k) for k in list(kw) if k in DEFAULTS})
    return pp, kw


def field_admissible(clear_d2, grid_w, f, clear_min2):
    """Af [Wc][Wc] bool; all ones without a field."""
    gw, f = int(grid_w), int(f)
    Wc = gw // f
    if clear_d2 is None:
        return np.ones((Wc, Wc), bool)
    ok = np.asarray(clear_d2, np.uint16).reshape(gw, gw).astype(np.int64) >= int(clear_min2)
    return ok.reshape(Wc, f, Wc, f).any(axis=(1, 3))


def window_admissible(win_pose, origin, Wc, cellc, half_xy):
    """Aw [Wc][Wc] bool; all ones without a window."""
    if win_pose is None:
        return np.ones((Wc, Wc), bool)
    t = np.arange(Wc).astype(np.float64)
    cx = float(origin[0]) + (t + 0.5) * float(cellc)
    cy = float(origin[1]) + (t + 0.5) * float(cellc)
    with np.errstate(invalid="ignore"):
        inx = np.abs(cx - float(win_pose[0])) <= float(half_xy)
        iny = np.abs(cy - float(win_pose[1])) <= float(half_xy)
    return iny[:, None] & inx[None, :]


def ieee_remainder(x, y):
    """remainder(x, y) of IEEE 754: NaN for a non-finite x (math.remainder raises on an infinity)."""
    return math.remainder(x, y) if math.isfinite(x) else math.nan


def heading_admissible(win_pose, n_head, head_step, half_theta):
    """H [n_head] bool; all ones without a window."""
    if win_pose is None:
        return np.ones(int(n_head), bool)
    wt, hs = float(win_pose[2]), float(head_step)
    return np.array([abs(ieee_remainder(float(k) * hs - wt, TWO_PI)) <= float(half_theta) for k in range(int(n_head))], bool)


def fine_clear(clear_d2, fine_pose, origin, grid_w, cell):
    """Step 5': clear_d2 at the cell of each refined pose, -1 for a bad pose or a cell off the map; zeros
    without a field."""
    K = len(fine_pose)
    if clear_d2 is None:
        return np.zeros(K, np.int32)
    gw, inv = int(grid_w), 1.0 / float(cell)
    D = np.asarray(clear_d2, np.uint16).reshape(gw, gw)
    out = np.full(K, -1, np.int32)
    for j, p in enumerate(np.asarray(fine_pose, np.float64)):
        if not (np.all(np.isfinite(p)) and np.all(np.isfinite(origin))):
            continue
        X0d = np.floor((p[0] - float(origin[0])) * inv)
        Y0d = np.floor((p[1] - float(origin[1])) * inv)
        if not (abs(X0d) < 1048576.0 and abs(Y0d) < 1048576.0):
            continue
        X0, Y0 = int(X0d), int(Y0d)
        if 0 <= X0 < gw and 0 <= Y0 < gw:
            out[j] = int(D[Y0, X0])
    return out


def relocalize(L, origin, xy, clear_d2=None, win_pose=None, pose_in=None, P_in=None, fine_rot0=None, rot=None,
               head_rot=None, **kw):
    """One robot: reloc_ref.relocalize's dict, of the masked volume, plus n_admit [2], fine_clear2 [K],
    and admissible [n_head][Wc][Wc] bool (the set itself, for the tests)."""
    pp, kw = split_params(**kw)
    q, rest, max_range = rr.split_params(**kw)
    p = mmr.params(**rest)
    f, K, nh = int(q["factor"]), int(q["n_cand"]), int(q["n_head"])
    gw = int(p["grid_w"])
    Wc, cellc = gw // f, float(p["cell"]) * f
    origin = np.asarray(origin, np.float64).reshape(2)
    if head_rot is None:
        head_rot = rr.head_table(nh, q["head_step"])
    A = field_admissible(clear_d2, gw, f, pp["clear_min2"]) & window_admissible(win_pose, origin, Wc, cellc, pp["half_xy"])
    H = heading_admissible(win_pose, nh, q["head_step"], pp["half_theta"])
    adm = H[:, None, None] & A[None]
    C = rr.coarse_map(L, gw, f, p["occ_min"])
    pts = rr.used_points(xy, max_range)
    Sc = np.zeros((nh, Wc, Wc), np.int32)
    if H.any() and A.any():  # (the headings outside H are zeros whatever they score)
        Sc[H] = np.where(A[None], rr.coarse_scores(C, pts, np.asarray(head_rot)[H], cellc), 0)
    cand, cand_pose = rr.candidates(Sc, K, origin, cellc, q["head_step"])
    fine = [mmr.match(L, origin, cand_pose[j], xy, None if fine_rot0 is None else fine_rot0[j], rot, **rest)
            for j in range(K)]
    out = dict(n_occ=np.int32(C.sum()), n_used=np.int32(len(pts)), coarse_scores=Sc, cand=cand, cand_pose=cand_pose,
               fine_pose=np.stack([m["pose_out"] for m in fine]), fine_delta=np.stack([m["delta"] for m in fine]),
               fine_best=np.stack([m["best"] for m in fine]), fine_nvalid=np.stack([m["n_valid"] for m in fine]),
               fine_rot0=np.stack([m["rot0"] for m in fine]),
               fine_flags=np.array([m["flags"] for m in fine], np.int32))
    out["n_admit"] = np.array([A.sum(), H.sum()], np.int32)
    out["fine_clear2"] = fine_clear(clear_d2, out["fine_pose"], origin, gw, p["cell"])
    # a rank that fails the clearance test is not eligible: to reloc_ref.select it is a WEAK one
    gate = out["fine_flags"].copy()
    if clear_d2 is not None:
        gate[out["fine_clear2"] < int(pp["clear_min2"])] |= mmr.WEAK
    out["result"], out["flags"] = rr.select(out["fine_pose"], out["fine_best"], gate, cand, q)
    out["flags"] = np.int32(out["flags"])
    pose_out = np.full(3, np.nan) if pose_in is None else np.array(pose_in, np.float64).reshape(3)
    P_out = np.zeros(9) if P_in is None else np.array(P_in, np.float64).reshape(9)
    if out["flags"] == 0:
        pose_out = out["fine_pose"][out["result"][0]].copy()
        sxy, sth = float(q["reset_sigma_xy"]), float(q["reset_sigma_theta"])
        P_out = np.diag([sxy * sxy, sxy * sxy, sth * sth]).reshape(9)
    out["pose_out"], out["P_out"], out["admissible"] = pose_out, P_out, adm
    return out


PER_RANK = rr.PER_RANK + ("fine_clear2",)
PER_ROBOT = rr.PER_ROBOT + ("n_admit",)


def relocalize_batch(L, origin, xy, pt_off, clear_d2=None, win_pose=None, pose_in=None, P_in=None, fine_rot0=None, **kw):
    """The batch form of the C ABI, as reloc_ref.relocalize_batch: clear_d2 [R, W, W], win_pose [R, 3]."""
    R = len(pt_off) - 1
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    rs = [relocalize(L[r], origin[r], xy[pt_off[r]:pt_off[r + 1]], None if clear_d2 is None else clear_d2[r],
                     None if win_pose is None else np.asarray(win_pose, np.float64).reshape(R, 3)[r],
                     None if pose_in is None else pose_in[r], None if P_in is None else np.asarray(P_in).reshape(R, 9)[r],
                     None if fine_rot0 is None else np.asarray(fine_rot0)[:, r], **kw) for r in range(R)]
    out = {k: np.stack([r[k] for r in rs], axis=1) for k in PER_RANK}
    out.update({k: np.stack([r[k] for r in rs]) for k in PER_ROBOT})
    return out
