"""What the fused polar loads (A1 inside every point load, xy = NULL) may be held to against the
CPU oracle, decided by the reference alone (NumPy and oracle.cpu; no HIP).

The kernels convert (theta_deg, dist_mm) with OCML's cos / sin, the oracle runs on
synth.polar_to_xy_ref (NumPy's): the two xy differ in the last bits, so exact equality of the
discrete outputs (draws, per-trial counts, masks, winners, landmark decisions) is only owed where
no residual sits within that disagreement of the threshold and no tie between trials is closer
than it.  DELTA0 is the largest per-coordinate disagreement (mm) the comparison is proven safe for;
margins() measures, for a batch, how many DELTA0 of room the oracle's own numbers leave:

  per chunk, trial t (draw pair i0, i1 of the oracle's chained stream) and point p
    o = (P[i0] + P[i1]) / 2, u = (P[i1] - P[i0]) / s, s = |P[i1] - P[i0]|   (the trial's line)
    t_p = (P[p] - o) . u,  r = |P[p] - o - t_p u|                           (offset along, residual)
    b = DELTA0 * (1 + 2 |t_p| / s)
  bounds how far r moves when every coordinate moves by at most DELTA0 (the point itself, plus
  the line turning about o by at most 2 DELTA0 / s).

  gap margin = min |r - threshold| / b            (>= 1: no count or mask can change)
  tie margin = min |sum_w - sum_t| / (D_w + D_t), D = sum_p (2 r b + b^2), over the winning trial w
               and every other trial t of the same count that drew another unordered pair
               (>= 1: the winner cannot change; the same pair swapped is the same line with a
               differently rounded sum, which the GPU test accepts as equal)

DELTA0: lslam_polar_to_xy against synth.polar_to_xy_ref over both batches below measured
max |dx| = 9.09e-13 mm = 0.5 ulp(8192) on the MI355X; 4x that, rounded up to a power
of two of ulp(8192), is 2 ulp(8192).  tests/test_gpu_parity.py::test_fused_polar_loads_vs_oracle
asserts the measured disagreement stays <= DELTA0.
"""
import functools

import numpy as np

from lidar_slam_amd import synth
from oracle import cpu

ULP_8192 = 2.0 ** -39          # ulp of a double in [8192, 16384): no coordinate here reaches 8192 mm
DELTA0 = 2 * ULP_8192          # 3.64e-12 mm
THRESHOLD = 20.0
MIN_MARGIN = 16.0
DISCRETE = ("n_inliers", "best_trial", "flags", "match_index", "landmark_id")


@functools.lru_cache(maxsize=None)
def batch(name):
    """The two batches of test_fused_polar_loads_equal_polar_kernel_then_xy, with the reference's xy
    (synth.polar_to_xy_ref), the seeds (= scan ids) and the trial count."""
    if name == "c3":
        ids = list(range(256))
        b = synth.make_batch(ids, 720)
        b["trials"] = 100
    elif name == "large":
        ids = list(range(24))
        b = synth.make_batch(ids, 600)
        S = len(ids)
        b["scan_chunk_off"] = np.arange(S + 1, dtype=np.int32)
        b["chunk_pt_off"] = (np.arange(S + 1) * 600).astype(np.int32)
        b["trials"] = 256
    else:
        raise KeyError(name)
    b["seeds"] = np.array(ids, np.uint32)
    assert np.array_equal(b["xy"], synth.polar_to_xy_ref(b["theta_deg"], b["dist_mm"]))
    return b


def oracle_trials(xy, sco, cpo, seeds, trials):
    """cpu.ransac(want_trials=True) per chunk, chained per scan: draws [C][T+1][2], cnt [C][T],
    sums [C][T] (NaN where the count is not the maximum), the model dicts and the masks."""
    C = int(sco[-1])
    draws = np.zeros((C, trials + 1, 2), np.int32)
    cnt = np.zeros((C, trials), np.int32)
    sums = np.zeros((C, trials))
    models, mask = [], np.zeros(int(cpo[-1]), np.uint8)
    for s in range(len(sco) - 1):
        st = cpu.MTState(seed=int(seeds[s]))
        for c in range(sco[s], sco[s + 1]):
            p0, p1 = cpo[c], cpo[c + 1]
            m, md, ex = cpu.ransac(xy[p0:p1], THRESHOLD, trials, state=st, want_trials=True)
            draws[c], cnt[c], sums[c] = ex["draws"], ex["cnt"], ex["sum"]
            mask[p0:p1] = m
            models.append(md)
    return dict(draws=draws, cnt=cnt, sums=sums, models=models, mask=mask)


@functools.lru_cache(maxsize=None)
def batch_trials(name):
    b = batch(name)
    return oracle_trials(b["xy"], b["scan_chunk_off"], b["chunk_pt_off"], b["seeds"], b["trials"])


def trial_geometry(P, draws, delta=DELTA0):
    """For the chunk's points P [N][2] and draw pairs [T][2]: r, |t_p|, b as [T][N], and s [T]."""
    A, B = P[draws[:, 0]], P[draws[:, 1]]
    o = (A + B) / 2
    d = B - A
    s = np.hypot(d[:, 0], d[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = d / s[:, None]
        e = P[None, :, :] - o[:, None, :]
        t = e[..., 0] * u[:, None, 0] + e[..., 1] * u[:, None, 1]
        rx = e[..., 0] - t * u[:, None, 0]
        ry = e[..., 1] - t * u[:, None, 1]
        r = np.sqrt(rx * rx + ry * ry)
        b = delta * (1 + 2 * np.abs(t) / s[:, None])
    return r, np.abs(t), b, s


def margins(name, delta=DELTA0):
    """Gap and tie margins of a batch (module docstring), where each is tightest, whether the NumPy
    count equals the oracle's for every trial, and the closest |r - threshold| in mm."""
    b, o = batch(name), batch_trials(name)
    sco, cpo, T = b["scan_chunk_off"], b["chunk_pt_off"], b["trials"]
    ecut = cpu.ecut(THRESHOLD)
    out = dict(gap=np.inf, tie=np.inf, gap_at=None, tie_at=None, closest_mm=np.inf, count_mismatch=[])
    for s in range(len(sco) - 1):
        for c in range(sco[s], sco[s + 1]):
            P = b["xy"][cpo[c]:cpo[c + 1]]
            dr = o["draws"][c, :T]
            r, _, bb, _ = trial_geometry(P, dr, delta)
            cnt = np.sum(r * r < ecut, axis=1)
            if not np.array_equal(cnt, o["cnt"][c]):
                out["count_mismatch"].append((s, c))
            gap = np.abs(r - THRESHOLD)
            g = gap / bb
            g = np.where(np.isnan(g), 0.0, g)  # a degenerate pair (s = 0) proves nothing
            i = np.unravel_index(np.argmin(g), g.shape)
            out["closest_mm"] = min(out["closest_mm"], float(np.nanmin(gap)))
            if g[i] < out["gap"]:
                out["gap"], out["gap_at"] = float(g[i]), dict(scan=s, chunk=c, trial=int(i[0]), point=int(i[1]), r=float(r[i]))
            w = o["models"][c]["best_trial"]
            if w < 0:
                continue
            ssum = np.sum(r * r, axis=1)
            D = np.sum(2 * r * bb + bb * bb, axis=1)
            pair_w = set(dr[w].tolist())
            for t in np.nonzero(o["cnt"][c] == o["cnt"][c][w])[0]:
                if t == w or set(dr[t].tolist()) == pair_w:
                    continue
                m = abs(ssum[w] - ssum[t]) / (D[w] + D[t])
                m = 0.0 if np.isnan(m) else float(m)
                if m < out["tie"]:
                    out["tie"], out["tie_at"] = m, dict(scan=s, chunk=c, winner=int(w), trial=int(t), count=int(o["cnt"][c][w]))
    return out


def discrete_outputs(name, xy):
    """What cpu.run_batch decides on xy that must not depend on the last bits: the mask, the integer
    fields of every chunk model and each scan's final list length."""
    b = batch(name)
    mask, _, models, lists = cpu.run_batch(xy, b["scan_chunk_off"], b["chunk_pt_off"], b["seeds"], THRESHOLD, b["trials"])
    out = {f: np.array([m[f] for m in models]) for f in DISCRETE}
    out["mask"] = mask
    out["list_len"] = np.array([len(L) for L in lists])
    return out


def perturbed(name, k, delta=DELTA0):
    """The batch's xy with every coordinate moved by +delta or -delta (seeded by k)."""
    xy = batch(name)["xy"]
    sign = np.random.default_rng(1000 + k).integers(0, 2, xy.shape) * 2.0 - 1.0
    return xy + sign * delta


def inlier_near_threshold(name, lo=19.2, hi=19.9):
    """(chunk, point, unit normal pointing away from the winning line): the batch's first inlier whose
    residual to its chunk's winning trial lies in (lo, hi) and which, moved 1 mm along that normal,
    is an outlier (by 0.1 mm at least) of every trial that could then win -- those within two of
    the best count: the winner loses one, another trial can gain at most this one point."""
    b, o = batch(name), batch_trials(name)
    cpo, T = b["chunk_pt_off"], b["trials"]
    for c in range(len(cpo) - 1):
        w = o["models"][c]["best_trial"]
        if w < 0:
            continue
        P = b["xy"][cpo[c]:cpo[c + 1]]
        pair = o["draws"][c, w]
        r = trial_geometry(P, pair[None, :])[0][0]
        rivals = o["cnt"][c] >= o["cnt"][c][w] - 2
        for p in np.nonzero((r > lo) & (r < hi))[0]:
            if not o["mask"][cpo[c] + p]:
                continue
            A, B = P[pair[0]], P[pair[1]]
            u = (B - A) / np.hypot(*(B - A))
            e = P[p] - (A + B) / 2
            n = e - (e @ u) * u
            n = n / np.hypot(*n)
            Q = P.copy()
            Q[p] += n
            if np.all(trial_geometry(Q, o["draws"][c, :T][rivals])[0][:, p] > THRESHOLD + 0.1):
                return c, int(p), n
    raise LookupError("no inlier within (%g, %g) mm of a winning line in %s" % (lo, hi, name))
