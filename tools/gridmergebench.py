"""Map-merge cost: lslam_grid_merge for many pairs at grid_w 512 on the bench room's grids, under a
rotation of 0.4 rad and under the identity, as a dry run (the statistics pass and a merge pass that ends
at the decision), and for a fleet whose pairs are all SKIPPED; beside a device-to-device copy of the
bytes the call must move, in the same session.

python tools/gridmergebench.py [--pairs 4096,256,1] [--points 720] [--rounds 3] [--reps 5] [--out profiles/gridmerge_bench.json]

Seed robot s (64 of them) sees the synthetic room from synth.scan_polar(s)'s pose; its grid is centred
on it and holds two grid updates of its revolution.  Pair m's source and destination are both seed
m % 64's grid (device copies); the rotation turns the source about the robot.  The gates are open
(min_support 0, max_contra_permille 1000) and the clamps are the ends of int16, so every call of a leg
merges, and changes every cell under a source value, however often it is repeated: ADD would otherwise
saturate at l_max after a few calls and stop storing.

The comparison: the call reads the source once and the destination twice, and writes the destination
once: four grids' bytes a pair at equal widths.  An lslam_d2d of two grids' bytes a pair moves as much
(reads them, writes them).  The direct gather reads the source in the merge pass again, so five grids'
bytes go through the caches; no ratio is fixed in advance.

There is no timing slot for the call: every figure is `reps` back-to-back calls between two lslam_sync
on the host clock, divided by `reps`, after a warm-up; the legs alternate, `rounds` times, and the
figures are medians over the rounds with minimum and maximum.  Pair 0 of every leg is asserted against
the NumPy definition (tests/gridmerge_ref.py) first.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gridmerge_ref as gm  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import MERGE_MERGED, MERGE_SKIPPED, OccupancyGrid  # noqa: E402

SEEDS = 64
OPEN = dict(min_support=0, max_contra_permille=1000)
CLAMPS = dict(l_min=-32768, l_max=32767)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def host_timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def seed_grids(ctx, Np):
    poses = np.array([synth.scan_polar(s)[2] for s in range(SEEDS)])
    revs = [synth.polar_to_xy_ref(*synth.scan_polar_at(poses[s], 2 * s, Np)) for s in range(SEEDS)]
    g = OccupancyGrid.centred_on(ctx, poses)
    sxy = ctx.to_device(np.concatenate(revs))
    for _ in range(2):
        g.step(sxy, np.arange(SEEDS + 1, dtype=np.int32), (np.arange(SEEDS + 1) * Np).astype(np.int32), pose=poses)
    return poses, g


def tiled(ctx, seed, poses, R):
    """R grids, grid m a device copy of seed grid m % 64."""
    g = OccupancyGrid.centred_on(ctx, poses[np.arange(R) % SEEDS], **CLAMPS)
    per = g.W * g.W * 2
    have = min(R, SEEDS)
    ctx.copy(g.logodds.addr, seed.logodds.addr, have * per)
    while have < R:
        n = min(have, R - have)
        ctx.copy(g.logodds.addr + have * per, g.logodds.addr, n * per)
        have += n
    ctx.sync()
    return g


class Leg:
    def __init__(self, ctx, seed, poses, R, kind):
        self.ctx, self.R, self.kind = ctx, R, kind
        self.src, self.dst = tiled(ctx, seed, poses, R), tiled(ctx, seed, poses, R)
        p = poses[np.arange(R) % SEEDS]
        th = 0.4 if kind == "rot 0.4" else 0.0
        c, s = np.cos(th), np.sin(th)
        # about the robot: xs = R (w - p) + p
        self.xf = ctx.to_device(np.stack([np.full(R, c), np.full(R, s), p[:, 0] - (c * p[:, 0] - s * p[:, 1]),
                                          p[:, 1] - (s * p[:, 0] + c * p[:, 1])], -1))
        self.idx = ctx.to_device(np.full(R, -1, np.int32)) if kind == "all skipped" else None
        self.grid_bytes = R * self.dst.W * self.dst.W * 2
        self.t = {}

    def first(self, g):
        out = np.empty((g.W, g.W), np.int16)
        _lib.check(_lib.load().lslam_d2h(self.ctx.handle, out.ctypes.data, g.logodds.addr, out.nbytes), "lslam_d2h")
        self.ctx.sync()
        return out

    def check(self):
        """Pair 0 of one call against the definition; returns its stats."""
        S0, L0 = self.first(self.src), self.first(self.dst)
        self.dst.merge(self.src, self.xf, src_index=self.idx, **OPEN)
        res = self.dst.merge_results()
        if self.kind == "all skipped":
            assert (res["flags"] == MERGE_SKIPPED).all() and not res["stats"].any() and np.array_equal(self.first(self.dst), L0)
            return [0] * 8
        ref = gm.merge(S0, self.src.origin_host[0], L0, self.dst.origin_host[0], self.xf.download()[0], **OPEN, **CLAMPS)
        assert res["flags"][0] == ref["flags"] == MERGE_MERGED and np.array_equal(res["stats"][0], ref["stats"])
        assert np.array_equal(self.first(self.dst), ref["dst"]) and (res["flags"] == MERGE_MERGED).all()
        return ref["stats"].tolist()

    def timed(self, reps):
        ctx = self.ctx
        add = lambda k, ms: self.t.setdefault(k, []).append(ms)
        add("merge_ms", host_timed(ctx, lambda: self.dst.merge(self.src, self.xf, src_index=self.idx, sync=False, **OPEN), reps))
        if self.kind == "all skipped":
            return
        add("dry_run_ms", host_timed(ctx, lambda: self.dst.merge(self.src, self.xf, dry_run=True, sync=False, **OPEN), reps))
        a, b = ctx.empty(2 * self.grid_bytes, np.uint8), ctx.empty(2 * self.grid_bytes, np.uint8)
        a.fill_zero()
        add("d2d_two_grids_a_pair_ms", host_timed(ctx, lambda: ctx.copy(b, a), reps))
        a.free()
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridmerge_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    counts = [int(r) for r in args.pairs.split(",")]
    poses, seed = seed_grids(ctx, args.points)
    legs = [Leg(ctx, seed, poses, r, kind) for r in counts for kind in ("rot 0.4", "identity")]
    legs.append(Leg(ctx, seed, poses, counts[0], "all skipped"))
    first = [leg.check() for leg in legs]
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/gridmergebench.py; legs alternate over %d rounds; every figure is %d back-to-back "
                   "calls between two lslam_sync on the host clock, per call; medians with min and max" % (args.rounds, args.reps),
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0].dst.W, "src_w": legs[0].src.W, "legs": []}
    for leg, st in zip(legs, first):
        row = {"transform": leg.kind, "pairs": leg.R, "stats_pair0": st, "grid_bytes": leg.grid_bytes}
        row.update({k: stats(v) for k, v in leg.t.items()})
        med = {k: statistics.median(v) for k, v in leg.t.items()}
        if "d2d_two_grids_a_pair_ms" in med:
            row["merge_to_d2d"] = round(med["merge_ms"] / med["d2d_two_grids_a_pair_ms"], 2)
            row["dry_run_to_merge"] = round(med["dry_run_ms"] / med["merge_ms"], 2)
            row["merge_GB_per_s_of_four_grids"] = round(4.0 * leg.grid_bytes / (med["merge_ms"] * 1e-3) / 1e9, 1)
        out["legs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
