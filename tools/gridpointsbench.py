"""Cost of reading maps as revolutions: lslam_grid_points for 1, 256 and 4096 robots at grid_w 512 on the
bench room's grids, and for a fleet whose grids are all empty; beside a device-to-device copy of the grids'
bytes, in the same session.

python tools/gridpointsbench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 5] [--out profiles/gridpoints_bench.json]

Seed robot s (64 of them) sees the synthetic room from synth.scan_polar(s)'s pose; its grid is centred on
it and holds two grid updates of its revolution.  Robot r's grid is a device copy of seed r % 64's.  The
anchor is each grid's centre, heading 0, given as a device array, so the host does nothing per call but the
call; cap and radius are the defaults (1024 slots, 8000 mm).

The comparison: the count pass reads every grid once and the write pass reads again the bands that hold a
cell in range, so at most two reads of the grids' bytes; the points written are few beside them (16 KiB of
slots a robot, zeroed first).  An lslam_d2d of the grids' bytes reads them once and writes them once: as
many bytes as the two passes move at most, the like-for-like floor.  An empty fleet's write pass reads the
counts only: about half.  No ratio is fixed in advance.

There is no timing slot for the call: every figure is `reps` back-to-back calls between two lslam_sync
on the host clock, divided by `reps`, after a warm-up; the legs alternate, `rounds` times, and the
figures are medians over the rounds with minimum and maximum.  Robot 0 of every leg is asserted against
the NumPy definition (tests/gridpoints_ref.py) first.
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

import gridpoints_ref as gp  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import GRIDPOINTS_EMPTY, GridScan, OccupancyGrid  # noqa: E402

SEEDS = 64


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
    """R grids, grid r a device copy of seed grid r % 64 (seed None: all empty)."""
    g = OccupancyGrid.centred_on(ctx, poses[np.arange(R) % SEEDS])
    if seed is None:
        return g
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
        self.grid = tiled(ctx, None if kind == "all empty" else seed, poses, R)
        self.scan = GridScan(self.grid)
        c = self.grid.origin_host + 0.5 * self.grid.W * float(self.grid.p.cell)
        self.anchor_host = np.concatenate([c, np.ones((R, 1)), np.zeros((R, 1))], 1)
        self.anchor = ctx.to_device(self.anchor_host)
        self.grid_bytes = R * self.grid.W * self.grid.W * 2
        self.t = {}

    def check(self):
        """Robot 0 of one call against the definition; returns its counts."""
        g = self.grid
        L0 = np.empty((g.W, g.W), np.int16)
        _lib.check(_lib.load().lslam_d2h(self.ctx.handle, L0.ctypes.data, g.logodds.addr, L0.nbytes), "lslam_d2h")
        self.ctx.sync()
        self.scan.step(self.anchor)
        res = self.scan.results()
        ref = gp.points(L0, g.origin_host[0], self.anchor_host[0], cell=float(g.p.cell))
        assert np.array_equal(res["xy"][0].view(np.uint64), ref["xy"].view(np.uint64))
        assert np.array_equal(res["counts"][0], ref["counts"]) and res["flags"][0] == ref["flags"]
        assert (res["flags"] == GRIDPOINTS_EMPTY).all() == (self.kind == "all empty")
        return ref["counts"].tolist()

    def timed(self, reps):
        ctx = self.ctx
        add = lambda k, ms: self.t.setdefault(k, []).append(ms)
        add("points_ms", host_timed(ctx, lambda: self.scan.step(self.anchor, sync=False), reps))
        a, b = ctx.empty(self.grid_bytes, np.uint8), ctx.empty(self.grid_bytes, np.uint8)
        a.fill_zero()
        add("d2d_grids_ms", host_timed(ctx, lambda: ctx.copy(b, a), reps))
        a.free()
        b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gridpoints_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    counts = [int(r) for r in args.robots.split(",")]
    poses, seed = seed_grids(ctx, args.points)
    legs = [Leg(ctx, seed, poses, r, "bench room") for r in counts]
    legs.append(Leg(ctx, seed, poses, counts[0], "all empty"))
    first = [leg.check() for leg in legs]
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/gridpointsbench.py; legs alternate over %d rounds; every figure is %d back-to-back "
                   "calls between two lslam_sync on the host clock, per call; medians with min and max" % (args.rounds, args.reps),
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0].grid.W, "cap": legs[0].scan.cap,
           "radius": float(legs[0].scan.p.radius), "legs": []}
    for leg, st in zip(legs, first):
        row = {"grids": leg.kind, "robots": leg.R, "counts_robot0": st, "grid_bytes": leg.grid_bytes}
        row.update({k: stats(v) for k, v in leg.t.items()})
        med = {k: statistics.median(v) for k, v in leg.t.items()}
        row["points_to_d2d"] = round(med["points_ms"] / med["d2d_grids_ms"], 2)
        row["points_GB_per_s_of_two_reads"] = round(2.0 * leg.grid_bytes / (med["points_ms"] * 1e-3) / 1e9, 1)
        out["legs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
