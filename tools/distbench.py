"""Distance-field cost: one default lslam_grid_distance call (grid_w 512, d_max 64) for many robots on
the bench room's grids, beside a device-to-device copy of twice the grids' bytes (logodds read once, d2
written once: the floor of any form) and a default lslam_grid_update call of the same session; and
lslam_field_score beside lslam_grid_raycast under the same revolutions.

python tools/distbench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 5] [--out profiles/dist_bench.json]

Seed robot s (64 of them) sees the synthetic room from synth.scan_polar(s)'s pose; its grid is centred
on it and holds two grid updates of its revolution (free cells at -82, walls at 170).  Robot r of a
fleet is seed r % 64: the grids are device copies, the revolutions and poses tiled.  Inputs are resident
on the device.  For the first robot count there are two more fleets: EMPTY maps (all cells unknown: the
early-out) and maps with one source cell in the middle (the longest searches).

There is no timing slot for these calls: every figure is `reps` back-to-back calls between two
lslam_sync on the host clock, divided by `reps`, after a warm-up; the legs alternate, `rounds` times,
and the figures are medians over the rounds with minimum and maximum.  Seed robot 0's field and score
are asserted against the NumPy definitions (tests/dist_ref.py, tests/fieldscore_ref.py) first.
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

import dist_ref as dr  # noqa: E402
import fieldscore_ref as fr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import DistanceField, GridRayCaster, OccupancyGrid  # noqa: E402

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


def seed_room(Np):
    poses, revs = [], []
    for s in range(SEEDS):
        p = synth.scan_polar(s)[2]
        revs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p, 2 * s, Np)))
        poses.append(p)
    return np.array(poses), revs


class Leg:
    """One fleet: its grids ("room", "empty" or "one source"), the field, the revolutions."""

    def __init__(self, ctx, R, Np, poses, revs, maps="room"):
        self.ctx, self.R, self.Np, self.maps = ctx, R, Np, maps
        n0 = min(R, SEEDS)
        idx = np.arange(R) % SEEDS
        self.poses = poses[idx]
        self.rev0 = revs[0]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.g = OccupancyGrid.centred_on(ctx, self.poses)
        self.f = DistanceField(self.g)
        self.d_xy = ctx.to_device(np.concatenate([revs[i] for i in idx]))
        self.d_pose = ctx.to_device(self.poses)
        W = self.g.W
        per = W * W * 2
        if maps == "room":
            seedg = OccupancyGrid.centred_on(ctx, poses[:n0])
            sxy = ctx.to_device(np.concatenate(revs[:n0]))
            for _ in range(2):
                seedg.step(sxy, np.arange(n0 + 1, dtype=np.int32), (np.arange(n0 + 1) * Np).astype(np.int32), pose=poses[:n0])
            ctx.copy(self.g.logodds.addr, seedg.logodds.addr, n0 * per)
            ctx.sync()
            self.scratch = OccupancyGrid.centred_on(ctx, self.poses)  # the timed grid updates go here
            self.rc = GridRayCaster(self.g)
        elif maps == "one source":
            one = np.zeros((n0, W, W), np.int16)
            one[:, W // 2, W // 2] = 170
            _lib.check(_lib.load().lslam_h2d(ctx.handle, self.g.logodds.ptr, one.ctypes.data, one.nbytes), "lslam_h2d")
            ctx.sync()
        if maps != "empty":
            have = n0
            while have < R:  # double what is there
                n = min(have, R - have)
                ctx.copy(self.g.logodds.addr + have * per, self.g.logodds.addr, n * per)
                have += n
            ctx.sync()
        self.grid_bytes = R * per
        self.t = {}

    def robot0(self, arr, dtype):
        W = self.g.W
        out = np.empty((W, W), dtype)
        _lib.check(_lib.load().lslam_d2h(self.ctx.handle, out.ctypes.data, arr.addr, out.nbytes), "lslam_d2h")
        self.ctx.sync()
        return out

    def check(self):
        """Robot 0's field, and for the room its score, against the definitions."""
        self.f.step()
        L0, d20 = self.robot0(self.g.logodds, np.int16), self.robot0(self.f.d2, np.uint16)
        d2, n_src, flags = dr.field(L0)
        assert np.array_equal(d20, d2)
        assert self.f.n_src.download()[0] == n_src and self.f.flags.download()[0] == flags
        assert {"room": n_src > 100, "empty": n_src == 0, "one source": n_src == 1}[self.maps]
        if self.maps == "room":
            self.f.score(self.d_xy, self.sco, self.off, pose=self.d_pose)
            res = self.f.score_results()
            stats_, clear2, sflags = fr.score(d2, self.rev0, self.poses[0], res["rot"][0], self.g.origin_host[0])
            assert np.array_equal(res["stats"][0], stats_) and res["clear2"][0] == clear2 and res["flags"][0] == sflags
        return int(n_src)

    def timed(self, reps):
        ctx = self.ctx
        add = lambda k, ms: self.t.setdefault(k, []).append(ms)
        add("dist_ms", host_timed(ctx, lambda: self.f.step(sync=False), reps))
        if self.maps != "room":
            return
        a, b = ctx.empty(2 * self.grid_bytes, np.uint8), ctx.empty(2 * self.grid_bytes, np.uint8)
        a.fill_zero()
        add("d2d_twice_the_grids_ms", host_timed(ctx, lambda: ctx.copy(b, a), reps))
        a.free()
        b.free()
        add("grid_update_ms", host_timed(ctx, lambda: self.scratch.step(self.d_xy, self.sco, self.off, pose=self.d_pose, sync=False), reps))
        add("field_score_ms", host_timed(ctx, lambda: self.f.score(self.d_xy, self.sco, self.off, pose=self.d_pose, sync=False), reps))
        add("raycast_ms", host_timed(ctx, lambda: self.rc.step(self.d_xy, self.sco, self.off, pose=self.d_pose, sync=False, want_stop=False), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dist_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    counts = [int(r) for r in args.robots.split(",")]
    poses, revs = seed_room(args.points)
    legs = [Leg(ctx, r, args.points, poses, revs) for r in counts]
    legs += [Leg(ctx, counts[0], args.points, poses, revs, "empty"), Leg(ctx, counts[0], args.points, poses, revs, "one source")]
    n_src = [leg.check() for leg in legs]
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/distbench.py; legs alternate over %d rounds; every figure is %d back-to-back "
                   "calls between two lslam_sync on the host clock, per call; medians with min and max" % (args.rounds, args.reps),
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0].g.W, "d_max": int(legs[0].f.p.d_max),
           "points_per_robot": args.points, "legs": []}
    for leg, n in zip(legs, n_src):
        row = {"maps": leg.maps, "robots": leg.R, "n_src_robot0": n, "grid_bytes": leg.grid_bytes}
        row.update({k: stats(v) for k, v in leg.t.items()})
        med = {k: statistics.median(v) for k, v in leg.t.items()}
        if "d2d_twice_the_grids_ms" in med:
            row["dist_to_d2d"] = round(med["dist_ms"] / med["d2d_twice_the_grids_ms"], 2)
            row["dist_to_grid_update"] = round(med["dist_ms"] / med["grid_update_ms"], 2)
            row["field_score_to_raycast"] = round(med["field_score_ms"] / med["raycast_ms"], 2)
            row["dist_GB_per_s"] = round(2.0 * leg.grid_bytes / (med["dist_ms"] * 1e-3) / 1e9, 1)
        out["legs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
