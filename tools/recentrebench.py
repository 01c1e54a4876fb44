"""Grid recentre cost: one lslam_grid_recentre call at the default grid (512 cells of 20 mm, 512 KiB per
robot) beside a device-to-device copy of the same bytes and the floor that the copy bandwidth gives.

python tools/recentrebench.py [--robots 4096,256,1] [--rounds 3] [--reps 7] [--out profiles/recentre_bench.json]

Cases, per robot count R: every robot moves by (32, 16) cells; and for the first count also one robot
in sixteen moves, and none moves.  A moving robot stands on cell (288, 272), the others on (256, 256);
quantum is the default 8 and margin 224, so that 32 cells off the middle is past the margin (at the
default margin of 128 the smallest shift is 128 cells; the bytes moved are nearly the same: every
destination cell is stored, and all but the strip that scrolls in is loaded).  The grids hold random
int16 values and stay where the last call left them: only the origin is put back before each timed
call, so every call decides and moves the same way.  Inputs are resident on the device.

The legs alternate, `rounds` times; per leg `reps` calls, each timed on its own with HIP events
(LSLAM_K_RECENTRE) after two untimed ones.  Beside each: `reps` lslam_d2d copies of as many bytes as
the moving robots' grids hold (one read and one write of each, what a recentre cannot do without),
timed back to back on the host clock after a warm-up and divided by `reps`; and the derived floor,
2 x those bytes / the copy bandwidth of the session (a 256 MiB copy, bytes read + bytes written per
second, as tools/gridbench.py measures it).  Figures are medians with minimum and maximum.  The first
call of every leg is asserted against the NumPy definition (tests/recentre_ref.py) for its first moving
robot and its first robot at rest.
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

import recentre_ref as rr  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import OccupancyGrid  # noqa: E402

MARGIN, QUANTUM = 224, 8
MOVING_CELL, RESTING_CELL, SHIFT = (288, 272), (256, 256), (32, 16)
SEED_ROBOTS = 16  # grids generated on the host; the rest are device copies of them


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


class Leg:
    def __init__(self, ctx, R, every):
        """R robots; robot r moves iff every > 0 and r % every == 0."""
        self.ctx, self.R, self.every = ctx, R, every
        self.g = OccupancyGrid(ctx, R)
        W, cell = self.g.W, float(self.g.p.cell)
        self.moving = np.array([every > 0 and r % every == 0 for r in range(R)])
        cells = np.where(self.moving[:, None], MOVING_CELL, RESTING_CELL).astype(np.float64)
        self.origin0 = np.array(self.g.origin_host)
        self.pose = np.concatenate([self.origin0 + (cells + 0.5) * cell, np.zeros((R, 1))], 1)
        self.d_pose = ctx.to_device(self.pose)
        rng = np.random.default_rng(R)
        n0 = min(R, SEED_ROBOTS)
        self.seed = rng.integers(-32768, 32768, (n0, W, W)).astype(np.int16)
        per = W * W * 2
        _lib.check(_lib.load().lslam_h2d(ctx.handle, self.g.logodds.ptr, self.seed.ctypes.data, self.seed.nbytes), "lslam_h2d")
        ctx.sync()
        have = n0
        while have < R:  # double what is there
            n = min(have, R - have)
            ctx.copy(self.g.logodds.addr + have * per, self.g.logodds.addr, n * per)
            have += n
        ctx.sync()
        self.moved_bytes = int(self.moving.sum()) * per
        self.ms, self.d2d_ms = [], []

    def robot_grid(self, r):
        W = self.g.W
        out = np.empty((W, W), np.int16)
        _lib.check(_lib.load().lslam_d2h(self.ctx.handle, out.ctypes.data, self.g.logodds.addr + r * W * W * 2, out.nbytes), "lslam_d2h")
        self.ctx.sync()
        return out

    def call(self, sync=True):
        self.g.origin.upload(self.origin0)
        self.g.recentre(self.d_pose, margin=MARGIN, quantum=QUANTUM, sync=sync)

    def check(self):
        """The first call against the definition: the first moving robot and the first at rest."""
        who = [int(np.flatnonzero(m)[0]) for m in (self.moving, ~self.moving) if m.any()]
        before = {r: self.robot_grid(r) for r in who}
        self.call()
        res = self.g.recentre_results()
        for r in who:
            L, origin, shift, flags = rr.recentre(before[r], self.pose[r], self.origin0[r], margin=MARGIN, quantum=QUANTUM)
            assert np.array_equal(self.robot_grid(r), L), r
            assert np.array_equal(res["origin"][r], origin) and np.array_equal(res["shift"][r], shift) and res["flags"][r] == flags, r
            assert tuple(shift) == (SHIFT if self.moving[r] else (0, 0))
        assert int((res["flags"] == rr.MOVED).sum()) == int(self.moving.sum()) and not np.any(res["flags"] & ~rr.MOVED)

    def timed(self, reps, warmup=2):
        ctx = self.ctx
        for _ in range(warmup):
            self.call()
        ctx.set_timing(True, kernels=[_lib.K_RECENTRE])
        for _ in range(reps):
            ctx.timing_reset()
            self.call()
            ms, n = ctx.timing(_lib.K_RECENTRE)
            assert n == 1
            self.ms.append(ms)
        ctx.set_timing(False)
        if self.moved_bytes:
            a, b = ctx.empty(self.moved_bytes, np.uint8), ctx.empty(self.moved_bytes, np.uint8)
            a.fill_zero()
            ctx.copy(b, a)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.copy(b, a)
            ctx.sync()
            self.d2d_ms.append((time.perf_counter() - t0) / reps * 1e3)
            a.free()
            b.free()


def copy_bandwidth(ctx, n=256 << 20, reps=5):
    a, b = ctx.empty(n, np.uint8), ctx.empty(n, np.uint8)
    a.fill_zero()
    ctx.copy(b, a)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.copy(b, a)
    ctx.sync()
    dt = (time.perf_counter() - t0) / reps
    a.free()
    b.free()
    return 2.0 * n / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recentre_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    counts = [int(r) for r in args.robots.split(",")]
    legs = [("all move", Leg(ctx, r, 1)) for r in counts]
    legs += [("one in sixteen moves", Leg(ctx, counts[0], 16)), ("none moves", Leg(ctx, counts[0], 0))]
    for _, leg in legs:
        leg.check()
    bw = copy_bandwidth(ctx)
    for _ in range(args.rounds):
        for _, leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/recentrebench.py; legs alternate over %d rounds; recentre by HIP events "
                   "per call, lslam_d2d on the host clock over back-to-back copies; medians with min and max" % args.rounds,
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0][1].g.W, "margin": MARGIN, "quantum": QUANTUM,
           "shift": list(SHIFT), "copy_GB_per_s": round(bw / 1e9, 1), "recentre": []}
    for what, leg in legs:
        floor_ms = 2.0 * leg.moved_bytes / bw * 1e3
        med = statistics.median(leg.ms)
        row = {"case": what, "robots": leg.R, "robots_moving": int(leg.moving.sum()), "moved_bytes": leg.moved_bytes,
               "recentre_ms": stats(leg.ms)}
        if leg.moved_bytes:
            row.update({"d2d_same_bytes_ms": stats(leg.d2d_ms), "floor_ms": round(floor_ms, 4),
                        "ratio_to_floor": round(med / floor_ms, 2), "ratio_to_d2d": round(med / statistics.median(leg.d2d_ms), 2),
                        "moved_GB_per_s": round(2.0 * leg.moved_bytes / (med * 1e-3) / 1e9, 1)})
        out["recentre"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
