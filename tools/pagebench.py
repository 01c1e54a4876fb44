"""What the canvas costs: one lslam_grid_recentre_paged call beside lslam_grid_recentre on the same
inputs, and flush and load beside a device-to-device copy of the window's bytes.

python tools/pagebench.py [--robots 4096,256,1] [--rounds 4] [--reps 7] [--canvas-w 1024] [--out profiles/page_bench.json]

The method is tools/recentrebench.py's.  grid_w 512, canvas_w 1024 (2 MiB of canvas a robot, 8.6 GB at
4096); the window starts in the middle of its canvas.  Cases, per robot count R: every robot moves by
(32, 16) cells; and for the first count also one robot in sixteen moves, and none moves.  A moving
robot stands on cell (288, 272), the others on (256, 256); quantum 8, margin 224.  Windows and
canvases hold random int16 values and stay where the last call left them: only origin and win are put
back before each timed call, so every call decides and moves the same way.

The legs alternate, `rounds` times, the paged leg of a case first in one round and its plain leg first in the
next; per leg `reps` calls, each timed on its own with HIP events
(LSLAM_K_RECENTRE: the paged call runs under the recentre's slot) after two untimed ones.  flush, load
and the lslam_d2d beside them have no slot: `reps` calls back to back on the host clock after a
warm-up, ended by a synchronise, divided by `reps`.

The floor of what paging adds is the strips' traffic: (32 x 512 + 16 x 480) cells leave and as many
enter, each read once and written once, 192,512 bytes a moving robot, over the copy bandwidth of the
session (a 256 MiB copy, bytes read + bytes written per second).  The first call of every paged leg is
asserted against the NumPy definition (tests/page_ref.py) for its first moving robot and its first
robot at rest.
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

import page_ref as pr  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import OccupancyGrid  # noqa: E402
from recentrebench import MARGIN, MOVING_CELL, QUANTUM, RESTING_CELL, SEED_ROBOTS, SHIFT, copy_bandwidth, stats  # noqa: E402

W = 512
STRIP_CELLS = SHIFT[0] * W + SHIFT[1] * (W - SHIFT[0])  # the cells that leave; as many enter
STRIP_BYTES = 2 * 2 * 2 * STRIP_CELLS                   # leaving and entering, read and written, 2 bytes a cell


def fill_random(ctx, arr, per, R, rng):
    """R robots' arrays of `per` int16 values: SEED_ROBOTS generated on the host, the rest device copies."""
    n0 = min(R, SEED_ROBOTS)
    seed = rng.integers(-32768, 32768, (n0, per)).astype(np.int16)
    _lib.check(_lib.load().lslam_h2d(ctx.handle, arr.ptr, seed.ctypes.data, seed.nbytes), "lslam_h2d")
    ctx.sync()
    have = n0
    while have < R:
        n = min(have, R - have)
        ctx.copy(arr.addr + have * per * 2, arr.addr, n * per * 2)
        have += n
    ctx.sync()


class Leg:
    def __init__(self, ctx, R, every, canvas_w):
        """R robots; robot r moves iff every > 0 and r % every == 0.  canvas_w None: the plain recentre."""
        self.ctx, self.R, self.every, self.paged = ctx, R, every, canvas_w is not None
        self.g = OccupancyGrid(ctx, R, canvas_w=canvas_w)
        assert self.g.W == W
        cell = float(self.g.p.cell)
        self.moving = np.array([every > 0 and r % every == 0 for r in range(R)])
        cells = np.where(self.moving[:, None], MOVING_CELL, RESTING_CELL).astype(np.float64)
        self.origin0 = np.array(self.g.origin_host)
        self.pose = np.concatenate([self.origin0 + (cells + 0.5) * cell, np.zeros((R, 1))], 1)
        self.d_pose = ctx.to_device(self.pose)
        rng = np.random.default_rng(R)
        fill_random(ctx, self.g.logodds, W * W, R, rng)
        if self.paged:
            self.win0 = self.g.win.download()
            fill_random(ctx, self.g.canvas, canvas_w * canvas_w, R, rng)
        self.ms = []

    def robot(self, arr, r, side):
        out = np.empty((side, side), np.int16)
        _lib.check(_lib.load().lslam_d2h(self.ctx.handle, out.ctypes.data, arr.addr + r * out.nbytes, out.nbytes), "lslam_d2h")
        self.ctx.sync()
        return out

    def call(self):
        if self.paged:
            self.g.win.upload(self.win0)
        self.g.origin.upload(self.origin0)  # (last in both legs: what precedes the timed call is the same)
        self.g.recentre(self.d_pose, margin=MARGIN, quantum=QUANTUM)

    def check(self):
        """The first paged call against the definition: the first moving robot and the first at rest."""
        if not self.paged:
            return self.call()
        g = self.g
        who = [int(np.flatnonzero(m)[0]) for m in (self.moving, ~self.moving) if m.any()]
        before = {r: (self.robot(g.logodds, r, W), self.robot(g.canvas, r, g.canvas_w)) for r in who}
        self.call()
        res = g.recentre_results()
        for r in who:
            ref = pr.recentre_paged(before[r][0], before[r][1], self.win0[r], self.pose[r], self.origin0[r], margin=MARGIN, quantum=QUANTUM)
            assert np.array_equal(self.robot(g.logodds, r, W), ref["L"]) and np.array_equal(self.robot(g.canvas, r, g.canvas_w), ref["canvas"]), r
            for key in ("origin", "shift", "flags", "win", "moved", "page_flags"):
                assert np.array_equal(res[key][r], ref[key]), (r, key)
            assert tuple(ref["shift"]) == (SHIFT if self.moving[r] else (0, 0))
            assert tuple(ref["moved"]) == ((STRIP_CELLS, STRIP_CELLS) if self.moving[r] else (0, 0))

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


def host_clock(ctx, fn, reps):
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--canvas-w", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "page_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    counts = [int(r) for r in args.robots.split(",")]
    cases = [("all move", r, 1) for r in counts] + [("one in sixteen moves", counts[0], 16), ("none moves", counts[0], 0)]
    legs = [(what, Leg(ctx, r, every, args.canvas_w), Leg(ctx, r, every, None)) for what, r, every in cases]
    for _, paged, plain in legs:
        paged.check()
        plain.check()
    bw = copy_bandwidth(ctx)
    for k in range(args.rounds):
        for _, paged, plain in legs:
            for leg in ((paged, plain) if k % 2 == 0 else (plain, paged)):  # (neither always follows the other)
                leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/pagebench.py; paged and plain legs alternate over %d rounds; recentres by HIP "
                   "events per call (LSLAM_K_RECENTRE), flush, load and lslam_d2d on the host clock over back-to-back calls; "
                   "medians with min and max" % args.rounds,
           "lib": _lib.load().lslam_version().decode(), "grid_w": W, "canvas_w": args.canvas_w, "margin": MARGIN, "quantum": QUANTUM,
           "shift": list(SHIFT), "strip_bytes_per_moving_robot": STRIP_BYTES, "copy_GB_per_s": round(bw / 1e9, 1), "recentre": [],
           "window": []}
    for what, paged, plain in legs:
        n_moving = int(paged.moving.sum())
        p, q = statistics.median(paged.ms), statistics.median(plain.ms)
        row = {"case": what, "robots": paged.R, "robots_moving": n_moving, "paged_ms": stats(paged.ms), "plain_ms": stats(plain.ms),
               "paged_over_plain": round(p / q, 3), "added_ms": round(p - q, 4)}
        if n_moving:
            floor_ms = n_moving * STRIP_BYTES / bw * 1e3
            row.update({"strip_bytes": n_moving * STRIP_BYTES, "strip_floor_ms": round(floor_ms, 4), "added_over_strip_floor": round((p - q) / floor_ms, 2)})
        out["recentre"].append(row)
    # flush and load, each beside a copy of the windows' bytes
    for what, paged, _ in legs[:len(counts)]:
        g, n = paged.g, paged.R * W * W * 2
        a, b = ctx.empty(n, np.uint8), ctx.empty(n, np.uint8)
        a.fill_zero()
        t = {"flush_ms": [], "load_ms": [], "d2d_window_bytes_ms": []}
        for _ in range(args.rounds):
            t["flush_ms"].append(host_clock(ctx, lambda: g.flush(sync=False), args.reps))
            t["load_ms"].append(host_clock(ctx, lambda: g.load(sync=False), args.reps))
            t["d2d_window_bytes_ms"].append(host_clock(ctx, lambda: ctx.copy(b, a), args.reps))
        a.free()
        b.free()
        row = {"robots": paged.R, "window_bytes": n}
        row.update({k: stats(v) for k, v in t.items()})
        d = statistics.median(t["d2d_window_bytes_ms"])
        row.update({"flush_over_d2d": round(statistics.median(t["flush_ms"]) / d, 2), "load_over_d2d": round(statistics.median(t["load_ms"]) / d, 2)})
        out["window"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
