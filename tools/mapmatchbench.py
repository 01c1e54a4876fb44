"""Scan-to-map matching cost: one default-window lslam_map_match call for many robots, beside a
default scan-match call of the same session.

python tools/mapmatchbench.py [--robots 4096,256,1] [--points 720] [--reps 20] [--warmup 3] [--cus 256]
                              [--out profiles/mapmatch_bench.json]

Robot r sees the synthetic room from synth.scan_polar(r)'s pose; its map (512 cells of 20 mm, centred
on it) is one lslam_grid_update of that revolution, made on the device; the revolution after a small
motion is the scan matcher's current scan and the localiser's revolution, the guess being the moved
pose off by up to 100 mm and 0.05 rad.  Inputs are resident on the device.  Per robot count three
calls alternate, `reps` times after `warmup` untimed rounds, each call timed on its own with HIP
events (LSLAM_K_MATCH, LSLAM_K_MAPMATCH): the scan-match call, the scan-to-map call, and the
scan-to-map call with the window read a lane per cell (LSLAM_MAPMATCH_FORM=cell: the form that maps
whose rows are not on 16-byte boundaries take, measured against the 16-byte groups that ship).
Figures are medians with minimum and maximum.  Also recorded: the ratio of the scan-to-map median to
the scan-match median, and the HBM bytes of the window reads: rows x columns of the window on the map
x 2 bytes per workgroup, times robots x rotation slices (the launcher's rule for `cus` compute
units), as bytes per call and over the call's whole time (window_GB_per_s).  Robot 0's result is
asserted against the NumPy definition (tests/mapmatch_ref.py), and both forms give the same bytes.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mapmatch_ref as mmr  # noqa: E402
import scanmatch_ref as smr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.localize import GridLocalizer  # noqa: E402
from lidar_slam_amd.mapping import OccupancyGrid  # noqa: E402
from lidar_slam_amd.odometry import ScanMatcher  # noqa: E402


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def slices(R, Nth, cus):
    """Rotation slices per robot: the rule of launch_match / launch_mapmatch."""
    ns = min(max((2 * cus + R - 1) // R, 1), Nth)
    per = (Nth + ns - 1) // ns
    return (Nth + per - 1) // per


class Leg:
    def __init__(self, ctx, R, Np):
        rng = np.random.default_rng(5)
        refs, curs, p0s, p1s = [], [], [], []
        for r in range(R):
            p0 = synth.scan_polar(r)[2]
            d = np.array([rng.uniform(-150, 150), rng.uniform(-60, 60), np.deg2rad(rng.uniform(-8, 8))])
            p1 = smr.compose(p0, d)
            refs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 2 * r, Np)))
            curs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p1, 2 * r + 1, Np)))
            p0s.append(p0)
            p1s.append(p1)
        self.ctx, self.R, self.Np = ctx, R, Np
        self.cur0 = curs[0]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.guess = np.array(p1s) + rng.uniform(-1.0, 1.0, (R, 3)) * [100.0, 100.0, 0.05]
        self.m = ScanMatcher(ctx, R)
        self.loc = GridLocalizer(ctx, R)
        self.g = OccupancyGrid.centred_on(ctx, np.array(p0s))
        self.d_ref, self.d_cur = ctx.to_device(np.concatenate(refs)), ctx.to_device(np.concatenate(curs))
        self.d_off = ctx.to_device(self.off)
        self.d_guess = ctx.to_device(self.guess)
        self.g.step(self.d_ref, self.sco, self.off, pose=np.array(p0s))  # the map: one revolution from p0
        self.match_ms, self.map_ms, self.cell_ms = [], [], []

    def match_call(self, sync=True):
        self.m.match(self.d_ref, self.d_off, self.d_cur, self.d_off, sync=sync)

    def map_call(self, sync=True):
        self.loc.step(self.d_cur, self.sco, self.off, grid=self.g, pose=self.d_guess, sync=sync)

    def cell_call(self, sync=True):
        os.environ["LSLAM_MAPMATCH_FORM"] = "cell"
        try:
            self.map_call(sync)
        finally:
            os.environ.pop("LSLAM_MAPMATCH_FORM", None)

    def check(self):
        """Robot 0 against the definition; returns the window's cells on the map, summed over robots."""
        W = self.g.W
        one = self.ctx.empty((W, W), np.int16)
        self.ctx.copy(one, self.g.logodds.addr, 2 * W * W)
        self.cell_call()
        other = self.loc.results()
        self.map_call()
        res = self.loc.results()
        for k in res:
            assert np.array_equal(res[k], other[k]), k
        want = mmr.match(one.download(), self.g.origin_host[0], self.guess[0], self.cur0, rot0=res["rot0"][0],
                         rot=self.loc.rot_host, grid_w=W)
        one.free()
        assert res["best"][0].tolist() == want["best"].tolist(), (res["best"][0], want["best"])
        assert res["flags"][0] == want["flags"] and np.array_equal(res["pose"][0], want["pose_out"])
        assert np.array_equal(res["n_valid"][0], want["n_valid"])
        half, ww = self.loc.p.win_w // 2, self.loc.p.win_w
        cell0 = np.floor((self.guess[:, :2] - self.g.origin_host) / self.g.p.cell).astype(np.int64) - half
        span = np.clip(np.minimum(cell0 + ww, W) - np.maximum(cell0, 0), 0, None)
        return int((span[:, 0] * span[:, 1]).sum()), res

    def timed(self, reps, warmup):
        ctx = self.ctx
        for _ in range(warmup):
            self.match_call()
            self.map_call()
            self.cell_call()
        ctx.set_timing(True, kernels=[_lib.K_MATCH, _lib.K_MAPMATCH])
        for _ in range(reps):
            for call, kid, acc in ((self.match_call, _lib.K_MATCH, self.match_ms), (self.map_call, _lib.K_MAPMATCH, self.map_ms),
                                   (self.cell_call, _lib.K_MAPMATCH, self.cell_ms)):
                ctx.timing_reset()
                call(sync=False)
                ms, n = ctx.timing(kid)
                assert n == 1
                acc.append(ms)
        ctx.set_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (MI355X: 256): the slice rule")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapmatch_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    out = {"note": "one session on one MI355X: tools/mapmatchbench.py; per robot count a scan-match call and a "
                   "scan-to-map call alternate; HIP events per call; medians with min and max",
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "reps": args.reps, "warmup": args.warmup,
           "legs": []}
    for R in (int(r) for r in args.robots.split(",")):
        leg = Leg(ctx, R, args.points)
        cells, res = leg.check()
        leg.timed(args.reps, args.warmup)
        ns = slices(R, leg.loc.Nth, args.cus)
        mm, sm = statistics.median(leg.map_ms), statistics.median(leg.match_ms)
        out["legs"].append({"robots": R, "map_w": leg.g.W, "window": [leg.loc.Nth, leg.loc.Nt, leg.loc.Nt],
                            "win_w": int(leg.loc.p.win_w), "slices_per_robot": ns,
                            "scan_match_ms": stats(leg.match_ms), "map_match_ms": stats(leg.map_ms),
                            "map_match_cell_per_lane_ms": stats(leg.cell_ms),
                            "ratio_to_scan_match": round(mm / sm, 3), "robots_per_s": round(R / mm * 1e3, 1),
                            "window_bytes_per_call": 2 * cells * ns,
                            "window_GB_per_s": round(2 * cells * ns / mm / 1e6, 1),
                            "flags_count": {str(f): int(np.count_nonzero(res["flags"] == f)) for f in np.unique(res["flags"])}})
        del leg
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
