"""Match-fusion cost: one default-window lslam_map_fuse call for many robots, beside the
lslam_map_match call of the same session that it extends.

python tools/mapfusebench.py [--robots 4096,256,1] [--points 720] [--reps 20] [--warmup 3]
                             [--out profiles/mapfuse_bench.json]

The inputs are those of tools/mapmatchbench.py: robot r sees the synthetic room from
synth.scan_polar(r)'s pose; its map (512 cells of 20 mm, centred on it) is one lslam_grid_update of
that revolution, made on the device; the revolution after a small motion is localised from the moved
pose off by up to 100 mm and 0.05 rad, and the filter's covariance is diag(100^2, 100^2, 0.05^2).
Inputs are resident on the device and neither call writes the filter back.  Per robot count the two
calls alternate, `reps` times after `warmup` untimed rounds, each call timed on its own with HIP
events (LSLAM_K_MAPMATCH, LSLAM_K_MAPFUSE).  Figures are medians with minimum and maximum.  Also
recorded: the ratio of the fuse median to the match median, the difference of the medians (the new
work: a second walk of the score volume, the moments and the FP64 update of thread 0), and the floor
of that work derived from two reads of the score volume at the 5.09 TB/s that a copy reached on an
MI355X (derived, not measured: most of the second walk is served by L2).  Robot 0's result is
asserted against the NumPy definition (tests/mapfuse_ref.py).
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

import mapfuse_ref as mfr  # noqa: E402
import scanmatch_ref as smr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.localize import GridLocalizer  # noqa: E402
from lidar_slam_amd.mapping import OccupancyGrid  # noqa: E402

COPY_TB_PER_S = 5.09
P_DIAG = (100.0 ** 2, 100.0 ** 2, 0.05 ** 2)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


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
        self.P = np.tile(np.diag(P_DIAG), (R, 1, 1))
        self.loc = GridLocalizer(ctx, R)
        self.g = OccupancyGrid.centred_on(ctx, np.array(p0s))
        d_ref = ctx.to_device(np.concatenate(refs))
        self.d_cur = ctx.to_device(np.concatenate(curs))
        self.d_guess = ctx.to_device(self.guess)
        self.d_P = ctx.to_device(self.P.reshape(R, 9))
        self.g.step(d_ref, self.sco, self.off, pose=np.array(p0s))  # the map: one revolution from p0
        self.match_ms, self.fuse_ms = [], []

    def match_call(self, sync=True):
        self.loc.step(self.d_cur, self.sco, self.off, grid=self.g, pose=self.d_guess, sync=sync)

    def fuse_call(self, sync=True):
        self.loc.fuse(self.d_cur, self.sco, self.off, grid=self.g, x=self.d_guess, P=self.d_P, write_back=False, sync=sync)

    def check(self):
        """Robot 0 against the definition; the match of the same inputs gives the same winner."""
        W = self.g.W
        one = self.ctx.empty((W, W), np.int16)
        self.ctx.copy(one, self.g.logodds.addr, 2 * W * W)
        self.match_call()
        m = self.loc.results()
        self.fuse_call()
        res = self.loc.results()
        for k in ("delta", "best", "n_valid", "rot0"):
            assert np.array_equal(res[k], m[k]), k
        want = mfr.fuse(one.download(), self.g.origin_host[0], self.guess[0], self.P[0], self.cur0, rot0=res["rot0"][0],
                        rot=self.loc.rot_host, grid_w=W)
        one.free()
        assert res["flags"][0] == want["flags"] and res["moments"][0].tolist() == want["moments"].tolist()
        for k, wk in (("pose", "pose_out"), ("P", "P_out"), ("z", "z"), ("Rm", "Rm"), ("nis", "nis")):
            assert np.array_equal(np.asarray(res[k][0]).view(np.uint64), np.asarray(want[wk], np.float64).view(np.uint64)), k
        return res

    def timed(self, reps, warmup):
        ctx = self.ctx
        for _ in range(warmup):
            self.match_call()
            self.fuse_call()
        ctx.set_timing(True, kernels=[_lib.K_MAPMATCH, _lib.K_MAPFUSE])
        for _ in range(reps):
            for call, kid, acc in ((self.match_call, _lib.K_MAPMATCH, self.match_ms), (self.fuse_call, _lib.K_MAPFUSE, self.fuse_ms)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapfuse_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    out = {"note": "one session on one MI355X: tools/mapfusebench.py; per robot count a scan-to-map call and a "
                   "match-fusion call of the same inputs alternate; HIP events per call; medians with min and max; "
                   "floor_ms is derived (two reads of the score volume at %.2f TB/s), not measured" % COPY_TB_PER_S,
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "reps": args.reps, "warmup": args.warmup,
           "legs": []}
    for R in (int(r) for r in args.robots.split(",")):
        leg = Leg(ctx, R, args.points)
        res = leg.check()
        leg.timed(args.reps, args.warmup)
        mm, fm = statistics.median(leg.match_ms), statistics.median(leg.fuse_ms)
        vol = 4 * R * leg.loc.Nth * leg.loc.Nt * leg.loc.Nt
        out["legs"].append({"robots": R, "map_w": leg.g.W, "window": [leg.loc.Nth, leg.loc.Nt, leg.loc.Nt],
                            "volume_bytes": vol, "map_match_ms": stats(leg.match_ms), "map_fuse_ms": stats(leg.fuse_ms),
                            "ratio_to_map_match": round(fm / mm, 4), "added_ms": round(fm - mm, 4),
                            "floor_ms": round(2 * vol / (COPY_TB_PER_S * 1e9), 4),
                            "robots_per_s": round(R / fm * 1e3, 1),
                            "flags_count": {str(f): int(np.count_nonzero(res["flags"] == f)) for f in np.unique(res["flags"])},
                            "nis_median": round(float(np.median(res["nis"])), 3)})
        del leg
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
