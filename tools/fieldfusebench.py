"""Field-fusion cost: one default lslam_field_fuse call (the alignment's launch, then one thread per robot
for the update) for many robots in the bench room's grids, from guesses one cell and 0.01 rad off the
poses the maps were built at, with P = diag(50^2, 50^2, 0.05^2); beside it, in the same session and on the
same inputs, a default lslam_field_align call, the fusion's derived floor but for one small launch, and a
default lslam_map_fuse call, the correlative matcher's form of the same step.

python tools/fieldfusebench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 5] [--out profiles/fieldfuse_bench.json]

The method is tools/fieldalignbench.py's: its fleets, grids and revolutions, inputs resident on the device,
no timing slot; every figure is `reps` back-to-back calls between two lslam_sync on the host clock, divided
by `reps`, after a warm-up; the legs alternate, `rounds` times, and the figures are medians over the rounds
with minimum and maximum.  The filter is only read (write_back=False), so that every call sees the same
inputs.  Seed robot 0's fusion is asserted against the NumPy definition (tests/fieldfuse_ref.py) first.
No threshold is set on the ratios.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import fieldfuse_ref as ffr  # noqa: E402
from distbench import host_timed, seed_room, stats  # noqa: E402
from fieldalignbench import AlignLeg  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import FIELDALIGN_REJECTED, FIELDFUSE_BAD_COV, FIELDFUSE_OUTLIER  # noqa: E402

P0 = np.diag([50.0 ** 2, 50.0 ** 2, 0.05 ** 2])


class FuseLeg(AlignLeg):
    def __init__(self, ctx, R, Np, poses, revs):
        super().__init__(ctx, R, Np, poses, revs)
        self.d_P = ctx.to_device(np.tile(P0.reshape(9), (R, 1)))

    def check(self):
        n_src = super().check()
        self.f.fuse(self.d_xy, self.sco, self.off, x=self.d_guess, P=self.d_P, write_back=False)
        res = self.f.fuse_results()
        want = ffr.fuse(self.robot0(self.f.d2, np.uint16), self.rev0, self.guess[0], P0, res["trace"][0][:, 3:5],
                        self.g.origin_host[0])
        for k in ("pose_out", "P_out", "z", "info", "info_f", "s2", "nis", "normal"):
            assert np.array_equal(np.asarray(res[k][0]), np.asarray(want[k])), k
        assert res["flags"][0] == want["flags"]
        err = res["pose_out"] - self.poses
        sig = np.sqrt(np.diagonal(res["P_out"], axis1=1, axis2=2))
        self.summary = {"rejected_by_align_share": round(float(np.mean((res["flags"] & FIELDALIGN_REJECTED) != 0)), 4),
                        "outlier_share": round(float(np.mean((res["flags"] & FIELDFUSE_OUTLIER) != 0)), 4),
                        "bad_cov_share": round(float(np.mean((res["flags"] & FIELDFUSE_BAD_COV) != 0)), 4),
                        "median_error_mm": round(float(np.median(np.hypot(err[:, 0], err[:, 1]))), 2),
                        "max_error_mm": round(float(np.hypot(err[:, 0], err[:, 1]).max()), 2),
                        "max_nis": round(float(res["nis"].max()), 3),
                        "median_sigma_mm_mm_mrad": [round(float(v), 3) for v in np.median(sig, 0) * [1.0, 1.0, 1e3]]}
        return n_src

    def timed(self, reps):
        ctx, f = self.ctx, self.f
        add = lambda k, ms: self.t.setdefault(k, []).append(ms)  # noqa: E731
        add("field_fuse_ms", host_timed(ctx, lambda: f.fuse(self.d_xy, self.sco, self.off, x=self.d_guess, P=self.d_P,
                                                            write_back=False, sync=False), reps))
        add("field_align_ms", host_timed(ctx, lambda: f.align(self.d_xy, self.sco, self.off, pose=self.d_guess, sync=False), reps))
        add("map_fuse_ms", host_timed(ctx, lambda: self.loc.fuse(self.d_xy, self.sco, self.off, grid=self.g, x=self.d_guess,
                                                                 P=self.d_P, write_back=False, sync=False), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldfuse_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    poses, revs = seed_room(args.points)
    legs = [FuseLeg(ctx, int(r), args.points, poses, revs) for r in args.robots.split(",")]
    for leg in legs:
        leg.check()
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/fieldfusebench.py; legs alternate over %d rounds; every figure is %d "
                   "back-to-back calls between two lslam_sync on the host clock, per call; medians with min and max; the "
                   "three calls read the same guesses and the same P" % (args.rounds, args.reps),
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0].g.W, "d_max": int(legs[0].f.p.d_max),
           "n_iter": int(legs[0].f.a.n_iter), "points_per_robot": args.points, "legs": []}
    for leg in legs:
        row = {"robots": leg.R}
        row.update(leg.summary)
        row.update({k: stats(v) for k, v in leg.t.items()})
        med = {k: statistics.median(v) for k, v in leg.t.items()}
        row["fuse_to_align"] = round(med["field_fuse_ms"] / med["field_align_ms"], 3)
        row["map_fuse_to_field_fuse"] = round(med["map_fuse_ms"] / med["field_fuse_ms"], 2)
        out["legs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
