"""Field-alignment cost: one default lslam_field_align call (n_iter 10) for many robots in the bench
room's grids, from guesses one cell and 0.01 rad off the poses the maps were built at; beside it, in the
same session, a default lslam_map_match call from the same guesses, and n_iter + 1 lslam_field_score
calls, the alignment's derived floor (one gather pass per evaluation, without the gradient's three more
corners, the reduction of ten sums or the solve).

python tools/fieldalignbench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 5] [--out profiles/fieldalign_bench.json]

The fleets, their grids and revolutions are tools/distbench.py's room legs (grid_w 512, d_max 64).
Inputs are resident on the device.  There is no timing slot for these calls: every figure is `reps`
back-to-back calls between two lslam_sync on the host clock, divided by `reps`, after a warm-up; the
legs alternate, `rounds` times, and the figures are medians over the rounds with minimum and maximum.
Seed robot 0's alignment is asserted against the NumPy definition (tests/fieldalign_ref.py) first.
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

import fieldalign_ref as far  # noqa: E402
from distbench import Leg, host_timed, seed_room, stats  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.localize import GridLocalizer  # noqa: E402
from lidar_slam_amd.mapping import FIELDALIGN_CONVERGED, FIELDALIGN_REJECTED  # noqa: E402


class AlignLeg(Leg):
    def __init__(self, ctx, R, Np, poses, revs):
        super().__init__(ctx, R, Np, poses, revs, "room")
        self.scratch = self.rc = None  # (distbench's other legs are not timed here)
        self.guess = self.poses + np.array([20.0, -20.0, 0.01])  # one default cell on each axis
        self.d_guess = ctx.to_device(self.guess)
        self.loc = GridLocalizer(ctx, R)

    def check(self):
        n_src = super().check()
        self.f.align(self.d_xy, self.sco, self.off, pose=self.d_guess)
        res = self.f.align_results()
        want = far.align(self.robot0(self.f.d2, np.uint16), self.rev0, self.guess[0], res["trace"][0][:, 3:5],
                         self.g.origin_host[0])
        assert np.array_equal(res["pose_out"][0], want["pose_out"]) and np.array_equal(res["normal"][0], want["normal"])
        assert res["iters"][0] == want["iters"] and res["flags"][0] == want["flags"]
        err = res["pose_out"] - self.poses
        self.summary = {"mean_iters": round(float(res["iters"].mean()), 2),
                        "converged_share": round(float(np.mean((res["flags"] & FIELDALIGN_CONVERGED) != 0)), 4),
                        "rejected_share": round(float(np.mean((res["flags"] & FIELDALIGN_REJECTED) != 0)), 4),
                        "median_error_mm": round(float(np.median(np.hypot(err[:, 0], err[:, 1]))), 2),
                        "max_error_mm": round(float(np.hypot(err[:, 0], err[:, 1]).max()), 2),
                        "max_error_mrad": round(float(1e3 * np.abs(err[:, 2]).max()), 3)}
        return n_src

    def timed(self, reps):
        ctx, f = self.ctx, self.f
        add = lambda k, ms: self.t.setdefault(k, []).append(ms)
        evals = int(f.a.n_iter) + 1

        def scores():
            for _ in range(evals):
                f.score(self.d_xy, self.sco, self.off, pose=self.d_guess, sync=False)
        add("field_align_ms", host_timed(ctx, lambda: f.align(self.d_xy, self.sco, self.off, pose=self.d_guess, sync=False), reps))
        add("field_scores_ms", host_timed(ctx, scores, reps))
        add("map_match_ms", host_timed(ctx, lambda: self.loc.step(self.d_xy, self.sco, self.off, grid=self.g, pose=self.d_guess,
                                                                   sync=False), reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fieldalign_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    poses, revs = seed_room(args.points)
    legs = [AlignLeg(ctx, int(r), args.points, poses, revs) for r in args.robots.split(",")]
    for leg in legs:
        leg.check()
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/fieldalignbench.py; legs alternate over %d rounds; every figure is %d "
                   "back-to-back calls between two lslam_sync on the host clock, per call; medians with min and max; "
                   "field_scores_ms is n_iter + 1 lslam_field_score calls" % (args.rounds, args.reps),
           "lib": _lib.load().lslam_version().decode(), "grid_w": legs[0].g.W, "d_max": int(legs[0].f.p.d_max),
           "n_iter": int(legs[0].f.a.n_iter), "points_per_robot": args.points, "legs": []}
    for leg in legs:
        row = {"robots": leg.R}
        row.update(leg.summary)
        row.update({k: stats(v) for k, v in leg.t.items()})
        med = {k: statistics.median(v) for k, v in leg.t.items()}
        row["align_to_scores"] = round(med["field_align_ms"] / med["field_scores_ms"], 2)
        row["map_match_to_align"] = round(med["map_match_ms"] / med["field_align_ms"], 2)
        out["legs"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
