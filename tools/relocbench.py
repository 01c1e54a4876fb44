"""Global relocalisation cost: one default lslam_map_relocalize call for many robots, its coarse stage
alone in both forms, and the K lslam_map_match calls that its fine stage amounts to.

python tools/relocbench.py [--robots 1,64,1024] [--points 720] [--reps 10] [--warmup 2]
                           [--out profiles/reloc_bench.json]

Every robot's map is the L-shaped room of tests/test_reloc_ref.py (512 cells of 20 mm, the walls one
cell thick); robot r sees it from a seeded pose inside the room, 720 beams with synth.scan_polar_at's
noise model.  Inputs are resident on the device.  Per robot count four calls alternate, `reps` times
after `warmup` untimed rounds, each timed on its own with HIP events: the whole call (LSLAM_K_RELOC),
the coarse stage alone (search, peaks and the K best; LSLAM_RELOC_STAGES=coarse), the coarse stage
alone with the plain search form, one addition per cell and point (LSLAM_RELOC_FORM=add: the form
that was measured and dropped), and K default lslam_map_match calls from the K candidate poses of the
whole call (LSLAM_K_MAPMATCH, summed): the fine stage's cost and the floor the coarse stage is judged
against.  Figures are medians with minimum and maximum.  Robot 0 is held to the caps of the CPU test
(30 mm, 0.0131 rad, no flag), and both search forms give the same candidates.
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

import test_reloc_ref as scenes  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.localize import GridLocalizer, GridRelocalizer  # noqa: E402
from lidar_slam_amd.mapping import OccupancyGrid  # noqa: E402


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def poses_in_the_room(R):
    """Seeded poses at least 500 mm from every wall of the L-shaped room."""
    rng = np.random.default_rng(11)
    out = []
    while len(out) < R:
        x, y = rng.uniform(500.0, 3500.0), rng.uniform(500.0, 2500.0)
        if x > 2500.0 and y > 1500.0:
            continue
        out.append((x, y, rng.uniform(0.0, 2 * np.pi)))
    return np.array(out)


class Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k in self.kw:
            os.environ.pop(k, None)


class Leg:
    def __init__(self, ctx, R, Np):
        self.ctx, self.R = ctx, R
        self.truth = poses_in_the_room(R)
        revs = [scenes.revolution(scenes.L_OUTLINE, p, 5000 + r, Np) for r, p in enumerate(self.truth)]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.grid = OccupancyGrid(ctx, R, origin=scenes.SCENE_ORIGIN)
        L = scenes.draw_walls(scenes.L_OUTLINE)
        self.grid.upload(np.ascontiguousarray(np.broadcast_to(L, (R,) + L.shape)))  # the same map for every robot
        self.d_xy = ctx.to_device(np.concatenate(revs))
        self.rel = GridRelocalizer(ctx, R)
        self.loc = GridLocalizer(ctx, R)
        self.K = self.rel.K
        self.whole_ms, self.coarse_ms, self.add_ms, self.fine_ms = [], [], [], []
        self.d_cand = None

    def whole_call(self, sync=True):
        self.rel.relocalize(self.d_xy, self.sco, self.off, grid=self.grid, sync=sync)

    def coarse_call(self, sync=True):
        with Env(LSLAM_RELOC_STAGES="coarse"):
            self.whole_call(sync)

    def add_call(self, sync=True):
        with Env(LSLAM_RELOC_STAGES="coarse", LSLAM_RELOC_FORM="add"):
            self.whole_call(sync)

    def fine_calls(self, sync=True):
        for j in range(self.K):
            self.loc.step(self.d_xy, self.sco, self.off, grid=self.grid, pose=self.d_cand[j], sync=False)
        if sync:
            self.ctx.sync()

    def check(self):
        self.add_call()
        other = self.rel.results()
        self.whole_call()
        res = self.rel.results()
        for k in ("cand", "n_occ", "n_used"):
            assert np.array_equal(res[k], other[k]), k
        assert res["flags"][0] == 0, res["flags"][0]
        dpos, dth = scenes.pose_error(res["pose"][0], self.truth[0])
        assert dpos <= scenes.CAP_MM and dth <= scenes.CAP_RAD, (dpos, dth)
        self.d_cand = [self.ctx.to_device(np.ascontiguousarray(res["cand_pose"][j])) for j in range(self.K)]
        ok = res["flags"] == 0
        err = np.array([scenes.pose_error(res["pose"][r], self.truth[r]) for r in np.nonzero(ok)[0]])
        return res, err

    def timed(self, reps, warmup):
        ctx = self.ctx
        legs = ((self.whole_call, _lib.K_RELOC, 1, self.whole_ms), (self.coarse_call, _lib.K_RELOC, 1, self.coarse_ms),
                (self.add_call, _lib.K_RELOC, 1, self.add_ms), (self.fine_calls, _lib.K_MAPMATCH, self.K, self.fine_ms))
        for _ in range(warmup):
            for call, _, _, _ in legs:
                call()
        ctx.set_timing(True, kernels=[_lib.K_RELOC, _lib.K_MAPMATCH])
        for _ in range(reps):
            for call, kid, n_want, acc in legs:
                ctx.timing_reset()
                call(sync=False)
                ms, n = ctx.timing(kid)
                assert n == n_want, (n, n_want)
                acc.append(ms)
        ctx.set_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="1,64,1024")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reloc_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    out = {"note": "one session on one MI355X: tools/relocbench.py; per robot count the whole call, the coarse stage alone "
                   "in both search forms and K map-match calls alternate; HIP events per call; medians with min and max",
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "reps": args.reps, "warmup": args.warmup,
           "legs": []}
    for R in (int(r) for r in args.robots.split(",")):
        leg = Leg(ctx, R, args.points)
        res, err = leg.check()
        leg.timed(args.reps, args.warmup)
        q = leg.rel.q
        whole, coarse, add, fine = (statistics.median(v) for v in (leg.whole_ms, leg.coarse_ms, leg.add_ms, leg.fine_ms))
        Wc = leg.grid.W // int(q.factor)
        out["legs"].append({"robots": R, "map_w": leg.grid.W, "coarse": [int(q.n_head), Wc, Wc], "n_cand": leg.K,
                            "whole_call_ms": stats(leg.whole_ms), "coarse_stage_ms": stats(leg.coarse_ms),
                            "coarse_stage_add_form_ms": stats(leg.add_ms), "k_map_match_calls_ms": stats(leg.fine_ms),
                            "coarse_over_fine": round(coarse / fine, 3), "whole_over_fine": round(whole / fine, 3),
                            "add_form_over_bit_sliced": round(add / coarse, 3),
                            "robots_per_s": round(R / whole * 1e3, 1),
                            "coarse_lookups_per_s": round(R * int(q.n_head) * Wc * Wc * args.points / coarse * 1e3, 1),
                            "flags_count": {str(f): int(np.count_nonzero(res["flags"] == f)) for f in np.unique(res["flags"])},
                            "found_worst_mm": round(float(err[:, 0].max()), 2), "found_worst_rad": round(float(err[:, 1].max()), 5)})
        del leg
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
