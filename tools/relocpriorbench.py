"""Relocalisation priors' cost: lslam_map_relocalize_prior against lslam_map_relocalize, in one session.

python tools/relocpriorbench.py [--robots 1,64,1024] [--points 720] [--reps 10] [--warmup 2]
                                [--out profiles/relocprior_bench.json]

The setup is tools/relocbench.py's: every robot's map is the L-shaped room of tests/test_reloc_ref.py
(512 cells of 20 mm), seen from a seeded pose inside it, 720 beams.  The map is the one a robot would
have drawn (tests/test_relocprior_ref.py): the same walls and free space, and unknown cells outside the
room, so that the NOT_FREE field of lslam_grid_distance tells the room from what surrounds it; the plain
call reads only the occupied cells and is the same on either map.  Per robot count four calls alternate,
each as the whole call and as its coarse stage alone (LSLAM_RELOC_STAGES=coarse), `reps` times after
`warmup` untimed rounds, each timed on its own with HIP events (LSLAM_K_RELOC):

    plain         lslam_map_relocalize
    null          lslam_map_relocalize_prior with neither prior: the plain call plus the admissibility pass
    field         the free-space prior alone (clear_min2 16)
    field_window  the free-space prior and a window of +-1000 mm, +-0.5 rad around a pose 600 mm and
                  0.3 rad off the truth

Figures are medians with minimum and maximum.  The shares come from n_admit and from the admissible bits
rebuilt on the host (tests/relocprior_ref.py): live spans are the (row, span of 32 cells) tasks that hold
an admissible cell.  floor = the plain coarse stage x live spans / all spans x admissible headings /
n_head: what the search would cost if only its additions counted.  Robot 0 of every call is held to the
caps of the CPU test; lost_of_found counts the robots that the plain call finds and a call with a prior does not.
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

import relocprior_ref as rp  # noqa: E402
import test_reloc_ref as scenes  # noqa: E402
import test_relocprior_ref as seen  # noqa: E402
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.localize import GridRelocalizer  # noqa: E402
from lidar_slam_amd.mapping import DistanceField, OccupancyGrid  # noqa: E402
from relocbench import Env, poses_in_the_room, stats  # noqa: E402

CALLS = ("plain", "null", "field", "field_window")


class Leg:
    def __init__(self, ctx, R, Np):
        self.ctx, self.R = ctx, R
        self.truth = poses_in_the_room(R)
        revs = [scenes.revolution(scenes.L_OUTLINE, p, 5000 + r, Np) for r, p in enumerate(self.truth)]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.grid = OccupancyGrid(ctx, R, origin=scenes.SCENE_ORIGIN)
        self.L = seen.seen_scene("L")[0]
        self.grid.upload(np.ascontiguousarray(np.broadcast_to(self.L, (R,) + self.L.shape)))  # the same map for every robot
        self.field = DistanceField(self.grid, mode=_lib.DIST_NOT_FREE)
        self.field.step()
        self.d_xy = ctx.to_device(np.concatenate(revs))
        self.stale = self.truth + seen.WINDOW_OFF
        self.d_stale = ctx.to_device(np.ascontiguousarray(self.stale))
        self.rel = GridRelocalizer(ctx, R)
        self.ms = {(c, s): [] for c in CALLS for s in ("whole", "coarse")}

    def call(self, which, sync=True):
        self.rel.relocalize(self.d_xy, self.sco, self.off, grid=self.grid, sync=sync, prior=which == "null",
                            field=self.field if which in ("field", "field_window") else None,
                            window=self.d_stale if which == "field_window" else None)

    def check(self):
        """The four calls' results; the shares of the two priors."""
        out, q = {}, self.rel.q
        for which in CALLS:
            self.call(which)
            out[which] = self.rel.results()
        plain = out["plain"]
        for k in plain:  # the identity
            a, b = (v[k].view(np.uint64) if v[k].dtype == np.float64 else v[k] for v in (plain, out["null"]))
            assert np.array_equal(a, b), k
        found = plain["flags"] == 0
        for which in CALLS:
            res = out[which]
            dpos, dth = scenes.pose_error(res["pose"][0], self.truth[0])
            assert res["flags"][0] == 0 and dpos <= scenes.CAP_MM and dth <= scenes.CAP_RAD, (which, res["flags"][0], dpos, dth)
            res["lost_of_found"] = int(np.count_nonzero(res["flags"][found] != 0))  # robots the plain call finds and this does not
        W, f = self.grid.W, int(q.factor)
        Wc, nspan = W // f, (W // f + 31) // 32
        d2 = self.field.d2.download()[0]
        assert np.array_equal(d2, seen.seen_scene("L")[1])
        Af = rp.field_admissible(d2, W, f, int(self.rel.pp.clear_min2))
        shares = {}
        for which, wins in (("field", [None]), ("field_window", self.stale)):
            live = cells = 0
            for w in wins:
                A = Af & rp.window_admissible(w, scenes.SCENE_ORIGIN, Wc, self.grid.p.cell * f, self.rel.pp.half_xy)
                pad = np.zeros((Wc, nspan * 32), bool)
                pad[:, :Wc] = A
                live += int(pad.reshape(Wc, nspan, 32).any(2).sum())
                cells += int(A.sum())
            n = len(wins)
            na = out[which]["n_admit"]
            assert int(na[:, 0].sum()) == cells * (self.R if n == 1 else 1), which
            shares[which] = {"cells": round(cells / n / (Wc * Wc), 4), "live_spans": round(live / n / (Wc * nspan), 4),
                             "headings": round(float(na[:, 1].mean()) / int(q.n_head), 4)}
        return out, shares

    def timed(self, reps, warmup):
        ctx = self.ctx
        legs = [(c, s) for c in CALLS for s in ("whole", "coarse")]

        def run(c, s, sync):
            if s == "coarse":
                with Env(LSLAM_RELOC_STAGES="coarse"):
                    self.call(c, sync)
            else:
                self.call(c, sync)

        for _ in range(warmup):
            for c, s in legs:
                run(c, s, True)
        ctx.set_timing(True, kernels=[_lib.K_RELOC])
        for _ in range(reps):
            for c, s in legs:
                ctx.timing_reset()
                run(c, s, False)
                ms, n = ctx.timing(_lib.K_RELOC)
                assert n == 1, n
                self.ms[(c, s)].append(ms)
        ctx.set_timing(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="1,64,1024")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relocprior_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    out = {"note": "one session on one MI355X: tools/relocpriorbench.py; per robot count the plain call, the prior call with "
                   "neither prior, with the field, and with the field and a window alternate, each whole and as its coarse "
                   "stage alone; HIP events per call; medians with min and max; floor = plain coarse x live spans x headings",
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "reps": args.reps, "warmup": args.warmup,
           "legs": []}
    for R in (int(r) for r in args.robots.split(",")):
        leg = Leg(ctx, R, args.points)
        res, shares = leg.check()
        leg.timed(args.reps, args.warmup)
        med = {k: statistics.median(v) for k, v in leg.ms.items()}
        q = leg.rel.q
        Wc = leg.grid.W // int(q.factor)
        row = {"robots": R, "map_w": leg.grid.W, "coarse": [int(q.n_head), Wc, Wc], "n_cand": leg.rel.K, "shares": shares,
               "flags_count": {c: {str(f): int(np.count_nonzero(res[c]["flags"] == f)) for f in np.unique(res[c]["flags"])}
                               for c in CALLS},
               "lost_of_found": {c: res[c]["lost_of_found"] for c in CALLS}}
        for c in CALLS:
            row[c] = {"whole_call_ms": stats(leg.ms[(c, "whole")]), "coarse_stage_ms": stats(leg.ms[(c, "coarse")]),
                      "coarse_over_plain": round(med[(c, "coarse")] / med[("plain", "coarse")], 3),
                      "whole_over_plain": round(med[(c, "whole")] / med[("plain", "whole")], 3)}
        row["null"]["coarse_minus_plain_ms"] = round(med[("null", "coarse")] - med[("plain", "coarse")], 4)
        row["null"]["whole_minus_plain_ms"] = round(med[("null", "whole")] - med[("plain", "whole")], 4)
        for c in ("field", "field_window"):
            s = shares[c]
            floor = med[("plain", "coarse")] * s["live_spans"] * s["headings"]
            row[c]["floor_ms"] = round(floor, 4)
            row[c]["coarse_over_floor"] = round(med[(c, "coarse")] / floor, 2)
        out["legs"].append(row)
        del leg
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
