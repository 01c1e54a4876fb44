"""Occupancy-grid mapping cost: one default lslam_grid_update call for many robots, beside the C3
step and a default scan-match call of the same session.

python tools/gridbench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 7]
                          [--no-c3] [--baseline-tree DIR] [--out profiles/grid_bench.json]

Robot r sees the synthetic room from synth.scan_polar(r)'s pose; its grid (512 cells of 20 mm) is
centred on it; the revolution after a small motion is the scan matcher's pair.  Inputs are
resident on the device.  The legs alternate, `rounds` times:
  * C3: `python bench.py --gpus 1 --steps 50 --warmup 10 --no-cpu-baseline` in a child process
    (and, with --baseline-tree, the same command in that checkout: the parent commit's build);
  * per robot count: `reps` scan-match calls, then `reps` times one grid call of every form
    (the shipped one and the forms that were measured and dropped, through LSLAM_GRID_FORM), each
    call timed on its own with HIP events (LSLAM_K_MATCH, LSLAM_K_GRID).
Figures are medians over all rounds, with minimum and maximum.  Also recorded: the copy bandwidth
of the session (a device-to-device copy of the grids, bytes read + bytes written per second), the
tiles a call touches (counted on the downloaded grids after one call from zero), the call's HBM
floor = 2 x the bytes of the touched tiles / that bandwidth, and the ratio of the shipped form to
it.  Robot 0's grid is asserted against the NumPy definition (tests/occgrid_ref.py).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import occgrid_ref as ogr  # noqa: E402
import scanmatch_ref as smr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import TILE, OccupancyGrid  # noqa: E402
from lidar_slam_amd.odometry import ScanMatcher  # noqa: E402

FORMS = ["64l", "128l", "64w", "128w"]  # tile side; a lane or a wave per ray.  FORMS[0] ships
C3_CMD = ["bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10", "--no-cpu-baseline"]


def c3_step(tree):
    """ms per C3 step from a child process running `tree`'s bench.py (its own library)."""
    env = {k: v for k, v in os.environ.items() if k not in ("LSLAM_LIB", "LSLAM_GRID_FORM")}
    out = subprocess.run([sys.executable] + C3_CMD, cwd=tree, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("bench.py failed in %s: %s" % (tree, out.stderr[-2000:]))
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


class Leg:
    """One robot count: the matcher's pair, the grid and their device inputs."""

    def __init__(self, ctx, R, Np):
        rng = np.random.default_rng(5)
        refs, curs, poses = [], [], []
        for r in range(R):
            p0 = synth.scan_polar(r)[2]
            d = np.array([rng.uniform(-150, 150), rng.uniform(-60, 60), np.deg2rad(rng.uniform(-8, 8))])
            p1 = smr.compose(p0, d)
            refs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 2 * r, Np)))
            curs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p1, 2 * r + 1, Np)))
            poses.append(p1)
        self.ctx, self.R, self.Np = ctx, R, Np
        self.poses = np.array(poses)
        self.cur0 = curs[0]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.m = ScanMatcher(ctx, R)
        self.g = OccupancyGrid.centred_on(ctx, self.poses)
        self.d_ref, self.d_cur = ctx.to_device(np.concatenate(refs)), ctx.to_device(np.concatenate(curs))
        self.d_off = ctx.to_device(self.off)
        self.d_pose = ctx.to_device(self.poses)
        self.match_ms = []
        self.grid_ms = {f: [] for f in FORMS}

    def grid_call(self, form, sync=True):
        os.environ["LSLAM_GRID_FORM"] = form
        self.g.step(self.d_cur, self.sco, self.off, pose=self.d_pose, sync=sync)

    def check_and_count(self):
        """Every form from zero: robot 0 against the definition, all forms the same bytes; the
        touched tiles of the shipped form's side and of the other."""
        want = None
        for form in FORMS:
            self.g.clear()
            self.grid_call(form)
            res = self.g.results()
            if want is None:
                L0, n_used, flags = ogr.update(np.zeros((self.g.W, self.g.W), np.int16), self.cur0, self.poses[0],
                                               res["rot"][0], self.g.origin_host[0])
                assert np.array_equal(res["logodds"][0], L0) and np.array_equal(res["n_used"][0], n_used)
                assert res["flags"][0] == flags
                want = res
            else:
                for k in ("logodds", "n_used", "flags", "rot"):
                    assert np.array_equal(res[k], want[k]), (form, k)
        nz = want["logodds"] != 0
        touched = {}
        for T in (128, 64):
            nt = self.g.W // T
            touched[T] = int(nz.reshape(self.R, nt, T, nt, T).any(axis=(2, 4)).sum())
        return touched, int(nz.sum())

    def copy_bandwidth(self, reps=5):
        """Bytes read + written per second by a device-to-device copy the size of the grids (at
        least 256 MiB: small copies measure the launch)."""
        n = max(self.g.logodds.nbytes, 256 << 20)
        a, b = self.ctx.empty(n, np.uint8), self.ctx.empty(n, np.uint8)
        a.fill_zero()
        self.ctx.copy(b, a)
        self.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            self.ctx.copy(b, a)
        self.ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        a.free()
        b.free()
        return 2.0 * n / dt

    def timed(self, reps, warmup=2):
        ctx = self.ctx
        for _ in range(warmup):
            self.m.match(self.d_ref, self.d_off, self.d_cur, self.d_off)
            self.grid_call(FORMS[0])
        ctx.set_timing(True, kernels=[_lib.K_MATCH, _lib.K_GRID])
        for _ in range(reps):
            ctx.timing_reset()
            self.m.match(self.d_ref, self.d_off, self.d_cur, self.d_off, sync=False)
            ms, n = ctx.timing(_lib.K_MATCH)
            assert n == 1
            self.match_ms.append(ms)
        for _ in range(reps):
            for form in FORMS:
                ctx.timing_reset()
                self.grid_call(form, sync=False)
                ms, n = ctx.timing(_lib.K_GRID)
                assert n == 1
                self.grid_ms[form].append(ms)
        ctx.set_timing(False)
        os.environ.pop("LSLAM_GRID_FORM", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-c3", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="another built checkout (the parent commit) whose C3 step "
                    "is measured in alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_bench.json"))
    args = ap.parse_args()
    assert FORMS[0] == "%dl" % TILE
    ctx = Context(0)
    legs = [Leg(ctx, int(r), args.points) for r in args.robots.split(",")]
    info = []
    for leg in legs:
        touched, cells = leg.check_and_count()
        info.append({"touched_tiles": touched, "cells_updated": cells, "copy_bytes_per_s": leg.copy_bandwidth()})
    c3, c3_base = [], []
    for _ in range(args.rounds):
        if not args.no_c3:
            c3.append(c3_step(ROOT))
            if args.baseline_tree:
                c3_base.append(c3_step(args.baseline_tree))
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/gridbench.py; legs alternate over %d rounds; HIP events per call; "
                   "medians with min and max" % args.rounds,
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "forms": FORMS, "shipped": FORMS[0],
           "grid": []}
    if c3:
        out["c3_ms_per_step"] = stats(c3)
    if c3_base:
        out["c3_ms_per_step_parent_build"] = stats(c3_base)
    for leg, inf in zip(legs, info):
        W = leg.g.W
        bw = inf["copy_bytes_per_s"]
        e = {"robots": leg.R, "grid_w": W, "grid_bytes": leg.g.logodds.nbytes, "match_ms": stats(leg.match_ms),
             "grid_ms": {f: stats(v) for f, v in leg.grid_ms.items()}, "cells_updated_per_call": inf["cells_updated"],
             "copy_GB_per_s": round(bw / 1e9, 1)}
        for T in (128, 64):
            tb = inf["touched_tiles"][T] * T * T * 2
            floor_ms = 2.0 * tb / bw * 1e3
            e["tile_%d" % T] = {"touched_tiles": inf["touched_tiles"][T], "of": leg.R * (W // T) ** 2,
                                "touched_bytes": tb, "hbm_floor_ms": round(floor_ms, 4),
                                "ratio_to_floor": round(statistics.median(leg.grid_ms["%d%s" % (T, FORMS[0][-1])]) / floor_ms, 2)}
        out["grid"].append(e)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
