"""Grid ray-casting cost: one default lslam_grid_raycast call for many robots in both forms, beside a
default lslam_grid_update call of the same session.

python tools/raycastbench.py [--robots 4096,256,1] [--points 720] [--rounds 3] [--reps 7] [--cus 256]
                             [--out profiles/raycast_bench.json]

Robot r sees the synthetic room from synth.scan_polar(r)'s pose; its grid (512 cells of 20 mm) is
centred on it and holds `--build` grid updates of the revolution (two by default: free cells at -82,
walls at 170), which is then cast through it at the same pose with the default thresholds.  Inputs
are resident on the device.  The legs alternate, `rounds` times; per robot count: `reps` grid-update
calls into a scratch grid, then `reps` times one ray-cast call of each form (the HBM form, which ships,
and through LSLAM_RAYCAST_FORM=lds the LDS form), each call timed on its own with HIP events (LSLAM_K_GRID,
LSLAM_K_RAYCAST) after two untimed calls.  Figures are medians over all rounds, with minimum and
maximum.  Also recorded: the copy bandwidth of the session (a device-to-device copy, bytes read +
bytes written per second, as tools/gridbench.py measures it), the bytes of the windows the LDS form's
workgroups read (every slice of a robot with points reads the robot's window, clipped to the map; the
launcher's slice rule is repeated here with `--cus` compute units), the HBM floor = those bytes / that
bandwidth, and the LDS form's ratio to it.  Both forms must give the same bytes, and robot 0 is
asserted against the NumPy definition (tests/raycast_ref.py).
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

import raycast_ref as rcr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import GridRayCaster, OccupancyGrid  # noqa: E402

FORMS = ["lds", "hbm"]
MAX_SLICES = 16  # lslam_raycast.h RAYCAST_MAX_SLICES


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def set_form(form):
    os.environ["LSLAM_RAYCAST_FORM"] = form


class Leg:
    """One robot count: the grids, the revolution and their device inputs."""

    def __init__(self, ctx, R, Np, build):
        poses, revs = [], []
        for r in range(R):
            p = synth.scan_polar(r)[2]
            revs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p, 2 * r, Np)))
            poses.append(p)
        self.ctx, self.R, self.Np = ctx, R, Np
        self.poses = np.array(poses)
        self.rev0 = revs[0]
        self.off = (np.arange(R + 1) * Np).astype(np.int32)
        self.sco = np.arange(R + 1, dtype=np.int32)
        self.g = OccupancyGrid.centred_on(ctx, self.poses)
        self.scratch = OccupancyGrid.centred_on(ctx, self.poses)  # the timed grid updates go here
        self.rc = GridRayCaster(self.g)
        self.d_xy = ctx.to_device(np.concatenate(revs))
        self.d_pose = ctx.to_device(self.poses)
        for _ in range(build):
            self.g.step(self.d_xy, self.sco, self.off, pose=self.d_pose)
        self.grid_ms = []
        self.ray_ms = {f: [] for f in FORMS}

    def cast(self, form, sync=True):
        set_form(form)
        self.rc.step(self.d_xy, self.sco, self.off, pose=self.d_pose, sync=sync)

    def check(self):
        """Both forms the same bytes; robot 0 against the definition.  Returns the class counts."""
        want = None
        for form in FORMS:
            self.cast(form)
            res = self.rc.results()
            if want is None:
                L0 = np.empty((self.g.W, self.g.W), np.int16)  # robot 0's grid alone
                _lib.check(_lib.load().lslam_d2h(self.ctx.handle, L0.ctypes.data, self.g.logodds.ptr, L0.nbytes), "lslam_d2h")
                self.ctx.sync()
                raw = (res["cls"] | (res["kind"] << 4))[:self.Np]
                cls, stop, counts, flags = rcr.cast(L0, self.rev0, self.poses[0], res["rot"][0], self.g.origin_host[0])
                assert np.array_equal(raw, cls) and np.array_equal(res["stop"][:self.Np], stop)
                assert np.array_equal(res["counts"][0], counts) and res["flags"][0] == flags
                want = res
            else:
                for k in ("cls", "kind", "stop", "counts", "flags", "rot"):
                    assert np.array_equal(res[k], want[k]), (form, k)
        os.environ.pop("LSLAM_RAYCAST_FORM", None)
        return want["counts"].sum(0).tolist(), int(want["stop"][:, 2].astype(np.int64).sum())

    def window_bytes(self, cus):
        """Bytes of the windows that the LDS form's workgroups read (module docstring)."""
        p = self.g.p
        Rc = int(np.floor(p.max_range * (1.0 / p.cell)))
        W = self.g.W
        ns = min(max(-(-2 * cus // self.R), 1), MAX_SLICES)
        per = (-(-self.Np // ns) + 63) & ~63
        used = -(-self.Np // per) if self.Np else 0
        c = np.floor((self.poses[:, :2] - self.g.origin_host) * (1.0 / p.cell)).astype(np.int64)
        lo, hi = np.maximum(c - Rc, 0), np.minimum(c + Rc + 1, W)
        cells = np.prod(np.maximum(hi - lo, 0), axis=1)
        return int(cells.sum()) * 2 * used, ns, used

    def copy_bandwidth(self, reps=5):
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
            self.scratch.step(self.d_xy, self.sco, self.off, pose=self.d_pose)
            for form in FORMS:
                self.cast(form)
        ctx.set_timing(True, kernels=[_lib.K_GRID, _lib.K_RAYCAST])
        for _ in range(reps):
            ctx.timing_reset()
            self.scratch.step(self.d_xy, self.sco, self.off, pose=self.d_pose, sync=False)
            ms, n = ctx.timing(_lib.K_GRID)
            assert n == 1
            self.grid_ms.append(ms)
        for _ in range(reps):
            for form in FORMS:
                ctx.timing_reset()
                self.cast(form, sync=False)
                ms, n = ctx.timing(_lib.K_RAYCAST)
                assert n == 1
                self.ray_ms[form].append(ms)
        ctx.set_timing(False)
        os.environ.pop("LSLAM_RAYCAST_FORM", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="4096,256,1")
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--build", type=int, default=2, help="grid updates that build the map before it is cast through")
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (the launcher's slice rule)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raycast_bench.json"))
    args = ap.parse_args()
    ctx = Context(0)
    legs = [Leg(ctx, int(r), args.points, args.build) for r in args.robots.split(",")]
    info = []
    for leg in legs:
        counts, steps = leg.check()
        wb, ns, used = leg.window_bytes(args.cus)
        info.append({"counts": counts, "steps": steps, "window_bytes": wb, "slices": ns, "slices_with_points": used,
                     "copy_bytes_per_s": leg.copy_bandwidth()})
    for _ in range(args.rounds):
        for leg in legs:
            leg.timed(args.reps)
    out = {"note": "one session on one MI355X: tools/raycastbench.py; legs alternate over %d rounds; HIP events per call; "
                   "medians with min and max" % args.rounds,
           "lib": _lib.load().lslam_version().decode(), "points": args.points, "forms": FORMS, "shipped": "hbm", "map_updates": args.build,
           "raycast": []}
    for leg, inf in zip(legs, info):
        bw = inf["copy_bytes_per_s"]
        floor_ms = inf["window_bytes"] / bw * 1e3
        lds = statistics.median(leg.ray_ms["lds"])
        out["raycast"].append({
            "robots": leg.R, "grid_w": leg.g.W, "grid_bytes": leg.g.logodds.nbytes, "grid_update_ms": stats(leg.grid_ms),
            "raycast_ms": {f: stats(v) for f, v in leg.ray_ms.items()},
            "lds_over_hbm": round(lds / statistics.median(leg.ray_ms["hbm"]), 3),
            "class_counts": inf["counts"], "steps_walked": inf["steps"], "slices_per_robot": inf["slices"],
            "slices_with_points": inf["slices_with_points"], "window_bytes_read": inf["window_bytes"],
            "copy_GB_per_s": round(bw / 1e9, 1), "hbm_floor_ms": round(floor_ms, 4), "lds_ratio_to_floor": round(lds / floor_ms, 2)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
