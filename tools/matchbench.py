"""LiDAR-only odometry cost: one default-window lslam_scan_match call for many robots.

python tools/matchbench.py [--robots 4096] [--points 720] [--reps 20] [--warmup 3]

Robot r's pair is a synthetic revolution and the same room seen after a small motion (inputs
resident on the device).  Each repeat is timed on its own with HIP events (LSLAM_K_MATCH); prints
one JSON object: the median ms per call, robots/s, and the look-up rate Ntheta Nt^2 points robots
per call against the chip's ds_read_b32 rate (128 B/clk/CU = 32 look-ups/clk/CU, 256 CUs at
2.4 GHz: 1.97e13 per second, MI355X_MICROARCH §LDS).  Robot 0's best is asserted against the
NumPy definition (tests/scanmatch_ref.py).
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

import scanmatch_ref as smr  # noqa: E402
from lidar_slam_amd import _lib, synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.odometry import ScanMatcher  # noqa: E402

LDS_LOOKUPS_PER_S = 32 * 256 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", type=int, default=4096)
    ap.add_argument("--points", type=int, default=720)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    R, Np = args.robots, args.points
    rng = np.random.default_rng(5)
    refs, curs = [], []
    for r in range(R):
        p0 = synth.scan_polar(r)[2]
        d = np.array([rng.uniform(-150, 150), rng.uniform(-60, 60), np.deg2rad(rng.uniform(-8, 8))])
        refs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 2 * r, Np)))
        curs.append(synth.polar_to_xy_ref(*synth.scan_polar_at(smr.compose(p0, d), 2 * r + 1, Np)))
    off = (np.arange(R + 1) * Np).astype(np.int32)
    ctx = Context(0)
    m = ScanMatcher(ctx, R)
    d_ref, d_cur = ctx.to_device(np.concatenate(refs)), ctx.to_device(np.concatenate(curs))
    d_off = ctx.to_device(off)
    for _ in range(args.warmup):
        m.match(d_ref, d_off, d_cur, d_off)
    res = m.results()
    want = smr.match(refs[0], curs[0], rot=m.rot_host)
    assert res["best"][0].tolist() == want["best"].tolist(), (res["best"][0], want["best"])
    assert abs(res["delta"][0] - want["delta"]).max() <= 1e-9
    ctx.set_timing(True, kernels=[_lib.K_MATCH])
    times = []
    for _ in range(args.reps):
        ctx.timing_reset()
        m.match(d_ref, d_off, d_cur, d_off, sync=False)
        ms, n = ctx.timing(_lib.K_MATCH)
        assert n == 1
        times.append(ms)
    ctx.set_timing(False)
    med = statistics.median(times)
    lookups = float(m.Nth) * m.Nt * m.Nt * Np * R
    out = {"config": "match", "robots": R, "points": Np, "window": [m.Nth, m.Nt, m.Nt], "reps": args.reps,
           "match_ms_median": med, "match_ms_min": min(times), "match_ms_max": max(times),
           "robots_per_s": R / med * 1e3, "lookups_per_call": lookups, "lookups_per_s": lookups / med * 1e3,
           "frac_lds_b32_rate": lookups / med * 1e3 / LDS_LOOKUPS_PER_S,
           "flags_any": int(np.count_nonzero(res["flags"]))}
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) and v < 1e6 else v) for k, v in out.items()}), flush=True)


if __name__ == "__main__":
    main()
