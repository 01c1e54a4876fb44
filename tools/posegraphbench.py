"""Times lslam_pose_graph on loop graphs: G = 1, 256 and 4096 graphs of N = 24 and N = 64 keyframes (the
circle loop of tests/posegraph_ref.py: N - 1 odometry edges and one closure, every default), with a default
lslam_field_align call of the same session beside them as the yardstick.  The method of
tools/fieldalignbench.py: host clock over five back-to-back calls between two lslam_sync, per call, medians of
three rounds with minimum and maximum.  Writes profiles/posegraph_bench.json.

    python tools/posegraphbench.py [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import posegraph_ref as pg  # noqa: E402
from lidar_slam_amd import synth  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.mapping import DistanceField, OccupancyGrid  # noqa: E402
from lidar_slam_amd.posegraph import PoseGraph, lds_bytes  # noqa: E402

CALLS, ROUNDS = 5, 3


def timed(ctx, call):
    call()
    ctx.sync()
    out = []
    for _ in range(ROUNDS):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            call()
        ctx.sync()
        out.append((time.perf_counter() - t0) / CALLS * 1e3)
    return {"ms": float(np.median(out)), "min": min(out), "max": max(out)}


def loop_fleet(ctx, G, N):
    """G loop graphs of N keyframes through the wrapper's own calls: sixteen distinct loops, repeated; the
    odometry edges are add_keyframe's (relative_pose of consecutive keyframes), the closure is the loop's."""
    loops = [pg.circle_loop(N, seed=s) for s in range(16)]
    graph = PoseGraph(ctx, G, max_nodes=N, max_edges=N)
    init = np.stack([loops[g % 16][1] for g in range(G)], 1)  # [N, G, 3]
    for k in range(N):
        graph.add_keyframe(init[k], odo_info=loops[0][4][0])
    graph.add_edge(N - 1, 0, np.stack([loops[g % 16][3][-1] for g in range(G)]), loops[0][4][-1])
    return graph


def align_yardstick(ctx, R):
    ids = list(range(200, 200 + R))
    poses = synth.trajectory(ids, 1, u=(146.0, 174.0))
    rev = synth.revolutions_at(poses[0], 0, ids)
    grid = OccupancyGrid(ctx, R, grid_w=512, origin=(-3120.0, -3620.0))
    grid.step(rev["xy"], rev["scan_chunk_off"], rev["chunk_pt_off"], pose=poses[0])
    field = DistanceField(grid)
    field.step()
    dxy = ctx.to_device(rev["xy"])
    guess = ctx.to_device(poses[0] + [20.0, -20.0, 0.01])
    return timed(ctx, lambda: field.align(dxy, rev["scan_chunk_off"], rev["chunk_pt_off"], pose=guess, sync=False))


def main():
    ctx = Context(0)
    out = {"method": "host clock over %d back-to-back calls between two syncs, median of %d rounds" % (CALLS, ROUNDS), "legs": []}
    for G in (1, 256, 4096):
        leg = {"graphs": G, "field_align": align_yardstick(ctx, G)}
        for N in (24, 64):
            graph = loop_fleet(ctx, G, N)
            t = timed(ctx, lambda: graph.solve(sync=False))
            res = graph.results()
            t.update(mean_iters=float(res["iters"].mean()), converged=float((res["flags"] == 4).mean()),
                     lds_bytes=lds_bytes(N, N))
            leg["N%d" % N] = t
            print(G, N, t, flush=True)
        print(G, "field_align", leg["field_align"], flush=True)
        out["legs"].append(leg)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "posegraph_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
