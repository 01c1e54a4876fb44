"""Times lslam_pose_graph_gate on loop graphs: G = 1, 256 and 4096 graphs of N = 24 and N = 64 keyframes (the circle
loop of tests/posegraph_ref.py with its N - 1 odometry edges as the trusted graph, every default) and 1, 4 and
16 candidates a graph (the loop's closure N - 1 -> 0, every second one moved 500 mm), without append, so that
every call judges the same graph.  Beside it in the same session lslam_pose_graph with n_iter = 1 on the same
graphs: one evaluation, one factorisation and one solve (and the evaluation behind the step), the work the gate
contains before its candidates; the ratio gate / solve is recorded per leg.  The method of
tools/posegraphbench.py: host clock over five back-to-back calls of the library between two lslam_sync, per call,
medians of three rounds with minimum and maximum.  Writes profiles/posegate_bench.json.

    python tools/posegatebench.py [--out FILE]
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
from lidar_slam_amd import _lib  # noqa: E402
from lidar_slam_amd.device import Context  # noqa: E402
from lidar_slam_amd.posegraph import POSEGATE_ACCEPTED, POSEGATE_OUTLIER, PoseGraph, gate_lds_bytes, gate_slots  # noqa: E402

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


def loop_fleet(ctx, G, N, C):
    """G loop graphs of N keyframes without their closure, through the wrapper's own calls: sixteen distinct loops,
    repeated; and the closures, per graph, for the candidates."""
    loops = [pg.circle_loop(N, seed=s) for s in range(16)]
    graph = PoseGraph(ctx, G, max_nodes=N, max_edges=N + C, max_cand=C, n_iter=1)
    init = np.stack([loops[g % 16][1] for g in range(G)], 1)  # [N, G, 3]
    for k in range(N):
        graph.add_keyframe(init[k], odo_info=loops[0][4][0])
    return graph, np.stack([loops[g % 16][3][-1] for g in range(G)]), loops[0][4][-1]


def gate_batch(graph):
    """The batch and params of the wrapper's last gate, to be called again as they stand."""
    b = _lib.PoseGateBatch()
    b.n_graphs = graph.G
    b.n_nodes, b.n_edges, b.pose = graph.n_nodes.addr, graph.n_edges.addr, graph.pose.addr
    b.edge_ij, b.edge_z, b.edge_info = graph.edge_ij.addr, graph.edge_z.addr, graph.edge_info.addr
    for name, buf in graph._gate.items():
        setattr(b, name, buf.addr)
    p = _lib.posegate_params(max_nodes=graph.Nc, max_edges=graph.Ec, max_cand=graph.Cc, damp_t=float(graph.p.damp_t),
                             damp_r=float(graph.p.damp_r))
    return b, p


def main():
    ctx = Context(0)
    out = {"method": "host clock over %d back-to-back calls between two syncs, median of %d rounds" % (CALLS, ROUNDS), "legs": []}
    for G in (1, 256, 4096):
        leg = {"graphs": G}
        for N in (24, 64):
            row = {}
            for C in (1, 4, 16):
                graph, z_loop, info_loop = loop_fleet(ctx, G, N, C)
                for c in range(C):
                    graph.propose(N - 1, 0, z_loop + [500.0 * (c % 2), 0.0, 0.0], info_loop)
                graph.gate(append=False)
                res = graph.gate_results()
                b, p = gate_batch(graph)
                t = timed(ctx, lambda: _lib.call("lslam_pose_graph_gate", ctx, b, p))
                again = graph.gate_results()
                assert all(res[k].tobytes() == again[k].tobytes() for k in res)
                slots = gate_slots(N, N + C, C)
                t.update(accepted=float((res["cand_flags"][:, :C] == POSEGATE_ACCEPTED).mean()),
                         outlier=float((res["cand_flags"][:, :C] == POSEGATE_OUTLIER).mean()),
                         lds_bytes=gate_lds_bytes(N, N + C, C, slots), slots=slots)
                row["C%d" % C] = t
                if C == 16:  # the yardstick on the same graphs: one Gauss-Newton step of the trusted graph
                    row["pose_graph_n_iter_1"] = timed(ctx, lambda: graph.solve(sync=False))
            for C in (1, 4, 16):
                row["C%d" % C]["ratio_to_pose_graph"] = row["C%d" % C]["ms"] / row["pose_graph_n_iter_1"]["ms"]
            leg["N%d" % N] = row
            print(G, N, json.dumps(row), flush=True)
        out["legs"].append(leg)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "posegate_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
