"""GPU parity of the pose-graph optimiser (lslam_pose_graph, PoseGraph, OccupancyGrid.redraw) against its
NumPy definition, tests/posegraph_ref.py.

Every double operation of the definition is rounded on its own and every sum has its order, so pose_out, chi2,
edge_chi2, iters and flags are compared EXACTLY (the doubles as bit patterns), the reference being fed the
(cos, sin) that the device wrote to trace; those are themselves held to 1e-15 against NumPy's, the bound of
tests/test_gpu_fieldalign.py.  Shapes: N = 2 (n = 3), 3, 22 and 23 (n = 63 and 66, either side of a wave), 64
(the largest LDS); E = 1 and E = E_cap; edges with i > j, into node 0, three on one pair; G = 1, 3 and 300
with graphs of different N and E in one call, flagged graphs between good ones.

The end-to-end case (N = 24 circle in synth's room, 2 robots; figures printed by the test): the closure found
by DistanceField.align, the poses and flags equal to the reference chain's bit for bit, and the redrawn map
contradicting fewer cells per thousand of a map drawn from the true poses than the drifted map does."""
import ctypes as C

import numpy as np
import pytest

import posegraph_ref as pg
from lidar_slam_amd import _lib, posegraph, synth

pytestmark = pytest.mark.gpu

CANARY = 8  # doubles on either side of pose_out


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Buffers:
    """The device arrays of one shape (G, Nc, Ec), reused between calls; every output starts as junk."""

    def __init__(self, ctx, G, Nc, Ec):
        self.ctx, self.G, self.Nc, self.Ec = ctx, G, Nc, Ec
        e = ctx.empty
        self.n_nodes, self.n_edges = e(G, np.int32), e(G, np.int32)
        self.pose = e((Nc, G, 3), np.float64)
        self.ij, self.z, self.info = e((G, Ec, 2), np.int32), e((G, Ec, 3), np.float64), e((G, Ec, 6), np.float64)
        self.out = e(Nc * G * 3 + 2 * CANARY, np.float64)
        self.trace = e((G, 33, Nc, 2), np.float64)
        self.chi2, self.echi = e((G, 2), np.float64), e((G, Ec), np.float64)
        self.iters, self.flags = e(G, np.int32), e(G, np.int32)

    def junk(self):
        for a in (self.out, self.trace, self.chi2, self.echi, self.iters, self.flags):
            a.upload(np.frombuffer(b"\xa5" * a.nbytes, np.uint8).view(a.dtype).reshape(a.shape))


def pack(graphs, Nc, Ec):
    """graphs: dicts of pose [<= Nc, 3], ij, z, info and optionally n_nodes, n_edges (what the device is told).
    -> node-major pose [Nc, G, 3] (slabs beyond a graph's poses hold a pattern), padded edges, counts."""
    G = len(graphs)
    pose = np.empty((Nc, G, 3))
    pose[:] = (np.arange(Nc * G * 3).reshape(Nc, G, 3) + 0.25) * -1.5  # what must be copied through
    ij, z, info = np.full((G, Ec, 2), 7, np.int32), np.full((G, Ec, 3), np.nan), np.full((G, Ec, 6), np.nan)  # (junk beyond E)
    nn, ne = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g, q in enumerate(graphs):
        p, e = np.asarray(q["pose"], np.float64), np.asarray(q["ij"], np.int32).reshape(-1, 2)
        pose[:len(p), g] = p
        ij[g, :len(e)], z[g, :len(e)], info[g, :len(e)] = e, q["z"], q["info"]
        nn[g], ne[g] = q.get("n_nodes", len(p)), q.get("n_edges", len(e))
    return pose, ij, z, info, nn, ne


def run(B, graphs, alias=False, junk=True, **params):
    """One lslam_pose_graph call compared with the reference, graph by graph; returns the device's outputs."""
    ctx, G, Nc, Ec = B.ctx, B.G, B.Nc, B.Ec
    assert len(graphs) == G
    pose, ij, z, info, nn, ne = pack(graphs, Nc, Ec)
    p = _lib.posegraph_params(max_nodes=Nc, max_edges=Ec, **params)
    if junk:
        B.junk()
    for buf, h in ((B.n_nodes, nn), (B.n_edges, ne), (B.pose, pose), (B.ij, ij), (B.z, z), (B.info, info)):
        buf.upload(h)
    canary = np.full(Nc * G * 3 + 2 * CANARY, -7.75)
    out_addr = B.out.addr + 8 * CANARY
    if alias:  # pose_out = pose: the poses are given inside the canaried buffer
        canary[CANARY:-CANARY] = pose.reshape(-1)
    B.out.upload(canary)
    b = _lib.PoseGraphBatch()
    b.n_graphs = G
    b.n_nodes, b.n_edges, b.pose = B.n_nodes.addr, B.n_edges.addr, (out_addr if alias else B.pose.addr)
    b.edge_ij, b.edge_z, b.edge_info = B.ij.addr, B.z.addr, B.info.addr
    b.pose_out, b.trace, b.chi2, b.edge_chi2 = out_addr, B.trace.addr, B.chi2.addr, B.echi.addr
    b.iters, b.flags = B.iters.addr, B.flags.addr
    _lib.call("lslam_pose_graph", ctx, b, p)
    ctx.sync()
    rows = int(p.n_iter) + 1
    raw = B.out.download()
    assert (raw[:CANARY] == -7.75).all() and (raw[-CANARY:] == -7.75).all(), "pose_out's neighbours were written"
    got = dict(pose_out=raw[CANARY:-CANARY].reshape(Nc, G, 3),
               trace=B.trace.download().reshape(-1)[:G * rows * Nc * 2].reshape(G, rows, Nc, 2),
               chi2=B.chi2.download(), edge_chi2=B.echi.download(), iters=B.iters.download(), flags=B.flags.download())
    if not alias:
        assert bits(B.pose.download()).tobytes() == bits(pose).tobytes()  # read only
    kw = {k: getattr(p, k) for k in ("n_iter", "damp_t", "damp_r", "eps_t", "eps_r")}
    worst = 0.0
    for g in range(G):
        ref = pg.solve(pose[:, g], ij[g], z[g], info[g], n_nodes=nn[g], n_edges=ne[g], trace=got["trace"][g], **kw)
        what = (g, int(nn[g]), int(ne[g]), ref["flags"], got["flags"][g])
        assert got["flags"][g] == ref["flags"] and got["iters"][g] == ref["iters"], what
        assert np.array_equal(bits(got["chi2"][g]), bits(ref["chi2"])), (what, got["chi2"][g], ref["chi2"])
        assert np.array_equal(bits(got["edge_chi2"][g]), bits(ref["edge_chi2"])), what
        assert np.array_equal(bits(got["pose_out"][:, g]), bits(ref["pose_out"])), what
        if ref["flags"] & (pg.REJECTED | pg.EMPTY):
            assert np.array_equal(bits(got["pose_out"][:, g]), bits(pose[:, g])), what
        # trace: zeros where nothing was evaluated, else the library's cos and sin within 1e-15 of NumPy's
        evaluated = ref["trace"].any(axis=(1, 2))  # (cos and sin are never both zero)
        assert not got["trace"][g][~evaluated].any(), what
        n_used = max(int(nn[g]), 0) if evaluated.any() else 0
        assert not got["trace"][g][:, n_used:].any(), what
        if evaluated.any():
            worst = max(worst, np.abs(got["trace"][g][evaluated][:, :n_used] - ref["trace"][evaluated][:, :n_used]).max())
    print("trace (cos, sin) error", worst)
    assert worst <= 1e-15
    return got


def graph_of(N, rng, extra):
    pose, ij, z, info = pg.random_graph(N, rng, extra)
    return dict(pose=pose, ij=ij, z=z, info=info)


@pytest.mark.parametrize("N", (2, 3, 22, 23, 64))
def test_shapes(ctx, N):
    """Three graphs a call: the full one with E = E_cap (i > j, into node 0, three edges on one pair), one with a
    single edge (every other node held by the damping alone), one a node smaller.  Then pose_out = pose, a second
    call into the same buffers without new junk, and the ends of n_iter."""
    rng = np.random.default_rng(800 + N)
    full = graph_of(N, rng, 2 * N)
    one = graph_of(N, rng, 0)
    one.update(ij=one["ij"][:1], z=one["z"][:1], info=one["info"][:1])
    small = graph_of(max(2, N - 1), rng, 3)
    Ec = 1024 if N == 64 else len(full["ij"])  # (N = 64 with max_edges = 1024 is the largest LDS, 155 KiB)
    B = Buffers(ctx, 3, N, Ec)
    graphs = [full, one, small]
    a = run(B, graphs)
    assert a["flags"][1] == pg.CONVERGED and not a["flags"][0] & (pg.EMPTY | pg.BAD_GRAPH)
    b = run(B, graphs, alias=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = run(B, graphs, junk=False)  # a second call into the same buffers
    for k in a:
        assert a[k].tobytes() == c[k].tobytes(), k
    z0 = run(B, graphs, n_iter=0)
    assert not z0["iters"].any() and np.array_equal(bits(z0["chi2"][:, 0]), bits(z0["chi2"][:, 1]))
    if N <= 23:
        r = run(B, graphs, n_iter=32, eps_t=0.0, eps_r=0.0)  # never CONVERGED: every step is made
        assert (r["iters"][~(r["flags"] & pg.REJECTED).astype(bool)] == 32).all()


def test_one_graph_and_many(ctx):
    """G = 1; then G = 300 (more than the CUs) with N and E varying from graph to graph and, between the good
    ones, EMPTY, BAD_GRAPH, SINGULAR and DIVERGED graphs, whose pose_out is pose bit for bit."""
    rng = np.random.default_rng(31)
    run(Buffers(ctx, 1, 5, 16), [graph_of(5, rng, 2)])
    Nc, Ec, G = 8, 24, 300
    graphs = []
    for g in range(G):
        N = int(rng.integers(2, Nc + 1))
        q = graph_of(N, rng, int(rng.integers(0, 4)))
        kind = g % 10
        if kind == 3:
            q["n_nodes"] = (1, 0, N)[g % 3]
            q["n_edges"] = (len(q["ij"]), 0, 0)[g % 3]  # EMPTY
        elif kind == 5:
            bad = g // 10 % 6
            if bad == 0:
                q["n_nodes"] = Nc + 1
            elif bad == 1:
                q["n_edges"] = (Ec + 1, -1)[g // 60 % 2]
            elif bad == 2:
                q["ij"] = q["ij"].copy()
                q["ij"][0] = [(0, N), (1, 1), (-1, 0)][g // 60 % 3]
            elif bad == 3:
                q["pose"] = q["pose"].copy()
                q["pose"][N - 1, g % 3] = (np.nan, np.inf)[g // 60 % 2]
            elif bad == 4:
                q["z"] = q["z"].copy()
                q["z"][0, 1] = -np.inf
            else:
                q["info"] = q["info"].copy()
                q["info"][len(q["ij"]) - 1, 4] = np.nan
        elif kind == 7:
            q["info"] = -q["info"]  # SINGULAR: a negative pivot
        elif kind == 9:
            q = dict(zip(("pose", "ij", "z", "info"), pg.diverging()))
        graphs.append(q)
    B = Buffers(ctx, G, Nc, Ec)
    r = run(B, graphs)
    f = r["flags"]
    assert (f[3::10] == pg.EMPTY).all() and (f[5::10] == pg.BAD_GRAPH).all()
    assert (f[7::10] & pg.SINGULAR).all() and (f[9::10] & pg.DIVERGED).all()
    assert (f[0::10] == pg.CONVERGED).sum() > 10
    run(B, graphs, alias=True, n_iter=1)
    # SINGULAR by an isolated node: no damping, graphs 0 and 2 hold every node, graph 1 leaves one out
    rng = np.random.default_rng(32)
    a, b, c = graph_of(5, rng, 0), graph_of(5, rng, 0), graph_of(4, rng, 1)
    b.update(ij=b["ij"][:3], z=b["z"][:3], info=b["info"][:3])
    r = run(Buffers(ctx, 3, 6, 12), [a, b, c], damp_t=0.0, damp_r=0.0)
    assert r["flags"][1] == pg.SINGULAR and not r["flags"][0] & pg.SINGULAR and not r["flags"][2] & pg.SINGULAR


def csr_of(rev):
    return rev["xy"], rev["scan_chunk_off"], rev["chunk_pt_off"]


def loops_in_the_room(R, N, **kw):
    truth, init, edges = [], [], []
    for r in range(R):
        t, i, ij, z, info = pg.circle_loop(N, seed=4000 + r, **kw)
        truth.append(t), init.append(i), edges.append((ij[:-1], z[:-1], info[:-1]))  # (the closure is the matcher's to find)
    return np.stack(truth, 1), np.stack(init, 1), edges  # [N, R, 3]


def test_wrapper_unsynced_and_errors(ctx):
    """PoseGraph: solve(sync=False) followed by an unsynced grid.step on node_pose(k) draws what a synced chain at
    the downloaded poses draws; the wrapper's own errors."""
    from lidar_slam_amd.mapping import OccupancyGrid
    R, N = 2, 6
    truth, init, edges = loops_in_the_room(R, N)
    revs = [synth.revolutions_at(truth[k], k, [300, 301]) for k in range(N)]
    graph = posegraph.PoseGraph(ctx, R, max_nodes=8, max_edges=16)
    odo = edges[0][2][0]
    for k in range(N):
        assert graph.add_keyframe(init[k], csr_of(revs[k]), odo_info=odo) == k
    for r in range(R):
        graph.add_edge(N - 1, 0, pg.relative_pose(truth[N - 1, r], truth[0, r]), [0.04, 0, 0, 0.04, 0, 4e4], graph=r)
    kw = dict(grid_w=256, origin=(-560.0, -1060.0))
    g1, g2 = OccupancyGrid(ctx, R, **kw), OccupancyGrid(ctx, R, **kw)
    dxy = ctx.to_device(revs[N - 1]["xy"])
    graph.solve(sync=False)
    g1.step(dxy, revs[N - 1]["scan_chunk_off"], revs[N - 1]["chunk_pt_off"], pose=graph.node_pose(N - 1), sync=False)
    ctx.sync()
    res = graph.results()
    assert (res["flags"] == pg.CONVERGED).all() and res["pose"].shape == (R, N, 3)
    for r in range(R):
        ref = pg.solve(graph.pose_host[:, r], graph.ij_host[r], graph.z_host[r], graph.info_host[r], n_nodes=N,
                       n_edges=int(graph.n_edges_host[r]), trace=res["trace"][r])
        assert np.array_equal(bits(res["pose"][r]), bits(ref["pose_out"][:N])) and res["flags"][r] == ref["flags"]
        assert np.array_equal(bits(graph.z_host[r, :N - 1]), bits(pg.relative_pose(init[:-1, r], init[1:, r])))
    g2.step(*csr_of(revs[N - 1]), pose=res["pose"][:, N - 1])
    assert g1.logodds.download().tobytes() == g2.logodds.download().tobytes()
    assert np.array_equal(bits(graph.node_pose(2).download()), bits(res["pose"][:, 2]))
    with pytest.raises(ValueError):
        graph.node_pose(N)
    with pytest.raises(ValueError):
        posegraph.PoseGraph(ctx, 1, max_nodes=65)
    with pytest.raises(TypeError):
        posegraph.PoseGraph(ctx, 1, trunc=1.0)
    with pytest.raises(ValueError):
        OccupancyGrid(ctx, 3, **kw).redraw(graph)


def test_end_to_end_loop_closure_and_redraw(ctx):
    """Two robots drive the N = 24 circle in synth's room; keyframes at the biased-odometry poses.  A grid from
    keyframes 0-2, the last keyframe's revolution aligned in its distance field from its drifted pose, the closure
    from closure_edge, solve, redraw."""
    from lidar_slam_amd.mapping import FIELDALIGN_REJECTED, DistanceField, OccupancyGrid
    R, N, ids = 2, 24, [310, 311]
    # (the bias keeps the last keyframe's drift inside the aligner's basin: 200 mm, 0.1 rad)
    truth, init, edges = loops_in_the_room(R, N, bias=(2.0, -1.5, 0.002))
    drift = [pg.pose_error(init[-1:, r], truth[-1:, r]) for r in range(R)]
    print("drift of the last keyframe", drift)
    assert all(d[0] < 150.0 and d[1] < 0.08 for d in drift)
    revs = [synth.revolutions_at(truth[k], k, ids) for k in range(N)]
    kw = dict(grid_w=256, origin=(-560.0, -1060.0))
    graph = posegraph.PoseGraph(ctx, R, max_nodes=N, max_edges=32)
    for k in range(N):
        graph.add_keyframe(init[k], csr_of(revs[k]), odo_info=edges[0][2][0])
    grid = OccupancyGrid(ctx, R, **kw)
    for k in range(3):
        grid.step(*csr_of(revs[k]), pose=init[k])
    field = DistanceField(grid)
    field.step()
    field.align(*csr_of(revs[N - 1]), pose=init[N - 1])
    al = field.align_results()
    assert not (al["flags"] & FIELDALIGN_REJECTED).any(), al["flags"]
    H = field.align_information()[0]
    for r in range(R):
        z, info = posegraph.closure_edge(init[0, r], al["pose_out"][r], H[r], cell=float(grid.p.cell))
        graph.add_edge(0, N - 1, z, info, graph=r)
    graph.solve()
    res = graph.results()
    for r in range(R):
        ref = pg.solve(graph.pose_host[:, r], graph.ij_host[r], graph.z_host[r], graph.info_host[r], n_nodes=N,
                       n_edges=int(graph.n_edges_host[r]), trace=res["trace"][r])
        assert res["flags"][r] == ref["flags"] == pg.CONVERGED and res["iters"][r] == ref["iters"]
        assert np.array_equal(bits(res["pose"][r]), bits(ref["pose_out"][:N]))
        before, after = pg.pose_error(init[:, r], truth[:, r]), pg.pose_error(res["pose"][r], truth[:, r])
        print("robot %d: worst pose error %.1f mm %.4f rad -> %.1f mm %.4f rad in %d steps"
              % (r, before[0], before[1], after[0], after[1], res["iters"][r]))
        assert after[0] < before[0] and after[1] < before[1]
    true_map, drifted = OccupancyGrid(ctx, R, **kw), OccupancyGrid(ctx, R, **kw)
    for k in range(N):
        true_map.step(*csr_of(revs[k]), pose=truth[k], sync=False)
        drifted.step(*csr_of(revs[k]), pose=init[k], sync=False)
    grid.redraw(graph)
    assert grid.steps == 3 + N
    identity = [1.0, 0.0, 0.0, 0.0]

    def permille(g):
        g.merge(true_map, identity, dry_run=True)
        s = g.merge_results()["stats"].astype(np.float64)
        return 1000.0 * s[:, 3] / np.maximum(s[:, 2] + s[:, 3], 1.0)
    bad, good = permille(drifted), permille(grid)
    print("contradicted cells per thousand against the true map: drifted %s, redrawn %s" % (bad, good))
    assert (good < bad).all()
