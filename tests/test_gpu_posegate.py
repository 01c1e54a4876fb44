"""GPU parity of the closure gate (lslam_pose_graph_gate, PoseGraph.propose / gate / relative_covariance) against
its NumPy definition, tests/posegate_ref.py.

Every double operation of the definition is rounded on its own and every sum has its order, so chi2, cand_nis,
cand_err, cand_cov, cand_flags, flags and, with append, the edge arrays and n_edges are compared EXACTLY (the
doubles as bit patterns), the reference being fed the (cos, sin) that the device wrote to trace; those are
themselves held to 1e-15 against NumPy's, the bound of tests/test_gpu_posegraph.py.  Shapes: N = 2 (n = 3), 3, 22
and 23 (n = 63 and 66, either side of a wave), 64 with max_edges = 1024 (the largest LDS, one candidate solved at
a time); C = 1 and C = C_cap = 64 (eight blocks of eight at N <= 23); candidates with i > j, into node 0, equal
ones, on a node that is not there, with a negative Omega; G = 1, 3 and 300 with graphs of different N, E and C
in one call, flagged graphs between good ones.  Every output starts as junk; cand_nis and the edge arrays'
tails stand between canaries.

The end-to-end case (N = 24 circle in synth's room, 2 robots; figures printed by the test): the closure found
by DistanceField.align and the same closure moved 500 mm proposed together, the first APPENDED and the second
OUTLIER, the poses equal bit for bit to those of a graph given the true closure alone, and the redrawn map
contradicting fewer cells per thousand of the true map than one redrawn from a plain solve given both."""
import numpy as np
import pytest

import posegate_ref as gr
import posegraph_ref as pg
import test_gpu_posegraph as tgp
import test_posegate_core as tpc
from lidar_slam_amd import _lib, posegraph, synth

pytestmark = pytest.mark.gpu

CANARY = 8  # doubles (or int32 pairs) round cand_nis and behind the edge arrays
bits = tgp.bits


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


class Buffers:
    """The device arrays of one shape (G, Nc, Ec, Cc), reused between calls; every output starts as junk."""

    def __init__(self, ctx, G, Nc, Ec, Cc):
        self.ctx, self.G, self.Nc, self.Ec, self.Cc = ctx, G, Nc, Ec, Cc
        e = ctx.empty
        self.n_nodes, self.n_edges, self.n_cand = e(G, np.int32), e(G, np.int32), e(G, np.int32)
        self.pose = e((Nc, G, 3), np.float64)
        self.ij, self.z, self.info = e(G * Ec * 2 + 2 * CANARY, np.int32), e(G * Ec * 3 + CANARY, np.float64), e(G * Ec * 6 + CANARY, np.float64)
        self.cij, self.cz, self.cinfo = e((G, Cc, 2), np.int32), e((G, Cc, 3), np.float64), e((G, Cc, 6), np.float64)
        self.trace, self.chi2 = e((G, Nc, 2), np.float64), e(G, np.float64)
        self.nis = e(G * Cc + 2 * CANARY, np.float64)
        self.err, self.cov = e((G, Cc, 3), np.float64), e((G, Cc, 6), np.float64)
        self.cf, self.flags = e((G, Cc), np.int32), e(G, np.int32)

    def junk(self):
        for a in (self.trace, self.chi2, self.err, self.cov, self.cf, self.flags):
            a.upload(np.frombuffer(b"\xa5" * a.nbytes, np.uint8).view(a.dtype).reshape(a.shape))


def pack_cand(graphs, Cc):
    G = len(graphs)
    cij, cz, cinfo = np.full((G, Cc, 2), 9, np.int32), np.full((G, Cc, 3), np.nan), np.full((G, Cc, 6), np.nan)  # (junk beyond C)
    nc = np.zeros(G, np.int32)
    for g, q in enumerate(graphs):
        c = np.asarray(q["cij"], np.int32).reshape(-1, 2)
        cij[g, :len(c)], cz[g, :len(c)], cinfo[g, :len(c)] = c, q["cz"], q["cinfo"]
        nc[g] = q.get("n_cand", len(c))
    return cij, cz, cinfo, nc


def run(B, graphs, junk=True, **params):
    """One lslam_pose_graph_gate call compared with the reference, graph by graph; returns the device's outputs."""
    ctx, G, Nc, Ec, Cc = B.ctx, B.G, B.Nc, B.Ec, B.Cc
    assert len(graphs) == G
    pose, ij, z, info, nn, ne = tgp.pack(graphs, Nc, Ec)
    cij, cz, cinfo, nc = pack_cand(graphs, Cc)
    p = _lib.posegate_params(max_nodes=Nc, max_edges=Ec, max_cand=Cc, **params)
    if junk:
        B.junk()
    for buf, h in ((B.n_nodes, nn), (B.n_edges, ne), (B.n_cand, nc), (B.pose, pose), (B.cij, cij), (B.cz, cz), (B.cinfo, cinfo)):
        buf.upload(h)
    B.ij.upload(np.concatenate([ij.reshape(-1), np.full(2 * CANARY, -77, np.int32)]))
    B.z.upload(np.concatenate([z.reshape(-1), np.full(CANARY, -7.75)]))
    B.info.upload(np.concatenate([info.reshape(-1), np.full(CANARY, -7.75)]))
    if junk:
        B.nis.upload(np.concatenate([np.full(CANARY, -7.75), np.full(G * Cc, np.nan), np.full(CANARY, -7.75)]))
    b = _lib.PoseGateBatch()
    b.n_graphs = G
    b.n_nodes, b.n_edges, b.pose = B.n_nodes.addr, B.n_edges.addr, B.pose.addr
    b.edge_ij, b.edge_z, b.edge_info = B.ij.addr, B.z.addr, B.info.addr
    b.n_cand, b.cand_ij, b.cand_z, b.cand_info = B.n_cand.addr, B.cij.addr, B.cz.addr, B.cinfo.addr
    b.trace, b.chi2, b.cand_nis, b.cand_err, b.cand_cov = B.trace.addr, B.chi2.addr, B.nis.addr + 8 * CANARY, B.err.addr, B.cov.addr
    b.cand_flags, b.flags = B.cf.addr, B.flags.addr
    _lib.call("lslam_pose_graph_gate", ctx, b, p)
    ctx.sync()
    raw, rij, rz, ri = B.nis.download(), B.ij.download(), B.z.download(), B.info.download()
    assert (raw[:CANARY] == -7.75).all() and (raw[-CANARY:] == -7.75).all(), "cand_nis' neighbours were written"
    assert (rij[-2 * CANARY:] == -77).all() and (rz[-CANARY:] == -7.75).all() and (ri[-CANARY:] == -7.75).all(), "the edge arrays' tails"
    got = dict(trace=B.trace.download(), chi2=B.chi2.download(), cand_nis=raw[CANARY:-CANARY].reshape(G, Cc), cand_err=B.err.download(),
               cand_cov=B.cov.download(), cand_flags=B.cf.download(), flags=B.flags.download(), n_edges=B.n_edges.download(),
               edge_ij=rij[:-2 * CANARY].reshape(G, Ec, 2), edge_z=rz[:-CANARY].reshape(G, Ec, 3), edge_info=ri[:-CANARY].reshape(G, Ec, 6))
    assert bits(B.pose.download()).tobytes() == bits(pose).tobytes()  # read only
    kw = {k: getattr(p, k) for k in ("damp_t", "damp_r", "nis_max", "append")}
    if not p.append:  # the edge arrays and n_edges are only read
        assert np.array_equal(got["n_edges"], ne) and np.array_equal(got["edge_ij"], ij)
        assert bits(got["edge_z"]).tobytes() == bits(z).tobytes() and bits(got["edge_info"]).tobytes() == bits(info).tobytes()
    worst = 0.0
    for g in range(G):
        ref = gr.gate(pose[:, g], ij[g], z[g], info[g], cij[g], cz[g], cinfo[g], n_nodes=nn[g], n_edges=ne[g], n_cand=nc[g],
                      trace=got["trace"][g], **kw)
        what = (g, int(nn[g]), int(ne[g]), int(nc[g]), ref["flags"], got["flags"][g])
        assert got["flags"][g] == ref["flags"], what
        assert np.array_equal(got["cand_flags"][g], ref["cand_flags"]), (what, got["cand_flags"][g], ref["cand_flags"])
        assert bits(got["chi2"][g]) == bits(ref["chi2"]), (what, got["chi2"][g], ref["chi2"])
        for k in ("cand_nis", "cand_err", "cand_cov"):
            assert np.array_equal(bits(got[k][g]), bits(ref[k])), (what, k)
        flagged = ref["flags"] != 0
        assert got["n_edges"][g] == (ne[g] if flagged else ref["n_edges"]), what
        assert np.array_equal(got["edge_ij"][g], ij[g] if flagged else ref["edge_ij"]), what
        assert np.array_equal(bits(got["edge_z"][g]), bits(z[g] if flagged else ref["edge_z"])), what
        assert np.array_equal(bits(got["edge_info"][g]), bits(info[g] if flagged else ref["edge_info"])), what
        # trace: zeros where nothing was evaluated, else the library's cos and sin within 1e-15 of NumPy's
        n_used = int(nn[g]) if ref["trace"].any() else 0
        assert not got["trace"][g][n_used:].any(), what
        if n_used:
            worst = max(worst, np.abs(got["trace"][g][:n_used] - ref["trace"][:n_used]).max())
    print("trace (cos, sin) error", worst)
    assert worst <= 1e-15
    return got


def graph_of(N, rng, extra, C):
    q = tgp.graph_of(N, rng, extra)
    q["cij"], q["cz"], q["cinfo"] = tpc.candidates(N, q["pose"], rng, C)
    # (every third one close to what the poses say, so that some are accepted whatever the graph)
    near = np.arange(C) % 3 == 0
    q["cz"][near] = pg.relative_pose(q["pose"][q["cij"][near, 0] % N], q["pose"][q["cij"][near, 1] % N]) + rng.normal(0, 1, (int(near.sum()), 3)) * [1.0, 1.0, 1e-3]
    return q


@pytest.mark.parametrize("N", (2, 3, 22, 23, 64))
def test_shapes(ctx, N):
    """Three graphs a call: the full one with C = C_cap = 64 and all but three of its edge slots taken, one with a
    single candidate, one a node smaller.  Without append the edges stay bit for bit; a second call into the same
    buffers without new junk; then append, which runs out of room in the full graph."""
    rng = np.random.default_rng(1100 + N)
    Cc = 64
    full = graph_of(N, rng, 2 * N, Cc)
    one = graph_of(N, rng, 0, 1)
    small = graph_of(max(2, N - 1), rng, 3, 5)
    Ec = 1024 if N == 64 else len(full["ij"]) + 3  # (N = 64 with max_edges = 1024 and 64 candidates is the largest LDS)
    if N == 64:
        full = graph_of(N, rng, Ec - 3 - (N + 3), Cc)
    assert len(full["ij"]) == Ec - 3
    B = Buffers(ctx, 3, N, Ec, Cc)
    graphs = [full, one, small]
    a = run(B, graphs)
    f = a["cand_flags"][0]
    assert not a["flags"].any() and f[2] == gr.BAD_EDGE and f[3] == gr.BAD_INFO and (f == gr.ACCEPTED).any() and (f == gr.OUTLIER).any()
    b = run(B, graphs, junk=False)  # a second call into the same buffers
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = run(B, graphs, append=1, nis_max=float("inf"))
    f = c["cand_flags"][0]
    assert c["n_edges"][0] == Ec and ((f & gr.APPENDED) != 0).sum() == 3 and ((f & gr.NO_ROOM) != 0).sum() >= 3
    d = run(B, graphs, append=1, damp_t=0.0, damp_r=0.0)
    assert not d["flags"].any()


def test_one_graph_and_many(ctx):
    """G = 1; then G = 300 (more than the CUs) with N, E and C varying from graph to graph and, between the good ones,
    EMPTY, BAD_GRAPH (n_cand out of range among them) and SINGULAR graphs, whose candidates stay UNJUDGED."""
    rng = np.random.default_rng(41)
    run(Buffers(ctx, 1, 5, 16, 3), [graph_of(5, rng, 2, 3)], append=1)
    Nc, Ec, Cc, G = 8, 16, 11, 300
    graphs = []
    for g in range(G):
        N = int(rng.integers(2, Nc + 1))
        q = graph_of(N, rng, int(rng.integers(0, 4)), int(rng.integers(0, Cc + 1)))
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
                q["n_cand"] = (Cc + 1, -1)[g // 60 % 2]
            else:
                q["info"] = q["info"].copy()
                q["info"][len(q["ij"]) - 1, 4] = np.nan
        elif kind == 7:
            q["info"] = -q["info"]  # SINGULAR: a negative pivot
        graphs.append(q)
    B = Buffers(ctx, G, Nc, Ec, Cc)
    r = run(B, graphs, append=1)
    f = r["flags"]
    assert (f[3::10] == pg.EMPTY).all() and (f[5::10] == pg.BAD_GRAPH).all() and (f[7::10] == pg.SINGULAR).all()
    assert not f[0::10].any() and not r["cand_flags"][3::10].any() and not r["cand_flags"][7::10].any()
    assert ((r["cand_flags"] & gr.APPENDED) != 0).sum() > 100 and ((r["cand_flags"] & gr.NO_ROOM) != 0).any()
    run(B, graphs, junk=False)
    # three graphs, C_cap = 1
    rng = np.random.default_rng(42)
    run(Buffers(ctx, 3, 6, 12, 1), [graph_of(5, rng, 0, 1), graph_of(6, rng, 1, 0), graph_of(4, rng, 1, 1)], append=1)


def looped_graph(ctx, R, N, init, revs, odo, **kw):
    graph = posegraph.PoseGraph(ctx, R, **kw)
    for k in range(N):
        assert graph.add_keyframe(init[k], tgp.csr_of(revs[k]), odo_info=odo) == k
    return graph


def test_wrapper_unsynced_and_errors(ctx):
    """PoseGraph: gate(sync=False), solve(sync=False) and an unsynced grid.step on node_pose(k) draw what the synced
    chain draws; the host mirrors after reconciliation are the device's edges; the wrapper's own errors."""
    from lidar_slam_amd.mapping import OccupancyGrid
    R, N = 2, 6
    truth, init, edges = tgp.loops_in_the_room(R, N)
    revs = [synth.revolutions_at(truth[k], k, [300, 301]) for k in range(N)]
    odo = edges[0][2][0]
    loop_info = [0.04, 0, 0, 0.04, 0, 4e4]
    graphs = [looped_graph(ctx, R, N, init, revs, odo, max_nodes=8, max_edges=16, max_cand=4) for _ in range(2)]
    for graph in graphs:
        for r in range(R):
            zt = pg.relative_pose(truth[N - 1, r], truth[0, r])
            graph.propose(N - 1, 0, zt + [500.0, 0.0, 0.0], loop_info, graph=r)
            graph.propose(N - 1, 0, zt, loop_info, graph=r)
    kw = dict(grid_w=256, origin=(-560.0, -1060.0))
    g1, g2 = OccupancyGrid(ctx, R, **kw), OccupancyGrid(ctx, R, **kw)
    dxy = ctx.to_device(revs[N - 1]["xy"])
    a, b = graphs
    a.gate(sync=False)
    a.solve(sync=False)
    g1.step(dxy, revs[N - 1]["scan_chunk_off"], revs[N - 1]["chunk_pt_off"], pose=a.node_pose(N - 1), sync=False)
    ctx.sync()
    assert (a.n_edges_host == N - 1).all()  # (not yet reconciled: nothing has read the mirrors)
    b.gate()
    assert (b.n_edges_host == N).all()
    b.solve()
    res = b.results()
    assert (res["flags"] == pg.CONVERGED).all()
    g2.step(*tgp.csr_of(revs[N - 1]), pose=res["pose"][:, N - 1])
    assert g1.logodds.download().tobytes() == g2.logodds.download().tobytes()
    ga, gb = a.gate_results(), b.gate_results()
    for k in ga:
        assert ga[k].tobytes() == gb[k].tobytes(), k
    assert (ga["cand_flags"][:, 0] == gr.OUTLIER).all() and (ga["cand_flags"][:, 1] == gr.ACCEPTED | gr.APPENDED).all()
    assert not ga["cand_flags"][:, 2:].any() and not ga["flags"].any()
    for graph in graphs:  # the mirrors are the device's edges
        ne = graph.n_edges.download()
        assert np.array_equal(ne, graph.n_edges_host) and (ne == N).all()
        assert np.array_equal(graph.edge_ij.download()[:, :N], graph.ij_host[:, :N]) and (graph.ij_host[:, N - 1] == (N - 1, 0)).all()
        assert np.array_equal(bits(graph.edge_z.download()[:, :N]), bits(graph.z_host[:, :N]))
        assert np.array_equal(bits(graph.edge_info.download()[:, :N]), bits(graph.info_host[:, :N]))
    for r in range(R):  # the reference on the mirrors gives the device's poses
        ref = pg.solve(a.pose_host[:, r], a.ij_host[r], a.z_host[r], a.info_host[r], n_nodes=N, n_edges=N, trace=a.results()["trace"][r])
        assert np.array_equal(bits(a.results()["pose"][r]), bits(ref["pose_out"][:N]))
    # an edge added behind an unsynced appending gate lands behind the appended one
    a.propose(0, 2, pg.relative_pose(init[0], init[2]), loop_info)
    a.gate(nis_max=float("inf"), sync=False)
    a.add_edge(1, 3, pg.relative_pose(init[1, 0], init[3, 0]), loop_info, graph=0)
    assert list(a.n_edges_host) == [N + 2, N + 1] and tuple(a.ij_host[0, N]) == (0, 2) and tuple(a.ij_host[0, N + 1]) == (1, 3)
    a.solve()
    assert np.array_equal(a.n_edges.download(), a.n_edges_host) and np.array_equal(a.edge_ij.download(), a.ij_host)
    # relative_covariance: the gate's cov of that pair, whatever z; the proposals stay
    b.propose(0, 3, [0.0, 0.0, 0.0], loop_info, graph=1)
    cov = b.relative_covariance(0, 3)
    assert cov.shape == (R, 6) and (cov[:, [0, 3, 5]] > 0).all() and len(b._cand[1]) == 1
    b.gate(append=False)
    assert np.array_equal(bits(b.gate_results()["cov"][1, 0]), bits(cov[1])) and (b.n_edges_host == N).all()
    xy, th = posegraph.closure_window(cov)
    assert xy.shape == (R,) and (xy > 0).all() and (th > 0).all()
    with pytest.raises(ValueError):
        b.relative_covariance(2, 2)
    with pytest.raises(ValueError):
        posegraph.PoseGraph(ctx, 1, max_cand=65)
    with pytest.raises(ValueError):
        posegraph.PoseGraph(ctx, 1).gate_results()
    with pytest.raises(ValueError):
        b.gate(nis_max=0.0)
    with pytest.raises(ValueError):
        for _ in range(5):
            b.propose(0, 1, [0.0, 0.0, 0.0], loop_info, graph=0)
    with pytest.raises(ValueError):
        b.propose(0, 1, [0.0, 0.0, 0.0], loop_info, graph=R)


def test_end_to_end_a_false_closure_is_kept_out_of_the_map(ctx):
    """The room of tests/test_gpu_posegraph.py's end-to-end case.  The closure found by DistanceField.align and the
    same closure with z moved 500 mm are proposed together; gate, solve and redraw run without a host wait."""
    from lidar_slam_amd.mapping import FIELDALIGN_REJECTED, DistanceField, OccupancyGrid
    R, N, ids = 2, 24, [310, 311]
    truth, init, edges = tgp.loops_in_the_room(R, N, bias=(2.0, -1.5, 0.002))
    revs = [synth.revolutions_at(truth[k], k, ids) for k in range(N)]
    kw = dict(grid_w=256, origin=(-560.0, -1060.0))
    odo = edges[0][2][0]
    gated, alone, both = (looped_graph(ctx, R, N, init, revs, odo, max_nodes=N, max_edges=32) for _ in range(3))
    grid = OccupancyGrid(ctx, R, **kw)
    for k in range(3):
        grid.step(*tgp.csr_of(revs[k]), pose=init[k])
    field = DistanceField(grid)
    field.step()
    field.align(*tgp.csr_of(revs[N - 1]), pose=init[N - 1])
    al = field.align_results()
    assert not (al["flags"] & FIELDALIGN_REJECTED).any(), al["flags"]
    H = field.align_information()[0]
    # the window in which to look for this closure, from the graph before it: it holds the drift that is there
    cov = gated.relative_covariance(0, N - 1)
    half_xy, half_th = posegraph.closure_window(cov)
    for r in range(R):
        d = pg.relative_pose(truth[0, r], truth[N - 1, r]) - pg.relative_pose(init[0, r], init[N - 1, r])
        print("robot %d: drift of the last keyframe in the first's frame %.1f mm %.4f rad, window %.1f mm %.4f rad"
              % (r, np.hypot(d[0], d[1]), abs(d[2]), half_xy[r], half_th[r]))
        assert np.hypot(d[0], d[1]) <= half_xy[r] and abs(d[2]) <= half_th[r]
    for r in range(R):
        z, info = posegraph.closure_edge(init[0, r], al["pose_out"][r], H[r], cell=float(grid.p.cell))
        zf = z + [500.0, 0.0, 0.0]
        gated.propose(0, N - 1, z, info, graph=r)
        gated.propose(0, N - 1, zf, info, graph=r)
        alone.add_edge(0, N - 1, z, info, graph=r)
        both.add_edge(0, N - 1, z, info, graph=r)
        both.add_edge(0, N - 1, zf, info, graph=r)
    good, plain = OccupancyGrid(ctx, R, **kw), OccupancyGrid(ctx, R, **kw)
    gated.gate(sync=False)
    gated.solve(sync=False)
    good.redraw(gated)
    alone.solve()
    both.solve(sync=False)
    plain.redraw(both)
    gres, res, want = gated.gate_results(), gated.results(), alone.results()
    print("d2 of the found closure %s, of the moved one %s" % (gres["nis"][:, 0], gres["nis"][:, 1]))
    assert (gres["cand_flags"][:, 0] == gr.ACCEPTED | gr.APPENDED).all() and (gres["cand_flags"][:, 1] == gr.OUTLIER).all()
    assert (res["flags"] == pg.CONVERGED).all() and np.array_equal(res["flags"], want["flags"])
    assert np.array_equal(bits(res["pose"]), bits(want["pose"]))
    for r in range(R):  # the device's verdicts are the reference's
        ref = gr.gate(gated.pose_host[:, r], gated.ij_host[r, :N - 1], gated.z_host[r, :N - 1], gated.info_host[r, :N - 1],
                      [[0, N - 1]] * 2, [gated.z_host[r, N - 1], gated.z_host[r, N - 1] + [500.0, 0.0, 0.0]],
                      [gated.info_host[r, N - 1]] * 2, n_nodes=N, trace=gated._gate["trace"].download()[r])
        assert list(ref["cand_flags"]) == [gr.ACCEPTED, gr.OUTLIER]
        assert np.array_equal(bits(ref["cand_nis"]), bits(gres["nis"][r, :2]))
    true_map = OccupancyGrid(ctx, R, **kw)
    for k in range(N):
        true_map.step(*tgp.csr_of(revs[k]), pose=truth[k], sync=False)
    identity = [1.0, 0.0, 0.0, 0.0]

    def permille(g):
        g.merge(true_map, identity, dry_run=True)
        s = g.merge_results()["stats"].astype(np.float64)
        return 1000.0 * s[:, 3] / np.maximum(s[:, 2] + s[:, 3], 1.0)
    bad, fine = permille(plain), permille(good)
    print("contradicted cells per thousand against the true map: a plain solve given both %s, gated %s" % (bad, fine))
    assert (fine < bad).all()
