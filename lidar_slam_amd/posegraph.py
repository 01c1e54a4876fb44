"""Loop closure: a batched 2-D pose graph per robot (``lslam_pose_graph``) and the redraw of a map from
its corrected keyframes.

Every grid is drawn from the filter's own poses, and a robot that drives a loop comes back with the
loop's drift in its pose.  ``GridLocalizer``, ``DistanceField.align`` and ``GridRelocalizer`` can measure
that error (the last revolution matched against the part of the map drawn at the start); ``PoseGraph``
is what the measurement is handed to.  Its nodes are keyframe poses, its edges relative poses: the
odometry between consecutive keyframes and the closures the caller found.  ``solve`` spreads the closures'
corrections back over the trajectories by damped Gauss-Newton on the device, all graphs in one launch,
and ``OccupancyGrid.redraw`` draws the maps again from the stored revolutions at the corrected poses::

    graph = PoseGraph(ctx, R, max_nodes=32)
    graph.add_keyframe(pose, (xy, sco, cpo), odo_info=odo)         # every few revolutions
    ...
    field.align(xy, sco, cpo, pose=pose_now)                       # the revisit, matched in the old map
    z, info = closure_edge(pose_first, found, field.align_information()[0][r], cell=20.0)
    graph.add_edge(last, 0, z, info, graph=r)
    graph.solve()
    grid.redraw(graph)

The corrected poses are node-major on the device: ``node_pose(k)`` is a [G, 3] slab that every map-side
call takes as its ``pose`` in place.  The definition is the comment on ``lslam_pose_graph`` in
include/lidarslam.h; tests/posegraph_ref.py is its NumPy form and the kernel matches it bit for bit,
given the (cos, sin) the library wrote to ``trace``.

A closure that is wrong destroys a map that was good, so closures are not added but proposed: ``gate``
(``lslam_pose_graph_gate``) judges every candidate against what the graph without it predicts, by the
innovation d2 = e^T (J Sigma J^T + Omega^-1)^-1 e with Sigma the graph's covariance, and only those within
``nis_max`` become edges, on the device::

    graph.propose(last, 0, z, info, graph=r)
    graph.gate(sync=False); graph.solve(sync=False); grid.redraw(graph)     # no host wait in between
    graph.gate_results()["cand_flags"]                                      # POSEGATE_APPENDED or POSEGATE_OUTLIER

``relative_covariance(i, j)`` is J Sigma J^T alone, where keyframe j is expected in keyframe i's frame, and
``closure_window`` turns it into the (half_xy, half_theta) of ``GridRelocalizer.relocalize(window=...)``.

Limits: the solve is dense, so at most 64 keyframes a graph; the solve itself has no robust kernel: a false
closure that reaches it pulls the whole graph, so it is rejected before, by ``gate``; candidates are judged
one by one against the trusted graph, not against each other; the covariance is the linearised one at the
poses given, with the damping in it as a weak prior on every node; a graph whose odometry information is
overconfident rejects true closures; closures are the caller's to detect; ``redraw`` replays every keyframe.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import Context, DeviceArray
from .slam import LandmarkMap

POSEGRAPH_EMPTY, POSEGRAPH_BAD_GRAPH = _lib.POSEGRAPH_EMPTY, _lib.POSEGRAPH_BAD_GRAPH
POSEGRAPH_CONVERGED, POSEGRAPH_SINGULAR, POSEGRAPH_DIVERGED = _lib.POSEGRAPH_CONVERGED, _lib.POSEGRAPH_SINGULAR, _lib.POSEGRAPH_DIVERGED
# a graph with one of these kept its poses bit for bit
POSEGRAPH_REJECTED = POSEGRAPH_BAD_GRAPH | POSEGRAPH_SINGULAR | POSEGRAPH_DIVERGED
POSEGATE_UNJUDGED, POSEGATE_ACCEPTED, POSEGATE_OUTLIER = _lib.POSEGATE_UNJUDGED, _lib.POSEGATE_ACCEPTED, _lib.POSEGATE_OUTLIER
POSEGATE_BAD_EDGE, POSEGATE_BAD_INFO = _lib.POSEGATE_BAD_EDGE, _lib.POSEGATE_BAD_INFO
POSEGATE_APPENDED, POSEGATE_NO_ROOM = _lib.POSEGATE_APPENDED, _lib.POSEGATE_NO_ROOM
_DOUBLES = ("damp_t", "damp_r", "eps_t", "eps_r")


def relative_pose(a, b):
    """z of an edge a -> b: the pose ``b`` seen from ``a``, (R(theta_a)^T (p_b - p_a), theta_b - theta_a).
    On the host, in NumPy: [3] and [3] -> [3]; [n, 3] and [n, 3] -> [n, 3].  The one place where z's bits
    are made; the library takes them as they are."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or a.shape[-1] != 3:
        raise ValueError("two poses (x, y, theta), or two arrays [n, 3] of them")
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    return np.stack([c * dx + s * dy, c * dy - s * dx, b[..., 2] - a[..., 2]], -1)


def closure_edge(pose_i, pose_j_found, info_world, cell=1.0):
    """A closure's (z [3], info [6]) from node i's pose and the pose a matcher FOUND for node j in the
    map that i drew: z = ``relative_pose(pose_i, pose_j_found)``.  ``info_world``: the 3 x 3 information
    of the found pose in the world's axes, positions in units of ``cell`` mm and the heading in rad (for
    example one robot's ``DistanceField.align_information()[0]``, in cells: cell = the grid's cell);
    it is rotated into i's frame and scaled to mm, then symmetrised: xx, xy, xt, yy, yt, tt."""
    pi = np.asarray(pose_i, np.float64)
    W = np.asarray(info_world, np.float64)
    if pi.shape != (3,) or W.shape != (3, 3):
        raise ValueError("pose_i [3], pose_j_found [3] and info_world [3, 3]")
    z = relative_pose(pi, pose_j_found)
    c, s, k = np.cos(pi[2]), np.sin(pi[2]), 1.0 / float(cell)
    T = np.array([[c * k, -s * k, 0.0], [s * k, c * k, 0.0], [0.0, 0.0, 1.0]])
    O = T.T @ W @ T
    O = 0.5 * (O + O.T)
    return z, np.array([O[0, 0], O[0, 1], O[0, 2], O[1, 1], O[1, 2], O[2, 2]])


def closure_window(cov, k=3.0):
    """The search window for a closure from ``relative_covariance``'s ``cov`` ([G, 6] or [6]: xx, xy, xt, yy, yt,
    tt in mm and rad): per graph (half_xy, half_theta) = k (the square root of the larger eigenvalue of the
    2 x 2 position block, the square root of tt), the figures for ``GridRelocalizer.relocalize(window=,
    half_xy=, half_theta=)``."""
    c = np.asarray(cov, np.float64)
    if c.shape[-1] != 6:
        raise ValueError("cov [n_graphs, 6] or [6]")
    a, b, d = c[..., 0], c[..., 1], c[..., 3]
    lam = 0.5 * (a + d) + np.sqrt((0.5 * (a - d)) ** 2 + b * b)
    return float(k) * np.sqrt(lam), float(k) * np.sqrt(c[..., 5])


def gate_lds_bytes(max_nodes, max_edges, max_cand, slots):
    """The gate kernel's dynamic LDS of one graph in bytes (lslam_posegate.h posegate_lds_bytes) when ``slots``
    candidates are solved together: the triangle, the undivided column, the poses, (cos, sin), chi per edge, 3
    right-hand sides a slot, the candidates' flags and the two flag words."""
    n = 3 * (int(max_nodes) - 1)
    return 8 * (n * (n + 1) // 2 + n + 5 * int(max_nodes) + int(max_edges) + 3 * int(slots) * n + (int(max_cand) + 1) // 2 + 1)


def gate_slots(max_nodes, max_edges, max_cand):
    """The candidates the gate kernel solves together (lslam_posegate.h posegate_slots): max_cand, at most 8, fewer
    where the LDS would pass 160 KiB, one at least.  The results do not depend on it."""
    s = min(int(max_cand), 8)
    while s > 1 and gate_lds_bytes(max_nodes, max_edges, max_cand, s) > 160 * 1024:
        s -= 1
    return s


def lds_bytes(max_nodes, max_edges):
    """The kernel's dynamic LDS of one graph in bytes (lslam_posegraph.h posegraph_lds_bytes): the packed triangle
    of the 3 (max_nodes - 1) unknowns, g, the undivided column, the poses twice, (cos, sin), chi per edge, and two
    doubles of flag words and the chi2 sum.  At most 160 KiB; what bounds the workgroups a CU holds."""
    n = 3 * (int(max_nodes) - 1)
    return 8 * (n * (n + 1) // 2 + 2 * n + 8 * int(max_nodes) + int(max_edges) + 2)


class _Slab(DeviceArray):
    """A [G, 3] float64 view of one node's slab of a node-major pose buffer (which it keeps alive)."""

    def __init__(self, base, k, G):
        self.ctx, self.shape, self.dtype, self.nbytes = base.ctx, (G, 3), np.dtype(np.float64), 24 * G
        self.ptr = C.c_void_p(base.addr + 24 * G * int(k))
        self._base = base

    def free(self):  # (the memory is the base's)
        self.ptr = C.c_void_p()


class PoseGraph:
    """G graphs on one GPU, one per robot, grown keyframe by keyframe: every ``add_keyframe`` appends one
    node to every graph.  ``max_nodes`` (2..64), ``max_edges`` (1..1024) and ``params``: n_iter, damp_t,
    damp_r, eps_t, eps_r (``lslam_posegraph_params``; defaults 10, 1e-6 /mm^2, 1e-3 /rad^2, 0.01 mm,
    1e-5 rad).  The keyframes' poses as given are kept; ``solve`` starts from them and writes the corrected
    poses to a buffer of its own, of which ``node_pose(k)`` is node k's [G, 3] slab."""

    REJECTED = POSEGRAPH_REJECTED

    def __init__(self, ctx: Context, n_graphs: int, max_nodes=48, max_edges=256, max_cand=16, **params):
        G = int(n_graphs)
        if G <= 0:
            raise ValueError("n_graphs must be > 0")
        unknown = set(params) - set(_DOUBLES) - {"n_iter"}
        if unknown:
            raise TypeError("unknown parameters: %s" % ", ".join(sorted(unknown)))
        kw = {k: float(v) for k, v in params.items() if k in _DOUBLES}
        if "n_iter" in params:
            kw["n_iter"] = int(params["n_iter"])
        self.ctx, self.G = ctx, G
        self.p = _lib.posegraph_params(max_nodes=int(max_nodes), max_edges=int(max_edges), **kw)
        # (a range error of params surfaces here, before anything is allocated)
        _lib.call("lslam_pose_graph", ctx, _lib.PoseGraphBatch(), self.p)
        Nc, Ec = int(self.p.max_nodes), int(self.p.max_edges)
        self.Nc, self.Ec = Nc, Ec
        self.n = 0  # keyframes so far
        self.pose_host = np.zeros((Nc, G, 3))
        self.n_edges_host = np.zeros(G, np.int32)
        self.ij_host = np.zeros((G, Ec, 2), np.int32)
        self.z_host = np.zeros((G, Ec, 3))
        self.info_host = np.zeros((G, Ec, 6))
        self.revolutions = []  # per keyframe, what add_keyframe was given
        self.pose = ctx.empty((Nc, G, 3), np.float64)
        self.pose_out = ctx.empty((Nc, G, 3), np.float64)
        self.n_nodes, self.n_edges = ctx.empty(G, np.int32), ctx.empty(G, np.int32)
        self.edge_ij = ctx.empty((G, Ec, 2), np.int32)
        self.edge_z, self.edge_info = ctx.empty((G, Ec, 3), np.float64), ctx.empty((G, Ec, 6), np.float64)
        self.trace = ctx.empty((G, 33, Nc, 2), np.float64)  # n_iter's upper end + 1: self.p.n_iter may change between calls
        self.chi2, self.edge_chi2 = ctx.empty((G, 2), np.float64), ctx.empty((G, Ec), np.float64)
        self.iters, self.flags = ctx.empty(G, np.int32), ctx.empty(G, np.int32)
        for a in (self.pose, self.pose_out):
            a.fill_zero()
        self._dirty = True  # the edges on the host are newer than the device's
        self.solves = 0
        # closure gating: the candidates proposed on the host, the gate's buffers (made at the first gate) and
        # the candidates of an appending gate whose verdicts the host mirrors have not yet seen
        self.Cc = int(max_cand)
        if not 1 <= self.Cc <= 64:
            raise ValueError("max_cand must be in [1, 64]")
        self._cand = [[] for _ in range(G)]
        self._gate = None
        self._pending = None
        self.gates = 0

    def _slab_upload(self, buf, k):
        h = np.ascontiguousarray(self.pose_host[k])
        _lib.check(self.ctx._L.lslam_h2d(self.ctx.handle, C.c_void_p(buf.addr + 24 * self.G * k), h.ctypes.data_as(C.c_void_p),
                                         h.nbytes), "lslam_h2d")
        self.ctx._inflight.append(h)

    def add_keyframe(self, pose, revolution=None, odo_info=None):
        """Append a node to every graph at ``pose`` [G, 3]: a host array, a float64 ``DeviceArray`` or a
        ``LandmarkMap`` (the device forms are downloaded: the odometry edge is made on the host).
        ``revolution``: what ``OccupancyGrid.redraw`` will draw at this keyframe, in the argument forms of
        ``OccupancyGrid.step``: a ``MapInput``, or a tuple (xy, scan_chunk_off, chunk_pt_off) of host arrays
        or with a ``DeviceArray`` xy, which is then read in place at the redraw and must still hold the
        revolution.  ``odo_info`` ([6], or [G, 6]: xx, xy, xt, yy, yt, tt in the previous keyframe's frame):
        adds the odometry edge from the previous keyframe, z = ``relative_pose(previous, pose)``.  Returns
        the node's index."""
        G, k = self.G, self.n
        if k >= self.Nc:
            raise ValueError("the graphs hold max_nodes = %d keyframes" % self.Nc)
        self._reconcile()
        if isinstance(pose, LandmarkMap):
            pose = pose.x
        if isinstance(pose, DeviceArray):
            if pose.dtype != np.float64 or pose.nbytes < 24 * G:
                raise ValueError("device pose must be float64 [n_graphs, 3]")
            pose = pose.download().reshape(-1)[:3 * G]
        hp = np.ascontiguousarray(pose, np.float64)
        if hp.size != 3 * G:
            raise ValueError("pose must hold n_graphs x 3 values")
        self.pose_host[k] = hp.reshape(G, 3)
        self._slab_upload(self.pose, k)
        self._slab_upload(self.pose_out, k)  # (node_pose(k) is the keyframe's own pose until a solve corrects it)
        self.revolutions.append(revolution)
        self.n = k + 1
        self._dirty = True  # (n_nodes on the device is one behind)
        if odo_info is not None and k > 0:
            info = np.broadcast_to(np.asarray(odo_info, np.float64).reshape(-1, 6), (G, 6))
            z = relative_pose(self.pose_host[k - 1], self.pose_host[k])
            for g in range(G):
                self.add_edge(k - 1, k, z[g], info[g], graph=g)
        return k

    def add_edge(self, i, j, z, info, graph=None):
        """Append the edge i -> j with measurement ``z`` [3] (the pose of j seen from i) and information
        ``info`` [6] (xx, xy, xt, yy, yt, tt, in i's frame, 1/mm^2 and 1/rad^2) to graph ``graph``
        (None: to every graph; z and info may then be [G, 3] and [G, 6])."""
        self._reconcile()
        graphs = range(self.G) if graph is None else [int(graph)]
        z = np.broadcast_to(np.asarray(z, np.float64).reshape(-1, 3), (len(graphs), 3))
        info = np.broadcast_to(np.asarray(info, np.float64).reshape(-1, 6), (len(graphs), 6))
        for q, g in enumerate(graphs):
            if not 0 <= g < self.G:
                raise ValueError("graph must be in 0..n_graphs-1")
            e = int(self.n_edges_host[g])
            if e >= self.Ec:
                raise ValueError("graph %d holds max_edges = %d edges" % (g, self.Ec))
            self.ij_host[g, e] = (int(i), int(j))
            self.z_host[g, e], self.info_host[g, e] = z[q], info[q]
            self.n_edges_host[g] = e + 1
        self._dirty = True

    def solve(self, sync=True):
        """Optimise every graph (``lslam_pose_graph``) from the keyframes' poses as given; the corrected
        poses go to ``node_pose``.  A graph flagged ``REJECTED`` keeps its poses bit for bit."""
        ctx, G = self.ctx, self.G
        self._upload_graph()
        b = _lib.PoseGraphBatch()
        b.n_graphs = G
        b.n_nodes, b.n_edges, b.pose = self.n_nodes.addr, self.n_edges.addr, self.pose.addr
        b.edge_ij, b.edge_z, b.edge_info = self.edge_ij.addr, self.edge_z.addr, self.edge_info.addr
        b.pose_out, b.trace, b.chi2, b.edge_chi2 = self.pose_out.addr, self.trace.addr, self.chi2.addr, self.edge_chi2.addr
        b.iters, b.flags = self.iters.addr, self.flags.addr
        _lib.call("lslam_pose_graph", ctx, b, self.p)
        self._rows = int(self.p.n_iter) + 1
        self.solves += 1
        if sync:
            ctx.sync()

    def _upload_graph(self):
        """The host's counts and edges to the device, if they are newer (an appending gate's accepted
        candidates are taken into the host mirrors first)."""
        if not self._dirty:
            return
        self._reconcile()
        nn = np.full(self.G, self.n, np.int32)
        for buf, h in ((self.n_nodes, nn), (self.n_edges, self.n_edges_host.copy()), (self.edge_ij, self.ij_host.copy()),
                       (self.edge_z, self.z_host.copy()), (self.edge_info, self.info_host.copy())):
            buf.upload_async(h)
        self._dirty = False

    def _reconcile(self):
        """Bring ij_host, z_host, info_host and n_edges_host up to the device's edges behind an appending gate:
        the downloaded cand_flags say which candidates it copied, in order.  (The download waits for the gate.)"""
        if self._pending is None:
            return
        n_cand, cij, cz, cinfo = self._pending
        self._pending = None
        cf = self._gate["cand_flags"].download()
        for g in range(self.G):
            for c in range(int(n_cand[g])):
                if cf[g, c] & POSEGATE_APPENDED:
                    e = int(self.n_edges_host[g])
                    self.ij_host[g, e], self.z_host[g, e], self.info_host[g, e] = cij[g, c], cz[g, c], cinfo[g, c]
                    self.n_edges_host[g] = e + 1

    def propose(self, i, j, z, info, graph=None):
        """A closure candidate i -> j for the next ``gate``, in ``add_edge``'s arguments: kept on the host until
        then.  At most ``max_cand`` a graph between two gates."""
        graphs = range(self.G) if graph is None else [int(graph)]
        z = np.broadcast_to(np.asarray(z, np.float64).reshape(-1, 3), (len(graphs), 3))
        info = np.broadcast_to(np.asarray(info, np.float64).reshape(-1, 6), (len(graphs), 6))
        for g in graphs:
            if not 0 <= g < self.G:
                raise ValueError("graph must be in 0..n_graphs-1")
            if len(self._cand[g]) >= self.Cc:
                raise ValueError("graph %d holds max_cand = %d candidates" % (g, self.Cc))
        for q, g in enumerate(graphs):
            self._cand[g].append((int(i), int(j), z[q].copy(), info[q].copy()))

    def _gate_call(self, cand, nis_max, append, at):
        ctx, G, Nc, Cc = self.ctx, self.G, self.Nc, self.Cc
        p = _lib.posegate_params(max_nodes=Nc, max_edges=self.Ec, max_cand=Cc, damp_t=float(self.p.damp_t),
                                 damp_r=float(self.p.damp_r), nis_max=float(nis_max), append=1 if append else 0)
        # (a range error of params surfaces here, before anything is allocated or uploaded)
        _lib.call("lslam_pose_graph_gate", ctx, _lib.PoseGateBatch(), p)
        if at is None:
            at = self.pose_out if self.solves else self.pose
        elif not isinstance(at, DeviceArray):
            h = np.ascontiguousarray(at, np.float64)
            if h.ndim != 3 or h.shape[1:] != (G, 3) or not self.n <= h.shape[0] <= Nc:
                raise ValueError("at must be node-major [keyframes..max_nodes, n_graphs, 3]")
            full = np.zeros((Nc, G, 3))
            full[:h.shape[0]] = h
            at = ctx.empty((Nc, G, 3), np.float64)
            at.upload_async(full)
        if at.dtype != np.float64 or at.nbytes != 24 * Nc * G:
            raise ValueError("device at must be float64 [max_nodes, n_graphs, 3], node-major")
        self._upload_graph()
        if self._gate is None:
            e = ctx.empty
            self._gate = {"n_cand": e(G, np.int32), "cand_ij": e((G, Cc, 2), np.int32), "cand_z": e((G, Cc, 3), np.float64),
                          "cand_info": e((G, Cc, 6), np.float64), "trace": e((G, Nc, 2), np.float64), "chi2": e(G, np.float64),
                          "cand_nis": e((G, Cc), np.float64), "cand_err": e((G, Cc, 3), np.float64),
                          "cand_cov": e((G, Cc, 6), np.float64), "cand_flags": e((G, Cc), np.int32), "flags": e(G, np.int32)}
        B = self._gate
        n_cand = np.array([len(c) for c in cand], np.int32)
        cij, cz, cinfo = np.zeros((G, Cc, 2), np.int32), np.zeros((G, Cc, 3)), np.zeros((G, Cc, 6))
        for g, cs in enumerate(cand):
            for c, (i, j, z, info) in enumerate(cs):
                cij[g, c], cz[g, c], cinfo[g, c] = (i, j), z, info
        for name, h in (("n_cand", n_cand), ("cand_ij", cij), ("cand_z", cz), ("cand_info", cinfo)):
            B[name].upload_async(h)
        b = _lib.PoseGateBatch()
        b.n_graphs = G
        b.n_nodes, b.n_edges, b.pose = self.n_nodes.addr, self.n_edges.addr, at.addr
        b.edge_ij, b.edge_z, b.edge_info = self.edge_ij.addr, self.edge_z.addr, self.edge_info.addr
        for name, buf in B.items():
            setattr(b, name, buf.addr)
        _lib.call("lslam_pose_graph_gate", ctx, b, p)
        self._at = at  # (kept alive until the call has run)
        self.gates += 1
        if append:
            self._pending = (n_cand, cij, cz, cinfo)

    def gate(self, nis_max=16.27, append=True, at=None, sync=True):
        """Judge every proposed candidate against the graph as it stands (``lslam_pose_graph_gate``): d2 within
        ``nis_max`` (16.27: chi-square, 3 dof, 0.1 %; inf: no gate) is ``POSEGATE_ACCEPTED``.  With ``append`` the
        accepted candidates become edges on the device (``POSEGATE_APPENDED``, or ``POSEGATE_NO_ROOM``), so that
        ``gate(sync=False); solve(sync=False); grid.redraw(graph)`` chains without a host wait; the host mirrors
        (``ij_host``, ``z_host``, ``info_host``, ``n_edges_host``) follow from the downloaded verdicts at the next
        call that reads them (``add_edge``, ``add_keyframe``, a ``solve`` behind either, ``gate_results``), or at
        once with ``sync``.  ``at``: the node-major poses at which the graph is linearised, a float64
        ``DeviceArray`` or host array [max_nodes, G, 3]; None: the last solve's output, or the keyframes' poses
        before any solve.  The covariance means what it should where those poses are the graph's optimum
        (``gate_results()["chi2"]`` is its chi2 there).  The proposals are cleared."""
        self._reconcile()
        self._gate_call(self._cand, nis_max, append, at)
        self._cand = [[] for _ in range(self.G)]
        if sync:
            self.ctx.sync()
            self._reconcile()

    def gate_results(self):
        """The last gate's nis [G, max_cand] (d2), err [G, max_cand, 3] (e), cov [G, max_cand, 6] (J Sigma J^T as
        xx, xy, xt, yy, yt, tt), cand_flags [G, max_cand] (``POSEGATE_*``), flags [G] (0 or ``POSEGRAPH_EMPTY``,
        ``POSEGRAPH_BAD_GRAPH``, ``POSEGRAPH_SINGULAR``) and chi2 [G] of the graph at the poses it was judged at."""
        if not self.gates:
            raise ValueError("no gate yet")
        self._reconcile()
        B = self._gate
        return {"nis": B["cand_nis"].download(), "err": B["cand_err"].download(), "cov": B["cand_cov"].download(),
                "cand_flags": B["cand_flags"].download(), "flags": B["flags"].download(), "chi2": B["chi2"].download()}

    def relative_covariance(self, i, j, at=None):
        """cov [G, 6] (xx, xy, xt, yy, yt, tt; mm and rad) of where keyframe j is expected in keyframe i's frame,
        J Sigma J^T of the graph as it stands: a gate without append of the one candidate i -> j whose z is the
        current relative pose.  It does not depend on that z.  Waits for the device; the proposals stay, the last
        gate's results are replaced.  A graph that the gate flags gives zeros."""
        i, j = int(i), int(j)
        if i == j or not (0 <= i < self.n and 0 <= j < self.n):
            raise ValueError("two different nodes in 0..%d" % (self.n - 1))
        self._reconcile()
        if at is None:
            poses = self.pose_out.download() if self.solves else self.pose_host
        else:
            poses = at.download() if isinstance(at, DeviceArray) else np.asarray(at, np.float64)
        z = relative_pose(poses[i], poses[j])
        one = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]
        self._gate_call([[(i, j, z[g], np.array(one))] for g in range(self.G)], float("inf"), False, at)
        return self._gate["cand_cov"].download()[:, 0]

    def node_pose(self, k):
        """Node k's corrected poses, a float64 ``DeviceArray`` [G, 3] on the device: a slab of the last
        ``solve``'s output (the keyframe's own pose until a solve), read in place by whatever takes a
        ``pose``, in stream order."""
        if not 0 <= int(k) < self.n:
            raise ValueError("node must be in 0..%d" % (self.n - 1))
        return _Slab(self.pose_out, k, self.G)

    def results(self):
        """The last solve's pose [G, n, 3] (n keyframes), trace [G, n_iter + 1, max_nodes, 2], chi2 [G, 2]
        (first and last evaluation), edge_chi2 [G, max_edges], iters [G], flags [G] (``POSEGRAPH_*``)."""
        if not self.solves:
            raise ValueError("no solve yet")
        G, E = self.G, self._rows
        pose = np.ascontiguousarray(self.pose_out.download()[:self.n].transpose(1, 0, 2))
        trace = self.trace.download().reshape(-1)[:G * E * self.Nc * 2].reshape(G, E, self.Nc, 2)
        return {"pose": pose, "trace": trace, "chi2": self.chi2.download(), "edge_chi2": self.edge_chi2.download(),
                "iters": self.iters.download(), "flags": self.flags.download()}
