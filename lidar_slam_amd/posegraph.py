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

Limits: the solve is dense, so at most 64 keyframes a graph; there is no robust kernel: a false closure
pulls the whole graph and shows as the largest ``edge_chi2``, but is not rejected; closures are the
caller's to detect; ``redraw`` replays every keyframe.
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

    def __init__(self, ctx: Context, n_graphs: int, max_nodes=48, max_edges=256, **params):
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
        if self._dirty:
            nn = np.full(G, self.n, np.int32)
            for buf, h in ((self.n_nodes, nn), (self.n_edges, self.n_edges_host.copy()), (self.edge_ij, self.ij_host.copy()),
                           (self.edge_z, self.z_host.copy()), (self.edge_info, self.info_host.copy())):
                buf.upload_async(h)
            self._dirty = False
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
