"""Occupancy-grid mapping: batched inverse-sensor-model updates (``lslam_grid_update``).

The reference's GUI draws every measured point of the last revolution and forgets it
(``mainWindow.py``, ``allSeries.replace``); the per-robot landmark list exists to feed ``hx``.
``OccupancyGrid`` keeps the picture: per robot a square grid of clamped log-odds in HBM, updated
from a revolution and the robot's pose.  Every beam is traced from the robot cell to its return;
the cells it crosses become freer, the cell it ends in more occupied.  It chains onto
``LandmarkMap``, whose posterior pose it reads on the device::

    odo.step(xy, scan_chunk_off, chunk_pt_off, lm)       # writes lm.u
    lm.step(xy, scan_chunk_off, chunk_pt_off)            # writes lm.x
    grid.recentre(pose=lm)                               # rolls the grid under a robot that nears its edge
    grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)  # reads lm.x and the points in place

The definition (robot cell, integer ray, per-revolution sum, one clamp per call) is the comment on
``lslam_grid_update`` in include/lidarslam.h; tests/occgrid_ref.py is its NumPy form and the kernel
matches it bit for bit, given the (cos, sin) that the library wrote to ``rot``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, staging
from .device import Context, DeviceArray
from .staging import Staging, _Grow

GRID_BAD_POSE, GRID_CLIPPED = _lib.GRID_BAD_POSE, _lib.GRID_CLIPPED
RECENTRE_BAD_POSE, RECENTRE_MOVED, RECENTRE_CLEARED = _lib.RECENTRE_BAD_POSE, _lib.RECENTRE_MOVED, _lib.RECENTRE_CLEARED
PAGE_LOST = _lib.PAGE_LOST
MERGE_ADD, MERGE_FILL = _lib.MERGE_ADD, _lib.MERGE_FILL
MERGE_MERGED, MERGE_WEAK, MERGE_CONFLICT = _lib.MERGE_MERGED, _lib.MERGE_WEAK, _lib.MERGE_CONFLICT
MERGE_SKIPPED, MERGE_BAD_XFORM = _lib.MERGE_SKIPPED, _lib.MERGE_BAD_XFORM
GRIDPOINTS_BAD_ANCHOR, GRIDPOINTS_EMPTY, GRIDPOINTS_DECIMATED = _lib.GRIDPOINTS_BAD_ANCHOR, _lib.GRIDPOINTS_EMPTY, _lib.GRIDPOINTS_DECIMATED
DIST_OCC, DIST_NOT_FREE, DIST_EMPTY, FIELD_BAD_POSE = _lib.DIST_OCC, _lib.DIST_NOT_FREE, _lib.DIST_EMPTY, _lib.FIELD_BAD_POSE
FIELDALIGN_BAD_POSE, FIELDALIGN_CONVERGED, FIELDALIGN_SINGULAR = _lib.FIELDALIGN_BAD_POSE, _lib.FIELDALIGN_CONVERGED, _lib.FIELDALIGN_SINGULAR
FIELDALIGN_FEW, FIELDALIGN_DIVERGED, FIELDALIGN_WEAK = _lib.FIELDALIGN_FEW, _lib.FIELDALIGN_DIVERGED, _lib.FIELDALIGN_WEAK
# an alignment with one of these left pose_out as the guess: the correlative matcher's or the relocaliser's case
FIELDALIGN_REJECTED = FIELDALIGN_BAD_POSE | FIELDALIGN_SINGULAR | FIELDALIGN_FEW | FIELDALIGN_DIVERGED | FIELDALIGN_WEAK
FIELDFUSE_OUTLIER, FIELDFUSE_BAD_COV = _lib.FIELDFUSE_OUTLIER, _lib.FIELDFUSE_BAD_COV
# a fusion with one of these left the filter's mean and covariance as they were
FIELDFUSE_REJECTED = FIELDALIGN_REJECTED | FIELDFUSE_OUTLIER | FIELDFUSE_BAD_COV
_FUSE_DOUBLES = ("sigma_min", "r_scale", "floor_t", "floor_r", "nis_max")
_ALIGN_DOUBLES = ("trunc", "damp_t", "damp_r", "eps_t", "eps_r", "max_shift", "max_turn")
_ALIGN_INTS = ("n_iter", "min_points", "min_permille")
TILE = 64  # cells a side of the kernel's tile (lslam_grid.h GRID_T): the tests place rays on its seams


def recentre_band_rows(grid_w):
    """Rows of a band of the recentre kernel (lslam_recentre_plan.h recentre_band_rows): as many whole
    rows as 16384 cells hold.  The tests place shifts on its seams."""
    return max(1, min(int(grid_w), 16384 // int(grid_w)))


def merge_transform(pose_in_dst, pose_in_src):
    """The transform (c, s, tx, ty) of ``OccupancyGrid.merge`` from one robot's pose (x, y, theta) known in
    both map frames, e.g. where it stands in its own map and where ``GridRelocalizer`` placed the same
    revolution in the other's: it takes the destination's world coordinates to the source's.
    theta = theta_src - theta_dst, (c, s) = (cos theta, sin theta), t = p_src - R(theta) p_dst.  On the
    host, in NumPy: [3] and [3] -> [4]; [n, 3] and [n, 3] -> [n, 4].  The library takes these bits as
    they are."""
    d, s = np.asarray(pose_in_dst, np.float64), np.asarray(pose_in_src, np.float64)
    if d.shape != s.shape or d.shape[-1] != 3:
        raise ValueError("two poses (x, y, theta), or two arrays [n, 3] of them")
    th = s[..., 2] - d[..., 2]
    c, sn = np.cos(th), np.sin(th)
    tx = s[..., 0] - (c * d[..., 0] - sn * d[..., 1])
    ty = s[..., 1] - (sn * d[..., 0] + c * d[..., 1])
    return np.stack([c, sn, tx, ty], -1)


class OccupancyGrid:
    """R robots' grids on one GPU.  ``params``: cell, max_range, grid_w, l_hit, l_miss, l_min, l_max
    (``lslam_grid_params``; defaults 20 mm, 8000 mm, 512, 85, -41, -200, 350; log-odds in 0.01 nat).
    ``origin`` [R, 2] (or one pair for all): the world coordinates of the corner of cell (0, 0);
    default: every grid centred on (0, 0).  ``recentre`` moves it, on the device; ``origin_host`` is
    the host's copy, refreshed on its next read after a ``recentre``.

    ``canvas_w``: a world canvas of ``canvas_w`` x ``canvas_w`` cells behind every robot's grid (16..2048;
    ``lslam_page_params``), which is then a window onto it: ``recentre`` writes the strip that leaves
    the window to the canvas and reads the strip that enters from it (``lslam_grid_recentre_paged``), so
    a robot that comes back finds the room it mapped.  Without it nothing is allocated and ``recentre``
    loses what scrolls off.  The canvas costs 2 canvas_w^2 bytes a robot: 8 MiB at 2048, 32 GiB for
    4096 robots; it does not grow, and what leaves it is lost (``PAGE_LOST``).  ``win`` [R, 2] (or one
    pair): the canvas coordinates of window cell (0, 0); default: the window in the middle of the
    canvas, rounded down to a multiple of 8 (the 16-byte path needs it so).  ``canvas_origin``, on the
    device and set once here, is origin - win * cell: the world corner of canvas cell (0, 0).  It stays
    the canvas' origin exactly while the origins are multiples of ``cell`` that FP64 holds exactly (the
    caveat of ``lslam_grid_recentre``'s two roundings)."""

    def __init__(self, ctx: Context, n_robots: int, origin=None, canvas_w=None, win=None, _view=None, **params):
        R = int(n_robots)
        if R <= 0:
            raise ValueError("n_robots must be > 0")
        self.ctx, self.R = ctx, R
        if canvas_w is None and win is not None:
            raise ValueError("win needs canvas_w")
        # (_view, world()'s: the params, origin and logodds of existing device buffers instead of new ones)
        self.p = _view[0] if _view else _lib.grid_params(**params)
        self.W = int(self.p.grid_w)
        half = 0.5 * self.W * self.p.cell
        o = np.full((R, 2), -half) if origin is None else np.asarray(origin, np.float64)
        self._origin_host = np.ascontiguousarray(np.broadcast_to(o, (R, 2)), np.float64)
        self._origin_stale = False  # a recentre may have moved the device's origin since the last read
        # (a range error of params surfaces here, from the first call, before anything large is allocated)
        _lib.call("lslam_grid_update", ctx, _lib.GridBatch(), self.p)
        if _view:
            self.origin, self.logodds = _view[1], _view[2]
            self._origin_stale = True  # (the first read downloads it)
        else:
            self.origin = ctx.to_device(self._origin_host)
            self.logodds = ctx.empty((R, self.W, self.W), np.int16)
            self.logodds.fill_zero()
        self.rot = ctx.empty((R, 2), np.float64)
        self.n_used = ctx.empty((R, 2), np.int32)
        self.flags = ctx.empty(R, np.int32)
        for a in (self.rot, self.n_used, self.flags):
            a.fill_zero()
        self._stage = Staging(ctx, R)
        self.steps = 0
        self._shift = self._rflags = None  # recentre's outputs, allocated by its first call
        self._merge = None  # merge's outputs (stats, flags), allocated by its first call
        self._merge_snap = None  # the sources' snapshot of a merge from this grid's own buffer
        self.canvas_w = self.canvas = None
        if canvas_w is not None:
            self._init_canvas(int(canvas_w), win)

    def _init_canvas(self, Cw, win):
        ctx, R = self.ctx, self.R
        if not 16 <= Cw <= 2048:  # (lslam_page_params.canvas_w's range, before the canvas is allocated)
            raise ValueError("canvas_w must be in [16, 2048]")
        self.pp = _lib.page_params(canvas_w=Cw)
        mid = (Cw - self.W) // 2 // 8 * 8
        w = np.full((R, 2), mid) if win is None else np.asarray(win)
        if not np.issubdtype(w.dtype, np.integer):
            raise ValueError("win must be integers")
        if w.size and (w.min() < -2 ** 31 or w.max() >= 2 ** 31):
            raise ValueError("win must fit 32 bits")
        w = np.ascontiguousarray(np.broadcast_to(w, (R, 2)), np.int32)
        self.canvas_w = Cw
        self.canvas = ctx.empty((R, Cw, Cw), np.int16)
        self.canvas.fill_zero()
        self.win = ctx.to_device(w)
        self.moved = ctx.empty((R, 2), np.int32)
        self.page_flags = ctx.empty(R, np.int32)
        for a in (self.moved, self.page_flags):
            a.fill_zero()
        self.canvas_origin = ctx.to_device(self._origin_host - w.astype(np.float64) * float(self.p.cell))

    def _page_batch(self):
        if self.canvas is None:
            raise ValueError("this grid has no canvas (canvas_w)")
        pg = _lib.PageBatch()
        pg.n_robots = self.R
        pg.canvas, pg.win, pg.moved, pg.flags = self.canvas.addr, self.win.addr, self.moved.addr, self.page_flags.addr
        return pg

    @property
    def origin_host(self):
        """origin [R, 2] on the host.  After a ``recentre`` the next read waits for the stream and
        downloads the 16 bytes per robot; without one it is the array given at construction."""
        if self._origin_stale:
            self._origin_host = self.origin.download()
            self._origin_stale = False
        return self._origin_host

    @classmethod
    def centred_on(cls, ctx, x0, **params):
        """One grid per row of ``x0`` [R, >= 2] (start poses), each centred on its robot's start."""
        x0 = np.asarray(x0, np.float64)
        x0 = x0.reshape(-1, x0.shape[-1])
        p = _lib.grid_params(**params)
        return cls(ctx, len(x0), origin=x0[:, :2] - 0.5 * p.grid_w * p.cell, **params)

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, pose=None, sync=True):
        """One revolution per robot, in the CSR layout of ``LandmarkMap.step`` / ``LidarOdometry.step``
        (host array, ``DeviceArray`` or a ``MapInput``).  Device points are read in place: the call
        is ordered on the context's stream, before whatever overwrites them later.  ``pose``
        [R, 3] (x, y, theta): a host array, a float64 ``DeviceArray`` (``lm.x``) or a ``LandmarkMap``."""
        ctx, R = self.ctx, self.R
        staging.require_pose(pose)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        dpose = self._stage.pose(pose, "grid")
        b = _lib.GridBatch()
        b.n_robots = R
        b.xy, b.pt_off, b.pose, b.origin = dxy.addr, doff.addr, dpose.addr, self.origin.addr
        b.logodds, b.rot, b.n_used, b.flags = self.logodds.addr, self.rot.addr, self.n_used.addr, self.flags.addr
        _lib.call("lslam_grid_update", ctx, b, self.p)
        self.steps += 1
        if sync:
            ctx.sync()

    def recentre(self, pose, margin=None, quantum=None, sync=True):
        """Roll every grid whose robot is within ``margin`` cells of an edge (``lslam_grid_recentre``):
        the grid and ``origin`` move by whole cells, multiples of ``quantum``, in place on the device,
        so that the robot's cell is back in the middle.  Without a canvas what scrolls off is lost and
        what scrolls in is unknown; with one (``canvas_w``) the strip that leaves goes to the canvas and
        the strip that enters comes from it (``lslam_grid_recentre_paged``), and only what leaves the
        canvas is lost.  ``pose`` as in ``step``; ``margin``, ``quantum``: ``lslam_recentre_params``
        (defaults 128 and 8 cells).  The localizers and ray casters built on this grid read ``origin`` on
        the device and follow."""
        ctx, R = self.ctx, self.R
        kw = {k: int(v) for k, v in (("margin", margin), ("quantum", quantum)) if v is not None}
        q = _lib.recentre_params(**kw)
        dpose = self._stage.pose(pose, "grid")
        if self._shift is None:
            self._shift, self._rflags = ctx.empty((R, 2), np.int32), ctx.empty(R, np.int32)
        b = _lib.RecentreBatch()
        b.n_robots = R
        b.pose, b.origin, b.logodds = dpose.addr, self.origin.addr, self.logodds.addr
        b.shift, b.flags = self._shift.addr, self._rflags.addr
        if self.canvas is None:
            _lib.call("lslam_grid_recentre", ctx, b, self.p, q)
        else:
            _lib.call("lslam_grid_recentre_paged", ctx, b, self._page_batch(), self.p, q, self.pp)
        self._origin_stale = True
        if sync:
            ctx.sync()

    def recentre_results(self):
        """The last ``recentre``'s shift [R, 2] (sx, sy in cells), flags [R] (RECENTRE_*) and the origin
        [R, 2] as it now stands; with a canvas also moved [R, 2] (cells stored to the canvas, cells loaded
        from it), win [R, 2] as it now stands and page_flags [R] (``PAGE_LOST``)."""
        if self._shift is None:
            raise ValueError("no recentre yet")
        out = {"shift": self._shift.download(), "flags": self._rflags.download(), "origin": self.origin_host}
        if self.canvas is not None:
            out.update(moved=self.moved.download(), win=self.win.download(), page_flags=self.page_flags.download())
        return out

    def flush(self, sync=True):
        """Write every window cell that is on the canvas to it (``lslam_grid_page_flush``): after it the
        canvas is the world view.  ``moved`` becomes (cells stored, 0)."""
        _lib.call("lslam_grid_page_flush", self.ctx, self._page_batch(), self.logodds.addr, self.p, self.pp)
        if sync:
            self.ctx.sync()

    def load(self, sync=True):
        """Fill the window from the canvas where it lies now, zero where it hangs off
        (``lslam_grid_page_load``): the start of a robot in a stored map.  ``moved`` becomes
        (0, cells loaded)."""
        _lib.call("lslam_grid_page_load", self.ctx, self._page_batch(), self.logodds.addr, self.p, self.pp)
        if sync:
            self.ctx.sync()

    def world(self, sync=True):
        """The world view as a grid: ``flush``, then an ``OccupancyGrid``-shaped view of ``canvas_w`` cells a
        side that SHARES the canvas buffer (``logodds`` is the canvas, ``origin`` is ``canvas_origin``).
        ``GridRelocalizer``, ``GridLocalizer``, ``GridRayCaster`` and ``DistanceField`` take it as they take
        a grid.  It is a view for reading: a ``step`` or ``recentre`` on it would write the canvas behind the
        window's back.  Its origin agrees with the window's exactly when the origins are multiples of
        ``cell`` that FP64 holds exactly."""
        self.flush(sync=sync)
        p = _lib.GridParams.from_buffer_copy(self.p)
        p.grid_w = self.canvas_w
        return OccupancyGrid(self.ctx, self.R, _view=(p, self.canvas_origin, self.canvas))

    def merge(self, src, xform, src_index=None, mode=MERGE_ADD, dry_run=False, sync=True, **gates):
        """Fold ``src``'s maps into this grid's (``lslam_grid_merge``): robot m's grid takes source grid
        ``src_index[m]`` (None: m), resampled under ``xform[m]`` = (c, s, tx, ty), which takes this grid's
        world coordinates to the source's (``merge_transform`` makes it from one pose known in both
        frames), checked against what this grid already holds and, if the two agree, added.

        ``src``: another ``OccupancyGrid`` or a ``world()`` view, of any width but of this grid's ``cell``.
        ``xform``: host [R, 4] (or one row for all) or a float64 ``DeviceArray``; ``src_index``: host
        integers [R] or an int32 ``DeviceArray``; an index outside 0..src.R-1 skips its robot
        (``MERGE_SKIPPED``).  ``mode``: ``MERGE_ADD`` adds the source's log-odds (the same evidence merged
        twice counts twice), ``MERGE_FILL`` writes only cells this grid does not know.  ``dry_run``:
        statistics and flags only.  ``gates``: occ_min, min_support, max_contra_permille
        (``lslam_gridmerge_params``; defaults 85, 64, 100): a robot whose source has fewer than
        ``min_support`` occupied cells next to occupied cells of this grid is ``MERGE_WEAK``, one with more
        than ``max_contra_permille`` of them in space this grid holds free is ``MERGE_CONFLICT`` (a wrong
        transform); either keeps its grid bit for bit.

        If ``src`` shares this grid's buffer (a grid merged into itself under a transform), the source
        grids are first copied to a snapshot allocated by the first such call (``lslam_d2d``): 2 W^2
        bytes a robot, kept for the grid's life."""
        ctx, R = self.ctx, self.R
        if not isinstance(src, OccupancyGrid):
            raise ValueError("src must be an OccupancyGrid (or a world() view)")
        if float(src.p.cell) != float(self.p.cell):
            raise ValueError("src has cell %r, this grid %r: a merge needs the same cell" % (float(src.p.cell), float(self.p.cell)))
        unknown = set(gates) - {"occ_min", "min_support", "max_contra_permille"}
        if unknown:
            raise TypeError("unknown parameters: %s" % ", ".join(sorted(unknown)))
        q = _lib.gridmerge_params(src_w=src.W, n_src=src.R, mode=int(mode), dry_run=int(bool(dry_run)),
                                  **{k: int(v) for k, v in gates.items()})
        # (a range error of params surfaces here, before anything is staged)
        _lib.call("lslam_grid_merge", ctx, _lib.GridMergeBatch(), self.p, q)
        dx = self._stage.per_robot("merge_xform", xform, 4, np.float64, "xform")
        di = None
        if src_index is not None:
            if not isinstance(src_index, DeviceArray) and not np.issubdtype(np.asarray(src_index).dtype, np.integer):
                raise ValueError("src_index must be integers")
            di = self._stage.per_robot("merge_index", src_index, 1, np.int32, "src_index")
        if self._merge is None:
            self._merge = (ctx.empty((R, 8), np.int32), ctx.empty(R, np.int32))
        slog = src.logodds
        if slog.addr == self.logodds.addr:
            if self._merge_snap is None:
                self._merge_snap = ctx.empty((R, self.W, self.W), np.int16)
            ctx.copy(self._merge_snap, slog)
            slog = self._merge_snap
        b = _lib.GridMergeBatch()
        b.n_pairs = R
        b.src, b.src_origin, b.src_index = slog.addr, src.origin.addr, (di.addr if di is not None else None)
        b.dst, b.dst_origin, b.xform = self.logodds.addr, self.origin.addr, dx.addr
        b.stats, b.flags = self._merge[0].addr, self._merge[1].addr
        _lib.call("lslam_grid_merge", ctx, b, self.p, q)
        if sync:
            ctx.sync()

    def merge_results(self):
        """The last ``merge``'s stats [R, 8] (cells on the source map, cells with a source value, supported,
        contradicted, new, known in both with equal sign, with opposite sign, changed) and flags [R]
        (``MERGE_*``)."""
        if self._merge is None:
            raise ValueError("no merge yet")
        return {"stats": self._merge[0].download(), "flags": self._merge[1].download()}

    def results(self):
        """logodds [R, W, W] int16 (row Y, 0.01 nat) and the last step's rot [R, 2], n_used [R, 2]
        (points traced, valid points beyond max_range), flags [R]."""
        return {"logodds": self.logodds.download(), "rot": self.rot.download(), "n_used": self.n_used.download(),
                "flags": self.flags.download()}

    def probability(self):
        """Occupancy probability [R, W, W] on the host: 1 - 1 / (1 + exp(L / 100))."""
        L = self.logodds.download().astype(np.float64)
        return 1.0 - 1.0 / (1.0 + np.exp(L / 100.0))

    def clear(self):
        """Zero every grid (unknown everywhere), on the stream."""
        self.logodds.fill_zero()

    def redraw(self, graph, sync=True):
        """Draw every grid again from a ``PoseGraph``'s keyframes: ``clear``, then one ``step`` per
        keyframe from the revolution stored with it at ``graph.node_pose(k)``, the corrected poses read on
        the device in stream order (after a ``graph.solve(sync=False)`` too).  Every keyframe is replayed,
        and only keyframes: what was drawn between them is gone.  A keyframe stored without a revolution
        is an error.  (Host revolutions are staged as ``step`` stages them.)"""
        if graph.G != self.R:
            raise ValueError("the graph holds %d robots, the grid %d" % (graph.G, self.R))
        revs = graph.revolutions[:graph.n]
        if any(r is None for r in revs):
            raise ValueError("a keyframe was stored without its revolution")
        self.clear()
        for k, rev in enumerate(revs):
            args = rev if isinstance(rev, (tuple, list)) else (rev,)
            self.step(*args, pose=graph.node_pose(k), sync=False)
        if sync:
            self.ctx.sync()

    def upload(self, logodds):
        """Replace the grids (tests, restarts): int16 [R, W, W]."""
        self.logodds.upload(np.ascontiguousarray(logodds, np.int16).reshape(self.R, self.W, self.W))


class GridRayCaster:
    """Reads ``grid`` beam by beam (``lslam_grid_raycast``): every beam of a revolution is walked
    from the pose through the robot's grid until the MAP says it stops (an occupied cell, an unknown
    one, or the range circle), and classed by where it actually returned: MATCH, NOVEL (a return in
    space the map holds free: a dynamic object), THROUGH (it passed a cell the map holds occupied:
    a stale map or a wrong pose), UNMAPPED.  ``params``: occ_min, free_max, tol
    (``lslam_raycast_params``; defaults 1, -1, 3 steps: L = 0 alone is unknown).  The grid's geometry and its device
    buffers are ``grid``'s, read in place::

        grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)
        rc.step(next_xy, scan_chunk_off, chunk_pt_off, pose=lm)   # before the next grid.step
        if rc.inconsistency().max() > 0.3: ...                    # the pose contradicts the map

    The definition is the comment on ``lslam_grid_raycast`` in include/lidarslam.h;
    tests/raycast_ref.py is its NumPy form and the kernel matches it bit for bit, given ``rot``."""

    def __init__(self, grid: OccupancyGrid, **params):
        self.grid, self.ctx, self.R = grid, grid.ctx, grid.R
        ctx, R = self.ctx, self.R
        self.p = _lib.raycast_params(**params)
        # (a range error of params surfaces here, before anything is allocated)
        _lib.call("lslam_grid_raycast", ctx, _lib.RaycastBatch(), grid.p, self.p)
        self.counts = ctx.empty((R, 8), np.int32)
        self.rot = ctx.empty((R, 2), np.float64)
        self.flags = ctx.empty(R, np.int32)
        for a in (self.counts, self.rot, self.flags):
            a.fill_zero()
        self._cls, self._stop = _Grow(ctx, np.uint8), _Grow(ctx, np.int32)
        self._stage = Staging(ctx, R)
        self._span = (0, 0)  # the last step's points in _cls and _stop: the first and the last point offset
        self.steps = 0

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, pose=None, sync=True, want_stop=True):
        """One revolution per robot, in the argument forms of ``OccupancyGrid.step``; ``pose`` [R, 3]:
        a host array, a float64 ``DeviceArray`` (``lm.x``) or a ``LandmarkMap``.  ``want_stop=False``
        leaves the stop cells out (``stop`` NULL): classes and counts only."""
        ctx, R, g = self.ctx, self.R, self.grid
        staging.require_pose(pose)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        dpose = self._stage.pose(pose, "grid")
        lo, P = int(self._stage.off_host[0]), int(self._stage.off_host[-1])
        b = _lib.RaycastBatch()
        b.n_robots = R
        b.xy, b.pt_off, b.pose, b.origin, b.logodds = dxy.addr, doff.addr, dpose.addr, g.origin.addr, g.logodds.addr
        b.cls = self._cls.reserve(P).addr
        b.stop = self._stop.reserve(3 * P).addr if want_stop else None
        b.counts, b.rot, b.flags = self.counts.addr, self.rot.addr, self.flags.addr
        _lib.call("lslam_grid_raycast", ctx, b, g.p, self.p)
        self._span, self._has_stop = (lo, P), bool(want_stop)  # (kept from the call that wrote them: a refused step leaves both)
        self.steps += 1
        if sync:
            ctx.sync()

    def _head(self, grow, lo, hi, width=1):
        """Items [lo, hi) x width of a grow-only buffer, on the host."""
        out = np.empty((hi - lo) * width, grow.dtype)
        if out.nbytes:
            src = C.c_void_p(grow.buf.addr + lo * width * grow.dtype.itemsize)
            _lib.call("lslam_d2h", self.ctx, out.ctypes.data_as(C.c_void_p), src, out.nbytes)
        self.ctx.sync()
        return out

    def results(self):
        """The last step's cls [P] (the class, 0..4), kind [P] (0 NONE, 1 UNKNOWN, 2 OCC), stop [P, 3]
        (ox, oy, i_h; None without ``want_stop``), counts [R, 8], rot [R, 2], flags [R]; P points in
        the order of the revolution, robot after robot."""
        if not self.steps:
            raise ValueError("no step yet")
        lo, hi = self._span
        raw = self._head(self._cls, lo, hi)
        stop = self._head(self._stop, lo, hi, 3).reshape(-1, 3) if self._has_stop else None
        return {"cls": raw & 15, "kind": raw >> 4, "stop": stop, "counts": self.counts.download(),
                "rot": self.rot.download(), "flags": self.flags.download()}

    def expected_range(self):
        """The range [P] (mm) at which the map expects every beam to return: cell * hypot(ox, oy) of the
        stop cell where the kind is OCC, inf elsewhere.  On the host."""
        r = self.results()
        if r["stop"] is None:
            raise ValueError("the last step left the stop cells out")
        st = r["stop"].astype(np.float64)
        return np.where(r["kind"] == _lib.RAYCAST_KIND_OCC, float(self.grid.p.cell) * np.hypot(st[:, 0], st[:, 1]), np.inf)

    def novel_mask(self):
        """bool [P]: the returns inside space the map holds free, the dynamic-object mask."""
        lo, hi = self._span
        return (self._head(self._cls, lo, hi) & 15) == _lib.RAYCAST_NOVEL

    def inconsistency(self):
        """Per robot, (NOVEL + THROUGH) / valid points that are not beyond (0 where there are none): the
        share of beams that contradict the map, the figure to gate a relocalisation on."""
        c = self.counts.download().astype(np.int64)
        den = c[:, 1:5].sum(1) - c[:, 5]
        return np.where(den > 0, (c[:, _lib.RAYCAST_NOVEL] + c[:, _lib.RAYCAST_THROUGH]) / np.maximum(den, 1), 0.0)


class DistanceField:
    """The exact distance field of ``grid`` (``lslam_grid_distance``): per cell the squared Euclidean
    distance, in cells, to the nearest source cell, saturated at ``d_max``^2; and its read under a
    revolution (``lslam_field_score``): how far the returns lie from the map's sources, and the robot's
    own clearance.  ``params``: mode (``DIST_OCC``: sources are the cells with L >= occ_min;
    ``DIST_NOT_FREE``: the cells with L > free_max and everything off the map), occ_min, free_max,
    d_max (``lslam_dist_params``; defaults OCC, 85, -1, 64 cells), trunc2, near2
    (``lslam_fieldscore_params``; defaults 625, 4); off2 is d_max^2; and trunc, damp_t, damp_r, eps_t,
    eps_r, max_shift, max_turn, n_iter, min_points, min_permille (``lslam_fieldalign_params``; defaults
    25 cells, 1, 100, 0.01 cell, 1e-4 rad, 200 mm, 0.1 rad, 10, 16, 500); and sigma_min, r_scale, floor_t,
    floor_r, nis_max (``lslam_fieldfuse_params``; defaults 0.5 cell, 1, 1 / sqrt(12) cell,
    (pi / 360) / sqrt(12) rad, 16.27).  The grid's geometry and its device buffers are ``grid``'s, read in
    place::

        grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)
        field.step()                                          # the field of the grid as it now stands
        field.score(xy, scan_chunk_off, chunk_pt_off, pose=lm)
        if field.clearance_mm().min() < 300.0: ...            # a robot is close to something

    and the tracker's loop, a few Gauss-Newton steps in the field from the filter's pose fused into the
    filter as a measurement (``lslam_field_fuse``), with the exhaustive search kept for the robots that
    lost track::

        grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)  # the map from the last revolution
        field.step()
        field.fuse(next_xy, scan_chunk_off, chunk_pt_off, lm=lm)  # a gated Kalman update of lm.x and lm.P in place
        lost = field.fuse_results()["flags"] & FIELDALIGN_REJECTED  # those robots kept their mean and covariance
        if lost.any():                                        # GridLocalizer: the 41 x 21 x 21 window
            loc.fuse(next_xy, scan_chunk_off, chunk_pt_off, grid=grid, lm=lm)

    (``field.align(.., pose=lm, pose_out=lm.x)`` is the same descent overwriting the mean alone.)

    The field is recomputed whole by every ``step``: there is no incremental update after a
    revolution.  After an ``OccupancyGrid.recentre`` the next ``step`` computes the moved grid's field
    and ``score`` reads the moved origin on the device.  The definitions are the comments on the two
    entry points in include/lidarslam.h; tests/dist_ref.py and tests/fieldscore_ref.py are their NumPy
    forms and the kernels match them bit for bit."""

    def __init__(self, grid: OccupancyGrid, **params):
        self.grid, self.ctx, self.R = grid, grid.ctx, grid.R
        ctx, R, W = self.ctx, self.R, grid.W
        dk = {k: int(params.pop(k)) for k in ("mode", "occ_min", "free_max", "d_max") if k in params}
        sk = {k: int(params.pop(k)) for k in ("trunc2", "near2") if k in params}
        ak = {k: float(params.pop(k)) for k in _ALIGN_DOUBLES if k in params}
        ak.update({k: int(params.pop(k)) for k in _ALIGN_INTS if k in params})
        fk = {k: float(params.pop(k)) for k in _FUSE_DOUBLES if k in params}
        if params:
            raise TypeError("unknown parameters: %s" % ", ".join(sorted(params)))
        self.p = _lib.dist_params(**dk)
        self.q = _lib.fieldscore_params(off2=min(int(self.p.d_max) ** 2, 65025), **sk)
        self.a = _lib.fieldalign_params(**ak)
        self.f = _lib.fieldfuse_params(**fk)
        # (a range error of params surfaces here, before anything large is allocated)
        _lib.call("lslam_grid_distance", ctx, _lib.DistBatch(), grid.p, self.p)
        _lib.call("lslam_field_score", ctx, _lib.FieldScoreBatch(), grid.p, self.q)
        _lib.call("lslam_field_align", ctx, _lib.FieldAlignBatch(), grid.p, self.a)
        _lib.call("lslam_field_fuse", ctx, _lib.FieldFuseBatch(), grid.p, self.a, self.f)
        self.d2 = ctx.empty((R, W, W), np.uint16)
        self.n_src = ctx.empty(R, np.int32)
        self.flags = ctx.empty(R, np.int32)
        self.rot = ctx.empty((R, 2), np.float64)
        self.stats = ctx.empty((R, 4), np.int64)
        self.clear2 = ctx.empty(R, np.int32)
        self.score_flags = ctx.empty(R, np.int32)
        for a in (self.n_src, self.flags, self.rot, self.stats, self.clear2, self.score_flags):
            a.fill_zero()
        self._stage = Staging(ctx, R)
        self.steps = self.scores = self.aligns = 0
        self._align = None  # align's outputs, allocated by its first call
        self._fuse = None   # fuse's own, likewise
        self._fused = False  # the last align or fuse was a fuse

    def step(self, sync=True):
        """The field of the grid's device buffer as it now stands."""
        ctx, g = self.ctx, self.grid
        b = _lib.DistBatch()
        b.n_robots = self.R
        b.logodds, b.d2, b.n_src, b.flags = g.logodds.addr, self.d2.addr, self.n_src.addr, self.flags.addr
        _lib.call("lslam_grid_distance", ctx, b, g.p, self.p)
        self.steps += 1
        if sync:
            ctx.sync()

    def score(self, xy, scan_chunk_off=None, chunk_pt_off=None, pose=None, sync=True):
        """One revolution per robot read in the field of the last ``step``, in the argument forms of
        ``OccupancyGrid.step``; ``pose`` [R, 3]: a host array, a float64 ``DeviceArray`` (``lm.x``) or a
        ``LandmarkMap``."""
        if not self.steps:
            raise ValueError("no step yet: the field has not been computed")
        ctx, g = self.ctx, self.grid
        staging.require_pose(pose)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        dpose = self._stage.pose(pose, "grid")
        b = _lib.FieldScoreBatch()
        b.n_robots = self.R
        b.xy, b.pt_off, b.pose, b.origin, b.d2 = dxy.addr, doff.addr, dpose.addr, g.origin.addr, self.d2.addr
        b.rot, b.stats, b.clear2, b.flags = self.rot.addr, self.stats.addr, self.clear2.addr, self.score_flags.addr
        _lib.call("lslam_field_score", ctx, b, g.p, self.q)
        self.scores += 1
        if sync:
            ctx.sync()

    def align(self, xy, scan_chunk_off=None, chunk_pt_off=None, pose=None, pose_out=None, sync=True):
        """One revolution per robot aligned in the field of the last ``step`` (``lslam_field_align``): at
        most ``n_iter`` damped Gauss-Newton steps from ``pose``, in one launch.  The argument forms are
        those of ``score``.  ``pose_out``: a float64 ``DeviceArray`` [R, 3] that receives the aligned
        pose, or the guess bit for bit where the flags reject it (``FIELDALIGN_REJECTED``); it may be
        the array ``pose`` is read from, e.g. the filter's ``lm.x``.  None: a buffer of the field's own."""
        if not self.steps:
            raise ValueError("no step yet: the field has not been computed")
        ctx, g, R = self.ctx, self.grid, self.R
        o = self._align_buffers()
        if pose_out is None:
            pose_out = o["pose_out"]
        if not isinstance(pose_out, DeviceArray) or pose_out.dtype != np.float64 or pose_out.nbytes < 24 * R:
            raise ValueError("pose_out must be a float64 DeviceArray [n_robots, 3]")
        staging.require_pose(pose)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        dpose = self._stage.pose(pose, "grid")
        b = _lib.FieldAlignBatch()
        b.n_robots = R
        b.xy, b.pt_off, b.pose, b.origin, b.d2 = dxy.addr, doff.addr, dpose.addr, g.origin.addr, self.d2.addr
        b.pose_out, b.trace, b.normal = pose_out.addr, o["trace"].addr, o["normal"].addr
        b.n_used, b.iters, b.flags = o["n_used"].addr, o["iters"].addr, o["flags"].addr
        _lib.call("lslam_field_align", ctx, b, g.p, self.a)
        self._align_out, self._align_rows, self._fused = pose_out, int(self.a.n_iter) + 1, False
        self.aligns += 1
        if sync:
            ctx.sync()

    def _align_buffers(self):
        ctx, R = self.ctx, self.R
        if self._align is None:
            rows = 33  # n_iter's upper end + 1: self.a.n_iter may change between calls
            self._align = dict(pose_out=ctx.empty((R, 3), np.float64), trace=ctx.empty((R, rows, 5), np.float64),
                               normal=ctx.empty((R, 10), np.int64), n_used=ctx.empty((R, 3), np.int32),
                               iters=ctx.empty(R, np.int32), flags=ctx.empty(R, np.int32))
        return self._align

    def fuse(self, xy, scan_chunk_off=None, chunk_pt_off=None, lm=None, x=None, P=None, write_back=True, sync=True):
        """The alignment of ``align`` fused into a filter (``lslam_field_fuse``): ``lm`` (a ``LandmarkMap``:
        its ``x`` and ``P``), or ``x`` [R, 3] and ``P`` [R, 9] as float64 ``DeviceArray``s, in the argument
        forms of ``GridLocalizer.fuse``.  The mean is the descent's guess; the aligned pose is a
        measurement of it whose information comes from the alignment's own normal equations, and the
        update is gated on the filter's uncertainty.  With ``write_back`` (the default) the updated mean
        and covariance are written over them in place; otherwise they go to buffers of this object's,
        and the filter is only read.  A robot with one of ``FIELDFUSE_REJECTED`` keeps the bits of its
        mean and covariance."""
        if not self.steps:
            raise ValueError("no step yet: the field has not been computed")
        ctx, g, R = self.ctx, self.grid, self.R
        x, P = staging.filter_arguments(lm, x, P, R, "grid")
        o = self._align_buffers()
        if self._fuse is None:
            self._fuse = dict(P=ctx.empty((R, 9), np.float64), z=ctx.empty((R, 3), np.float64),
                              info=ctx.empty((R, 9), np.float64), info_f=ctx.empty((R, 9), np.float64),
                              s2=ctx.empty(R, np.float64), nis=ctx.empty(R, np.float64))
        fo = self._fuse
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        pose_out, P_out = (x, P) if write_back else (o["pose_out"], fo["P"])
        b = _lib.FieldFuseBatch()
        b.a.n_robots = R
        b.a.xy, b.a.pt_off, b.a.pose, b.a.origin, b.a.d2 = dxy.addr, doff.addr, x.addr, g.origin.addr, self.d2.addr
        b.a.pose_out, b.a.trace, b.a.normal = pose_out.addr, o["trace"].addr, o["normal"].addr
        b.a.n_used, b.a.iters, b.a.flags = o["n_used"].addr, o["iters"].addr, o["flags"].addr
        b.P, b.P_out, b.z = P.addr, P_out.addr, fo["z"].addr
        b.info, b.info_f, b.s2, b.nis = fo["info"].addr, fo["info_f"].addr, fo["s2"].addr, fo["nis"].addr
        _lib.call("lslam_field_fuse", ctx, b, g.p, self.a, self.f)
        self._align_out, self._align_rows, self._fused, self._P_out = pose_out, int(self.a.n_iter) + 1, True, P_out
        self.aligns += 1
        if sync:
            ctx.sync()

    def fuse_results(self):
        """The last fuse's ``align_results`` (pose_out is the UPDATED mean) plus z [R, 3] (the aligned pose),
        info and info_f [R, 3, 3] (the alignment's information in mm and rad, plain and floored), s2 [R]
        (the noise variance, squared cells), nis [R] and P_out [R, 3, 3]; flags carry ``FIELDFUSE_*``."""
        if not self._fused:
            raise ValueError("no fuse yet")
        out, fo, R = self.align_results(), self._fuse, self.R
        out["z"], out["s2"], out["nis"] = fo["z"].download(), fo["s2"].download(), fo["nis"].download()
        out["info"], out["info_f"] = fo["info"].download().reshape(R, 3, 3), fo["info_f"].download().reshape(R, 3, 3)
        out["P_out"] = self._P_out.download().reshape(-1)[:9 * R].reshape(R, 3, 3)
        return out

    def align_results(self):
        """The last align's pose_out [R, 3], trace [R, n_iter + 1, 5] (px, py, theta, cos, sin of every
        evaluation, zeros beyond the last), normal [R, 10] int64 (the last evaluation's J^T J, J^T r and
        r^2, times 2^20), n_used [R, 3] (points used at the first and at the last evaluation, valid
        points in range), iters [R], flags [R] (``FIELDALIGN_*``)."""
        if not self.aligns:
            raise ValueError("no align yet")
        o, E = self._align, self._align_rows
        trace = o["trace"].download().reshape(-1)[:self.R * E * 5].reshape(self.R, E, 5)
        return {"pose_out": self._align_out.download().reshape(-1)[:3 * self.R].reshape(self.R, 3), "trace": trace,
                "normal": o["normal"].download(), "n_used": o["n_used"].download(), "iters": o["iters"].download(),
                "flags": o["flags"].download()}

    def align_information(self):
        """The last align's Gauss-Newton information matrix H [R, 3, 3] = J^T J and vector g [R, 3] =
        J^T r at its last evaluation, as float64 in cells and rad (without the damping): inv(H) times
        the residual variance is the natural covariance of pose_out; ``fuse`` is the call that fuses it."""
        if not self.aligns:
            raise ValueError("no align yet")
        n = self._align["normal"].download().astype(np.float64) / float(2 ** 20)
        H = np.empty((self.R, 3, 3))
        for (i, j), k in {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}.items():
            H[:, i, j] = H[:, j, i] = n[:, k]
        return H, n[:, 6:9].copy()

    def results(self):
        """The last step's d2 [R, W, W] uint16, n_src [R], flags [R] (``DIST_EMPTY``)."""
        if not self.steps:
            raise ValueError("no step yet")
        return {"d2": self.d2.download(), "n_src": self.n_src.download(), "flags": self.flags.download()}

    def score_results(self):
        """The last score's stats [R, 4] int64 (sum of min(v, trunc2), points scored, near points,
        points off the map), clear2 [R], rot [R, 2], flags [R] (``FIELD_BAD_POSE``)."""
        if not self.scores:
            raise ValueError("no score yet")
        return {"stats": self.stats.download(), "clear2": self.clear2.download(), "rot": self.rot.download(),
                "flags": self.score_flags.download()}

    def clearance_mm(self):
        """Per robot, cell * sqrt(clear2): the distance from the robot cell of the last ``score`` to the
        nearest source, saturated at cell * d_max (0 for a bad pose)."""
        return float(self.grid.p.cell) * np.sqrt(self.clear2.download().astype(np.float64))

    def near_share(self):
        """Per robot, near points / points scored (0 where there are none)."""
        s = self.stats.download()
        return np.where(s[:, 1] > 0, s[:, 2] / np.maximum(s[:, 1], 1), 0.0)

    def mean_d2(self):
        """Per robot, the mean of min(v, trunc2) over the points scored (0 where there are none): the
        beam-end-point score, in squared cells."""
        s = self.stats.download()
        return np.where(s[:, 1] > 0, s[:, 0] / np.maximum(s[:, 1], 1), 0.0)


class GridScan:
    """``grid``'s maps as revolutions (``lslam_grid_points``): per robot the occupied cells (L >= ``occ_min``)
    within ``radius`` of an anchor pose, as points in that pose's frame, on the device.  It is what a
    stored map, a ``world()`` canvas or the map of a robot that has gone offers where a revolution is asked
    for::

        scan = GridScan(other_grid)
        scan.step()                                            # anchors: the grids' centres, heading 0
        reloc.relocalize(scan.input, grid=grid)                # where those anchors lie in ``grid``
        xform = merge_transform(reloc.results()["pose"], scan.anchor_pose)
        grid.merge(other_grid, xform)                          # (``align_maps`` is these four lines)

    ``cap``: slots per robot (1..65536); a robot with more cells in range keeps every stride-th in
    row-major order (``GRIDPOINTS_DECIMATED``; not uniform in space).  ``radius`` (mm) defaults to the
    grid's ``max_range``; a larger one is refused, since the matchers drop points beyond it.  A map seen as
    a scan has no occlusion and a thick wall weighs more than a thin one.  The grid's device buffers are
    read in place, and nothing of them comes to the host."""

    def __init__(self, grid: OccupancyGrid, cap=1024, radius=None, occ_min=85):
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("grid must be an OccupancyGrid (or a world() view)")
        self.grid, self.ctx, self.R = grid, grid.ctx, grid.R
        ctx, R = self.ctx, self.R
        radius = float(grid.p.max_range) if radius is None else float(radius)
        if radius > float(grid.p.max_range):
            raise ValueError("radius %r is beyond the grid's max_range %r: the matchers drop those points" % (radius, float(grid.p.max_range)))
        self.p = _lib.gridpoints_params(radius=radius, occ_min=int(occ_min), cap=int(cap))
        # (a range error of params surfaces here, before anything is allocated)
        _lib.call("lslam_grid_points", ctx, _lib.GridPointsBatch(), grid.p, self.p)
        cap = self.cap = int(self.p.cap)
        if R * cap >= 2 ** 31:
            raise ValueError("n_robots * cap must be below 2^31")
        self.xy = ctx.empty((R * cap, 2), np.float64)
        self.pt_off = ctx.empty(R + 1, np.int32)
        self.counts = ctx.empty((R, 4), np.int32)
        self.flags = ctx.empty(R, np.int32)
        self._bands = ctx.empty((R, _lib.GRIDPOINTS_BANDS, 2), np.int32)  # the count pass's scratch
        self._stage = Staging(ctx, R, pose=False)
        self.input = staging.MapInput()
        self.input.xy = self.xy
        self.input.sco = np.arange(R + 1, dtype=np.int64)
        self.input.cpo = np.arange(R + 1, dtype=np.int64) * cap
        self.anchor_pose = None  # host [R, 3] of the last step, None after a step with a device anchor
        self.steps = 0

    def step(self, anchor=None, sync=True):
        """The points of the grids as they now stand.  ``anchor``: host poses [R, 3] (x, y, theta) in each
        map's world frame, or one pose for all, from which (ax, ay, cos theta, sin theta) are made on the
        host in NumPy; or a float64 ``DeviceArray`` [R, 4] of (ax, ay, c, s), used in place; default: each
        grid's centre with theta = 0 (which reads ``origin_host``: after a ``recentre`` that waits for the
        stream)."""
        ctx, R, g = self.ctx, self.R, self.grid
        if isinstance(anchor, DeviceArray):
            self.anchor_pose = None
            da = self._stage.per_robot("anchor", anchor, 4, np.float64, "anchor")
        else:
            if anchor is None:
                pose = np.concatenate([g.origin_host + 0.5 * g.W * float(g.p.cell), np.zeros((R, 1))], 1)
            else:
                pose = np.asarray(anchor, np.float64)
                if pose.size not in (3, 3 * R):
                    raise ValueError("anchor must hold 3 values (x, y, theta), or n_robots x 3")
                pose = np.broadcast_to(pose.reshape(-1, 3), (R, 3))
            self.anchor_pose = np.array(pose, np.float64)
            p = self.anchor_pose
            da = self._stage.per_robot("anchor", np.stack([p[:, 0], p[:, 1], np.cos(p[:, 2]), np.sin(p[:, 2])], -1), 4,
                                       np.float64, "anchor")
        b = _lib.GridPointsBatch()
        b.n_robots = R
        b.logodds, b.origin, b.anchor = g.logodds.addr, g.origin.addr, da.addr
        b.xy, b.pt_off, b.counts, b.flags = self.xy.addr, self.pt_off.addr, self.counts.addr, self.flags.addr
        b.band_counts = self._bands.addr
        _lib.call("lslam_grid_points", ctx, b, g.p, self.p)
        self.steps += 1
        if sync:
            ctx.sync()

    def results(self):
        """The last step's xy [R, cap, 2] (robot r's points are the first ``counts[r, 3]``, zeros behind
        them), counts [R, 4] (occupied cells, those in range, stride, points) and flags [R]
        (``GRIDPOINTS_*``)."""
        if not self.steps:
            raise ValueError("no step yet")
        return {"xy": self.xy.download().reshape(self.R, self.cap, 2), "counts": self.counts.download(),
                "flags": self.flags.download()}


def align_maps(dst, src, relocalizer, scan=None, anchor=None, **reloc_kw):
    """The transform that ``dst.merge(src, xform)`` needs, found from the two maps alone: ``scan`` (a
    ``GridScan`` of ``src``, made with its defaults if None) is stepped at ``anchor`` (host poses, as
    ``GridScan.step``; default: the centres of ``src``'s grids), ``relocalizer`` (a ``GridRelocalizer`` of as
    many robots) finds every anchor in ``dst``'s map m (``relocalize(scan.input, grid=dst, **reloc_kw)``:
    ``field=`` and ``window=`` pass through), and ``merge_transform`` makes xform from the found pose and the
    anchor's, on the host (24 bytes a robot; the call synchronises).

    Returns xform [R, 4], pose [R, 3] (the anchors in ``dst``'s frames), flags [R] (the relocaliser's
    ``RELOC_*``) and counts [R, 4] (``GridScan.results``).  A LOST or AMBIGUOUS pair has a NaN pose and
    hence a NaN transform, which ``dst.merge`` answers with ``MERGE_BAD_XFORM`` and leaves that destination
    bit for bit: that is the one mechanism, nothing is filtered here.  The relocaliser's ``min_permille``
    asks that share of the source's walls within the scan's radius to exist in ``dst``: for maps that
    overlap less, lower it, or move the anchor and shrink the radius to the shared part."""
    if not isinstance(dst, OccupancyGrid) or not isinstance(src, OccupancyGrid):
        raise ValueError("dst and src must be OccupancyGrids (or world() views)")
    if not (src.R == dst.R == relocalizer.R):
        raise ValueError("src holds %d robots, dst %d, the relocalizer %d" % (src.R, dst.R, relocalizer.R))
    if float(src.p.cell) != float(dst.p.cell):
        raise ValueError("src has cell %r, dst %r: aligning needs the same cell" % (float(src.p.cell), float(dst.p.cell)))
    if scan is None:
        scan = GridScan(src)
    elif not isinstance(scan, GridScan) or scan.grid is not src:
        raise ValueError("scan must be a GridScan of src")
    if isinstance(anchor, DeviceArray):
        raise ValueError("align_maps needs the anchor on the host: merge_transform reads it there")
    scan.step(anchor, sync=False)
    relocalizer.relocalize(scan.input, grid=dst, sync=True, **reloc_kw)
    res = relocalizer.results()
    return {"xform": merge_transform(res["pose"], scan.anchor_pose), "pose": res["pose"], "flags": res["flags"],
            "counts": scan.counts.download()}
