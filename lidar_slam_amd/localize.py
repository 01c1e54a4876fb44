"""Localisation in the occupancy grid: batched scan-to-map matching (``lslam_map_match``).

``OccupancyGrid`` is written from the filter's poses; ``GridLocalizer`` reads it back.  It takes one
revolution per robot, a pose guess and the robot's log-odds grid, searches a window of rotations and
whole-cell translations around the guess for the pose that lays the most points onto occupied
cells, and returns that pose -- or the guess itself where the overlay is too poor to trust
(``MAPMATCH_WEAK``).  It is the absolute correction that needs no straight walls, and the way back
for a filter whose pose is off: a bad start pose, a run of ``MATCH_EDGE`` odometry, a restart with a
stored grid.

``step`` with ``write_back=True`` overwrites the filter's mean with the corrected pose and leaves its
covariance alone.  ``fuse`` (``lslam_map_fuse``) makes the correction a measurement update instead:
the match becomes a measurement of the pose with a covariance taken from the whole score volume
(wide along a corridor's walls, one search quantum across them), and the filter's mean and
covariance are updated by a Kalman step on the device, gated on the innovation's Mahalanobis
distance (``MAPFUSE_OUTLIER``).  So packets -> revolutions -> odometry -> filter -> localise -> grid
never leave HBM::

    odo.step(xy, scan_chunk_off, chunk_pt_off, lm)             # writes lm.u
    lm.step(xy, scan_chunk_off, chunk_pt_off)                  # writes lm.x, lm.P
    loc.fuse(xy, scan_chunk_off, chunk_pt_off, grid=grid, lm=lm)   # updates lm.x, lm.P
    grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)       # maps from the updated pose

The grid was drawn from the filter's own poses, so the match is not independent of the prior;
``r_scale`` (a factor on the match covariance) is the knob for that.

The definitions are the comments on ``lslam_map_match`` and ``lslam_map_fuse`` in
include/lidarslam.h; tests/mapmatch_ref.py and tests/mapfuse_ref.py are their NumPy forms and the
kernels match them bit for bit, given the (cos, sin) that the library wrote to ``rot0``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import Context, DeviceArray
from .mapping import OccupancyGrid
from .odometry import _Grow, rot_table
from .slam import LandmarkMap, MapInput

MAPMATCH_EMPTY, MAPMATCH_EDGE = _lib.MAPMATCH_EMPTY, _lib.MAPMATCH_EDGE
MAPMATCH_BAD_POSE, MAPMATCH_WEAK = _lib.MAPMATCH_BAD_POSE, _lib.MAPMATCH_WEAK
MAPFUSE_OUTLIER, MAPFUSE_BAD_COV = _lib.MAPFUSE_OUTLIER, _lib.MAPFUSE_BAD_COV

_FUSE_KEYS = ("r_scale", "nis_max", "cut_permille")


class GridLocalizer:
    """R robots per call on one GPU.  ``params``: theta_step, win_w, smear, k_trans, k_theta, occ_min,
    min_permille (``lslam_mapmatch_params``; defaults pi/360, 512, 2, 10, 20, 85, 500), and for
    ``fuse`` r_scale, nis_max, cut_permille (``lslam_mapfuse_params``; defaults 1.0, 16.27, 900).
    The cell size and the map's width are the grid's, given with each step."""

    def __init__(self, ctx: Context, n_robots: int, **params):
        R = int(n_robots)
        if R <= 0:
            raise ValueError("n_robots must be > 0")
        self.ctx, self.R = ctx, R
        self.fp = _lib.mapfuse_params(**{k: params.pop(k) for k in _FUSE_KEYS if k in params})
        self.p = _lib.mapmatch_params(**params)
        # (a range error of params surfaces here, from the first call)
        _lib.check(_lib.load().lslam_map_match(ctx.handle, C.byref(_lib.MapMatchBatch()), C.byref(_lib.grid_params()),
                                               C.byref(self.p)), "lslam_map_match")
        _lib.check(_lib.load().lslam_map_fuse(ctx.handle, C.byref(_lib.MapFuseBatch()), C.byref(_lib.grid_params()),
                                              C.byref(self.p), C.byref(self.fp)), "lslam_map_fuse")
        self.Nt, self.Nth = 2 * self.p.k_trans + 1, 2 * self.p.k_theta + 1
        self.rot_host = rot_table(self.p.k_theta, self.p.theta_step)
        self.rot = ctx.to_device(self.rot_host)
        self.pose = ctx.empty((R, 3), np.float64)  # pose_out, unless a step writes back
        self.delta = ctx.empty((R, 3), np.float64)
        self.best = ctx.empty((R, 4), np.int32)
        self.n_valid = ctx.empty((R, 2), np.int32)
        self.rot0 = ctx.empty((R, 2), np.float64)
        self.flags = ctx.empty(R, np.int32)
        for a in (self.pose, self.delta, self.best, self.n_valid, self.rot0, self.flags):
            a.fill_zero()
        self.scores = None
        self._xy = _Grow(ctx, np.float64)
        self._off = ctx.empty(R + 1, np.int32)
        self._guess = ctx.empty((R, 3), np.float64)
        self._have_scores = False
        self._out = self.pose
        self._fused = None  # fuse's buffers (P, z, Rm, nis, moments), made by the first fuse
        self._P_out = None
        self.steps = 0

    def _revolutions(self, xy, scan_chunk_off, chunk_pt_off, grid):
        """The checks of a step's revolutions and grid: (device xy, point offsets per robot)."""
        R = self.R
        if isinstance(xy, MapInput):
            xy, scan_chunk_off, chunk_pt_off = xy.xy, xy.sco, xy.cpo
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("grid is required (an OccupancyGrid)")
        if grid.R != R:
            raise ValueError("the grid holds %d robots, the localizer %d" % (grid.R, R))
        sco = np.ascontiguousarray(scan_chunk_off, np.int64).reshape(-1)
        cpo = np.ascontiguousarray(chunk_pt_off, np.int64).reshape(-1)
        if sco.size != R + 1:
            raise ValueError("one revolution per robot: scan_chunk_off needs n_robots + 1 entries")
        off = cpo[sco]
        p0, p1 = int(off[0]), int(off[-1])
        if p0 < 0 or np.any(np.diff(off) < 0) or p1 >= 2 ** 31:
            raise ValueError("inconsistent CSR offsets")
        if isinstance(xy, DeviceArray):
            if xy.dtype != np.float64 or xy.nbytes < 16 * p1:
                raise ValueError("device xy must be float64 [n, 2] with n >= the last point offset")
            dxy = xy
        else:
            h = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
            if h.shape[0] < p1:
                raise ValueError("xy holds fewer points than chunk_pt_off describes")
            dxy = self._xy.put_host(h[p0:p1])
            off = off - p0
        return dxy, off

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, grid=None, pose=None, write_back=False,
             want_scores=False, sync=True):
        """One revolution per robot, in the CSR layout of ``OccupancyGrid.step`` (host array,
        ``DeviceArray`` or a ``MapInput``; device points are read in place).  ``grid``: the
        ``OccupancyGrid`` to localise in (its logodds, origin and parameters).  ``pose`` [R, 3]
        (x, y, theta), the guess: a host array, a float64 ``DeviceArray`` or a ``LandmarkMap``
        (its ``x``).  ``write_back``: with a device pose, the result is written over it (a robot
        whose match is EMPTY, WEAK or BAD_POSE keeps its bits); otherwise it goes to ``self.pose``."""
        R = self.R
        if pose is None and isinstance(grid, OccupancyGrid) and grid.R == R:  # (the grid's errors come first)
            raise ValueError("pose is required (host [R, 3], a DeviceArray or a LandmarkMap)")
        dxy, off = self._revolutions(xy, scan_chunk_off, chunk_pt_off, grid)
        if isinstance(pose, LandmarkMap):
            if pose.R != R:
                raise ValueError("the map holds %d robots, the localizer %d" % (pose.R, R))
            pose = pose.x
        if isinstance(pose, DeviceArray):
            if pose.dtype != np.float64 or pose.nbytes < 24 * R:
                raise ValueError("device pose must be float64 [n_robots, 3]")
            dpose = pose
        else:
            if write_back:
                raise ValueError("write_back needs a device pose (a DeviceArray or a LandmarkMap)")
            hp = np.ascontiguousarray(pose, np.float64)
            if hp.size != 3 * R:
                raise ValueError("pose must hold n_robots x 3 values")
            dpose = self._guess
            dpose.upload_async(hp.reshape(R, 3))
        dout = dpose if write_back else self.pose
        b = _lib.MapMatchBatch()
        self._fill(b, dxy, off, dpose, dout, grid, want_scores)
        self._P_out = None
        _lib.check(_lib.load().lslam_map_match(self.ctx.handle, C.byref(b), C.byref(grid.p), C.byref(self.p)),
                   "lslam_map_match")
        self.steps += 1
        if sync:
            self.ctx.sync()

    def _fill(self, b, dxy, off, dpose, dout, grid, want_scores):
        """The fields of a ``MapMatchBatch`` for one call."""
        R = self.R
        doff = self._off
        doff.upload_async(np.ascontiguousarray(off, np.int32))
        b.n_robots = R
        b.xy, b.pt_off, b.pose, b.origin = dxy.addr, doff.addr, dpose.addr, grid.origin.addr
        b.logodds, b.rot = grid.logodds.addr, self.rot.addr
        b.pose_out, b.delta, b.best = dout.addr, self.delta.addr, self.best.addr
        b.n_valid, b.rot0, b.flags = self.n_valid.addr, self.rot0.addr, self.flags.addr
        if want_scores:
            if self.scores is None:
                self.scores = self.ctx.empty((R, self.Nth, self.Nt, self.Nt), np.int32)
            b.scores = self.scores.addr
        self._have_scores = bool(want_scores)
        self._out = dout

    def fuse(self, xy, scan_chunk_off=None, chunk_pt_off=None, grid=None, lm=None, x=None, P=None, write_back=True,
             want_scores=False, sync=True):
        """The match of ``step`` fused into a filter: ``lm`` (a ``LandmarkMap``: its ``x`` and ``P``), or
        ``x`` [R, 3] and ``P`` [R, 9] as float64 ``DeviceArray``s.  The mean is the search's guess.
        With ``write_back`` (the default) the updated mean and covariance are written over them in
        place; otherwise they go to ``self.pose`` and a buffer of this object's, and the filter is
        only read.  A robot whose match is EMPTY, WEAK, BAD_POSE, OUTLIER or BAD_COV keeps the bits
        of its mean and covariance."""
        ctx, R = self.ctx, self.R
        if lm is not None:
            if x is not None or P is not None:
                raise ValueError("give lm, or x and P")
            if not isinstance(lm, LandmarkMap):
                raise ValueError("lm must be a LandmarkMap")
            if lm.R != R:
                raise ValueError("the map holds %d robots, the localizer %d" % (lm.R, R))
            x, P = lm.x, lm.P
        if not isinstance(x, DeviceArray) or not isinstance(P, DeviceArray):
            raise ValueError("fuse needs the filter on the device: lm (a LandmarkMap), or x and P (DeviceArrays)")
        if x.dtype != np.float64 or x.nbytes < 24 * R:
            raise ValueError("device x must be float64 [n_robots, 3]")
        if P.dtype != np.float64 or P.nbytes < 72 * R:
            raise ValueError("device P must be float64 [n_robots, 9]")
        dxy, off = self._revolutions(xy, scan_chunk_off, chunk_pt_off, grid)
        if self._fused is None:
            self._fused = {"P": ctx.empty((R, 9), np.float64), "z": ctx.empty((R, 3), np.float64),
                           "Rm": ctx.empty((R, 9), np.float64), "nis": ctx.empty(R, np.float64),
                           "moments": ctx.empty((R, 10), np.int64)}
            for a in self._fused.values():
                a.fill_zero()
        fb = self._fused
        b = _lib.MapFuseBatch()
        self._fill(b.m, dxy, off, x, x if write_back else self.pose, grid, want_scores)
        self._P_out = P if write_back else fb["P"]
        b.P, b.P_out = P.addr, self._P_out.addr
        b.z, b.Rm, b.nis, b.moments = fb["z"].addr, fb["Rm"].addr, fb["nis"].addr, fb["moments"].addr
        _lib.check(_lib.load().lslam_map_fuse(ctx.handle, C.byref(b), C.byref(grid.p), C.byref(self.p), C.byref(self.fp)),
                   "lslam_map_fuse")
        self.steps += 1
        if sync:
            ctx.sync()

    def results(self):
        """The last step's pose [R, 3] (the corrected pose, or the guess where the match was not
        accepted), delta [R, 3] (world frame: dx, dy, dtheta), best [R, 4] (k, jy, jx, score),
        n_valid [R, 2] (occupied cells in the window, valid points), rot0 [R, 2], flags [R], plus
        scores [R, Ntheta, Nt, Nt] when asked for.  After a ``fuse``: pose is the updated mean, and
        P [R, 3, 3] the updated covariance, z [R, 3] the match as a measurement, Rm [R, 3, 3] its
        covariance, nis [R] and moments [R, 10] (int64) come with it."""
        out = {"pose": self._out.download().reshape(-1, 3)[:self.R], "delta": self.delta.download(),
               "best": self.best.download(), "n_valid": self.n_valid.download(), "rot0": self.rot0.download(),
               "flags": self.flags.download()}
        if self._have_scores:
            out["scores"] = self.scores.download()
        if self._P_out is not None:  # the last call was a fuse
            out["P"] = self._P_out.download().reshape(-1, 3, 3)[:self.R]
            out["z"], out["nis"] = self._fused["z"].download(), self._fused["nis"].download()
            out["Rm"] = self._fused["Rm"].download().reshape(-1, 3, 3)
            out["moments"] = self._fused["moments"].download()
        return out
