"""Localisation in the occupancy grid: batched scan-to-map matching (``lslam_map_match``).

``OccupancyGrid`` is written from the filter's poses; ``GridLocalizer`` reads it back.  It takes one
revolution per robot, a pose guess and the robot's log-odds grid, searches a window of rotations and
whole-cell translations around the guess for the pose that lays the most points onto occupied
cells, and returns that pose -- or the guess itself where the overlay is too poor to trust
(``MAPMATCH_WEAK``).  It is the absolute correction that needs no straight walls, and the way back
for a filter whose pose is off: a bad start pose, a run of ``MATCH_EDGE`` odometry, a restart with a
stored grid.  With ``write_back=True`` the corrected pose replaces the filter's on the device, so
packets -> revolutions -> odometry -> filter -> localise -> grid never leave HBM::

    odo.step(xy, scan_chunk_off, chunk_pt_off, lm)                               # writes lm.u
    lm.step(xy, scan_chunk_off, chunk_pt_off)                                    # writes lm.x
    loc.step(xy, scan_chunk_off, chunk_pt_off, grid=grid, pose=lm, write_back=True)  # corrects lm.x
    grid.step(xy, scan_chunk_off, chunk_pt_off, pose=lm)                         # maps from the corrected pose

The definition (robot cell, look-up window, scores, winner, gate, output pose) is the comment on
``lslam_map_match`` in include/lidarslam.h; tests/mapmatch_ref.py is its NumPy form and the kernels
match it bit for bit, given the (cos, sin) that the library wrote to ``rot0``.
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


class GridLocalizer:
    """R robots per call on one GPU.  ``params``: theta_step, win_w, smear, k_trans, k_theta, occ_min,
    min_permille (``lslam_mapmatch_params``; defaults pi/360, 512, 2, 10, 20, 85, 500).  The cell
    size and the map's width are the grid's, given with each step."""

    def __init__(self, ctx: Context, n_robots: int, **params):
        R = int(n_robots)
        if R <= 0:
            raise ValueError("n_robots must be > 0")
        self.ctx, self.R = ctx, R
        self.p = _lib.mapmatch_params(**params)
        # (a range error of params surfaces here, from the first call)
        _lib.check(_lib.load().lslam_map_match(ctx.handle, C.byref(_lib.MapMatchBatch()), C.byref(_lib.grid_params()),
                                               C.byref(self.p)), "lslam_map_match")
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
        self.steps = 0

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, grid=None, pose=None, write_back=False,
             want_scores=False, sync=True):
        """One revolution per robot, in the CSR layout of ``OccupancyGrid.step`` (host array,
        ``DeviceArray`` or a ``MapInput``; device points are read in place).  ``grid``: the
        ``OccupancyGrid`` to localise in (its logodds, origin and parameters).  ``pose`` [R, 3]
        (x, y, theta), the guess: a host array, a float64 ``DeviceArray`` or a ``LandmarkMap``
        (its ``x``).  ``write_back``: with a device pose, the result is written over it (a robot
        whose match is EMPTY, WEAK or BAD_POSE keeps its bits); otherwise it goes to ``self.pose``."""
        ctx, R = self.ctx, self.R
        if isinstance(xy, MapInput):
            xy, scan_chunk_off, chunk_pt_off = xy.xy, xy.sco, xy.cpo
        if not isinstance(grid, OccupancyGrid):
            raise ValueError("grid is required (an OccupancyGrid)")
        if grid.R != R:
            raise ValueError("the grid holds %d robots, the localizer %d" % (grid.R, R))
        if pose is None:
            raise ValueError("pose is required (host [R, 3], a DeviceArray or a LandmarkMap)")
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
        doff = self._off
        doff.upload_async(np.ascontiguousarray(off, np.int32))
        b = _lib.MapMatchBatch()
        b.n_robots = R
        b.xy, b.pt_off, b.pose, b.origin = dxy.addr, doff.addr, dpose.addr, grid.origin.addr
        b.logodds, b.rot = grid.logodds.addr, self.rot.addr
        b.pose_out, b.delta, b.best = dout.addr, self.delta.addr, self.best.addr
        b.n_valid, b.rot0, b.flags = self.n_valid.addr, self.rot0.addr, self.flags.addr
        if want_scores:
            if self.scores is None:
                self.scores = ctx.empty((R, self.Nth, self.Nt, self.Nt), np.int32)
            b.scores = self.scores.addr
        self._have_scores = bool(want_scores)
        self._out = dout
        _lib.check(_lib.load().lslam_map_match(ctx.handle, C.byref(b), C.byref(grid.p), C.byref(self.p)),
                   "lslam_map_match")
        self.steps += 1
        if sync:
            ctx.sync()

    def results(self):
        """The last step's pose [R, 3] (the corrected pose, or the guess where the match was not
        accepted), delta [R, 3] (world frame: dx, dy, dtheta), best [R, 4] (k, jy, jx, score),
        n_valid [R, 2] (occupied cells in the window, valid points), rot0 [R, 2], flags [R], plus
        scores [R, Ntheta, Nt, Nt] when asked for."""
        out = {"pose": self._out.download().reshape(-1, 3)[:self.R], "delta": self.delta.download(),
               "best": self.best.download(), "n_valid": self.n_valid.download(), "rot0": self.rot0.download(),
               "flags": self.flags.download()}
        if self._have_scores:
            out["scores"] = self.scores.download()
        return out
