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

``GridRelocalizer`` (``lslam_map_relocalize``) finds the pose that a guess cannot reach: the start in
a stored grid, the kidnapped robot.  It needs no guess.  A coarse correlative search over every
coarse cell of the grid and every heading gives the K best separated peaks, ``lslam_map_match``
refines each, and the best refined pose is returned unless a second, distinct one scores nearly as
well (``RELOC_AMBIGUOUS``: a room that looks the same after a half turn) or none passes the fine
matcher's gates (``RELOC_LOST``).  With ``lm`` a found robot's mean and covariance are re-seated in
the filter on the device; the others keep theirs::

    grid.upload(stored)                                        # a restart
    rel.relocalize(xy, scan_chunk_off, chunk_pt_off, grid=grid, lm=lm)

Two priors narrow the coarse search to the candidates a robot can have (``lslam_map_relocalize_prior``):
``field``, the ``DIST_NOT_FREE`` distance field of the grid, admits only coarse cells with free space in
them, and rejects a refined pose that stands on a cell with less clearance than ``clear_min2``;
``window``, a stale pose, admits only the cells within ``half_xy`` and the headings within ``half_theta``
of it, so a filter that drifted a metre does not pay the whole-grid search, and the half-turn twin that
the stale pose rules out is not a rival::

    free = DistanceField(grid, mode=DIST_NOT_FREE)
    free.step()
    rel.relocalize(xy, scan_chunk_off, chunk_pt_off, grid=grid, lm=lm, field=free, window=lm.x)

The definitions are the comments on ``lslam_map_match``, ``lslam_map_fuse`` and
``lslam_map_relocalize`` (and ``lslam_map_relocalize_prior``) in include/lidarslam.h;
tests/mapmatch_ref.py, tests/mapfuse_ref.py, tests/reloc_ref.py and tests/relocprior_ref.py are
their NumPy forms and the kernels match them bit for bit, given the
(cos, sin) that the library wrote to ``rot0``.
"""
from __future__ import annotations

import numpy as np

from . import _lib, staging
from .device import Context, DeviceArray
from .mapping import DistanceField, OccupancyGrid
from .odometry import rot_table
from .slam import LandmarkMap
from .staging import Staging

MAPMATCH_EMPTY, MAPMATCH_EDGE = _lib.MAPMATCH_EMPTY, _lib.MAPMATCH_EDGE
MAPMATCH_BAD_POSE, MAPMATCH_WEAK = _lib.MAPMATCH_BAD_POSE, _lib.MAPMATCH_WEAK
MAPFUSE_OUTLIER, MAPFUSE_BAD_COV = _lib.MAPFUSE_OUTLIER, _lib.MAPFUSE_BAD_COV

RELOC_LOST, RELOC_AMBIGUOUS = _lib.RELOC_LOST, _lib.RELOC_AMBIGUOUS

_FUSE_KEYS = ("r_scale", "nis_max", "cut_permille")
_RELOC_KEYS = ("head_step", "n_head", "factor", "n_cand", "ambig_permille", "dup_mm", "dup_rad", "reset_sigma_xy",
               "reset_sigma_theta")
_PRIOR_KEYS = ("half_xy", "half_theta", "clear_min2")


def head_table(n_head, head_step):
    """(cos, sin) of k * head_step, [n_head, 2] float64: the coarse search's headings.  As with
    ``rot_table`` the library never computes these itself: the caller's bits are the definition."""
    a = np.arange(int(n_head)).astype(np.float64) * float(head_step)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))


def _check_grid(grid, R):
    if not isinstance(grid, OccupancyGrid):
        raise ValueError("grid is required (an OccupancyGrid)")
    if grid.R != R:
        raise ValueError("the grid holds %d robots, the localizer %d" % (grid.R, R))


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
        _lib.call("lslam_map_match", ctx, _lib.MapMatchBatch(), _lib.grid_params(), self.p)
        _lib.call("lslam_map_fuse", ctx, _lib.MapFuseBatch(), _lib.grid_params(), self.p, self.fp)
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
        self._stage = Staging(ctx, R)
        self._have_scores = False
        self._out = self.pose
        self._fused = None  # fuse's buffers (P, z, Rm, nis, moments), made by the first fuse
        self._P_out = None
        self.steps = 0

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, grid=None, pose=None, write_back=False,
             want_scores=False, sync=True):
        """One revolution per robot, in the CSR layout of ``OccupancyGrid.step`` (host array,
        ``DeviceArray`` or a ``MapInput``; device points are read in place).  ``grid``: the
        ``OccupancyGrid`` to localise in (its logodds, origin and parameters).  ``pose`` [R, 3]
        (x, y, theta), the guess: a host array, a float64 ``DeviceArray`` or a ``LandmarkMap``
        (its ``x``).  ``write_back``: with a device pose, the result is written over it (a robot
        whose match is EMPTY, WEAK or BAD_POSE keeps its bits); otherwise it goes to ``self.pose``."""
        _check_grid(grid, self.R)  # (the grid's errors come first)
        staging.require_pose(pose)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        if write_back and not isinstance(pose, (DeviceArray, LandmarkMap)):
            raise ValueError("write_back needs a device pose (a DeviceArray or a LandmarkMap)")
        dpose = self._stage.pose(pose, "localizer")
        dout = dpose if write_back else self.pose
        b = _lib.MapMatchBatch()
        self._fill(b, dxy, doff, dpose, dout, grid, want_scores)
        self._P_out = None
        _lib.call("lslam_map_match", self.ctx, b, grid.p, self.p)
        self.steps += 1
        if sync:
            self.ctx.sync()

    def _fill(self, b, dxy, doff, dpose, dout, grid, want_scores):
        """The fields of a ``MapMatchBatch`` for one call."""
        R = self.R
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
        x, P = staging.filter_arguments(lm, x, P, R, "localizer")
        _check_grid(grid, R)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        if self._fused is None:
            self._fused = {"P": ctx.empty((R, 9), np.float64), "z": ctx.empty((R, 3), np.float64),
                           "Rm": ctx.empty((R, 9), np.float64), "nis": ctx.empty(R, np.float64),
                           "moments": ctx.empty((R, 10), np.int64)}
            for a in self._fused.values():
                a.fill_zero()
        fb = self._fused
        b = _lib.MapFuseBatch()
        self._fill(b.m, dxy, doff, x, x if write_back else self.pose, grid, want_scores)
        self._P_out = P if write_back else fb["P"]
        b.P, b.P_out = P.addr, self._P_out.addr
        b.z, b.Rm, b.nis, b.moments = fb["z"].addr, fb["Rm"].addr, fb["nis"].addr, fb["moments"].addr
        _lib.call("lslam_map_fuse", ctx, b, grid.p, self.p, self.fp)
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


class GridRelocalizer:
    """R robots per call on one GPU.  ``params``: head_step, n_head, factor, n_cand, ambig_permille,
    dup_mm, dup_rad, reset_sigma_xy, reset_sigma_theta (``lslam_reloc_params``; defaults 2 pi / 180,
    180, 4, 8, 900, 100.0, 0.0873, 50.0, 0.05) and the fine matcher's (``lslam_mapmatch_params``, as
    ``GridLocalizer``), and for a call with ``field`` or ``window`` half_xy, half_theta, clear_min2
    (``lslam_relocprior_params``; defaults 1000.0 mm, 0.5 rad, 16).  The cell size, the map's width and
    max_range are the grid's, given with each call."""

    _PER_RANK = (("cand", 4, np.int32), ("cand_pose", 3, np.float64), ("fine_pose", 3, np.float64),
                 ("fine_delta", 3, np.float64), ("fine_best", 4, np.int32), ("fine_nvalid", 2, np.int32),
                 ("fine_rot0", 2, np.float64), ("fine_flags", 1, np.int32))

    def __init__(self, ctx: Context, n_robots: int, **params):
        R = int(n_robots)
        if R <= 0:
            raise ValueError("n_robots must be > 0")
        self.ctx, self.R = ctx, R
        self.q = _lib.reloc_params(**{k: params.pop(k) for k in _RELOC_KEYS if k in params})
        self.pp = _lib.relocprior_params(**{k: params.pop(k) for k in _PRIOR_KEYS if k in params})
        self.p = _lib.mapmatch_params(**params)
        # (a range error of params surfaces here, from the first call)
        _lib.call("lslam_map_relocalize", ctx, _lib.RelocBatch(), _lib.grid_params(), self.p, self.q)
        _lib.call("lslam_map_relocalize_prior", ctx, _lib.RelocPriorBatch(), _lib.grid_params(), self.p, self.q, self.pp)
        K = self.K = int(self.q.n_cand)
        self.rot_host = rot_table(self.p.k_theta, self.p.theta_step)
        self.rot = ctx.to_device(self.rot_host)
        self.head_rot_host = head_table(self.q.n_head, self.q.head_step)
        self.head_rot = ctx.to_device(self.head_rot_host)
        self.pose = ctx.empty((R, 3), np.float64)  # pose_out, unless a call re-seats a filter
        self.n_occ, self.n_used = ctx.empty(R, np.int32), ctx.empty(R, np.int32)
        self.result, self.flags = ctx.empty((R, 8), np.int32), ctx.empty(R, np.int32)
        self.ranks = {n: ctx.empty((K, R, w) if w > 1 else (K, R), dt) for n, w, dt in self._PER_RANK}
        for a in (self.n_occ, self.n_used, self.result, self.flags) + tuple(self.ranks.values()):
            a.fill_zero()
        self.coarse = None
        self._stage = Staging(ctx, R, pose=False)  # (the window's buffer comes with the first prior call's)
        self._have_coarse = False
        self._out, self._P_out = self.pose, None
        self._prior = None  # a prior call's own buffers (n_admit, fine_clear2, the window), made by the first
        self._have_prior = False
        self.calls = 0

    def set_budget(self, nbytes):
        """Bytes of coarse-score scratch per chunk of robots (``lslam_set_reloc_budget``; <= 0: the
        default).  No result depends on it."""
        _lib.call("lslam_set_reloc_budget", self.ctx, int(nbytes))

    def relocalize(self, xy, scan_chunk_off=None, chunk_pt_off=None, grid=None, lm=None, want_coarse=False, sync=True,
                   field=None, window=None, prior=False):
        """One revolution per robot, in the forms ``GridLocalizer.step`` accepts; ``grid``: the
        ``OccupancyGrid`` to find the robots in.  With ``lm`` (a ``LandmarkMap``) the pose of a found,
        unambiguous robot is written over ``lm.x`` and diag(reset_sigma_xy^2, reset_sigma_xy^2,
        reset_sigma_theta^2) over its ``lm.P``; LOST and AMBIGUOUS robots keep the bits of both.
        Without it the poses go to ``self.pose``, NaN where none was found.

        ``field``: a ``DistanceField`` of ``grid`` in ``DIST_NOT_FREE`` mode, stepped, with
        d_max^2 >= clear_min2: the free-space prior.  ``window`` [R, 3]: a stale pose (a host array, a
        float64 ``DeviceArray`` such as ``lm.x``, or a ``LandmarkMap``), the centre of the search
        window; it is read before ``lm.x`` is written.  With either the call is
        ``lslam_map_relocalize_prior``; with neither it is ``lslam_map_relocalize`` as before, unless
        ``prior`` asks for ``lslam_map_relocalize_prior`` all the same: the same results bit for bit, plus
        ``n_admit`` (every cell, every heading) and ``fine_clear2`` (zeros)."""
        ctx, R, K = self.ctx, self.R, self.K
        if field is not None:
            if not isinstance(field, DistanceField):
                raise ValueError("field must be a DistanceField")
            if field.grid is not grid:
                raise ValueError("field must be the distance field of grid")
            if int(field.p.mode) != _lib.DIST_NOT_FREE:
                raise ValueError("field must be a DIST_NOT_FREE distance field (mode=DIST_NOT_FREE)")
            if int(field.p.d_max) ** 2 < int(self.pp.clear_min2):
                raise ValueError("field saturates below clear_min2: d_max^2 must be >= clear_min2")
            if not field.steps:
                raise ValueError("no step yet: the field has not been computed")
        if lm is not None:
            if not isinstance(lm, LandmarkMap):
                raise ValueError("lm must be a LandmarkMap")
            if lm.R != R:
                raise ValueError("the map holds %d robots, the localizer %d" % (lm.R, R))
        _check_grid(grid, R)
        dxy, doff = self._stage.revolution(xy, scan_chunk_off, chunk_pt_off)
        b = _lib.RelocBatch()
        b.n_robots = R
        b.xy, b.pt_off, b.origin, b.logodds = dxy.addr, doff.addr, grid.origin.addr, grid.logodds.addr
        b.rot, b.head_rot = self.rot.addr, self.head_rot.addr
        b.n_occ, b.n_used, b.result, b.flags = self.n_occ.addr, self.n_used.addr, self.result.addr, self.flags.addr
        for n, _, _ in self._PER_RANK:
            setattr(b, n, self.ranks[n].addr)
        if lm is not None:
            self._out, self._P_out = lm.x, lm.P
            b.P_out = lm.P.addr
        else:
            self._out, self._P_out = self.pose, None
            self.pose.upload_async(np.full((R, 3), np.nan))
        b.pose_out = self._out.addr
        if want_coarse:
            Wc = grid.W // int(self.q.factor)
            shape = (R, int(self.q.n_head), Wc, Wc)
            if self.coarse is None or self.coarse.shape != shape:
                self.coarse = ctx.empty(shape, np.int32)
            b.coarse_scores = self.coarse.addr
        self._have_coarse = bool(want_coarse)
        self._have_prior = field is not None or window is not None or bool(prior)
        if self._have_prior:
            self._relocalize_prior(b, grid, field, window)
        else:
            _lib.call("lslam_map_relocalize", ctx, b, grid.p, self.p, self.q)
        self.calls += 1
        if sync:
            ctx.sync()

    def _relocalize_prior(self, b, grid, field, window):
        """``lslam_map_relocalize_prior`` with the filled ``RelocBatch`` b."""
        ctx, R, K = self.ctx, self.R, self.K
        if self._prior is None:
            self._prior = {"n_admit": ctx.empty((R, 2), np.int32), "fine_clear2": ctx.empty((K, R), np.int32),
                           "window": ctx.empty((R, 3), np.float64)}
            for a in self._prior.values():
                a.fill_zero()
            self._stage.pose_buf = self._prior["window"]
        pb = _lib.RelocPriorBatch()
        pb.r = b
        pb.n_admit, pb.fine_clear2 = self._prior["n_admit"].addr, self._prior["fine_clear2"].addr
        if field is not None:
            pb.clear_d2 = field.d2.addr
        if window is not None:
            pb.win_pose = self._stage.pose(window, "localizer", "window").addr
        _lib.call("lslam_map_relocalize_prior", ctx, pb, grid.p, self.p, self.q, self.pp)

    def results(self):
        """The last call's pose [R, 3] (``lm.x`` after a call with ``lm``), flags [R] (RELOC_*),
        result [R, 8] (winner rank, its k, ty, tx, coarse score, fine score, best rival's rank or -1,
        its fine score), n_occ [R], n_used [R], per rank j < K cand [K, R, 4], cand_pose [K, R, 3] and
        the fine matcher's fine_pose, fine_delta, fine_best, fine_nvalid, fine_rot0, fine_flags
        [K, R, ..]; P [R, 3, 3] after a call with ``lm``; coarse_scores [R, n_head, Wc, Wc] when asked for;
        after a call with ``field`` or ``window`` n_admit [R, 2] (admissible coarse cells, admissible
        headings) and fine_clear2 [K, R] (the field at each refined pose's cell)."""
        out = {"pose": self._out.download().reshape(-1, 3)[:self.R], "flags": self.flags.download(),
               "result": self.result.download(), "n_occ": self.n_occ.download(), "n_used": self.n_used.download()}
        for n, _, _ in self._PER_RANK:
            out[n] = self.ranks[n].download()
        if self._P_out is not None:
            out["P"] = self._P_out.download().reshape(-1, 3, 3)[:self.R]
        if self._have_coarse:
            out["coarse_scores"] = self.coarse.download()
        if self._have_prior:
            out["n_admit"], out["fine_clear2"] = self._prior["n_admit"].download(), self._prior["fine_clear2"].download()
        return out
