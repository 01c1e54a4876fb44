"""LiDAR-only odometry: batched correlative scan matching (``lslam_scan_match``).

The reference's robot is an RPLidar on a platform without encoders (``robot.py`` holds a pose and
nothing else), yet the filter's predict needs the wheel speeds ``u = [vl, vr]``
(``UKFMethods.py:17-24``).  Two consecutive revolutions give the motion between them:

* ``ScanMatcher``: R scan pairs per call -> ``delta`` (tx, ty, dtheta: the pose of the current
  frame in the previous one), the winner, flags, optionally the whole integer score volume
  and the wheel speeds that the filter's ``fx`` turns back into (tx, dtheta);
* ``LidarOdometry``: keeps each robot's previous revolution on the device and feeds
  ``LandmarkMap.u``, so packets -> revolutions -> odometry -> map -> filter never leave HBM::

      odo.step(xy, scan_chunk_off, chunk_pt_off, lm)   # writes lm.u on the device
      lm.step(xy, scan_chunk_off, chunk_pt_off)        # no u given: uses it

The definition (grid, scores, tie-break, refinement) is the comment on ``lslam_scan_match`` in
include/lidarslam.h; tests/scanmatch_ref.py is its NumPy form and the kernels match it bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _lib, staging
from .device import Context, DeviceArray
from .staging import _Grow, _as_device

MATCH_EMPTY, MATCH_EDGE = _lib.MATCH_EMPTY, _lib.MATCH_EDGE


def rot_table(k_theta, theta_step):
    """(cos, sin) of (k - k_theta) * theta_step, [2 k_theta + 1, 2] float64.  The library never
    computes these itself: the caller's bits are the definition."""
    a = (np.arange(2 * int(k_theta) + 1) - int(k_theta)) * float(theta_step)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], -1))


class ScanMatcher:
    """R scan pairs per call on one GPU.  ``params``: cell, theta_step, grid_w, smear, k_trans,
    k_theta (``lslam_match_params``; defaults 20 mm, pi/360, 512, 2, 10, 20)."""

    def __init__(self, ctx: Context, n_robots: int, **params):
        R = int(n_robots)
        if R <= 0:
            raise ValueError("n_robots must be > 0")
        self.ctx, self.R = ctx, R
        self.p = _lib.match_params(**params)
        self.Nt, self.Nth = 2 * self.p.k_trans + 1, 2 * self.p.k_theta + 1
        self.rot_host = rot_table(self.p.k_theta, self.p.theta_step)
        self.rot = ctx.to_device(self.rot_host)
        self.delta = ctx.empty((R, 3), np.float64)
        self.best = ctx.empty((R, 4), np.int32)
        self.n_valid = ctx.empty((R, 2), np.int32)
        self.flags = ctx.empty(R, np.int32)
        self.scores = None
        self.u = None
        self._g = {k: _Grow(ctx, np.float64 if k.endswith("xy") else np.int32)
                   for k in ("ref_xy", "ref_off", "cur_xy", "cur_off")}
        self._have_scores = False
        self._last_u = None

    def match(self, ref_xy, ref_off, cur_xy, cur_off, u_out=None, ukf=None, want_scores=False, sync=True):
        """Robot r: reference points ref_xy[ref_off[r]:ref_off[r+1]] (the previous revolution, in
        its own frame) against cur_xy[cur_off[r]:cur_off[r+1]].  Host arrays or ``DeviceArray``s
        (device offsets: int32 [R + 1]; device points are trusted to cover them).  With ``ukf``
        (a ``_lib.UkfParams``: dt, wheel_radius, wheel_base) the wheel speeds go to ``u_out``
        (a float64 [R, 2] ``DeviceArray``; default: the matcher's own ``u``)."""
        R = self.R
        offs = []
        for name, off in (("ref_off", ref_off), ("cur_off", cur_off)):
            if not isinstance(off, DeviceArray):
                off = np.ascontiguousarray(off, np.int32).reshape(-1)
                if off.size != R + 1 or np.any(np.diff(off) < 0) or off[0] < 0:
                    raise ValueError("%s must hold n_robots + 1 non-decreasing offsets" % name)
            offs.append(off)
        need = [0 if isinstance(o, DeviceArray) else 2 * int(o[-1]) for o in offs]
        d_ref = _as_device(self._g["ref_xy"], ref_xy, np.float64, need[0])
        d_cur = _as_device(self._g["cur_xy"], cur_xy, np.float64, need[1])
        d_roff = _as_device(self._g["ref_off"], offs[0], np.int32, R + 1)
        d_coff = _as_device(self._g["cur_off"], offs[1], np.int32, R + 1)
        b = _lib.MatchBatch()
        b.n_scans = R
        b.ref_xy, b.ref_off, b.cur_xy, b.cur_off = d_ref.addr, d_roff.addr, d_cur.addr, d_coff.addr
        b.rot = self.rot.addr
        b.delta, b.best, b.n_valid, b.flags = self.delta.addr, self.best.addr, self.n_valid.addr, self.flags.addr
        if want_scores:
            if self.scores is None:
                self.scores = self.ctx.empty((R, self.Nth, self.Nt, self.Nt), np.int32)
            b.scores = self.scores.addr
        self._have_scores = bool(want_scores)
        if ukf is not None:
            if u_out is None:
                if self.u is None:
                    self.u = self.ctx.empty((R, 2), np.float64)
                u_out = self.u
            if u_out.dtype != np.float64 or u_out.nbytes < 16 * R:
                raise ValueError("u_out must be float64 [n_robots, 2]")
            b.ukf_u = u_out.addr
        elif u_out is not None:
            raise ValueError("u_out needs ukf (dt, wheel_radius, wheel_base)")
        self._last_u = u_out
        _lib.call("lslam_scan_match", self.ctx, b, self.p, ukf)
        if sync:
            self.ctx.sync()

    def results(self):
        """The last call's delta [R, 3], best [R, 4] (k, jy, jx, score), flags [R], n_valid [R, 2],
        plus scores [R, Ntheta, Nt, Nt] when asked for and u [R, 2] when computed."""
        out = {"delta": self.delta.download(), "best": self.best.download(), "flags": self.flags.download(),
               "n_valid": self.n_valid.download()}
        if self._have_scores:
            out["scores"] = self.scores.download()
        if self._last_u is not None:
            out["u"] = self._last_u.download().reshape(-1, 2)[:self.R]
        return out


class LidarOdometry:
    """Scan-to-scan odometry for R robots: ``step`` takes one revolution per robot in the CSR
    layout of ``LandmarkMap.step`` and matches it against the previous one, kept on the device."""

    def __init__(self, ctx: Context, n_robots: int, **params):
        self.ctx, self.R = ctx, int(n_robots)
        self.matcher = ScanMatcher(ctx, n_robots, **params)
        # the matcher's own copies of the previous and the current revolution: [0] previous
        self._xy = [_Grow(ctx, np.float64), _Grow(ctx, np.float64)]
        self._off = [ctx.empty(self.R + 1, np.int32), ctx.empty(self.R + 1, np.int32)]
        self._n = [0, 0]
        self.steps = 0

    def step(self, xy, scan_chunk_off=None, chunk_pt_off=None, lm=None, sync=True):
        """Robot r's points: chunk_pt_off[scan_chunk_off[r]] .. chunk_pt_off[scan_chunk_off[r+1]]
        of ``xy`` (host array, ``DeviceArray`` or a ``MapInput``).  The first call stores the
        revolution and writes u = 0; later calls match previous -> current and, given a
        ``LandmarkMap`` ``lm``, write the wheel speeds into ``lm.u`` on the device (with lm's dt,
        wheel radius and wheel base), where ``lm.step(...)`` without ``u`` finds them.  Given device
        points and ``sync=False`` a step waits for the host only where a longer revolution grows a copy."""
        ctx, R = self.ctx, self.R
        xy, off = staging.point_offsets(xy, scan_chunk_off, chunk_pt_off, R)
        p0 = int(off[0])
        n = int(off[-1]) - p0
        # the caller's device array may be an express ring that the next step overwrites: copy
        cur = self._xy[1].reserve(2 * n)
        if self.steps == 0:
            self._xy[0].reserve(2 * n)  # both copies are sized by the first step: the second one's grow would sync
        if isinstance(xy, DeviceArray):
            staging.check_device_points(xy, off)
            if n:
                ctx.copy(cur, xy.addr + 16 * p0, 16 * n)
        else:
            self._xy[1].put_host(staging.points_on_host(xy, off))
        # on the stream, behind the match that read this buffer two steps ago (ctx._inflight holds the array)
        self._off[1].upload_async(np.ascontiguousarray(off - p0, np.int32))
        self._n[1] = n
        if self.steps == 0:
            if lm is not None:
                lm.u.fill_zero()
        else:
            if lm is not None and lm.R != R:
                raise ValueError("the map holds %d robots, the odometry %d" % (lm.R, R))
            self.matcher.match(self._xy[0].buf, self._off[0], cur, self._off[1],
                               u_out=None if lm is None else lm.u, ukf=None if lm is None else lm.up, sync=False)
        self._xy.reverse()
        self._off.reverse()
        self._n.reverse()
        self.steps += 1
        if sync:
            ctx.sync()

    def results(self):
        """The last match's results (``ScanMatcher.results``); None after the first step."""
        return self.matcher.results() if self.steps > 1 else None
