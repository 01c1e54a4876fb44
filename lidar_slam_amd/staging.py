"""Argument staging of the Python wrappers: the forms that a revolution, a pose and a filter may be
given in -> device buffers.

A revolution comes in the CSR layout of ``LandmarkMap.step`` as host arrays, as a ``DeviceArray`` read in
place, or as a ``MapInput``; a pose as a host [R, 3], a float64 ``DeviceArray`` or a ``LandmarkMap``.
``point_offsets`` is the one reading of the CSR arguments; ``Staging`` holds the device buffers that a
wrapper uploads the host forms into, one ``Staging`` per wrapper: uploads are ordered on the stream, so
a call in flight keeps its own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import DeviceArray
from .slam import LandmarkMap, MapInput


class _Grow:
    """A grow-only device buffer of one dtype, filled from host arrays or device arrays."""

    def __init__(self, ctx, dtype):
        self.ctx, self.dtype, self.buf = ctx, np.dtype(dtype), None

    def reserve(self, n):
        if self.buf is None or self.buf.shape[0] < n:
            self.ctx.sync()  # work in flight may still use the old allocation
            self.buf = self.ctx.empty(max(int(n), 1), self.dtype)
        return self.buf

    def put_host(self, arr):
        arr = np.ascontiguousarray(arr, self.dtype).reshape(-1)
        b = self.reserve(arr.size)
        if arr.nbytes:
            _lib.check(self.ctx._L.lslam_h2d(self.ctx.handle, b.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes),
                       "lslam_h2d")
            self.ctx._inflight.append(arr)
            self.ctx.sync()  # arr may be a temporary
        return b


def _as_device(grow, x, dtype, min_items):
    """x (host array or DeviceArray) -> a DeviceArray holding at least min_items items of dtype."""
    if isinstance(x, DeviceArray):
        if x.dtype != np.dtype(dtype) or x.nbytes < min_items * np.dtype(dtype).itemsize:
            raise ValueError("device array must be %s with at least %d items" % (np.dtype(dtype), min_items))
        return x
    h = np.ascontiguousarray(x, dtype).reshape(-1)
    if h.size < min_items:
        raise ValueError("array holds %d items, %d needed" % (h.size, min_items))
    return grow.put_host(h)


def point_offsets(xy, scan_chunk_off, chunk_pt_off, R):
    """One revolution per robot in CSR form -> (xy, off): ``xy`` as given, or the points of a
    ``MapInput`` (whose offsets then replace the other two arguments); off [R + 1] int64, robot r's
    points are xy[off[r]:off[r + 1]].  The last offset fits an int32."""
    if isinstance(xy, MapInput):
        xy, scan_chunk_off, chunk_pt_off = xy.xy, xy.sco, xy.cpo
    sco = np.ascontiguousarray(scan_chunk_off, np.int64).reshape(-1)
    cpo = np.ascontiguousarray(chunk_pt_off, np.int64).reshape(-1)
    if sco.size != R + 1:
        raise ValueError("one revolution per robot: scan_chunk_off needs n_robots + 1 entries")
    off = cpo[sco]
    if off[0] < 0 or np.any(np.diff(off) < 0) or off[-1] >= 2 ** 31:
        raise ValueError("inconsistent CSR offsets")
    return xy, off


def points_on_host(xy, off):
    """Host ``xy`` -> the points off[0]:off[-1] as float64 [n, 2]."""
    h = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    if h.shape[0] < off[-1]:
        raise ValueError("xy holds fewer points than chunk_pt_off describes")
    return h[off[0]:off[-1]]


def check_device_points(xy, off):
    if xy.dtype != np.float64 or xy.nbytes < 16 * int(off[-1]):
        raise ValueError("device xy must be float64 [n, 2] with n >= the last point offset")


def require_pose(pose):
    if pose is None:
        raise ValueError("pose is required (host [R, 3], a DeviceArray or a LandmarkMap)")


def filter_arguments(lm, x, P, R, noun):
    """The filter of a ``fuse``: ``lm`` (a ``LandmarkMap``), or ``x`` and ``P`` -> the device (x, P).
    ``noun``: what the caller calls itself where it counts robots."""
    if lm is not None:
        if x is not None or P is not None:
            raise ValueError("give lm, or x and P")
        if not isinstance(lm, LandmarkMap):
            raise ValueError("lm must be a LandmarkMap")
        if lm.R != R:
            raise ValueError("the map holds %d robots, the %s %d" % (lm.R, noun, R))
        x, P = lm.x, lm.P
    if not isinstance(x, DeviceArray) or not isinstance(P, DeviceArray):
        raise ValueError("fuse needs the filter on the device: lm (a LandmarkMap), or x and P (DeviceArrays)")
    if x.dtype != np.float64 or x.nbytes < 24 * R:
        raise ValueError("device x must be float64 [n_robots, 3]")
    if P.dtype != np.float64 or P.nbytes < 72 * R:
        raise ValueError("device P must be float64 [n_robots, 9]")
    return x, P


class Staging:
    """A wrapper's staging buffers: ``xy``, the grow-only points of a host revolution; ``off``, the
    [R + 1] int32 point offsets of the last revolution, and ``off_host``, the host's copy (int64);
    ``pose_buf``, the [R, 3] float64 that a host pose is uploaded to (``pose=False``: the owner sets it
    before the first ``pose`` call).  A wrapper calls ``revolution`` and ``pose`` in the order of its own
    checks."""

    def __init__(self, ctx, R, pose=True):
        self.R = R
        self.xy = _Grow(ctx, np.float64)
        self.off = ctx.empty(R + 1, np.int32)
        self.pose_buf = ctx.empty((R, 3), np.float64) if pose else None
        self.off_host = np.zeros(R + 1, np.int64)
        self._per_robot = {}  # per_robot's buffers, by name

    def revolution(self, xy, scan_chunk_off, chunk_pt_off):
        """The argument forms of ``OccupancyGrid.step`` -> device (xy, pt_off).  Host points are uploaded
        as the slice that the robots own, with offsets from its start; device points are read in place."""
        xy, off = point_offsets(xy, scan_chunk_off, chunk_pt_off, self.R)
        if isinstance(xy, DeviceArray):
            check_device_points(xy, off)
        else:
            xy, off = self.xy.put_host(points_on_host(xy, off)), off - off[0]
        self.off.upload_async(np.ascontiguousarray(off, np.int32))
        self.off_host = off
        return xy, self.off

    def pose(self, pose, noun, what="pose"):
        """The pose forms of ``OccupancyGrid.step`` -> a device [R, 3] float64.  ``noun``: what the
        owner calls itself where it counts robots; ``what``: the argument's name in the messages."""
        R = self.R
        require_pose(pose)
        if isinstance(pose, LandmarkMap):
            if pose.R != R:
                raise ValueError("the map holds %d robots, the %s %d" % (pose.R, noun, R))
            pose = pose.x
        if isinstance(pose, DeviceArray):
            if pose.dtype != np.float64 or pose.nbytes < 24 * R:
                raise ValueError("device %s must be float64 [n_robots, 3]" % what)
            return pose
        hp = np.ascontiguousarray(pose, np.float64)
        if hp.size != 3 * R:
            raise ValueError("%s must hold n_robots x 3 values" % what)
        self.pose_buf.upload_async(hp.reshape(R, 3))
        return self.pose_buf

    def per_robot(self, name, arr, width, dtype, what):
        """A per-robot argument of ``width`` items of ``dtype`` -> a device [R, width]: a ``DeviceArray`` is
        read in place; a host array (one row for all, or a row per robot) is uploaded, as ``pose`` is, to
        a buffer of this object's kept under ``name`` and allocated by its first use."""
        R, dtype = self.R, np.dtype(dtype)
        if isinstance(arr, DeviceArray):
            if arr.dtype != dtype or arr.nbytes < R * width * dtype.itemsize:
                raise ValueError("device %s must be %s [n_robots, %d]" % (what, dtype, width))
            return arr
        h = np.asarray(arr)
        if h.size not in (width, R * width):
            raise ValueError("%s must hold %d values, or n_robots x %d" % (what, width, width))
        h = np.ascontiguousarray(np.broadcast_to(h.reshape(-1, width), (R, width)), dtype)
        bufs = self._per_robot
        if name not in bufs:
            bufs[name] = self.off.ctx.empty((R, width), dtype)
        bufs[name].upload_async(h)
        return bufs[name]
