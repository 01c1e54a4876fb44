"""The paged rolling grid's definition (tests/page_ref.py) held to what it is for, on the CPU, and the
C ABI of the three calls without a device.

(a) the world view (the canvas with the window laid over it) is the same before and after a paged
    recentre, at every canvas cell; and the reference equals a cell-by-cell loop over the definition;
(b) a walk of 12 recentres with writes into the window between them: the flushed canvas equals a model
    that applies the same writes to one fixed Cw x Cw array; one walk leaves the canvas: LOST, the
    zeros that enter, the counts in moved;
(c) a window that goes out and comes back holds the bits it started with, where the plain recentre
    holds zeros;
(d) sizes, defaults, and the checks that need no device.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import page_ref as pr
import recentre_ref as rr
from test_recentre_ref import bits

CELL = 20.0
WALK_STEPS = 12
# the walks of (b), shared with tests/test_gpu_page.py: quantum 8 with everything on 8 cells (the 16-byte
# path), and quantum 1 at a width that is no multiple of 8
WALKS = {
    "groups": dict(W=16, Cw=64, quantum=8, win=(24, 24), seed=1),
    "cells": dict(W=24, Cw=64, quantum=1, win=(19, 22), seed=2),
}


def rnd16(rng, shape):
    return rng.integers(-32768, 32768, shape).astype(np.int16)


def pose_for(origin, W, sx, sy, theta=0.25):
    """With margin = W / 2 a pose on the middle of cell (W / 2 + sx, W / 2 + sy) gives the shift (sx, sy) at
    quantum 1, and at quantum 8 when sx and sy are multiples of 8; (0, 0) included."""
    return np.append(rr.pose_for_shift(origin, CELL, W, sx, sy), theta)


def kw_for(W, quantum):
    return dict(grid_w=W, cell=CELL, margin=W // 2, quantum=quantum)


def make_walk(name):
    """12 (shift, write) steps that keep the window on the canvas.  A write is (y0, y1, x0, x1, values): what
    a map update would do to the window after the recentre."""
    w = WALKS[name]
    W, Cw, q = w["W"], w["Cw"], w["quantum"]
    rng = np.random.default_rng(w["seed"])
    win = np.array(w["win"], np.int64)
    steps = []
    while len(steps) < WALK_STEPS:
        k = len(steps)
        if k == 5:
            s = np.array([0, 0])  # a recentre that finds the robot in the middle
        elif k in (3, 9):
            s = -steps[k - 1][0]  # straight back: the strip that left returns
        else:
            s = q * rng.integers(-W // q - 1, W // q + 2, 2) if k == 7 else q * rng.integers(-2 * 8 // q, 2 * 8 // q + 1, 2)
        if np.any(win + s < 0) or np.any(win + s + W > Cw):
            continue
        win = win + s
        y0, x0 = rng.integers(0, W - 3, 2)
        y1, x1 = y0 + rng.integers(1, W - y0 + 1), x0 + rng.integers(1, W - x0 + 1)
        steps.append((s, (int(y0), int(y1), int(x0), int(x1), rnd16(rng, (y1 - y0, x1 - x0)))))
    return steps


def run_walk_ref(name, plain=False):
    """The walk through the reference: (L, canvas, win, origin, model, per-step results)."""
    w = WALKS[name]
    W, Cw = w["W"], w["Cw"]
    kw = kw_for(W, w["quantum"])
    L, canvas, model = np.zeros((W, W), np.int16), np.zeros((Cw, Cw), np.int16), np.zeros((Cw, Cw), np.int16)
    win, origin = np.array(w["win"], np.int32), np.array([-400.0, 260.0])
    log = []
    for s, (y0, y1, x0, x1, v) in make_walk(name):
        pose = pose_for(origin, W, *s)
        if plain:
            L, origin, shift, flags = rr.recentre(L, pose, origin, **kw)
            win = win + shift
            o = dict(shift=shift)
        else:
            o = pr.recentre_paged(L, canvas, win, pose, origin, **kw)
            L, canvas, win, origin = o["L"], o["canvas"], o["win"], o["origin"]
        assert tuple(o["shift"]) == tuple(s)
        log.append(o)
        L = L.copy()
        L[y0:y1, x0:x1] = v
        model[win[1] + y0:win[1] + y1, win[0] + x0:win[0] + x1] = v
    return L, canvas, win, origin, model, log


# ---- (a) ----

def definition_by_loops(L, canvas, win, sx, sy):
    """Steps 2 to 4 of the definition, a cell at a time."""
    W, Cw = L.shape[0], canvas.shape[0]
    wx, wy = int(win[0]), int(win[1])
    canvas, L1 = canvas.copy(), np.zeros_like(L)
    stored = loaded = lost = 0
    for y in range(W):
        for x in range(W):
            if not (0 <= x - sx < W and 0 <= y - sy < W):
                if 0 <= wx + x < Cw and 0 <= wy + y < Cw:
                    canvas[wy + y, wx + x] = L[y, x]
                    stored += 1
                else:
                    lost = 1
    for y in range(W):
        for x in range(W):
            if 0 <= x + sx < W and 0 <= y + sy < W:
                L1[y, x] = L[y + sy, x + sx]
            elif 0 <= wx + sx + x < Cw and 0 <= wy + sy + y < Cw:
                L1[y, x] = canvas[wy + sy + y, wx + sx + x]
                loaded += 1
    return L1, canvas, (wx + sx, wy + sy), (stored, loaded), lost


def shifts_for(W):
    return [(0, 0), (3, 0), (0, -5), (-8, 0), (0, 8), (8, -8), (-3, 7), (5, 9), (W - 1, 1), (W, 0), (0, -W), (W + 3, -2),
            (-2, -W - 1), (-5000, 16)]


def wins_for(W, Cw):
    """Inside; half off each edge; wholly off on each side and far off."""
    return [((Cw - W) // 2, (Cw - W) // 2 + 1), (0, 0), (Cw - W, Cw - W), (-W // 2, 3), (Cw - W // 2, 3), (5, -W // 2),
            (5, Cw - W // 2), (-W // 2, Cw - W // 2), (-W, 4), (Cw, 4), (4, -W - 7), (4, Cw + 9), (-3 * Cw, 2 * Cw),
            (2 ** 31 - 1 - W, 0), (-2 ** 31, -2 ** 31 + 5)]


@pytest.mark.parametrize("W,Cw", [(16, 40), (16, 64), (24, 40), (24, 64)])
def test_world_view_is_invariant(W, Cw):
    rng = np.random.default_rng(W * 100 + Cw)
    origin = np.array([40.0, -60.0])
    n_lost = n_loaded = 0
    for win in wins_for(W, Cw):
        for sx, sy in shifts_for(W):
            if not (-2 ** 31 <= win[0] + sx < 2 ** 31 and -2 ** 31 <= win[1] + sy < 2 ** 31):
                continue
            L, canvas = rnd16(rng, (W, W)), rnd16(rng, (Cw, Cw))
            before = pr.world_view(L, canvas, win)
            o = pr.recentre_paged(L, canvas, win, pose_for(origin, W, sx, sy), origin, **kw_for(W, 1))
            assert tuple(o["shift"]) == (sx, sy) and o["flags"] == ((rr.MOVED | (rr.CLEARED if max(abs(sx), abs(sy)) >= W else 0))
                                                                    if (sx or sy) else 0)
            assert np.array_equal(pr.world_view(o["L"], o["canvas"], o["win"]), before), (win, sx, sy)
            L1, c1, w1, moved, lost = definition_by_loops(L, canvas, win, sx, sy)
            assert np.array_equal(o["L"], L1) and np.array_equal(o["canvas"], c1), (win, sx, sy)
            assert tuple(o["win"]) == w1 and tuple(o["moved"]) == moved and o["page_flags"] == lost, (win, sx, sy)
            n_lost += lost
            n_loaded += moved[1] > 0
    assert n_lost > 20 and n_loaded > 20


def test_bad_pose_and_zero_shift_change_nothing():
    W, Cw = 16, 40
    rng = np.random.default_rng(3)
    L, canvas, win, origin = rnd16(rng, (W, W)), rnd16(rng, (Cw, Cw)), (7, 9), np.array([0.0, 20.0])
    for pose, flag in ((pose_for(origin, W, 0, 0), 0), (np.array([np.nan, 0.0, 0.0]), rr.BAD_POSE),
                       (np.array([1e300, 0.0, 0.0]), rr.BAD_POSE)):
        o = pr.recentre_paged(L, canvas, win, pose, origin, **kw_for(W, 1))
        assert np.array_equal(o["L"], L) and np.array_equal(o["canvas"], canvas) and tuple(o["win"]) == win
        assert not o["moved"].any() and o["page_flags"] == 0 and o["flags"] == flag and not o["shift"].any()
        assert np.array_equal(bits(o["origin"]), bits(origin))


# ---- (b) ----

@pytest.mark.parametrize("name", list(WALKS))
def test_walk_against_a_fixed_canvas(name):
    L, canvas, win, origin, model, log = run_walk_ref(name)
    assert len(log) == WALK_STEPS and not any(o["page_flags"] for o in log)  # the walk stays on the canvas
    assert sum(o["moved"][1] > 0 for o in log) >= 8
    flushed, moved = pr.flush(L, canvas, win)
    assert np.array_equal(flushed, model)
    assert moved.tolist() == [L.size, 0]
    # the window is the model's cells under it, and a load from the flushed canvas gives it back
    W = L.shape[0]
    assert np.array_equal(L, model[win[1]:win[1] + W, win[0]:win[0] + W])
    back, moved = pr.load(flushed, win, W)
    assert np.array_equal(back, L) and moved.tolist() == [0, L.size]
    # the plain recentre on the same walk has lost cells that the paged window holds
    Lp = run_walk_ref(name, plain=True)[0]
    assert np.any((Lp == 0) & (L != 0)) and np.array_equal(Lp[Lp != 0], L[Lp != 0])


def test_walk_off_the_canvas():
    W, Cw = 16, 40
    kw = kw_for(W, 8)
    rng = np.random.default_rng(8)
    L, canvas = rnd16(rng, (W, W)) | 1, np.zeros((Cw, Cw), np.int16)  # (no cell of the window is 0)
    win, origin = np.array([Cw - W, 8], np.int32), np.array([0.0, 0.0])
    want = [((8, 0), (8 * W, 0), 0), ((8, 0), (8 * W, 0), 0), ((-8, 0), (0, 8 * W), pr.LOST),
            ((0, -16), (8 * W, 8 * (W - 8)), pr.LOST), ((48, 0), (8 * (W - 8), 0), pr.LOST), ((-64, 8), (0, W * W), pr.LOST)]
    first = L.copy()
    for (sx, sy), moved, flag in want:
        o = pr.recentre_paged(L, canvas, win, pose_for(origin, W, sx, sy), origin, **kw)
        assert tuple(o["shift"]) == (sx, sy) and tuple(o["moved"]) == moved and o["page_flags"] == flag, (sx, sy, o["moved"])
        L, canvas, win, origin = o["L"], o["canvas"], o["win"], o["origin"]
        if (sx, sy) == (8, 0):
            assert not L[:, W - 8:].any()  # what enters from beyond the canvas is unknown
    assert tuple(win) == (Cw - W - 8, 0)
    # the first strip that left on the canvas is where it was: canvas columns Cw - W .. Cw - W + 8, rows 8 .. 8 + W
    assert np.array_equal(canvas[8:8 + W, Cw - W:Cw - W + 8], first[:, :8])


# ---- (c) ----

@pytest.mark.parametrize("W,s,q", [(16, (8, 0), 8), (16, (-8, 16), 8), (24, (5, -3), 1), (24, (0, 30), 1)])
def test_out_and_back(W, s, q):
    Cw = 64
    rng = np.random.default_rng(W + s[0])
    L0 = rnd16(rng, (W, W)) | 1
    kw = kw_for(W, q)
    origin0 = np.array([200.0, -40.0])
    L, canvas, win, origin = L0, np.zeros((Cw, Cw), np.int16), (24, 16), origin0
    Lp, op = L0, origin0
    for sx, sy in (s, (-s[0], -s[1])):
        o = pr.recentre_paged(L, canvas, win, pose_for(origin, W, sx, sy), origin, **kw)
        L, canvas, win, origin = o["L"], o["canvas"], o["win"], o["origin"]
        Lp, op = rr.recentre(Lp, pose_for(op, W, sx, sy), op, **kw)[:2]
    assert np.array_equal(L, L0) and tuple(win) == (24, 16) and np.array_equal(bits(origin), bits(origin0))
    gone = pr.leaving(W, *s)
    assert gone.any() and not Lp[gone].any() and np.array_equal(Lp[~gone], L0[~gone])  # the plain call: zeros there


# ---- (d) ----

def test_abi_sizes_defaults_and_constants():
    from lidar_slam_amd import _lib, mapping
    L = _lib.load()
    got = (C.c_int64 * 2)()
    assert L.lslam_page_abi_sizes(got, 2) == 2 and list(got) == [16, 40]
    assert list(got) == [C.sizeof(_lib.PageParams), C.sizeof(_lib.PageBatch)]
    one = (C.c_int64 * 2)(-1, -1)
    assert L.lslam_page_abi_sizes(one, 1) == 2 and list(one) == [16, -1] and L.lslam_page_abi_sizes(None, 2) == 2
    B = _lib.PageBatch
    assert [(f, getattr(B, f).offset) for f, _ in B._fields_] == [("n_robots", 0), ("reserved", 4), ("canvas", 8), ("win", 16),
                                                                 ("moved", 24), ("flags", 32)]
    p = _lib.page_params()
    assert p.canvas_w == 2048 and list(p.reserved) == [0, 0, 0]
    assert _lib.PAGE_LOST == mapping.PAGE_LOST == pr.LOST == 1
    assert _lib.ABI_VERSION == 6 and b"(abi 6," in L.lslam_version()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lidarslam.h")).read()
    assert re.search(r"LSLAM_K_COUNT = 16\b", hdr) and re.search(r"#define LSLAM_ABI_VERSION\s+6\b", hdr)  # no new timing slot
    assert re.search(r"LSLAM_PAGE_LOST = 1\b", hdr)
    # the older tables are unchanged
    nine = (C.c_int64 * 9)()
    assert L.lslam_abi_sizes(nine, 9) == 9 and list(nine) == [112, 56, 56, 128, 232, 48, 48, 32, 96]
    four = (C.c_int64 * 4)()
    assert L.lslam_dist_abi_sizes(four, 4) == 4 and list(four) == [16, 40, 16, 80]
    for fn, want in ((L.lslam_grid_abi_sizes, [40, 72]), (L.lslam_mapmatch_abi_sizes, [32, 112]),
                     (L.lslam_mapfuse_abi_sizes, [24, 160]), (L.lslam_reloc_abi_sizes, [56, 176]),
                     (L.lslam_raycast_abi_sizes, [16, 88]), (L.lslam_recentre_abi_sizes, [16, 48])):
        t = (C.c_int64 * 2)()
        assert fn(t, 2) == 2 and list(t) == want
    assert all(hasattr(mapping.OccupancyGrid, m) for m in ("flush", "load", "world"))


def _batches(n=1):
    from lidar_slam_amd import _lib
    b, pg = _lib.RecentreBatch(), _lib.PageBatch()
    b.n_robots = pg.n_robots = n
    for i, f in enumerate(("pose", "origin", "logodds", "shift", "flags")):
        setattr(b, f, (i + 1) << 32)
    for i, f in enumerate(("canvas", "win", "moved", "flags")):
        setattr(pg, f, (i + 8) << 32)
    return b, pg


def _err(st):
    from lidar_slam_amd import _lib
    assert st == _lib.LSLAM_ERR_ARG
    return _lib.load().lslam_last_error().decode()


def test_checks_come_before_the_context():
    """Every call with ctx = NULL: the message says how far it came."""
    from lidar_slam_amd import _lib
    L = _lib.load()
    g, q, pp = _lib.grid_params(grid_w=64), _lib.recentre_params(margin=32), _lib.page_params(canvas_w=128)
    ref = C.byref

    def paged(b, pg, g=g, q=q, pp=pp):
        return _err(L.lslam_grid_recentre_paged(None, b and ref(b), pg and ref(pg), g and ref(g), q and ref(q), pp and ref(pp)))

    b, pg = _batches()
    assert paged(b, pg) == "page: ctx is NULL"
    assert paged(b, pg, pp=None) == "page: params is NULL" and paged(b, pg, q=None) == "recentre: params is NULL"
    for cw in (15, 2049, 0, -8):
        assert "canvas_w must be in [16, 2048]" in paged(b, pg, pp=_lib.page_params(canvas_w=cw))
    assert "margin" in paged(b, pg, q=_lib.recentre_params(margin=33))
    assert paged(None, pg) == "page: batch is NULL" and paged(b, None) == "page: batch is NULL"
    for f in ("pose", "origin", "logodds"):
        b, pg = _batches()
        setattr(b, f, None)
        assert paged(b, pg) == "page: missing input (pose, origin, logodds, win, canvas)"
    for f in ("win", "canvas"):
        b, pg = _batches()
        setattr(pg, f, None)
        assert paged(b, pg) == "page: missing input (pose, origin, logodds, win, canvas)"
    for which, f in ((0, "shift"), (0, "flags"), (1, "moved"), (1, "flags")):
        bb = _batches()
        setattr(bb[which], f, None)
        assert paged(*bb) == "page: missing output (shift, flags, moved, page flags)"
    b, pg = _batches()
    pg.n_robots = 2
    assert paged(b, pg) == "page: n_robots of the two batches differ"
    b.n_robots = -1
    assert paged(b, pg) == "page: negative n_robots"
    # an overlap of the canvas and the window's grids, from either side
    for n, canvas in ((1, (3 << 32) + 64 * 64 * 2 - 2), (1, (3 << 32) - 128 * 128 * 2 + 2), (3, (3 << 32) + 64 * 64 * 2 * 2)):
        b, pg = _batches(n)
        pg.canvas = canvas
        assert paged(b, pg) == "page: canvas overlaps logodds"
    b, pg = _batches(1)
    pg.canvas = (3 << 32) + 64 * 64 * 2  # back to back is no overlap
    assert paged(b, pg) == "page: ctx is NULL"
    # an empty call needs no pointer
    assert paged(_lib.RecentreBatch(), _lib.PageBatch()) == "page: ctx is NULL"

    for fn, first in ((L.lslam_grid_page_flush, "missing input (logodds, win)"), (L.lslam_grid_page_load, "missing input (canvas, win)")):
        b, pg = _batches()
        pg.flags = None  # (neither call touches the flags)
        assert _err(fn(None, ref(pg), 3 << 32, ref(g), ref(pp))) == "page: ctx is NULL"
        assert _err(fn(None, None, 3 << 32, ref(g), ref(pp))) == "page: batch is NULL"
        assert _err(fn(None, ref(pg), 3 << 32, ref(g), None)) == "page: params is NULL"
        assert "canvas_w" in _err(fn(None, ref(pg), 3 << 32, ref(g), ref(_lib.page_params(canvas_w=8))))
        pg.win = None
        assert _err(fn(None, ref(pg), 3 << 32, ref(g), ref(pp))) == "page: " + first
        b, pg = _batches()
        pg.moved = None
        assert "page: missing output" in _err(fn(None, ref(pg), 3 << 32, ref(g), ref(pp)))
        b, pg = _batches()
        assert "page: missing" in _err(fn(None, ref(pg), None, ref(g), ref(pp)))
        pg.canvas = (3 << 32) + 2
        assert _err(fn(None, ref(pg), 3 << 32, ref(g), ref(pp))) == "page: canvas overlaps logodds"
        assert _err(fn(None, ref(_lib.PageBatch()), None, ref(g), ref(pp))) == "page: ctx is NULL"
