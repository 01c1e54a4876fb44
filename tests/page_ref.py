"""NumPy reference of the paged rolling grid (include/lidarslam.h, lslam_grid_recentre_paged,
lslam_grid_page_flush, lslam_grid_page_load), written straight from the definition, cell by cell
sets and no strips: the tests hold the kernels and the strip plan to it bit for bit.

Steps 0 to 3 (robot cell, bad pose, shift, new origin) are tests/recentre_ref.py's.  Python integers
stand for the definition's 64-bit arithmetic; win is stored as int32.
"""
import numpy as np

import recentre_ref as rr

LOST = 1


def on_canvas(W, Cw, wx, wy):
    """bool [W, W] (row y): window cell (x, y) is on the canvas."""
    x = int(wx) + np.arange(W, dtype=np.int64)
    y = int(wy) + np.arange(W, dtype=np.int64)
    return ((y >= 0) & (y < Cw))[:, None] & ((x >= 0) & (x < Cw))[None, :]


def leaving(W, sx, sy):
    """bool [W, W]: window cell (x, y) whose destination (x - sx, y - sy) is off the window."""
    c = np.arange(W, dtype=np.int64)
    keep_x, keep_y = (c - sx >= 0) & (c - sx < W), (c - sy >= 0) & (c - sy < W)
    return ~(keep_y[:, None] & keep_x[None, :])


def entering(W, sx, sy):
    """bool [W, W]: destination cell (x, y) whose source (x + sx, y + sy) is off the window."""
    return leaving(W, -sx, -sy)


def window_to_canvas(canvas, L, wx, wy, mask):
    """canvas[wy + y][wx + x] = L[y][x] for the cells of mask (all on the canvas), in place."""
    ys, xs = np.nonzero(mask)
    canvas[ys + int(wy), xs + int(wx)] = L[ys, xs]
    return len(ys)


def canvas_to_window(L, canvas, wx, wy, mask):
    ys, xs = np.nonzero(mask)
    L[ys, xs] = canvas[ys + int(wy), xs + int(wx)]
    return len(ys)


def world_view(L, canvas, win):
    """The canvas with the window laid over it."""
    V = np.array(canvas, np.int16)
    window_to_canvas(V, L, win[0], win[1], on_canvas(L.shape[0], V.shape[0], win[0], win[1]))
    return V


def recentre_paged(L, canvas, win, pose, origin, **kw):
    """One robot: L [W, W], canvas [Cw, Cw] int16, win (2,) -> dict of L, canvas, win, moved, page_flags and
    the recentre batch's origin, shift, flags.  The inputs are left as they are."""
    p = rr.params(**kw)
    W = int(p["grid_w"])
    L = np.array(L, np.int16).reshape(W, W)
    canvas = np.array(canvas, np.int16)
    Cw = canvas.shape[0]
    wx, wy = int(win[0]), int(win[1])
    L1, origin1, shift, flags = rr.recentre(L, pose, origin, **kw)  # steps 0 to 3, and step 4 where the source is on the window
    sx, sy = int(shift[0]), int(shift[1])
    out = dict(L=L1, canvas=canvas, win=np.array([wx, wy], np.int32), moved=np.zeros(2, np.int32), page_flags=0,
               origin=origin1, shift=shift, flags=flags)
    if sx == 0 and sy == 0:
        return out
    # 2. store
    leave, on = leaving(W, sx, sy), on_canvas(W, Cw, wx, wy)
    stored = window_to_canvas(canvas, L, wx, wy, leave & on)
    lost = bool((leave & ~on).any())
    # 3. the entering cells (rr.recentre left them 0)
    enter, on1 = entering(W, sx, sy), on_canvas(W, Cw, wx + sx, wy + sy)
    assert not L1[enter].any()
    loaded = canvas_to_window(L1, canvas, wx + sx, wy + sy, enter & on1)
    # 4.
    out.update(win=np.array([wx + sx, wy + sy], np.int64).astype(np.int32), moved=np.array([stored, loaded], np.int32),
               page_flags=LOST if lost else 0)
    return out


def recentre_paged_batch(L, canvas, win, pose, origin, **kw):
    """R robots -> dict of stacked arrays."""
    pose = np.asarray(pose, np.float64).reshape(-1, 3)
    R = len(pose)
    origin = np.asarray(origin, np.float64).reshape(R, 2)
    win = np.asarray(win).reshape(R, 2)
    outs = [recentre_paged(L[r], canvas[r], win[r], pose[r], origin[r], **kw) for r in range(R)]
    res = {k: np.stack([np.asarray(o[k]) for o in outs]) for k in outs[0]}
    res["page_flags"] = res["page_flags"].astype(np.int32)
    res["flags"] = res["flags"].astype(np.int32)
    return res


def flush(L, canvas, win):
    """One robot -> (canvas', moved)."""
    canvas = np.array(canvas, np.int16)
    n = window_to_canvas(canvas, L, win[0], win[1], on_canvas(L.shape[0], canvas.shape[0], win[0], win[1]))
    return canvas, np.array([n, 0], np.int32)


def load(canvas, win, W):
    """One robot -> (L, moved)."""
    L = np.zeros((W, W), np.int16)
    n = canvas_to_window(L, np.asarray(canvas, np.int16), win[0], win[1], on_canvas(W, canvas.shape[0], win[0], win[1]))
    return L, np.array([0, n], np.int32)
