"""The stream-order contract of the map side (include/lidarslam.h: every entry point is asynchronous on
the context, a later call sees an earlier call's outputs), held with ``sync=False`` throughout.

Every map-side entry point is held bit for bit to its NumPy definition elsewhere, one call and one host
sync at a time.  Here the calls run back to back on device-staged revolutions (``LandmarkMap.upload``,
so no call uploads points and none waits for the host), and every compared byte must equal the same
calls on a fresh context with a host sync after each.  The room is ``room_run()`` of
tests/test_occgrid_ref.py: eight robots, five revolutions, 256-cell grids.

a. The revolution loop of the README, nine calls a revolution, all state snapshot per revolution with
   device-to-device copies on the stream, for both hypothesis sources; the synced twin is also held to
   the definitions at the last revolution (a loop that is wrong in both orders must not pass).  A
   counter on ``ctx.sync`` holds the loop to no host sync at all after the warm-up revolution.
b. The two regimes of the hazard planner (csrc/lslam_hazards.h).  Distinct (pointer, length) ranges
   that the launchers register, read from ``note_outs``, ``remember_outputs`` and ``lslam_h2d`` /
   ``lslam_d2d`` / ``lslam_memset``, counted over a context's life because the ``outs`` set is emptied
   only by a producer that waits for ``ev_call``:
   * the loop of (a), per revolution: scan match 5 (delta, best, n_valid, flags, lm.u), pipeline 8
     (mask, models, the two MT states, landmarks, lmk_count, x, P), recentre 4 (logodds, origin, shift,
     flags), grid update 3 more (rot, n_used, flags), distance 3, ray cast 3, score 4, map fuse 9 (delta,
     best, n_valid, rot0, flags, z, Rm, nis, moments; pose_out and P_out are x and P again, the scratch
     volume is not registered), field fuse 10 (z, trace, normal, n_used, iters, flags, info, info_f, s2,
     nis): 49 with MT19937 (the Philox source has no producer, so no planner).  The first revolution
     matches nothing and registers 44; the second one's scan match brings the 49th, ``outs`` overflows,
     the producer of the ``lm.step`` behind it waits for ``ev_call`` and empties the set, the calls up
     to the next scan match fill it again: from the second revolution on every producer waits.  The
     snapshots add 40 copy destinations a revolution, beyond the 32 of ``copies``: every producer waits
     for ``ev_copy`` as well.
   * the short loop (``lm.step``, ``field.fuse``): grid update 4 and distance 3 in the set-up,
     pipeline 8, field fuse 10: 25 ranges, below 48, so ``outs`` never overflows and no producer ever
     waits for ``ev_call``.  The first ``lm.step`` waits for ``ev_copy`` (the set-up's uploads) and
     empties ``copies``; after it the loop adds ``field._off`` and five snapshot destinations a
     revolution: 26, below 32.  The MT chain therefore keeps speculating (hazard level 1) while the
     fusions rewrite ``lm.x`` and ``lm.P`` between its calls; it is compared with its synced twin and
     with ``LSLAM_MT_SPECULATE=0``.
c. Writer -> reader pairs, each behind a ballast: one ``lslam_grid_distance`` of a separate one-robot
   grid that touches nothing else, enqueued first so that the stream's tail is ahead of the host when
   the pair is enqueued.  Before the writer its destinations hold the previous revolution's valid
   values: an early read gives a wrong but plausible result.

   The ballast against the enqueue, measured on an MI355X.  ``lslam_grid_distance`` has no timing slot
   (``lslam_timing`` knows ids 0..15, none of them the transform's: tools/distbench.py), so the ballast
   is timed as that tool times it, back-to-back calls between two host syncs; the enqueue time is the
   host clock around a pair's calls.  One robot at 1024 cells and d_max 64 takes 0.78 ms, at 2048 and
   d_max 40 0.41 ms, at 2048 and d_max 64 2.76 ms, at 2048 and d_max 128 3.0 ms: too short.  The
   ballast here is 2048 cells, d_max 160, one source every 389 x 381 cells (the search goes wide): 4.48
   ms.  A pair is enqueued in 58 us (recentre -> grid.step) to 165 us (relocalize -> lm.step); the
   slowest ever seen was 332 us (odo.step -> lm.step, the first pair of a process).  The ballast is 27
   times the usual slowest pair and 13 times the slowest seen.  test_ballast_outlasts_the_enqueue prints
   both figures.
"""
import ctypes as C
import gc
import os
import time

import numpy as np
import pytest

import dist_ref as dr
import fieldfuse_ref as ffr
import occgrid_ref as ogr
from test_fieldscore_ref import ROOM_DIST
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, room_run

pytestmark = pytest.mark.gpu

LOOSE = dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)  # the association tolerances of the end-to-end tests
P0, RD = np.diag([25.0, 25.0, 1e-4]), [25.0, 1e-4] * 8
FUSE_KEYS = ("flags", "iters", "n_used", "normal", "trace", "z", "s2", "info", "info_f", "nis", "pose_out", "P_out")

BALLAST_W, BALLAST_DMAX, BALLAST_EVERY = 2048, 160, 389  # (c) of the module's docstring


def fresh_context():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def waiting_context():
    """A context whose MT producer never speculates (LSLAM_MT_SPECULATE=0 is read at its creation)."""
    old = os.environ.get("LSLAM_MT_SPECULATE")
    os.environ["LSLAM_MT_SPECULATE"] = "0"
    try:
        return fresh_context()
    finally:
        if old is None:
            del os.environ["LSLAM_MT_SPECULATE"]
        else:
            os.environ["LSLAM_MT_SPECULATE"] = old


def on_fresh(make, fn, *args):
    """fn on a context of its own; what fn allocated is freed before the context goes."""
    ctx = make()
    try:
        return fn(ctx, *args)
    finally:
        gc.collect()
        ctx.close()


@pytest.fixture(scope="module")
def room():
    return room_run()


class SyncCounter:
    """Counts ``ctx.sync()``: every object syncs through its context's method, so wrapping the instance
    attribute sees them all (uploads and downloads included)."""

    def __init__(self, ctx):
        self.n = 0
        real = ctx.sync

        def counted():
            self.n += 1
            real()
        ctx.sync = counted


class Snap:
    """State snapshots.  On the stream: device-to-device copies into an arena allocated before the loop,
    read back after the last sync.  Synced: a download on the spot."""

    def __init__(self, ctx, on_stream, nbytes=16 << 20):
        self.ctx, self.on_stream, self.top, self.index, self.got = ctx, on_stream, 0, [], {}
        self.arena = ctx.empty(nbytes, np.uint8) if on_stream else None

    def take(self, tag, items):
        for name, a, n in items:
            if self.on_stream:
                off = self.top
                self.top += (n + 255) & ~255
                assert self.top <= self.arena.nbytes, "snapshot arena too small"
                self.ctx.copy(self.arena.addr + off, a, n)
                self.index.append(((tag, name), off, n))
            else:
                out = np.empty(n, np.uint8)
                from lidar_slam_amd import _lib
                _lib.check(self.ctx._L.lslam_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), a.ptr, n), "lslam_d2h")
                self.ctx.sync()
                self.got[(tag, name)] = out.tobytes()

    def fetch(self):
        """After the caller's sync: {(tag, name): bytes}."""
        if self.on_stream:
            h = self.arena.download()
            self.got = {k: h[off:off + n].tobytes() for k, off, n in self.index}
        return self.got


class Rig:
    """The objects of the revolution loop on one context, the five revolutions staged on the device."""

    def __init__(self, ctx, room, hyp="mt19937", extras=False, odo_kw=None, field_kw=None):
        from lidar_slam_amd.localize import GridLocalizer, GridRelocalizer
        from lidar_slam_amd.mapping import DistanceField, GridRayCaster, OccupancyGrid
        from lidar_slam_amd.odometry import LidarOdometry
        from lidar_slam_amd.slam import LandmarkMap
        self.ctx, self.hyp = ctx, hyp
        self.poses, self.revs = room
        R = self.R = len(ROOM_ROBOTS)
        self.lm = LandmarkMap(ctx, R, lmk_capacity=256, seeds=ROOM_ROBOTS, x0=self.poses[0], P0=P0, R_diag=RD, hyp=hyp, **LOOSE)
        self.odo = LidarOdometry(ctx, R, **(odo_kw or {}))
        self.grid = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **ROOM_KW)
        self.field = DistanceField(self.grid, **dict(ROOM_DIST, **(field_kw or {})))
        self.caster = GridRayCaster(self.grid)
        self.loc = GridLocalizer(ctx, R)
        self.reloc = GridRelocalizer(ctx, R) if extras else None
        self.inp = [self.lm.upload(r["xy"], r["scan_chunk_off"], r["chunk_pt_off"]) for r in self.revs]
        self.P = int(self.revs[0]["chunk_pt_off"][-1])
        assert all(int(r["chunk_pt_off"][-1]) == self.P for r in self.revs)  # no staging buffer grows after the first

    def revolution(self, k, sync, before_grid=None, after_field=None, before_fuse=None):
        """The nine calls of the README's loop on revolution k; the hooks are the synced twin's reads."""
        inp, lm, grid, field = self.inp[k], self.lm, self.grid, self.field
        self.odo.step(inp, lm=lm, sync=sync)
        lm.step(inp, sync=sync)
        grid.recentre(pose=lm, margin=128, quantum=8, sync=sync)
        if before_grid:
            before_grid()
        grid.step(inp, pose=lm, sync=sync)
        field.step(sync=sync)
        if after_field:
            after_field()
        self.caster.step(inp, pose=lm, sync=sync)
        field.score(inp, pose=lm, sync=sync)
        self.loc.fuse(inp, grid=grid, lm=lm, sync=sync)
        if before_fuse:
            before_fuse()
        field.fuse(inp, lm=lm, sync=sync)

    def filter_state(self):
        lm, R = self.lm, self.R
        out = [("lm.x", lm.x, 24 * R), ("lm.P", lm.P, 72 * R), ("landmarks", lm.landmarks, lm.landmarks.nbytes),
               ("lmk_count", lm.lmk_count, 4 * R)]
        if self.hyp == "mt19937":
            out.append(("mt_state", lm._mt[0], 2500 * R))
        return out

    def state(self):
        """(name, device array, bytes) of everything the loop leaves behind; the bytes are what the calls
        write (the trace holds n_iter + 1 rows of its 33, the class buffer P bytes)."""
        lm, grid, field, caster, loc, R = self.lm, self.grid, self.field, self.caster, self.loc, self.R
        out = self.filter_state() + [("lm.u", lm.u, 16 * R)]
        out += [("logodds", grid.logodds, grid.logodds.nbytes), ("origin", grid.origin, 16 * R), ("grid.rot", grid.rot, 16 * R),
                ("grid.n_used", grid.n_used, 8 * R), ("grid.flags", grid.flags, 4 * R), ("shift", grid._shift, 8 * R),
                ("recentre.flags", grid._rflags, 4 * R)]
        out += [("d2", field.d2, field.d2.nbytes), ("n_src", field.n_src, 4 * R)]
        a, f = field._align, field._fuse
        out += [("fuse.trace", a["trace"], R * (int(field.a.n_iter) + 1) * 40), ("fuse.normal", a["normal"], 80 * R),
                ("fuse.n_used", a["n_used"], 12 * R), ("fuse.iters", a["iters"], 4 * R), ("fuse.flags", a["flags"], 4 * R),
                ("fuse.z", f["z"], 24 * R), ("fuse.info", f["info"], 72 * R), ("fuse.info_f", f["info_f"], 72 * R),
                ("fuse.s2", f["s2"], 8 * R), ("fuse.nis", f["nis"], 8 * R)]
        m = loc._fused
        out += [("loc.delta", loc.delta, 24 * R), ("loc.best", loc.best, 16 * R), ("loc.n_valid", loc.n_valid, 8 * R),
                ("loc.rot0", loc.rot0, 16 * R), ("loc.flags", loc.flags, 4 * R), ("loc.z", m["z"], 24 * R),
                ("loc.Rm", m["Rm"], 72 * R), ("loc.nis", m["nis"], 8 * R), ("loc.moments", m["moments"], 80 * R)]
        out += [("cls", caster._cls.buf, self.P), ("counts", caster.counts, 32 * R), ("caster.flags", caster.flags, 4 * R)]
        out += [("stats", field.stats, 32 * R), ("clear2", field.clear2, 4 * R), ("score.flags", field.score_flags, 4 * R)]
        return out


def as_array(got, key, dtype, shape):
    return np.frombuffer(got[key], dtype).reshape(shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_runs(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, "%s: %d of %d snapshots differ, first %s" % (what, len(bad), len(a), sorted(bad)[:6])


# ---- a. the whole loop ----

def run_loop(ctx, room, hyp, sync, check=False):
    """The five revolutions; {(revolution, name): bytes}.  Unsynced: revolution 0 is the warm-up (first
    allocations, the scratch's growth, the odometry's first store) and ends with one sync; from then to
    the end of the loop nothing may sync."""
    rig = Rig(ctx, room, hyp)
    snap = Snap(ctx, on_stream=not sync)
    counter = SyncCounter(ctx)
    last = len(rig.inp) - 1
    for k in range(last + 1):
        hooks = reference_hooks(rig, k) if check and k == last else {}
        rig.revolution(k, sync, **hooks)
        snap.take(k, rig.state())
        if k == 0 and not sync:
            ctx.sync()
            counter.n = 0
    if not sync:
        assert counter.n == 0, "%d host syncs in the unsynced revolutions 1..%d" % (counter.n, last)
        ctx.sync()
    if check:
        assert_fuse_reference(rig, last)
    return snap.fetch()


def reference_hooks(rig, k):
    """The synced twin at revolution k against the definitions, each fed the device's own inputs."""
    rev, grid, field, lm, R = rig.revs[k], rig.grid, rig.field, rig.lm, rig.R
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    seen = {}

    def before_grid():
        seen["L"], seen["pose"], seen["origin"] = grid.logodds.download(), lm.x.download(), grid.origin_host.copy()

    def after_field():
        L = grid.logodds.download()
        want = ogr.update_batch(seen["L"], rev["xy"], off, seen["pose"], grid.rot.download(), seen["origin"], **ROOM_KW)[0]
        assert np.array_equal(L, want), "grid.logodds differs from occgrid_ref"
        seen["d2"] = dr.field_batch(L, **ROOM_DIST)[0]
        assert np.array_equal(field.d2.download(), seen["d2"]), "d2 differs from dist_ref"

    def before_fuse():
        seen["x"], seen["P"] = lm.x.download(), lm.P.download().reshape(R, 3, 3)

    rig.seen = seen
    return dict(before_grid=before_grid, after_field=after_field, before_fuse=before_fuse)


def assert_fuse_reference(rig, k):
    rev, seen, R = rig.revs[k], rig.seen, rig.R
    res = rig.field.fuse_results()
    want = ffr.fuse_batch(seen["d2"], rev["xy"], rev["chunk_pt_off"][rev["scan_chunk_off"]], seen["x"], seen["P"], res["trace"],
                          rig.grid.origin_host, ROOM_KW, **ROOM_DIST)
    for key in FUSE_KEYS:
        assert same_bits(np.asarray(res[key]), np.asarray(want[key]).astype(res[key].dtype)), "field.fuse %s differs from fieldfuse_ref" % key
    assert same_bits(rig.lm.x.download(), res["pose_out"]) and same_bits(rig.lm.P.download().reshape(R, 3, 3), res["P_out"])


@pytest.mark.parametrize("hyp", ["mt19937", "philox"])
def test_whole_loop_unsynced_equals_synced(room, hyp):
    """(a) of the module's docstring.  The closed loop's pose error against the true poses is printed and
    not capped (no cap has been derived for it); measured on an MI355X after five revolutions: at most
    4.72 mm and 2.83 mrad with MT19937, 4.72 mm and 4.81 mrad with Philox, all eight robots updated by
    both fusions in every revolution."""
    from lidar_slam_amd import _lib
    R, K = len(ROOM_ROBOTS), len(room[1])
    loose_run = on_fresh(fresh_context, run_loop, room, hyp, False)
    synced = on_fresh(fresh_context, run_loop, room, hyp, True, True)
    assert_same_runs(loose_run, synced, "unsynced against synced, %s" % hyp)
    for k in range(K):
        for name, mask in (("grid.flags", _lib.GRID_BAD_POSE), ("recentre.flags", _lib.RECENTRE_BAD_POSE),
                           ("caster.flags", _lib.RAYCAST_BAD_POSE), ("score.flags", _lib.FIELD_BAD_POSE),
                           ("loc.flags", _lib.MAPMATCH_BAD_POSE | _lib.MAPFUSE_BAD_COV),
                           ("fuse.flags", _lib.FIELDALIGN_BAD_POSE | _lib.FIELDFUSE_BAD_COV)):
            f = as_array(synced, (k, name), np.int32, (R,))
            assert not (f & mask).any(), (k, name, f)
    assert any(as_array(synced, (k, "shift"), np.int32, (R, 2)).any() for k in range(K))  # the grids did roll
    from lidar_slam_amd.localize import MAPMATCH_BAD_POSE, MAPMATCH_EMPTY, MAPMATCH_WEAK
    from lidar_slam_amd.mapping import FIELDFUSE_REJECTED
    kept = {"loc.flags": MAPMATCH_EMPTY | MAPMATCH_WEAK | MAPMATCH_BAD_POSE | _lib.MAPFUSE_OUTLIER | _lib.MAPFUSE_BAD_COV,
            "fuse.flags": FIELDFUSE_REJECTED}
    for name, mask in kept.items():  # both write-backs did write: robots updated per revolution
        n = [int(((as_array(synced, (k, name), np.int32, (R,)) & mask) == 0).sum()) for k in range(K)]
        print(hyp, name, "robots updated per revolution", n)
        assert sum(n[1:]) > 0, (name, n)
    x = as_array(synced, (K - 1, "lm.x"), np.float64, (R, 3))
    Pf = as_array(synced, (K - 1, "lm.P"), np.float64, (R, 3, 3))
    assert same_bits(Pf, Pf.transpose(0, 2, 1)) and np.all(np.linalg.eigvalsh(Pf)[:, 0] > 0)
    err = x - room[0][K - 1]
    print(hyp, "pose error after the closed loop: mm", np.hypot(err[:, 0], err[:, 1]).round(2), "mrad", (1e3 * np.abs(err[:, 2])).round(3))


# ---- b. below the planner's set sizes: the MT chain speculates beside the fusions ----

def run_short_loop(ctx, room, sync):
    # (no gate: this filter claims 5 mm on a map that it did not draw, and the gate would refuse every fusion)
    rig = Rig(ctx, room, field_kw=dict(nis_max=np.inf))
    lm, grid, field = rig.lm, rig.grid, rig.field
    for k, rev in enumerate(rig.revs):  # the map, from the true poses
        grid.step(rig.inp[k], pose=rig.poses[k])
    field.step()
    lm.u.upload(np.tile([146.0, 174.0], (rig.R, 1)))  # the wheel speeds of room_run, once: no odometry here
    ctx.sync()
    snap = Snap(ctx, on_stream=not sync, nbytes=2 << 20)
    counter = SyncCounter(ctx)
    for k in range(len(rig.inp)):
        lm.step(rig.inp[k], sync=sync)
        field.fuse(rig.inp[k], lm=lm, sync=sync)
        snap.take(k, rig.filter_state())
    if not sync:
        assert counter.n == 0, "%d host syncs in the unsynced short loop" % counter.n
        ctx.sync()
    got = snap.fetch()
    res = field.fuse_results()
    for key in FUSE_KEYS:
        got[("last fuse", key)] = np.ascontiguousarray(res[key]).tobytes()
    return got


def test_short_loop_speculates_beside_the_fusions(room):
    runs = {name: on_fresh(make, run_short_loop, room, sync)
            for name, make, sync in (("unsynced", fresh_context, False), ("synced", fresh_context, True),
                                     ("unsynced, LSLAM_MT_SPECULATE=0", waiting_context, False))}
    R, K = len(ROOM_ROBOTS), len(room[1])
    for name in list(runs)[1:]:
        assert_same_runs(runs["unsynced"], runs[name], "unsynced against " + name)
    x = [as_array(runs["synced"], (k, "lm.x"), np.float64, (R, 3)) for k in range(K)]
    assert not same_bits(x[0], x[K - 1])  # the filter did move
    flags = np.frombuffer(runs["synced"][("last fuse", "flags")], np.int32)
    from lidar_slam_amd.mapping import FIELDFUSE_REJECTED
    print("the last fusion's flags", flags)
    assert ((flags & FIELDFUSE_REJECTED) == 0).sum() >= R // 2, flags  # and the fusions did write into it


# ---- c. writer -> reader pairs behind a busy stream ----

class Ballast:
    """One distance transform of a one-robot grid of its own: nothing else reads or writes its buffers."""

    def __init__(self, ctx, W=BALLAST_W, d_max=BALLAST_DMAX, every=BALLAST_EVERY):
        from lidar_slam_amd.mapping import DistanceField, OccupancyGrid
        self.grid = OccupancyGrid(ctx, 1, grid_w=W)
        L = np.full((1, W, W), -100, np.int16)
        L[0, ::every, ::every - 8] = 200  # sparse sources: the search goes wide before it finds one
        self.grid.upload(L)
        self.field = DistanceField(self.grid, d_max=d_max)

    def enqueue(self):
        self.field.step(sync=False)


def pair_rig(ctx, room, odo_kw=None):
    """Four synced revolutions of the loop, every object warm: each destination of the pairs below holds
    the previous revolution's valid values."""
    rig = Rig(ctx, room, extras=True, odo_kw=odo_kw)
    for k in range(4):
        rig.revolution(k, True)
        rig.loc.step(rig.inp[k], grid=rig.grid, pose=rig.lm)
        rig.field.align(rig.inp[k], pose=rig.lm)
    rig.reloc.relocalize(rig.inp[3], grid=rig.grid)
    rig.ballast = Ballast(ctx)
    ctx.sync()
    return rig


def pair_state(rig):
    loc, field, rel, odo, R = rig.loc, rig.field, rig.reloc, rig.odo.matcher, rig.R
    out = rig.state()
    out += [("loc.pose", loc.pose, 24 * R), ("align.pose_out", field._align["pose_out"], 24 * R)]
    out += [("reloc.pose", rel.pose, 24 * R), ("reloc.result", rel.result, 32 * R), ("reloc.flags", rel.flags, 4 * R)]
    out += [("reloc." + n, rel.ranks[n], rel.ranks[n].nbytes) for n, _, _ in rel._PER_RANK]
    out += [("odo.delta", odo.delta, 24 * R), ("odo.best", odo.best, 16 * R), ("odo.flags", odo.flags, 4 * R)]
    return out


def loc_state(rig):
    loc, R = rig.loc, rig.R
    return [("loc.pose", loc.pose, 24 * R), ("loc.delta", loc.delta, 24 * R), ("loc.best", loc.best, 16 * R), ("loc.flags", loc.flags, 4 * R)]


def align_state(rig):
    a, R = rig.field._align, rig.R
    return [("align.pose_out", a["pose_out"], 24 * R), ("align.normal", a["normal"], 80 * R), ("align.flags", a["flags"], 4 * R)]


def odo_state(rig):
    m, R = rig.odo.matcher, rig.R
    return [("odo.delta", m.delta, 24 * R), ("odo.best", m.best, 16 * R), ("lm.u", rig.lm.u, 16 * R)]


def far_pose(rig):
    """Host poses far enough from the grids' centres that a recentre must roll every grid."""
    return rig.poses[4] + np.array([400.0, -240.0, 0.0])


# every pair runs on revolution 4 (k = 4); s: the calls' sync flag; snap: for what a later call overwrites
def _lm(rig, s):
    rig.lm.step(rig.inp[4], sync=s)


def _recentre(rig, s):
    rig.grid.recentre(pose=far_pose(rig), margin=128, quantum=8, sync=s)


def p_odo_lm(rig, s, snap):
    rig.odo.step(rig.inp[4], lm=rig.lm, sync=s)
    _lm(rig, s)


def p_lm_grid(rig, s, snap):
    _lm(rig, s)
    rig.grid.step(rig.inp[4], pose=rig.lm, sync=s)


def p_lm_recentre(rig, s, snap):
    _lm(rig, s)
    rig.grid.recentre(pose=rig.lm, margin=128, quantum=1, sync=s)  # quantum 1: every millimetre of lm.x counts


def p_lm_loc(rig, s, snap):
    _lm(rig, s)
    rig.loc.step(rig.inp[4], grid=rig.grid, pose=rig.lm, write_back=True, sync=s)


def p_lm_caster(rig, s, snap):
    _lm(rig, s)
    rig.caster.step(rig.inp[4], pose=rig.lm, sync=s)


def p_lm_align(rig, s, snap):
    _lm(rig, s)
    rig.field.align(rig.inp[4], pose=rig.lm, sync=s)


def p_fieldfuse_lm(rig, s, snap):
    rig.field.fuse(rig.inp[4], lm=rig.lm, sync=s)
    _lm(rig, s)


def p_locfuse_lm(rig, s, snap):
    rig.loc.fuse(rig.inp[4], grid=rig.grid, lm=rig.lm, sync=s)
    _lm(rig, s)


def p_reloc_lm(rig, s, snap):
    rig.reloc.relocalize(rig.inp[4], grid=rig.grid, lm=rig.lm, sync=s)
    _lm(rig, s)


def p_recentre_grid(rig, s, snap):
    _recentre(rig, s)
    rig.grid.step(rig.inp[4], pose=rig.lm, sync=s)


def p_recentre_field_align(rig, s, snap):
    _recentre(rig, s)
    rig.field.step(sync=s)
    rig.field.align(rig.inp[4], pose=rig.lm, sync=s)


def p_recentre_loc(rig, s, snap):
    _recentre(rig, s)
    rig.loc.step(rig.inp[4], grid=rig.grid, pose=rig.lm, sync=s)


def p_recentre_caster(rig, s, snap):
    _recentre(rig, s)
    rig.caster.step(rig.inp[4], pose=rig.lm, sync=s)


def p_grid_twice(rig, s, snap):
    rig.grid.step(rig.inp[4], pose=rig.poses[4], sync=s)
    snap.take("first", [("grid.rot", rig.grid.rot, 16 * rig.R), ("logodds", rig.grid.logodds, rig.grid.logodds.nbytes)])
    rig.grid.step(rig.inp[4], pose=rig.poses[2], sync=s)


def p_loc_twice(rig, s, snap):
    rig.loc.step(rig.inp[4], grid=rig.grid, pose=rig.poses[4], sync=s)
    snap.take("first", loc_state(rig))
    rig.loc.step(rig.inp[4], grid=rig.grid, pose=rig.poses[2], sync=s)


def p_align_twice(rig, s, snap):
    rig.field.align(rig.inp[4], pose=rig.poses[4], sync=s)
    snap.take("first", align_state(rig))
    rig.field.align(rig.inp[4], pose=rig.poses[2], sync=s)


def p_shared_scratch(rig, s, snap):
    """Three users of the context's score volume in a row, the middle one (the odometry, built with a
    smaller window) with another volume size, none given a ``scores`` of its own."""
    rig.loc.step(rig.inp[4], grid=rig.grid, pose=rig.lm, sync=s)
    snap.take("first", loc_state(rig))
    rig.odo.step(rig.inp[4], lm=rig.lm, sync=s)
    snap.take("second", odo_state(rig))
    rig.loc.fuse(rig.inp[4], grid=rig.grid, lm=rig.lm, sync=s)


PAIRS = [p_odo_lm, p_lm_grid, p_lm_recentre, p_lm_loc, p_lm_caster, p_lm_align, p_fieldfuse_lm, p_locfuse_lm, p_reloc_lm,
         p_recentre_grid, p_recentre_field_align, p_recentre_loc, p_recentre_caster, p_grid_twice, p_loc_twice, p_align_twice,
         p_shared_scratch]
ODO_KW = {p_shared_scratch: dict(k_trans=6, k_theta=12)}


def pair_on(ctx, room, pair, sync):
    rig = pair_rig(ctx, room, ODO_KW.get(pair))
    snap = Snap(ctx, on_stream=True, nbytes=8 << 20)
    counter = SyncCounter(ctx)
    if not sync:
        rig.ballast.enqueue()
    t0 = time.perf_counter()
    pair(rig, sync, snap)
    dt = time.perf_counter() - t0
    if not sync:
        assert counter.n == 0, "%d host syncs inside the unsynced pair" % counter.n
    snap.take("end", pair_state(rig))
    ctx.sync()
    return snap.fetch(), dt


def run_pair(room, pair, sync):
    """On a fresh context: (snapshots, the host seconds that enqueuing the pair took)."""
    return on_fresh(fresh_context, pair_on, room, pair, sync)


def time_ballast(ctx, reps=3):
    b = Ballast(ctx)
    b.enqueue()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        b.enqueue()
    ctx.sync()
    return (time.perf_counter() - t0) / reps


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: p.__name__[2:])
def test_pair_behind_a_busy_stream(room, pair):
    R = len(ROOM_ROBOTS)
    got, dt = run_pair(room, pair, sync=False)
    want, _ = run_pair(room, pair, sync=True)
    print("%s: enqueued in %.0f us" % (pair.__name__[2:], 1e6 * dt))
    assert_same_runs(got, want, pair.__name__[2:])
    if pair.__name__.startswith("p_recentre"):
        from lidar_slam_amd import _lib
        assert (as_array(want, ("end", "recentre.flags"), np.int32, (R,)) & _lib.RECENTRE_MOVED).all()  # the readers had something to follow
    if pair in (p_grid_twice, p_loc_twice, p_align_twice):  # the two poses give two answers: a refilled staging buffer would show
        name = {p_grid_twice: "grid.rot", p_loc_twice: "loc.pose", p_align_twice: "align.pose_out"}[pair]
        assert want[("first", name)] != want[("end", name)]


def test_ballast_outlasts_the_enqueue(room):
    """Prints the two figures of the module docstring's (c): the ballast's time (back-to-back calls
    between two syncs) and three pairs' enqueue times.  The ballast must be at least ten times the
    enqueue time for the pairs to run behind a busy stream."""
    ballast = on_fresh(fresh_context, time_ballast)
    dts = [run_pair(room, pair, sync=False)[1] for pair in (p_odo_lm, p_lm_loc, p_recentre_field_align)]
    print("ballast %.2f ms; three pairs enqueued in %s ms" % (1e3 * ballast, [round(1e3 * dt, 3) for dt in dts]))
    assert ballast >= 10 * min(dts)  # (the quickest: a host that was interrupted once does not fail the suite)
