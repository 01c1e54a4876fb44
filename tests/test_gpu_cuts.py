"""The consensus's box terms, cutoffs and owning scan computed ahead (cut_lane_kernel, launched with
seed_kernel on the seeding stream in a fresh-stream pipeline call) against the consensus computing
them itself (explicit draws: no seeding, so no cut kernel): the same draws through both paths must
give byte-identical masks, chunk records and trial counts.  The batches are ragged (chunk sizes
1..128, scans of 0..9 chunks), so the cut kernel's owning-scan search leaves its proportional
guess, and one batch is polar (points converted on load in both kernels).  Repeated calls on one
pipeline cycle the four-buffer cut ring.

test_points_rewritten_between_calls: the cut kernel runs on the seeding stream, which waits for
what the producer reads and not for the points.  The points of one pipeline are rewritten between
calls without a host sync -- by a device copy, or by lslam_polar_to_xy -- behind a 1 GiB copy that
keeps the rewrite pending while the next call is enqueued; a cut kernel that read them then would
see the previous set, whose box is 256 times smaller or larger.  Every call must give the results
of the set it was given (explicit draws, synced on both sides).  The planner's decision itself is
pinned without a GPU in test_hazards.py (points_copied, points_written)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def _ragged(rng, S):
    per = rng.integers(0, 10, S)
    per[0] = max(per[0], 1)
    sco = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
    C = int(sco[-1])
    sizes = rng.integers(1, 129, C)
    sizes[rng.random(C) < 0.6] = 100  # mostly C3-sized chunks, ragged around them
    cpo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return sco, cpo


def _walls(rng, cpo):
    """Per chunk: a noisy segment of a line plus a few outliers (mm)."""
    P = int(cpo[-1])
    xy = np.empty((P, 2))
    for c in range(len(cpo) - 1):
        p0, p1 = cpo[c], cpo[c + 1]
        n = p1 - p0
        ang = rng.uniform(0, np.pi)
        t = np.linspace(-1500, 1500, n)
        o = rng.uniform(-4000, 4000, 2)
        pts = o + np.outer(t, [np.cos(ang), np.sin(ang)]) + rng.normal(0, 8, (n, 2))
        k = rng.random(n) < 0.15
        pts[k] += rng.normal(0, 600, (int(k.sum()), 2))
        xy[p0:p1] = pts
    return xy


def _fields(r):
    m = r["models"]
    return r["mask"].tobytes(), m.tobytes(), r["counts"].tobytes()


@pytest.mark.parametrize("polar", [False, True])
def test_precomputed_cuts_equal_in_kernel(ctx, polar):
    from lidar_slam_amd import pipeline as pl
    rng = np.random.default_rng(7 + polar)
    S = 600
    sco, cpo = _ragged(rng, S)
    xy = _walls(rng, cpo)
    kw = dict(max_trials=100, want_counts=True, want_yproj=False)
    if polar:
        th = np.degrees(np.arctan2(xy[:, 1], xy[:, 0]))
        dd = np.hypot(xy[:, 0], xy[:, 1])
        pts = dict(xy=None, theta_deg=th, dist_mm=dd)
    else:
        pts = dict(xy=xy)
    seeds = rng.integers(0, 2**32, S, dtype=np.uint64).astype(np.uint32)
    mt = pl.ScanPipeline(ctx, scan_chunk_off=sco, chunk_pt_off=cpo, seeds=seeds, want_draws=True, **pts, **kw)
    runs = []
    for _ in range(6):  # the cut ring has four buffers: wrap it
        mt.run(sync=False)
        ctx.sync()
        runs.append(mt.results())
    a = runs[0]
    for r in runs[1:]:
        assert _fields(r) == _fields(a)
    ex = pl.ScanPipeline(ctx, scan_chunk_off=sco, chunk_pt_off=cpo, hyp="explicit", hyp_draws=a["draws"], **pts, **kw)
    ex.run()
    b = ex.results()
    assert a["mask"].tobytes() == b["mask"].tobytes()
    assert a["counts"].tobytes() == b["counts"].tobytes()
    am, bm = a["models"], b["models"]
    for f in am.dtype.names:
        assert am[f].tobytes() == bm[f].tobytes(), f


REWRITE_S, REWRITE_CHUNKS, REWRITE_N = 2048, 7, 100


@pytest.fixture(scope="module")
def rewrite_sets(ctx):
    """The two point sets of test_points_rewritten_between_calls (2048 scans x 7 chunks of 100 points),
    the seeds and the MT draws of that shape (a synced call: the draws depend on seeds and sizes
    only), and two unrelated 1 GiB device buffers."""
    from lidar_slam_amd import pipeline as pl
    rng = np.random.default_rng(23)
    S, K, N = REWRITE_S, REWRITE_CHUNKS, REWRITE_N
    sco = (np.arange(S + 1) * K).astype(np.int32)
    cpo = (np.arange(S * K + 1) * N).astype(np.int32)
    wide = _walls(rng, cpo)
    # the same walls scaled by 1/256 about each chunk's own origin (its centroid): boxes of a few mm
    cen = np.repeat(wide.reshape(S * K, N, 2).mean(1), N, axis=0)
    tight = cen + (wide - cen) / 256.0
    seeds = rng.integers(0, 2**32, S, dtype=np.uint64).astype(np.uint32)
    mt = pl.ScanPipeline(ctx, wide, sco, cpo, seeds=seeds, max_trials=100, want_draws=True, want_yproj=False)
    mt.run()
    draws = mt.results()["draws"]
    big = [ctx.empty(1 << 30, np.uint8) for _ in range(2)]
    yield dict(sco=sco, cpo=cpo, seeds=seeds, draws=draws, sets=[tight, wide], big=big)
    for b in big:
        b.free()


def _polar(xy):
    return np.degrees(np.arctan2(xy[:, 1], xy[:, 0])), np.hypot(xy[:, 0], xy[:, 1])


@pytest.mark.parametrize("form", ["xy", "polar", "polar_to_xy"])
def test_points_rewritten_between_calls(ctx, rewrite_sets, form):
    from lidar_slam_amd import _lib
    from lidar_slam_amd import pipeline as pl
    g = rewrite_sets
    sco, cpo, big = g["sco"], g["cpo"], g["big"]
    P = int(cpo[-1])
    kw = dict(max_trials=100, want_counts=True, want_yproj=False)
    L = _lib.load()
    # per set: the staged device arrays and what the pipeline reads of them on the host side
    staged, expected = [], []
    for xy in g["sets"]:
        if form == "xy":
            pts = dict(xy=xy)
            staged.append([ctx.to_device(xy)])
        else:
            th, dd = _polar(xy)
            staged.append([ctx.to_device(th), ctx.to_device(dd)])
            pts = dict(xy=None, theta_deg=th, dist_mm=dd) if form == "polar" else dict(xy=pl.polar_to_xy(ctx, th, dd))
        ex = pl.ScanPipeline(ctx, scan_chunk_off=sco, chunk_pt_off=cpo, hyp="explicit", hyp_draws=g["draws"], **pts, **kw)
        ex.run()
        expected.append(ex.results())
        del ex
    assert _fields(expected[0]) != _fields(expected[1])
    if form == "xy":
        mt = pl.ScanPipeline(ctx, g["sets"][1], sco, cpo, seeds=g["seeds"], **kw)
        dst = [mt.inputs["xy"]]
    elif form == "polar":
        th, dd = _polar(g["sets"][1])
        mt = pl.ScanPipeline(ctx, None, sco, cpo, seeds=g["seeds"], theta_deg=th, dist_mm=dd, **kw)
        dst = [mt.inputs["theta_deg"], mt.inputs["dist_mm"]]
    else:
        dev_xy = ctx.empty((P, 2), np.float64)
        dev_xy.fill_zero()
        mt = pl.ScanPipeline(ctx, dev_xy, sco, cpo, seeds=g["seeds"], **kw)
    ctx.sync()
    for call in range(6):  # tight, wide, ...: every call's points differ from the call before; the cut ring wraps
        k = call & 1
        ctx.copy(big[1], big[0])  # keeps the rewrite behind it pending while the call is enqueued
        if form == "polar_to_xy":
            _lib.check(L.lslam_polar_to_xy(ctx.handle, staged[k][0].ptr, staged[k][1].ptr, dev_xy.ptr, P), "lslam_polar_to_xy")
        else:
            for d, s in zip(dst, staged[k]):
                ctx.copy(d, s)
        mt.run(sync=False)
        ctx.sync()
        r, e = mt.results(), expected[k]
        assert r["mask"].tobytes() == e["mask"].tobytes(), (form, call)
        assert r["counts"].tobytes() == e["counts"].tobytes(), (form, call)
        for f in r["models"].dtype.names:
            assert r["models"][f].tobytes() == e["models"][f].tobytes(), (form, call, f)
