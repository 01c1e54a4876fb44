"""Grow-only device buffers of the context (DevBuf, csrc/lslam_ctx.h): a larger batch on a used
context frees and reallocates scratch that earlier calls, still in flight, read and write.  One
context runs small, larger and small batches again with no host sync between the runs; every
result must equal, byte for byte, the same batch on a fresh context.  The seed states alternate
between two buffers and the chunk cutoffs go round a ring of four, so the MT shapes run four
small and four larger calls before the last small one: every one of those buffers grows while
used.  Then the context is destroyed and a new one repeats the first run.  The two map-side buffers,
the score volume of the matchers (mscr) and the relocalisation's scratch (rscr), grow under
device-staged calls of their own: small, large, small, no host sync between the calls."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _context():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def _synth_batch(n_scans):
    from lidar_slam_amd import synth
    return synth.make_batch(list(range(n_scans)))


def _one_big_chunk_batch(n_scans, n=200):
    """One chunk of n > 128 points per scan: the model / count / select kernels and their scratch."""
    from lidar_slam_amd import synth
    xy = [synth.polar_to_xy_ref(*synth.scan_polar(100 + s, n_beams=n)[:2]) for s in range(n_scans)]
    off = np.arange(n_scans + 1, dtype=np.int32)
    return {"xy": np.ascontiguousarray(np.concatenate(xy)), "scan_chunk_off": off, "chunk_pt_off": off * n}


def _pipeline(ctx, b):
    from lidar_slam_amd.pipeline import ScanPipeline
    S = len(b["scan_chunk_off"]) - 1
    return ScanPipeline(ctx, b["xy"], b["scan_chunk_off"], b["chunk_pt_off"], seeds=np.arange(S, dtype=np.uint32),
                        want_state=True)


def _mt_bytes(p):
    r = p.results()
    return r["mask"].tobytes(), r["models"].tobytes(), r["mt_state"].tobytes()


def _fresh(fn, *args):
    """fn on a context of its own."""
    ctx = _context()
    try:
        return fn(ctx, *args)
    finally:
        gc.collect()
        ctx.close()


def _run_mt(ctx, batches):
    ps = [_pipeline(ctx, b) for b in batches]  # (the uploads sync; the runs below do not)
    for p in ps:
        p.run(sync=False)
    ctx.sync()
    return [_mt_bytes(p) for p in ps]


def _check_mt(ctx, small, large):
    ref = {id(b): _fresh(_run_mt, [b])[0] for b in (small, large)}
    order = [small] * 4 + [large] * 4 + [small]
    for i, (b, got) in enumerate(zip(order, _run_mt(ctx, order))):
        for name, x, y in zip(("mask", "models", "mt_state"), got, ref[id(b)]):
            assert x == y, "run %d (%d scans): %s differs from a fresh context" % (i, len(b["scan_chunk_off"]) - 1, name)


def _express_bytes(rv):
    rv.fetch()
    return (rv.n_scans, rv.n_chunks, rv.n_points, rv.resume, rv.scan_chunk_off.tobytes(), rv.chunk_pt_off.tobytes(),
            rv.xy_host().tobytes())


def _run_express(ctx, streams):
    from lidar_slam_amd.express import ExpressRevolutions
    rvs = [ExpressRevolutions(ctx, len(pk)) for pk in streams]
    for rv, pk in zip(rvs, streams):
        rv.upload(pk)
    for rv in rvs:
        rv.launch()
    ctx.sync()
    return [_express_bytes(rv) for rv in rvs]


def _staged(ctx, rev):
    """A revolution per robot staged on the device (the form ``LandmarkMap.upload`` returns): no call
    that is given one uploads points or waits for the host."""
    from lidar_slam_amd.slam import MapInput
    inp = MapInput()
    inp.sco, inp.cpo = np.ascontiguousarray(rev["scan_chunk_off"], np.int32), np.ascontiguousarray(rev["chunk_pt_off"], np.int32)
    inp.xy = ctx.to_device(np.ascontiguousarray(rev["xy"], np.float64))
    inp.off = ctx.to_device(np.ascontiguousarray(inp.cpo[inp.sco], np.int32))  # the scan matcher's point offsets
    return inp


MATCH_SMALL, MATCH_LARGE = dict(grid_w=256, k_trans=1, k_theta=1), dict(grid_w=256)  # 3 x 3 x 3 and 41 x 21 x 21 scores a robot


def _run_match(ctx, revs, kws):
    """One ``ScanMatcher`` per entry of kws, every one matching revolution 0 -> 1 into the context's own
    score volume (no ``scores`` given), no host sync between the calls."""
    from lidar_slam_amd.odometry import ScanMatcher
    R = len(revs[0]["scan_chunk_off"]) - 1
    a, b = _staged(ctx, revs[0]), _staged(ctx, revs[1])
    ms = [ScanMatcher(ctx, R, **kw) for kw in kws]
    ctx.sync()
    for m in ms:
        m.match(a.xy, a.off, b.xy, b.off, sync=False)
    ctx.sync()
    return [tuple(sorted((k, v.tobytes()) for k, v in m.results().items())) for m in ms]


def test_score_volume_regrows_under_a_running_pick():
    """``mscr``, the score volume of a scan-match or scan-to-map call: 27 scores a robot, then 18081,
    then 27 again.  The grow frees the volume that the first call's pick kernel may still read."""
    from test_occgrid_ref import room_run
    revs = room_run()[1]
    ref = {"small": _fresh(_run_match, revs, [MATCH_SMALL])[0], "large": _fresh(_run_match, revs, [MATCH_LARGE])[0]}
    assert ref["small"] != ref["large"]
    got = _fresh(_run_match, revs, [MATCH_SMALL, MATCH_LARGE, MATCH_SMALL])
    for i, name in enumerate(("small", "large", "small")):
        assert got[i] == ref[name], "match %d (%s) differs from a fresh context" % (i, name)


RELOC_MAPS = (dict(grid_w=64, cell=80.0), dict(grid_w=256, cell=20.0))  # the same 5.12 m, 16 and 64 coarse cells a side


def _run_reloc(ctx, room, which, budget):
    """One grid and one ``GridRelocalizer`` per entry of which (an index into RELOC_MAPS), the grids drawn
    from the true poses; then every relocalisation with no host sync between the calls, each into the
    context's own coarse volume (no ``want_coarse``)."""
    from lidar_slam_amd.localize import GridRelocalizer
    from lidar_slam_amd.mapping import OccupancyGrid
    from test_occgrid_ref import ROOM_ORIGIN
    poses, revs = room
    R = poses.shape[1]
    inps = [_staged(ctx, rev) for rev in revs]
    grids, rels = [], []
    for i in which:
        g = OccupancyGrid(ctx, R, origin=ROOM_ORIGIN, **RELOC_MAPS[i])
        for k, inp in enumerate(inps[:4]):
            g.step(inp, pose=poses[k])
        grids.append(g)
        rels.append(GridRelocalizer(ctx, R, win_w=RELOC_MAPS[i]["grid_w"]))
    if budget:
        rels[0].set_budget(budget)
    ctx.sync()
    for g, rel in zip(grids, rels):
        rel.relocalize(inps[4], grid=g, sync=False)
    ctx.sync()
    return [tuple(sorted((k, v.tobytes()) for k, v in rel.results().items())) for rel in rels]


@pytest.mark.parametrize("budget", [0, 3 * 180 * 64 * 64 * 4], ids=["one chunk", "chunks of three robots"])
def test_reloc_scratch_regrows_under_a_running_search(budget):
    """``rscr``, the relocalisation's coarse volume and peak keys: a 64-cell map, a 256-cell map, the
    64-cell map again.  With the small budget the 256-cell call runs its eight robots in chunks of
    three, three and two, each reusing the volume that the chunk before it has just read."""
    from test_occgrid_ref import room_run
    room = room_run()
    ref = [_fresh(_run_reloc, room, [i], budget)[0] for i in (0, 1)]
    assert ref[0] != ref[1]
    got = _fresh(_run_reloc, room, [0, 1, 0], budget)
    for i, j in enumerate((0, 1, 0)):
        assert got[i] == ref[j], "relocalisation %d (%d cells) differs from a fresh context" % (i, RELOC_MAPS[j]["grid_w"])


def test_buffers_regrow_under_running_work_and_context_recreate(golden):
    small, large = _synth_batch(4), _synth_batch(64)
    first = _fresh(_run_mt, [small])[0]
    ctx = _context()
    try:
        # producer slots, seed states, chunk cutoffs, draws scratch, replay flags
        _check_mt(ctx, small, large)
        # large-chunk consensus scratch
        _check_mt(ctx, _one_big_chunk_batch(4), _one_big_chunk_batch(32))
        # express revolution scratch
        pk = golden("express.npz")["capA_packets"]
        streams = [pk[:40], pk, pk[:40]]
        ref = [_fresh(_run_express, [s])[0] for s in streams[:2]]
        assert ref[0][0] >= 1 and ref[1][0] > ref[0][0]
        got = _run_express(ctx, streams)
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[0]
    finally:
        gc.collect()
        ctx.close()
    # a new context on the same device after the destroy
    assert _fresh(_run_mt, [small])[0] == first
