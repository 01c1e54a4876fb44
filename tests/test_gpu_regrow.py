"""Grow-only device buffers of the context (DevBuf, csrc/lslam_ctx.h): a larger batch on a used
context frees and reallocates scratch that earlier calls, still in flight, read and write.  One
context runs small, larger and small batches again with no host sync between the runs; every
result must equal, byte for byte, the same batch on a fresh context.  The seed states alternate
between two buffers and the chunk cutoffs go round a ring of four, so the MT shapes run four
small and four larger calls before the last small one: every one of those buffers grows while
used.  Then the context is destroyed and a new one repeats the first run."""
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
