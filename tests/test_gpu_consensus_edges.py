"""The large-chunk consensus (model_kernel -> count_kernel<PPL> -> select_kernel) against the CPU
oracle at the edge of every count form: the cases of tests/consensus_edges.py, one batch per launch.

tests/test_consensus_edges.py shows from the oracle alone what each case can see.  Here every
chunk is compared with oracle.cpu.ransac(want_trials=True) on the same points and hypotheses:
per-trial counts (every trial the oracle ran), masks, best_trial / n_draws / flags / n_inliers, and
ox, oy, ux, uy, a, b equal or both NaN.  No tolerances: the outputs are discrete, or computed in a
written order that the oracle restates.  draws_out is compared for chunks of 3 points or more (a
smaller chunk makes no draws; its row is not written).
"""
import numpy as np
import pytest

import consensus_edges as ce
from oracle import cpu as orc

pytestmark = pytest.mark.gpu

REAL_FIELDS = ("ox", "oy", "ux", "uy", "a", "b")
INT_FIELDS = ("best_trial", "n_draws", "flags", "n_inliers")


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def _run(ctx, b, thr=ce.THRESHOLD, **kw):
    from lidar_slam_amd.pipeline import ScanPipeline
    p = ScanPipeline(ctx, b.xy, b.scan_chunk_off, b.chunk_pt_off, threshold=thr, max_trials=b.trials,
                     want_draws=True, want_counts=True, **kw)
    p.run()
    return p.results()


def _first(diff):
    i = np.nonzero(diff)[0]
    return int(i[0]) if len(i) else -1


def _check_chunk(b, c, r, ref, draws_in=None):
    """Chunk c of the call's results r against the oracle's (mask, model, cnt, sum)."""
    mask, md, cnt, _ = ref
    lab = b.label(c)
    T = b.trials
    cpo = b.chunk_pt_off
    m = r["models"][c]
    got_cnt = r["counts"][c]
    if b.chunks[c].n < 3:
        assert not got_cnt.any(), "%s: counts of a chunk without trials are not a zero row" % lab
    else:
        ran = T if not md["flags"] & orc.FLAG_EARLY_STOP else md["n_draws"] - 1
        bad = _first(got_cnt[:ran] != cnt[:ran])
        assert bad < 0, "%s: first differing trial %d (pair %s): count %d, oracle %d; %d trials differ" % (
            lab, bad, r["draws"][c][bad].tolist(), got_cnt[bad], cnt[bad],
            int(np.sum(got_cnt[:ran] != cnt[:ran])))
        if draws_in is not None:
            bad = _first(np.any(r["draws"][c] != draws_in, axis=1))
            assert bad < 0, "%s: draws_out differs from the input at draw %d" % (lab, bad)
    for f in INT_FIELDS:
        assert m[f] == md[f], "%s: %s = %d, oracle %d (oracle best trial %d of count %d)" % (
            lab, f, m[f], md[f], md["best_trial"], cnt[md["best_trial"]] if md["best_trial"] >= 0 else -1)
    got_mask = r["mask"][cpo[c]:cpo[c + 1]]
    bad = _first(got_mask != mask)
    assert bad < 0, "%s: mask differs first at point %d (%d points differ)" % (lab, bad, int(np.sum(got_mask != mask)))
    for f in REAL_FIELDS:
        assert m[f] == md[f] or (np.isnan(m[f]) and np.isnan(md[f])), "%s: %s = %r, oracle %r" % (lab, f, m[f], md[f])


def _check_explicit(ctx, fn, *args, thr=ce.THRESHOLD):
    b = fn(*args)
    ref = ce.oracle_batch(fn, *args, thr=thr)
    assert ce.select_lds_bytes(max(b.sizes), b.trials) <= ce.LDS_LIMIT
    r = _run(ctx, b, thr, hyp="explicit", hyp_draws=b.draws)
    for c in range(len(b.chunks)):
        _check_chunk(b, c, r, ref[c], draws_in=b.draws[c])


@pytest.mark.parametrize("name", list(ce.MATRIX))
def test_count_forms_vs_oracle(ctx, name):
    """One entry of the shape matrix: the largest chunk selects the count form, the other sizes
    sit at its first size, either side of a wave row, at a partial and a full (n8200: a second and a
    partial third) tile, and far below it (mostly NaN filler lanes); N < 3 chunks ride along."""
    _check_explicit(ctx, ce.matrix_batch, name)


@pytest.mark.parametrize("trials", ce.HYP_EDGE_T)
@pytest.mark.parametrize("n_max", list(ce.HYP_EDGE_SIZES))
def test_hypothesis_block_edges_vs_oracle(ctx, n_max, trials):
    """T at the edges of the 64-trial flush group and of the 1024-hypothesis block (partial last
    group, partial last block, nt = 1, no trials at all) on band, twin, dups and line chunks."""
    _check_explicit(ctx, ce.hyp_edge_batch, n_max, trials)


@pytest.mark.parametrize("thr", [0.0, np.inf])
@pytest.mark.parametrize("name", ["n1024", "n8200"])
def test_threshold_edges_vs_oracle(ctx, name, thr):
    """thr = 0 (nothing is an inlier) and thr = inf (!cheap: every hypothesis recounted exactly,
    every trial tied at M = N) on band, line, flat and cloud chunks."""
    _check_explicit(ctx, ce.matrix_batch, name, ce.THR_VARIANTS, thr=thr)


def _check_mt(ctx, b):
    S = len(b.scan_chunk_off) - 1
    seeds = np.arange(S, dtype=np.uint32) * 7919 + 11
    r = _run(ctx, b, seeds=seeds, want_state=True)
    stops = 0
    for s in range(S):
        st = orc.MTState(seed=int(seeds[s]))
        for c in range(b.scan_chunk_off[s], b.scan_chunk_off[s + 1]):
            mask, md, ex = orc.ransac(b.chunks[c].xy, ce.THRESHOLD, b.trials, state=st, want_trials=True)
            nd = md["n_draws"]
            bad = _first(np.any(r["draws"][c, :nd] != ex["draws"][:nd], axis=1))
            assert bad < 0, "%s: draw %d differs from the oracle's stream" % (b.label(c), bad)
            _check_chunk(b, c, r, (mask, md, ex["cnt"], ex["sum"]))
            stops += bool(md["flags"] & orc.FLAG_EARLY_STOP)
        assert np.array_equal(r["mt_state"][s, :624], st.key) and r["mt_state"][s, 624] == st.pos.value, \
            "batch %s: end state of scan %d differs" % (b.name, s)
    return stops


def test_mt19937_early_stop_replay_vs_oracle(ctx):
    """The n1024 sizes (PPL 4) on the kernel's own MT19937 streams, several chunks per scan with a
    flat chunk in the middle of three scans: it stops at trial 0 and the scan is replayed from
    where it stopped.  Against the oracle chained through MTState: every draw the oracle made, the
    consensus outputs, each scan's end state.

    This case found the replay's draw-resolution tables sized for the batch's largest chunk alone
    (build_args, lslam_launch.h): a 130-point chunk resolves in 8 slots where a 1024-point one needs 2,
    its j1s row ran into the draws in LDS and the chunk's first two draws came back as 0 / 1."""
    assert _check_mt(ctx, ce.mt_batch()) >= 3


@pytest.mark.parametrize("name", list(ce.MT_RAGGED))
def test_mt19937_replay_of_ragged_scans_vs_oracle(ctx, name):
    """Replayed scans whose chunk sizes mix the resolve's slot regimes (64 slots at 3 points, 8 from
    17 to 512, 2 above) under one largest chunk, below and above the 128-point consensus split."""
    assert _check_mt(ctx, ce.mt_ragged_batch(name)) >= 2


def test_philox_draw_writeback_vs_oracle(ctx):
    """The n2048 batch (PPL 8) on Philox hypotheses: model_kernel writes the draws that
    select_kernel and draws_out read.  They are distinct and in range, and the oracle fed with them
    gives the call's own counts, masks and models."""
    b = ce.matrix_batch("n2048")
    r = _run(ctx, b, hyp="philox")
    d = r["draws"]
    for c, ch in enumerate(b.chunks):
        assert ch.n >= 3
        assert np.all(d[c, :, 0] != d[c, :, 1]), b.label(c)
        assert d[c].min() >= 0 and d[c].max() < ch.n, b.label(c)
        mask, md, ex = orc.ransac(ch.xy, ce.THRESHOLD, b.trials, hyp=d[c], want_trials=True)
        _check_chunk(b, c, r, (mask, md, ex["cnt"], ex["sum"]))
