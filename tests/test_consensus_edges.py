"""The cases of tests/consensus_edges.py are what they claim, from the CPU oracle alone (no GPU).

A case that cannot see its class of error does not count: each family is checked at every size it
is used at, each planted pair where it is said to sit, and for the band families a WRONG inlier
test restated in NumPy must give a count that differs from the oracle's on every chunk it applies to.
"""
import numpy as np
import pytest

import consensus_edges as ce
from oracle import cpu as orc

EXPLICIT = [("matrix", k) for k in ce.MATRIX] + [("hyp", n, t) for n in ce.HYP_EDGE_SIZES for t in ce.HYP_EDGE_T]
# a family's claim about ties needs planted trials: 15 of them from T = 63 on (every fourth trial)
T_CLAIMS = 63


def _get(key):
    fn = ce.matrix_batch if key[0] == "matrix" else ce.hyp_edge_batch
    return fn(*key[1:]), ce.oracle_batch(fn, *key[1:])


def _id(key):
    return "-".join(str(k) for k in key)


def test_matrix_restates_the_launcher():
    """MATRIX next to the constants of launch_chunks_large / count_kernel (consensus_edges.py names
    them): every count form has an entry whose largest chunk is the form's upper edge, with chunks
    at the first size of the form, one point either side of a wave row, a partial and a full tile,
    and a chunk of the small-chunk kernel's size that rides along."""
    assert [ce.ppl_of(n) for n in (129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 8200)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16, 16]
    seen = set()
    for name, (sizes, T, ppl) in ce.MATRIX.items():
        n_max = max(sizes)
        assert n_max > ce.SMALL_CHUNK_MAX and ce.ppl_of(n_max) == ppl, name
        seen.add(ppl)
        tile = ce.CNT_TPB * ppl
        if name != "n8200":
            assert n_max == tile and n_max - 1 in sizes, name          # a full tile and one lane short of it
            assert tile // 2 + 1 in sizes, name                        # the form's first size
        assert min(s for s in sizes if s >= 3) < tile // 2 or ppl == 1, name   # mostly NaN filler lanes
        assert ce.select_lds_bytes(n_max, T) <= ce.LDS_LIMIT, name
        b = ce.matrix_batch(name)
        assert b.sizes == list(sizes) * ce.REPEATS[name] and b.trials == T
        assert len(b.scan_chunk_off) - 1 >= 3 and b.scan_chunk_off[-1] == len(b.chunks)
    assert seen == {1, 2, 4, 8, 16}
    s8200 = ce.MATRIX["n8200"][0]
    tile = ce.CNT_TPB * ce.PPL_MAX
    assert tile + 1 in s8200 and 2 * tile in s8200 and 2 * tile - 1 in s8200 and 2 * tile + 8 in s8200
    assert any(s <= ce.SMALL_CHUNK_MAX for s in ce.MATRIX["n256"][0]) and 2 in ce.MATRIX["n256"][0]
    # T of the matrix: a partial flush group, full groups, one trial past a group
    assert {T % ce.FLUSH_GROUP for _, T, _ in ce.MATRIX.values()} >= {0, 1, 63}
    # every variant appears in every entry with >= 17 chunks, and each size meets several families
    for name in ce.MATRIX:
        b = ce.matrix_batch(name)
        by_size = {}
        for ch in b.chunks:
            by_size.setdefault(ch.n, set()).add(ch.variant)
        assert all(len(v) >= 2 for n, v in by_size.items() if n >= 3), name
        if len(b.chunks) >= len(ce.VARIANTS) and min(b.sizes) >= ce.MIN_FAMILY_N:
            assert {ch.variant for ch in b.chunks} == set(ce.VARIANTS), name
    used = {ch.variant for name in ce.MATRIX for ch in ce.matrix_batch(name).chunks}
    assert used == set(ce.VARIANTS)


def test_hyp_edges_restates_the_count_loop():
    B, G = ce.CNT_HYP_BLOCK, ce.FLUSH_GROUP
    want = {0, 1, G - 1, G, G + 1, B - 1, B, B + 1, B + G - 1, B + G, 2 * B + 1}
    assert set(ce.HYP_EDGE_T) == want
    assert [ce.ppl_of(n) for n in ce.HYP_EDGE_SIZES] == [2, 8]
    for n_max, sizes in ce.HYP_EDGE_SIZES.items():
        assert max(sizes) == n_max
        for T in ce.HYP_EDGE_T:
            assert ce.select_lds_bytes(n_max, T) <= ce.LDS_LIMIT
            b = ce.hyp_edge_batch(n_max, T)
            assert [c.variant for c in b.chunks] == list(ce.HYP_EDGE_VARIANTS)
            assert {c.family for c in b.chunks} == {"band", "twin", "dups", "line"}
    assert ce.select_lds_bytes(8200, 70) <= ce.LDS_LIMIT and ce.select_lds_bytes(1025, 2049) <= ce.LDS_LIMIT
    assert ce.select_lds_bytes(8200, 2049) > ce.LDS_LIMIT   # the bound is a real one


def test_builder_is_deterministic_and_any_size():
    for v in ce.VARIANTS:
        for n in (3, 16, 17, 129, 1000):
            a, b = ce.make_chunk(v, n, 5), ce.make_chunk(v, n, 5)
            assert a.xy.shape == (n, 2) and np.array_equal(a.xy, b.xy, equal_nan=True), (v, n)
            d0, p0 = ce.hypotheses(a, 70, 9)
            d1, p1 = ce.hypotheses(b, 70, 9)
            assert np.array_equal(d0, d1) and p0 == p1
            assert np.all(d0[:, 0] != d0[:, 1]) and d0.min() >= 0 and d0.max() < n, (v, n)
    ce.matrix_batch.cache_clear()
    a = ce.matrix_batch("n512")
    ce.matrix_batch.cache_clear()
    b = ce.matrix_batch("n512")
    assert a is not b and np.array_equal(a.xy, b.xy, equal_nan=True) and np.array_equal(a.draws, b.draws)
    ce.oracle_batch.cache_clear()


def test_points_are_where_the_families_say():
    ulp = np.spacing
    for n in (64, 130, 1025):
        b = ce.make_chunk("band_axis", n)
        off = np.arange(n) % 4 == 1
        assert np.all(b.xy[~off, 1] == 0) and set(np.abs(b.xy[off, 1])) <= set(ce.THR5)
        assert len(set(np.abs(b.xy[off, 1]))) == len(set(ce.THR5)) == 3 and {-1.0, 1.0} == set(np.sign(b.xy[off, 1]))
        r = ce.make_chunk("band_rot", n)
        assert np.array_equal(r.xy[:, 0] - 1000.0, b.xy[:, 1] + 1000.0 - 1000.0) and np.all(r.xy[~off, 0] == 1000.0)
        s = ce.make_chunk("band_slant", n)
        assert np.all(s.xy[~off, 1] == 2 * s.xy[~off, 0])
        assert np.max(np.abs(np.abs(s.xy[off, 1] - 2 * s.xy[off, 0]) / ce.SQRT5 - 20.0)) < 1e-12
        # float-band: both cutoffs of the count kernels (k = -25.6 and +38.4 high-dword units
        # expressed in 2^-24) and float32's own rounding of 20 are straddled, on both sides of the line
        f = ce.make_chunk("float_axis", n)
        offf = np.arange(n) % 2 == 1
        k = (np.abs(f.xy[offf, 1]) / 20.0 - 1.0) * 2.0 ** 24
        assert np.all(f.xy[~offf, 1] == 0) and np.all(k == np.round(2 * k) / 2)   # exact multiples of 0.5
        for side in (1.0, -1.0):
            ks = set(k[np.sign(f.xy[offf, 1]) == side]) if n >= 130 else set(k)
            assert {-0.5, 0.0, 0.5} <= set(k)
            assert min(ks) < -25.6 < max(x for x in ks if x < 0) and min(x for x in ks if x > 0) < 38.4 < max(ks), (n, side)
        assert {-26.0, -25.0, 38.0, 39.0} <= set(k)
        # offset: still within ulps OF THE COORDINATE of the threshold after the translation
        o = ce.make_chunk("off_band", n)
        v = 3 * (o.xy[:, 0] - ce.OFFSET[0]) - 4 * (o.xy[:, 1] - ce.OFFSET[1])   # exact; 5 x the distance
        assert np.all(v[~off] == 0) and np.min(o.xy[:, 0]) >= 3e5 - 12 and np.max(o.xy[:, 1]) < -1.9e5
        dev = (np.abs(v[off]) - 100.0) / (4 * ulp(2.0e5))
        assert {0.0, 1.0, -1.0, 2.0, -2.0} <= set(dev) <= set(float(s * k) for k in ce.ULP_STEPS for s in (1, -1))
        assert np.sum(dev == 0) >= len(dev) // 3 and np.ptp(o.xy[:, 0]) ** 2 * 2 < 5e5 * 21   # E2 << Rb ecut_q
        w = ce.make_chunk("off_wide", n)
        lv = ce.OFFSET[1] + 2 * (w.xy[:, 0] - ce.OFFSET[0])
        assert np.all(w.xy[~off, 1] == lv[~off])
        assert np.all(np.abs(np.abs(w.xy[off, 1] - lv[off]) - 20.0 * ce.SQRT5) <= 4 * ulp(2.0e5))
        assert np.ptp(w.xy[:, 0]) >= 1.0e5 and np.ptp(w.xy[:, 0]) ** 2 > 1e3 * 5e5 * 21   # E2 >> Rb ecut_q
        of = ce.make_chunk("off_float", n)
        kk = (np.abs(of.xy[offf, 1] - ce.OFFSET[1]) / 20.0 - 1.0) * 2.0 ** 24
        assert np.max(np.abs(kk - k)) < 1e-4 and np.all(of.xy[~offf, 1] == ce.OFFSET[1])
        t = ce.make_chunk("twin", n)
        h = n // 2
        assert np.array_equal(t.xy[:h, 0], t.xy[h:2 * h, 0]) and np.array_equal(t.xy[h:2 * h, 1], 100.0 - t.xy[:h, 1])
        tu = ce.make_chunk("twin_ulp", n)
        assert np.array_equal(tu.xy[tu.lines[0]], t.xy[:h]) and np.array_equal(tu.xy[tu.lines[1]], t.xy[h:2 * h])
        assert list(tu.lines[1][:2]) == [2 * h - 1, 2 * h - 2] and len(tu.lines[0]) == len(tu.lines[1]) == h
        for v in ("dups3", "dups4"):
            d = ce.make_chunk(v, n)
            assert d.dups and all(len(g) >= 2 and np.all(d.xy[g] == d.xy[g[0]]) for g in d.dups)
        assert np.isnan(ce.make_chunk("nan", n).xy).sum() == 1 and np.isinf(ce.make_chunk("inf", n).xy).sum() == 1
    assert np.isposinf(ce.make_chunk("inf", 1025).xy).sum() == 1 and np.isneginf(ce.make_chunk("inf", 130).xy).sum() == 1


@pytest.mark.parametrize("key", EXPLICIT, ids=_id)
def test_planted_pairs_sit_where_stated(key):
    b, _ = _get(key)
    T = b.trials
    w = ce.plant_trials(T)
    if T >= 9:
        t0, t1 = w["reverse"]
        assert (t0, t1) == (7, T - 1)
        assert (t0 // ce.FLUSH_GROUP != t1 // ce.FLUSH_GROUP) == (T > ce.FLUSH_GROUP)
        assert (t0 // ce.CNT_HYP_BLOCK != t1 // ce.CNT_HYP_BLOCK) == (T > ce.CNT_HYP_BLOCK)
    if T > ce.CNT_HYP_BLOCK + 2:
        assert any(t >= ce.CNT_HYP_BLOCK for t in w["dup"]) and any(t >= ce.CNT_HYP_BLOCK for t in w["main"])
    for c, ch in enumerate(b.chunks):
        d, held = b.draws[c], b.plants[c]
        assert d.shape == (T + 1, 2)
        if ch.n < 3:
            continue
        assert np.all(d[:, 0] != d[:, 1]) and d.min() >= 0 and d.max() < ch.n, b.label(c)
        assert held["twice"] == w["twice"] and held["reverse"] == w["reverse"], b.label(c)
        if ch.lines:
            assert [t for t, _ in held["main"]] == w["main"], b.label(c)
        for t, ln in held["main"]:
            i0, i1 = d[t]
            assert i0 in ch.lines[ln] and i1 in ch.lines[ln] and not np.array_equal(ch.xy[i0], ch.xy[i1]), (b.label(c), t)
        if ch.family == "dups":
            assert held["dup"] == w["dup"], b.label(c)
        for t in held["dup"]:
            assert d[t, 0] != d[t, 1] and np.array_equal(ch.xy[d[t, 0]], ch.xy[d[t, 1]]), (b.label(c), t)
        if held["twice"]:
            assert np.array_equal(d[3], d[4]), b.label(c)
        if held["reverse"]:
            assert np.array_equal(d[7], d[T - 1][::-1]), b.label(c)
        if ch.variant.startswith("twin") and len(held["main"]) >= 2:   # a hypothesis, then its mirror image
            (ta, la), (tb, lb) = held["main"][0], held["main"][1]
            assert (la, lb) == (0, 1)
            pa, pb = ch.xy[d[ta]], ch.xy[d[tb]]
            assert np.array_equal(pa[:, 0], pb[:, 0]) and np.array_equal(pb[:, 1], 100.0 - pa[:, 1]), b.label(c)


def _ulps_apart(a, b):
    return abs(float(a) - float(b)) / np.spacing(max(abs(float(a)), abs(float(b))))


@pytest.mark.parametrize("key", EXPLICIT, ids=_id)
def test_families_do_what_they_claim(key):
    b, ref = _get(key)
    T = b.trials
    for c, ch in enumerate(b.chunks):
        mask, md, cnt, sm = ref[c]
        lab = b.label(c)
        if ch.n < 3:
            assert md["flags"] == orc.FLAG_N_TOO_SMALL and not cnt.any(), lab
            continue
        if T == 0:
            assert md["best_trial"] == -1 and md["flags"] & orc.FLAG_NO_INLIERS, lab
            continue
        M = int(cnt.max())
        tied = np.nonzero(cnt == M)[0]
        if ch.variant == "line":
            assert np.all(cnt == ch.n), lab
            if ch.n >= ce.MIN_FAMILY_N:
                assert md["n_draws"] == T + 1 and not md["flags"] & orc.FLAG_EARLY_STOP, lab
                assert not np.isnan(sm).any() and np.all(sm > 0) and np.max(sm) < 1e-18, lab
        elif ch.variant == "flat":
            assert md["flags"] & orc.FLAG_EARLY_STOP and md["best_trial"] == 0 and md["n_draws"] == 2, lab
            assert sm[0] == 0.0, lab
        elif ch.family == "twin" and T >= T_CLAIMS:
            assert M == ch.n // 2 and len(tied) >= 4 and len(set(sm[tied])) >= 2, lab
            assert not md["flags"] & orc.FLAG_EARLY_STOP, lab
            # a hypothesis and its mirror image have equal counts
            main = b.plants[c]["main"]
            for (ta, la), (tb, lb) in zip(main[0::2], main[1::2]):
                assert (la, lb) == (0, 1) and cnt[ta] == cnt[tb], (lab, ta, tb)
            if ch.variant == "twin_ulp":
                s = np.sort(sm[tied])
                close = [(x, y) for x, y in zip(s[:-1], s[1:]) if x != y and _ulps_apart(x, y) <= 16]
                assert close, (lab, "no two tied sums within 16 ulps that differ")
        elif ch.family == "dups" and T >= 3:
            A, Bp = ch.xy[b.draws[c, :T, 0]], ch.xy[b.draws[c, :T, 1]]
            o, u = ce._models(ch.xy, b.draws[c, :T])
            un = u[:, 0] ** 2 + u[:, 1] ** 2
            assert np.any(np.abs(un - 1.0) > 2.0 ** -46), lab
            assert np.any(np.all(A == Bp, axis=1)), lab
        elif ch.family == "nonfinite":
            assert md["flags"] & orc.FLAG_VALID and md["n_inliers"] >= 2, lab
            assert all(np.isfinite(md[f]) for f in ("ox", "oy", "ux", "uy", "a", "b")), lab
            bad = np.nonzero(~np.isfinite(ch.xy).all(axis=1))[0]
            assert len(bad) == 1 and not mask[bad[0]], lab
        elif ch.variant == "cloud":
            assert md["flags"] & orc.FLAG_VALID and not md["flags"] & orc.FLAG_EARLY_STOP, lab


def test_nonfinite_flags_as_the_small_golden_case(golden):
    """tests/golden/edge.npz pins a 50-point chunk with one NaN point (valid, the point never an
    inlier): the large nonfinite chunks get the same flags from the oracle, and a hypothesis through
    the bad point counts nothing."""
    g = golden("edge.npz")
    k = list(g["names"]).index("nan_point")
    xy = g["xy"][g["off"][k]:g["off"][k + 1]]
    assert g["err"][k] == 0
    _, md, _ = orc.ransac(xy, float(g["thr"][k]), int(g["trials"][k]), state=orc.MTState(seed=int(g["seeds"][k])))
    small = md["flags"]
    assert small & orc.FLAG_VALID
    seen = 0
    for key in EXPLICIT[:len(ce.MATRIX)]:
        b, ref = _get(key)
        for c, ch in enumerate(b.chunks):
            if ch.family != "nonfinite":
                continue
            _, md, cnt, _ = ref[c]
            assert md["flags"] == small, b.label(c)
            bad = int(np.nonzero(~np.isfinite(ch.xy).all(axis=1))[0][0])
            d = np.array([[bad, (bad + 1) % ch.n], [0, 1]] * 2, np.int32)[:3]
            _, _, ex = orc.ransac(ch.xy, ce.THRESHOLD, 2, hyp=d, want_trials=True)
            assert ex["cnt"][0] == 0 and ex["cnt"][1] >= 2, b.label(c)
            seen += 1
    assert seen >= 2 * len(ce.MATRIX) - 2


@pytest.mark.parametrize("key", EXPLICIT, ids=_id)
def test_wrong_counts_disagree_with_the_oracle(key):
    """Controls: a count without the exact deferral (a), and float32 compares of |r| against
    sqrt(ecut) (b: <, c: <=), each a plain NumPy restatement, must differ from the oracle's count on
    at least one trial of every chunk they apply to (consensus_edges.CONTROL_VARIANTS).  (b) and (c)
    are wrong by construction on any hypothesis along the line, so they are held from T = 1; (a)
    differs by the rounding of single residuals, so it is held where fifteen planted trials exist."""
    b, ref = _get(key)
    T = b.trials
    ecut = orc.ecut(ce.THRESHOLD)
    applied = 0
    for c, ch in enumerate(b.chunks):
        for which, variants in ce.CONTROL_VARIANTS.items():
            if ch.variant not in variants or ch.n < ce.MIN_FAMILY_N or T < (T_CLAIMS if which == "a" else 1):
                continue
            wrong = ce.control_counts(ch.xy, b.draws[c], ecut, which)
            n_diff = int(np.sum(wrong != ref[c][2]))
            assert n_diff >= 1, "%s: control (%s) agrees with the oracle on all %d trials" % (b.label(c), which, T)
            applied += 1
    if key[0] == "matrix" or T >= T_CLAIMS:
        assert applied >= 1, key


def test_axis_parallel_lines_cannot_see_control_a():
    """Why (a) is not asked of band_axis / band_rot / float_axis / off_float: for a hypothesis along
    an axis-parallel line the cross product and the reference's projection are the same exact number."""
    b, ref = _get(("matrix", "n512"))
    ecut = orc.ecut(ce.THRESHOLD)
    n = 0
    for c, ch in enumerate(b.chunks):
        if ch.variant in ("band_axis", "band_rot", "float_axis", "off_float"):
            t = [t for t, _ in b.plants[c]["main"]]
            assert np.array_equal(ce.control_counts(ch.xy, b.draws[c], ecut, "a")[t], ref[c][2][t]), b.label(c)
            n += 1
    assert n >= 3


def test_threshold_and_mt_batches():
    for name in ("n1024", "n8200"):
        b = ce.matrix_batch(name, ce.THR_VARIANTS)
        assert {ch.family for ch in b.chunks} == {"band", "line", "flat", "cloud"}
        assert b.sizes == ce.matrix_batch(name).sizes
        for thr, flag in ((0.0, orc.FLAG_NO_INLIERS), (np.inf, orc.FLAG_VALID)):
            ref = ce.oracle_batch(ce.matrix_batch, name, ce.THR_VARIANTS, thr=thr)
            for c, ch in enumerate(b.chunks):
                _, md, cnt, _ = ref[c]
                assert md["flags"] & flag, (b.label(c), thr)
                assert np.all(cnt == (0 if thr == 0.0 else ch.n)), (b.label(c), thr)
    m = ce.mt_batch()
    assert m.sizes == list(ce.MATRIX["n1024"][0]) * len(ce.MT_SCANS) and ce.ppl_of(max(m.sizes)) == 4
    per = len(ce.MATRIX["n1024"][0])
    assert list(np.diff(m.scan_chunk_off)) == [per] * len(ce.MT_SCANS)
    mid = [s for s in range(len(ce.MT_SCANS)) if "flat" in [ch.variant for ch in m.chunks[s * per + 1:(s + 1) * per - 1]]]
    assert len(mid) >= 3


def test_mt_ragged_batches_mix_the_resolve_regimes():
    """MT_RAGGED: every scan starts with a chunk that stops at trial 0 (so the fix-up replays it), and
    its chunk sizes fall in at least two of the resolve's slot regimes (mt_nslot, lslam_rng.h: a
    power of two >= RB + ceil(64 / (n - 1)), RB = 4 up to 512 points and 1 above) whose slot count
    exceeds the largest chunk's own."""
    def nslot(n):
        need = (4 if n <= 512 else 1) + -(-64 // max(n - 1, 2))
        return 1 << (need - 1).bit_length()
    assert [nslot(n) for n in (3, 10, 17, 130, 512, 513, 1024)] == [64, 16, 8, 8, 8, 2, 2]
    for name in ce.MT_RAGGED:
        b = ce.mt_ragged_batch(name)
        per = len(ce.MT_RAGGED[name][0])
        assert list(np.diff(b.scan_chunk_off)) == [per, per]
        own = nslot(max(b.sizes))
        for s in range(2):
            ch = b.chunks[s * per:(s + 1) * per]
            assert ch[0].variant == "flat" and all(c.variant == v for c, (v, _) in zip(ch, ce.MT_RAGGED[name][0]))
            _, md, _ = orc.ransac(ch[0].xy, ce.THRESHOLD, b.trials, state=orc.MTState(seed=1))
            assert md["flags"] & orc.FLAG_EARLY_STOP and md["n_draws"] == 2
            assert len({nslot(c.n) for c in ch}) >= 2 and max(nslot(c.n) for c in ch) > own, name
