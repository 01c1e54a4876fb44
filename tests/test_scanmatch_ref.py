"""CPU checks of the scan matcher's definition (tests/scanmatch_ref.py, the NumPy form of the
comment on lslam_scan_match in include/lidarslam.h) and of the host side of its C ABI.  The GPU
parity tests are in test_gpu_scanmatch.py.

* The definition recovers motion: 24 synthetic pairs within the default window come back within
  the search's quantisation (one cell per axis, one rotation step).  The reference alone, run on
  the CPU, gives maxima of 3.92 mm, 4.59 mm and 0.174 degrees.
* The tie-break order: score, then the smallest d^2, then the smallest flat index.
* ABI: defaults, struct sizes, parameter validation (needs no device).
"""
import ctypes as C

import numpy as np
import pytest

import scanmatch_ref as smr
from lidar_slam_amd import _lib, synth


def motion_pair(r, d):
    """Scans (ref, cur) of pose p0 = scan_polar(500 + r)'s and of p0 composed with d in p0's frame."""
    p0 = synth.scan_polar(500 + r)[2]
    p1 = smr.compose(p0, d)
    ref = synth.polar_to_xy_ref(*synth.scan_polar_at(p0, 10 * r))
    cur = synth.polar_to_xy_ref(*synth.scan_polar_at(p1, 10 * r + 1))
    return ref, cur


def motions(n=24):
    rng = np.random.default_rng(3)
    return [np.array([rng.uniform(-150, 150), rng.uniform(-60, 60), np.deg2rad(rng.uniform(-8, 8))])
            for _ in range(n)]


def test_spec_recovers_motion():
    p = smr.params()
    worst = np.zeros(3)
    for r, d in enumerate(motions()):
        ref, cur = motion_pair(r, d)
        m = smr.match(ref, cur)
        err = np.abs(m["delta"] - d)
        worst = np.maximum(worst, err)
        print(r, m["delta"], d, err, m["flags"])
        assert err[0] <= p["cell"] and err[1] <= p["cell"], (r, err)
        assert err[2] <= p["theta_step"], (r, err)
        assert not (m["flags"] & smr.EDGE), r
        assert m["n_valid"].tolist() == [720, 720]
    print("worst", worst[0], worst[1], np.rad2deg(worst[2]))


TIE = dict(smear=0, cell=100.0, grid_w=16, k_trans=4, k_theta=0)


def cells(*c):
    return np.array([[(x + .5) * 100.0, (y + .5) * 100.0] for x, y in c])


def test_tie_break_prefers_the_smallest_motion():
    # shifts +1 and -3 both score 1: d^2 decides (the flat index alone would pick -3)
    m = smr.match(cells((1, 0), (-3, 0)), cells((0, 0)), **TIE)
    assert m["best"].tolist() == [0, 4, 5, 1]
    assert m["scores"][0, 4].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert m["delta"][0] == 100.0 and m["delta"][1] == 0.0
    assert m["flags"] == smr.EDGE  # one rotation: the winner is on the window's border in theta


def test_tie_break_then_the_flat_index():
    # shifts -2 and +2: the same score and d^2, the smaller flat index wins
    m = smr.match(cells((0, 0), (4, 0)), cells((2, 0)), **TIE)
    assert m["best"].tolist() == [0, 4, 2, 1]
    assert m["delta"][0] == -200.0


def test_empty_and_invalid_points():
    bad = np.array([[np.nan, 1.0], [np.inf, 2.0], [0.0, 0.0]])
    m = smr.match(cells((0, 0)), bad, **TIE)
    assert m["flags"] == smr.EMPTY and m["best"].tolist() == [0, 4, 4, 0] and not m["delta"].any()
    assert m["n_valid"].tolist() == [1, 0]
    m = smr.match(np.zeros((0, 2)), cells((0, 0)), **TIE)
    assert m["flags"] == smr.EMPTY and m["n_valid"].tolist() == [0, 1]


def test_smear_is_the_clipped_chebyshev_cone():
    G = smr.lookup_grid(cells((-8, -8), (3, 2)), smr.params(**dict(TIE, smear=2)))
    assert G[0, :4].tolist() == [3, 2, 1, 0] and G[:4, 0].tolist() == [3, 2, 1, 0]  # clipped at the corner
    assert G[10, 11] == 3 and G[12, 13] == 1 and G[9, 13] == 1 and G[13, 11] == 0


def test_match_params_default():
    p = _lib.match_params()
    assert (p.cell, p.theta_step, p.grid_w, p.smear, p.k_trans, p.k_theta) == (20.0, np.pi / 360, 512, 2, 10, 20)
    assert p.theta_step == smr.DEFAULTS["theta_step"]


def test_match_struct_sizes():
    got = (C.c_int64 * 9)()
    assert _lib.load().lslam_abi_sizes(got, 9) == 9
    assert got[7] == C.sizeof(_lib.MatchParams) == 32
    assert got[8] == C.sizeof(_lib.MatchBatch) == 96


@pytest.mark.parametrize("field,value", [("grid_w", 14), ("grid_w", 514), ("grid_w", 129), ("smear", -1), ("smear", 3),
                                         ("k_trans", -1), ("k_trans", 16), ("k_theta", -1), ("k_theta", 32),
                                         ("cell", 0.0), ("theta_step", -1.0)])
def test_match_validation_needs_no_device(field, value):
    """Parameters are checked before the context: no device is touched."""
    L = _lib.load()
    b = _lib.MatchBatch()
    ok = _lib.match_params()
    assert L.lslam_scan_match(None, C.byref(b), C.byref(ok), None) == _lib.LSLAM_ERR_ARG
    assert b"ctx" in L.lslam_last_error()  # valid parameters, an empty batch: only the context is missing
    p = _lib.match_params(**{field: value})
    assert L.lslam_scan_match(None, C.byref(b), C.byref(p), None) == _lib.LSLAM_ERR_ARG
    assert field.encode() in L.lslam_last_error()


def test_match_missing_pointers():
    L = _lib.load()
    b = _lib.MatchBatch()
    b.n_scans = 1
    assert L.lslam_scan_match(None, C.byref(b), C.byref(_lib.match_params()), None) == _lib.LSLAM_ERR_ARG
    assert b"missing input" in L.lslam_last_error()
    b.n_scans = -1
    assert L.lslam_scan_match(None, C.byref(b), C.byref(_lib.match_params()), None) == _lib.LSLAM_ERR_ARG
