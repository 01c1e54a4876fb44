"""The conditions under which the fused polar loads are held exactly to the CPU oracle
(tests/polar_ref.py), checked on the reference alone: both batches leave at least MIN_MARGIN times
DELTA0 of room at the inlier threshold and between tied trials, and cpu.run_batch itself does not
change a discrete output when every coordinate moves by DELTA0 -- while a move across the
threshold does.  These are properties of the inputs: if a NumPy release moves polar_to_xy_ref far
enough to break them, the failure names the scan."""
import numpy as np
import pytest

import polar_ref as pr

BATCHES = ["c3", "large"]


@pytest.mark.parametrize("name", BATCHES)
def test_margins(name):
    m = pr.margins(name)
    print("%s: gap margin %.3g at %s; tie margin %.3g at %s; closest residual %.3g mm from the threshold"
          % (name, m["gap"], m["gap_at"], m["tie"], m["tie_at"], m["closest_mm"]))
    assert not m["count_mismatch"], "NumPy count != oracle cnt in (scan, chunk) %s" % m["count_mismatch"][:5]
    assert m["gap"] >= pr.MIN_MARGIN, m["gap_at"]
    assert m["tie"] >= pr.MIN_MARGIN, m["tie_at"]


def test_delta0_is_a_power_of_two_of_the_ulp():
    assert pr.ULP_8192 == np.spacing(8192.0)
    assert pr.DELTA0 / pr.ULP_8192 in (1.0, 2.0, 4.0, 8.0, 16.0)
    for name in BATCHES:
        assert np.abs(pr.batch(name)["xy"]).max() < 8192.0


@pytest.mark.parametrize("name", BATCHES)
def test_perturbation_leaves_discrete_outputs(name):
    b = pr.batch(name)
    base = pr.discrete_outputs(name, b["xy"])
    assert int(base["mask"].sum()) > 0 and int(np.sum(base["flags"] & 1)) > 0
    sco, cpo = b["scan_chunk_off"], b["chunk_pt_off"]
    for k in range(8):
        xy = pr.perturbed(name, k)
        assert np.max(np.abs(xy - b["xy"])) <= pr.DELTA0 and np.any(xy != b["xy"])
        got = pr.discrete_outputs(name, xy)
        for f, v in base.items():
            if np.array_equal(v, got[f]):
                continue
            i = int(np.nonzero(v != got[f])[0][0])
            if f == "mask":
                i = int(np.searchsorted(cpo, i, side="right") - 1)
            scan = i if f == "list_len" else int(np.searchsorted(sco, i, side="right") - 1)
            pytest.fail("perturbation %d changes %s in scan %d of %s" % (k, f, scan, name))
    # the control: one inlier moved by 1 mm across the threshold changes its chunk's mask
    c, p, n = pr.inlier_near_threshold(name)
    xy = b["xy"].copy()
    xy[cpo[c] + p] += n * 1.0
    got = pr.discrete_outputs(name, xy)
    sl = slice(cpo[c], cpo[c + 1])
    assert not np.array_equal(got["mask"][sl], base["mask"][sl]), (c, p)
