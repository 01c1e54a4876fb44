"""The UKF edge fixtures (tests/golden/ukf_edges.npz, make_ukf_edges.py): every lane-group
width at its smallest odd L with a partly filled second workgroup, full covariances, per-slot
R, sigma bearings that straddle +-pi, an update alone, non-default parameters.

CPU side.  The fixtures regenerate; the float64 NumPy oracle (the stand-in for a correct
kernel) stays within 2.5e-6 of the 50-digit values on every case and component, a quarter of the
project's 1e-5, so a kernel whose last bits differ from the oracle's has fourfold headroom;
and each class of error the cases are meant to catch (a linear bearing mean, a noise entry
taken from the wrong slot, a transposed covariance term, a dropped landmark) moves the oracle
past 1e-5 on its case.  tests/test_gpu_ukf_edges.py holds the HIP kernels to 1e-5 on them."""
import numpy as np
import pytest

from oracle import ukf as oukf
from oracle import ukf_exact as ux

CAP = 2.5e-6
TOL = 1e-5
WIDTHS = (1, 2, 3, 5, 9, 17, 33, 65, 129)
W_CASES = tuple("w%d" % L for L in WIDTHS)
CASES = W_CASES + ("behind", "behind_map", "update_only", "params")
PG = dict(zip(WIDTHS, (1, 1, 2, 4, 8, 16, 32, 64, 64)))


def case(golden, name):
    g = golden("ukf_edges.npz")
    keys = ("x", "P", "u", "z", "lmk", "R_diag", "x_exact", "P_exact", "flags", "dt", "Q", "alpha", "beta", "kappa")
    return {k: g[name + "_" + k] for k in keys}


def params(c):
    return dict(dt=float(c["dt"]), Q=c["Q"], alpha=float(c["alpha"]), beta=float(c["beta"]), kappa=float(c["kappa"]))


def oracle_errors(c, **over):
    """component_errors of the float64 oracle on case c, with some inputs replaced."""
    a = dict(c, **{k: v for k, v in over.items() if k in c})
    kw = {k: v for k, v in over.items() if k not in c}
    f = int(c["flags"])
    xo, Po = oukf.ukf_batch(a["x"], a["P"], a["u"], a["z"], a["lmk"], a["R_diag"], predict=bool(f & 1),
                            update=bool(f & 2), **params(c), **kw)
    return ux.component_errors(xo, Po, c["x_exact"], c["P_exact"])


def test_shapes_enter_every_group_width(golden):
    for L in WIDTHS:
        c = case(golden, "w%d" % L)
        Pg = 1
        while Pg < (L + 1) // 2 and Pg < 64:
            Pg <<= 1
        assert Pg == PG[L] and c["lmk"].shape == (4 * (64 // Pg) + 1, L, 2)
        # distinct inputs per filter and per slot, full covariances
        assert len({tuple(r) for r in c["u"]}) == len(c["u"]) and np.all(np.abs(c["u"]) <= 5)
        assert len(set(c["R_diag"])) == 2 * L
        assert np.all(np.abs(c["x"][:, :2]) <= 200)
        assert np.all(np.abs(c["P"][:, [0, 0, 1], [1, 2, 2]]) > 0)
        assert np.array_equal(c["P"], c["P"].transpose(0, 2, 1)) and np.all(np.linalg.eigvalsh(c["P"]) > 0)
        d = np.linalg.norm(c["lmk"] - c["x"][:, None, :2], axis=2)
        assert d.min() >= 300 - 1e-9 and d.max() <= 3000 + 1e-9
    assert int(case(golden, "update_only")["flags"]) == 2
    p = case(golden, "params")
    assert (float(p["dt"]), float(p["alpha"]), float(p["beta"]), float(p["kappa"])) == (0.02, 1e-3, 1.5, 1.0)
    assert np.all(np.abs(p["Q"][[0, 0, 1], [1, 2, 2]]) > 0) and np.all(np.linalg.eigvalsh(p["Q"]) > 0)


def test_fixtures_regenerate(golden):
    for name in CASES:
        c = case(golden, name)
        S = len(c["x"])
        f = int(c["flags"])
        for s in sorted({0, S // 2, S - 1}):   # the tail filter is the one alone in its workgroup
            x, P = ux.to_float(*ux.step(c["x"][s], c["P"][s], c["u"][s], c["z"][s], c["lmk"][s], c["R_diag"],
                                        predict=bool(f & 1), update=bool(f & 2), **params(c)))
            assert np.array_equal(x, c["x_exact"][s]) and np.array_equal(P, c["P_exact"][s]), (name, s)


@pytest.mark.parametrize("name", CASES)
def test_float64_oracle_within_the_cap(golden, name):
    err = oracle_errors(case(golden, name))
    for k, v in err.items():
        assert v <= CAP, (name, err)


@pytest.mark.parametrize("name", ["behind", "behind_map"])
def test_behind_sigma_bearings_straddle_pi(golden, name):
    c = case(golden, name)
    assert np.array_equal(c["u"][:, 0], c["u"][:, 1])
    assert list(c["x"][:4, 2]) == [np.pi - 1e-7, -np.pi + 1e-7, 0.0, np.pi / 2]
    for s in range(len(c["x"])):
        b = oukf.update_sigma_bearings(c["x"][s], c["P"][s], c["u"][s], c["lmk"][s])
        assert int(np.sum(oukf.straddles(b))) >= 5, (name, s)


def _z_mean_linear(sigmas, Wm):
    """z_mean_centred without the circular mean: bearings averaged as plain numbers."""
    d = sigmas - sigmas[0]
    return sigmas[0] + np.dot(Wm, d)


@pytest.mark.parametrize("name", ["behind", "behind_map"])
def test_control_linear_bearing_mean(golden, name):
    c = case(golden, name)
    xo, Po = np.zeros((8, 3)), np.zeros((8, 3, 3))
    for s in range(8):
        f = oukf.UKF(6, z_mean_fn=_z_mean_linear)
        f.x, f.P, f.R = c["x"][s].copy(), c["P"][s].copy(), np.diag(c["R_diag"])
        f.predict(c["u"][s])
        f.update(c["z"][s], [tuple(p) for p in c["lmk"][s]])
        xo[s], Po[s] = f.x, f.P
    err = ux.component_errors(xo, Po, c["x_exact"], c["P_exact"])
    assert max(err.values()) > TOL, err


@pytest.mark.parametrize("name", W_CASES[1:])
def test_control_noise_of_slot_zero_everywhere(golden, name):
    c = case(golden, name)
    err = oracle_errors(c, R_diag=np.tile(c["R_diag"][:2], len(c["R_diag"]) // 2))
    assert max(err.values()) > TOL, (name, err)


def test_control_transposed_covariance_term(golden):
    c = case(golden, "w9")
    P = c["P"].copy()
    P[:, 0, 1], P[:, 0, 2] = c["P"][:, 0, 2], c["P"][:, 0, 1]
    P[:, 1, 0], P[:, 2, 0] = P[:, 0, 1], P[:, 0, 2]
    keep = np.linalg.eigvalsh(P).min(1) > 1e-3   # the swap leaves some P indefinite: no step to compare
    assert keep.sum() >= len(P) // 2
    sub = dict(c, **{k: c[k][keep] for k in ("x", "u", "z", "lmk", "x_exact", "P_exact")})
    err = oracle_errors(sub, P=P[keep])
    assert max(err.values()) > TOL, err


@pytest.mark.parametrize("name", ["w3", "w129"])
def test_control_last_landmark_dropped(golden, name):
    c = case(golden, name)
    err = oracle_errors(c, z=c["z"][:, :-2], lmk=c["lmk"][:, :-1], R_diag=c["R_diag"][:-2])
    assert max(err.values()) > TOL, (name, err)
