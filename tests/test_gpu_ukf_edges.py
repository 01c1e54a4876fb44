"""The lane-group UKF (lslam_ukf.h ukf_step_group, ukf_group_kernel) against the 50-digit step
at its edge shapes (tests/golden/ukf_edges.npz, tests/test_ukf_edges.py): every group width
Pg = 1 .. 64 with one filter alone in a second workgroup, full covariances, a per-slot R
diagonal, sigma bearings on both sides of +-pi, an update alone, non-default parameters; a
chained run on in/out state; the sigma-cache kernel; and the stand-alone step's refusal of
LSLAM_UKF_MAP.  Bound: 1e-5 per component (x, y relative, theta absolute, P relative to
max|P|), the project's bound for the UKF (tests/test_gpu_ukf_exact.py TOL)."""
import ctypes as C

import numpy as np
import pytest

from oracle import ukf as oukf
from oracle import ukf_exact as ux
from test_gpu_ukf_exact import TOL
from test_ukf_edges import CASES, W_CASES, case, params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def _pipeline(ctx, c, S=None, **over):
    from lidar_slam_amd.pipeline import ScanPipeline
    S = len(c["x"]) if S is None else S
    L = c["lmk"].shape[1]
    ukf = dict(n_landmarks=L, x=c["x"][:S], P=c["P"][:S], u=c["u"][:S], z=c["z"][:S], lmk=c["lmk"][:S],
               R_diag=c["R_diag"], flags=int(c["flags"]), dt=float(c["dt"]), Q=list(c["Q"].reshape(9)),
               alpha=float(c["alpha"]), beta=float(c["beta"]), kappa=float(c["kappa"]))
    ukf.update(over)
    return ScanPipeline(ctx, np.zeros((1, 2)), np.zeros(S + 1, np.int32), np.zeros(1, np.int32), ukf=ukf)


@pytest.mark.parametrize("name", CASES)
def test_hip_ukf_edge_case(ctx, golden, name):
    c = case(golden, name)
    p = _pipeline(ctx, c)
    p.run_ukf_only()
    r = p.results()
    x, P = r["ukf_x"], r["ukf_P"]
    err = ux.component_errors(x, P, c["x_exact"], c["P_exact"])
    print("ukf_edges %s %s" % (name, err))
    if name in W_CASES:   # name the filter: the last one is alone in the second workgroup
        for s in range(len(x)):
            e = ux.component_errors(x[s:s + 1], P[s:s + 1], c["x_exact"][s:s + 1], c["P_exact"][s:s + 1])
            for k, tol in TOL.items():
                assert e[k] <= tol, (name, "filter %d of %d" % (s, len(x)), e)
    for k, tol in TOL.items():
        assert err[k] <= tol, (name, err)


def test_chained_steps_on_in_out_state(ctx, golden):
    """Three consecutive steps on the same ukf_x / ukf_P buffers with new u and z uploaded in
    between; each step against the exact step from the device's previous state."""
    c = case(golden, "w9")
    S, L = 4, 9
    p = _pipeline(ctx, c, S=S)
    rng = np.random.default_rng(3)
    x_prev, P_prev = c["x"][:S].copy(), c["P"][:S].copy()
    u, z = c["u"][:S].copy(), c["z"][:S].copy()
    for step in range(3):
        if step:
            u = rng.uniform(-5, 5, (S, 2))
            z = c["z"][:S] + 0.3 * np.sqrt(c["R_diag"]) * rng.standard_normal((S, 2 * L))
            z[:, 1::2] = np.vectorize(oukf.normalize_angle)(z[:, 1::2])
            p.upload_async(ukf_u=u, ukf_z=z)
        p.run_ukf_only()
        r = p.results()
        xe, Pe = ux.ukf_batch_exact(x_prev, P_prev, u, z, c["lmk"][:S], c["R_diag"], **params(c))
        err = ux.component_errors(r["ukf_x"], r["ukf_P"], xe, Pe)
        print("ukf_edges chained step %d %s" % (step, err))
        for k, tol in TOL.items():
            assert err[k] <= tol, (step, err)
        assert not np.array_equal(r["ukf_x"], x_prev)
        x_prev, P_prev = r["ukf_x"].copy(), r["ukf_P"].copy()


def test_sigma_cache_update_after_x_was_reassigned(ctx, golden):
    """ukf_group_kernel<2>: predict stores the re-drawn sigma points, the update after ``x`` was
    assigned uses THEM with the new x (filterpy's sigmas_f)."""
    from lidar_slam_amd.ukf import UnscentedKalmanFilter
    c = case(golden, "w3")
    s = 0
    f = UnscentedKalmanFilter(dim_z=6, ctx=ctx)
    f.x, f.P, f.Q, f.R = c["x"][s].copy(), c["P"][s].copy(), c["Q"].copy(), np.diag(c["R_diag"])
    f.predict(u=c["u"][s])
    xe, Pe = ux.to_float(*ux.step(c["x"][s], c["P"][s], c["u"][s], c["z"][s], c["lmk"][s], c["R_diag"], update=False))
    err = ux.component_errors(f.x[None], f.P[None], xe[None], Pe[None])
    print("ukf_edges sigma cache predict %s" % err)
    assert max(err.values()) <= 1e-5, err
    sig = np.array(f.sigmas_f)
    assert np.array_equal(sig[0], f.x) and np.all(np.abs(sig[1:] - sig[0]).max(1) > 0)
    f.x = f.x + np.array([1e-3, -2e-3, 1e-5])
    x1, P1 = np.array(f.x), np.array(f.P)
    f.update(c["z"][s], landmarks=[tuple(q) for q in c["lmk"][s]])
    xe, Pe = ux.to_float(*ux.step(x1, P1, c["u"][s], c["z"][s], c["lmk"][s], c["R_diag"], predict=False, sigmas=sig))
    err = ux.component_errors(np.array(f.x)[None], np.array(f.P)[None], xe[None], Pe[None])
    print("ukf_edges sigma cache update %s" % err)
    for k, tol in TOL.items():
        assert err[k] <= tol, err


def test_stand_alone_step_refuses_map_mode(ctx, golden):
    """lslam_ukf_step has no one-wave form: LSLAM_UKF_MAP without the association pass is an
    argument error (build_args), and nothing is written."""
    from lidar_slam_amd import _lib
    c = case(golden, "w9")
    p = _pipeline(ctx, c, flags=_lib.UKF_MAP | _lib.UKF_PREDICT | _lib.UKF_UPDATE)
    rc = _lib.load().lslam_ukf_step(ctx.handle, C.byref(p.batch), C.byref(p.up))
    assert rc == _lib.LSLAM_ERR_ARG
    with pytest.raises(ValueError):
        p.run_ukf_only()
    ctx.sync()
    r = p.results()
    assert np.array_equal(r["ukf_x"], c["x"]) and np.array_equal(r["ukf_P"], c["P"])
