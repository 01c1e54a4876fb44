"""Generate tests/golden/ukf_edges.npz: UKF steps in 50-digit arithmetic at the kernels' edge shapes.

    python tests/golden/make_ukf_edges.py

Same layout and conventions as make_ukf_exact.py (PARITY UNPINNED: these vectors pin the
rounding of the float64 implementations, not the algorithm): per case a batch of filters with
its inputs (x, P, u, z, landmark positions, R diagonal, flags, dt, Q, alpha, beta, kappa) and
the exact step's (x, P) rounded once to float64 (oracle/ukf_exact.py).  Cases:

  w1 w2 w3 w5 w9 w17 w33 w65 w129
           L = the number in the name: every lane-group width Pg = 1, 1, 2, 4, 8, 16, 32, 64,
           64 of ukf_group_kernel at its smallest (odd) L, so the lanes of a group own unequal
           landmark counts.  S = 4 (64 / Pg) + 1 filters: one full 4-wave workgroup plus one
           filter alone in a second.  Every filter has its own inputs: a full SPD P
           D (A A^T / 3 + I / 2) D, D = diag(sqrt(.1, .1, .05)), u uniform in +-5,
           z = hx(x) + 0.3 sqrt(R) N(0, 1); R's diagonal differs per measurement slot (distance
           variance in [.1, 1], angle variance in [.01, .2]).
           Magnitudes: 20 <= |x|, |y| <= 60 mm and landmarks 300..1500 mm from the robot.  They
           are set by the float64 form's own error, which must stay below 2.5e-6 on every
           component (tests/test_ukf_edges.py) so that 1e-5 judges the kernel and not the
           alpha = 1e-4 weights (~1e8, 1.7e7): those multiply the rounding of sigma - mean
           differences, so P's relative error grows with |x| (2.9e-6 at |x| <= 200, 1.1e-5 at
           3000), the error of the predicted distance, and through it theta's, with the landmark
           distance (3.7e-6 rad at 3000 mm), and x_rel is an absolute error below |x| = 1.
  behind   8 filters, L = 6, u0 = u1 (straight drive: the predict keeps the heading); landmark j
           at bearing pi + DELTAS[j] from the heading, so the seven sigma bearings of a landmark
           lie on both sides of +-pi (asserted below for >= 5 of the 6 per filter); headings
           pi - 1e-7, -pi + 1e-7, 0, pi / 2 and four random ones; full P, per-slot R
  behind_map  the same with the landmark-map tuning P0 = diag(25, 25, 1e-4), R = [25, 1e-4]
  update_only  8 filters, L = 5, flags = LSLAM_UKF_UPDATE alone, full P, per-slot R
  params   8 filters, L = 9, dt = 0.02, a full SPD Q, alpha = 1e-3, beta = 1.5, kappa = 1
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import blaspin  # noqa: E402  (pins OPENBLAS_CORETYPE; must precede numpy)
import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.environ.get("LSLAM_GOLDEN_OUT", HERE)
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)

from oracle import ukf as oukf  # noqa: E402
from oracle import ukf_exact as ux  # noqa: E402

WIDTHS = (1, 2, 3, 5, 9, 17, 33, 65, 129)
DELTAS = (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-3)
XY_MIN, XY_MAX = 20.0, 60.0   # |x|, |y| of the poses (mm)
R_MIN, R_MAX = 300.0, 1500.0  # landmark distance from the robot (mm)
DEFAULTS = dict(dt=oukf.DT, Q=np.eye(3) * 0.001, alpha=1e-4, beta=2.0, kappa=0.0)


def group_width(L):
    """launch_ukf_group's lanes per filter: the smallest power of two >= ceil(L / 2), at most 64."""
    Pg = 1
    while Pg < (L + 1) // 2 and Pg < 64:
        Pg <<= 1
    return Pg


def full_P(rng, S):
    A = rng.standard_normal((S, 3, 3))
    D = np.diag(np.sqrt([.1, .1, .05]))
    P = D @ (A @ A.transpose(0, 2, 1) / 3 + 0.5 * np.eye(3)) @ D
    return (P + P.transpose(0, 2, 1)) / 2


def slot_R(rng, L):
    return np.stack([rng.uniform(.1, 1.0, L), rng.uniform(.01, .2, L)], 1).reshape(2 * L)


def poses(rng, S):
    xy = rng.uniform(XY_MIN, XY_MAX, (S, 2)) * rng.choice([-1.0, 1.0], (S, 2))
    return np.concatenate([xy, rng.uniform(-np.pi, np.pi, (S, 1))], 1)


def measure(rng, x, lmk, Rd, noise=0.3):
    z = np.stack([oukf.transfer_function(x[s], lmk[s]) for s in range(len(x))])
    z = z + noise * np.sqrt(Rd) * rng.standard_normal(z.shape)
    for s in range(len(z)):
        for j in range(1, z.shape[1], 2):
            z[s, j] = oukf.normalize_angle(z[s, j])
    return z


def ring_landmarks(rng, x, L):
    r, a = rng.uniform(R_MIN, R_MAX, (len(x), L)), rng.uniform(-np.pi, np.pi, (len(x), L))
    return x[:, None, :2] + np.stack([r * np.cos(a), r * np.sin(a)], -1)


def behind_landmarks(rng, x):
    r = rng.uniform(R_MIN, R_MAX, (len(x), len(DELTAS)))
    a = x[:, 2:3] + np.pi + np.array(DELTAS)[None]
    return x[:, None, :2] + np.stack([r * np.cos(a), r * np.sin(a)], -1)


def case(name, x, P, u, z, lmk, Rd, flags=3, **params):
    t = time.time()
    par = dict(DEFAULTS, **params)
    xe, Pe = ux.ukf_batch_exact(x, P, u, z, lmk, Rd, predict=bool(flags & 1), update=bool(flags & 2), **par)
    print("%-11s %3d filters, L=%3d: %.1fs" % (name, len(x), lmk.shape[1], time.time() - t), flush=True)
    d = dict(x=x, P=P, u=u, z=z, lmk=lmk, R_diag=Rd, x_exact=xe, P_exact=Pe, flags=np.int32(flags))
    d.update({k: np.float64(v) for k, v in par.items()})
    return {name + "_" + k: v for k, v in d.items()}


def main():
    out = {}
    rng = np.random.default_rng(20261019)
    for L in WIDTHS:
        S = 4 * (64 // group_width(L)) + 1
        x, P, u, Rd = poses(rng, S), full_P(rng, S), rng.uniform(-5, 5, (S, 2)), slot_R(rng, L)
        lmk = ring_landmarks(rng, x, L)
        out.update(case("w%d" % L, x, P, u, measure(rng, x, lmk, Rd), lmk, Rd))
    # behind: the sigma bearings straddle +-pi
    S, L = 8, len(DELTAS)
    x = poses(rng, S)
    x[:4, 2] = [np.pi - 1e-7, -np.pi + 1e-7, 0.0, np.pi / 2]
    u = np.repeat(rng.uniform(1, 5, (S, 1)), 2, 1)
    lmk = behind_landmarks(rng, x)
    for name, P, Rd in (("behind", full_P(rng, S), slot_R(rng, L)),
                        ("behind_map", np.tile(np.diag([25.0, 25.0, 1e-4]), (S, 1, 1)), np.array([25.0, 1e-4] * L))):
        for s in range(S):
            n = int(np.sum(oukf.straddles(oukf.update_sigma_bearings(x[s], P[s], u[s], lmk[s]))))
            assert n >= 5, (name, s, n)
        out.update(case(name, x, P, u, measure(rng, x, lmk, Rd), lmk, Rd))
    # update only
    S, L = 8, 5
    x, P, Rd = poses(rng, S), full_P(rng, S), slot_R(rng, L)
    lmk = ring_landmarks(rng, x, L)
    out.update(case("update_only", x, P, rng.uniform(-5, 5, (S, 2)), measure(rng, x, lmk, Rd), lmk, Rd, flags=2))
    # non-default parameters
    S, L = 8, 9
    x, P, Rd = poses(rng, S), full_P(rng, S), slot_R(rng, L)
    lmk = ring_landmarks(rng, x, L)
    A = rng.standard_normal((3, 3))
    Q = 1e-3 * (A @ A.T / 3 + 0.5 * np.eye(3))
    Q = (Q + Q.T) / 2
    out.update(case("params", x, P, rng.uniform(-5, 5, (S, 2)), measure(rng, x, lmk, Rd), lmk, Rd,
                    dt=0.02, Q=Q, alpha=1e-3, beta=1.5, kappa=1.0))
    blaspin.save_npz(os.path.join(OUT, "ukf_edges.npz"), **out)
    print("ukf_edges.npz", os.path.getsize(os.path.join(OUT, "ukf_edges.npz")), "bytes")


if __name__ == "__main__":
    main()
