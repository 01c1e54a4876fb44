"""The one-wave LDS form of the UKF (lslam_ukf.h ukf_step: all of landmark-map mode) against
the 50-digit step (oracle/ukf_exact.py), at the slot counts where its loops take another path.

tests/test_gpu_map.py runs it with 8 slots against the float64 oracle: 7 * 8 = 56 (sigma,
landmark) pairs, so every `e = lane; e < npair; e += 64` loop and the per-landmark loop run one
trip, 2 L = 16 never reaches the remainder of the four-way unrolled G / b sum, and a uniform
R_diag cannot tell rinv[m] from rinv of another slot.  Here:

  slots = 9    the revolutions' own 8 chunks; 2 L = 18 leaves the unrolled sum a remainder of 2
               (slot 8, which no chunk fills: the remainder adds zeros)
  slots = 10   7 * 10 = 70 pairs: a second trip of the pair loops
  slots = 9    again with every revolution cut into 9 chunks of 80 points: slot 8 is active, so
               the remainder adds a measurement
  slots = 72   every 720-point revolution cut into 72 chunks of 10 points: a second trip of
               the per-landmark loop, active measurement slots >= 64

with an R diagonal that differs per slot.  Per step and robot the chunk flags and match_index
equal oracle/slam.py's, so the device updated with the oracle's measurement set; then the
device's (x, P) is held to ukf_exact.step over exactly those measurements, started from the
device's previous state, at 1e-5 per component (x, y relative, theta absolute, P relative to
max|P|: the project's bound for the UKF)."""
import numpy as np
import pytest

from lidar_slam_amd import synth
from oracle import cpu as orc
from oracle import slam as osl
from oracle import ukf_exact as ux

ROBOTS = [100, 101, 102, 103, 104, 105]
STEPS = 2
U = (2.0, 2.5)
P0 = np.diag([25.0, 25.0, 1e-4])
LOOSE = dict(tol_a=0.1, tol_b=100.0, tol_dist=1000.0)
TOL = 1e-5
RUNS = [(9, 8), (10, 8), (9, 9), (72, 72)]   # (slots, chunks per revolution)


def slot_R(slots):
    """Per-slot R diagonal: distance variance in [15, 40] mm^2, angle variance in [0.5e-4, 2e-4] rad^2."""
    rng = np.random.default_rng(72)
    return np.stack([rng.uniform(15.0, 40.0, slots), rng.uniform(0.5e-4, 2e-4, slots)], 1).reshape(2 * slots)


def start_poses(poses):
    return poses[0] + np.random.default_rng(9).normal(0, [3.0, 3.0, 0.01], (len(ROBOTS), 3))


def revolutions(poses, k, chunks):
    """Step k's revolutions; for other than their own 8 chunks each 720-point revolution is
    re-cut into ``chunks`` equal ones."""
    rev = synth.revolutions_at(poses[k + 1], k, ROBOTS)
    if chunks != 8:
        n = len(rev["xy"])
        assert n == 720 * len(ROBOTS)
        rev["chunk_pt_off"] = np.arange(0, n + 1, 720 // chunks, dtype=np.int32)
        rev["scan_chunk_off"] = np.arange(len(ROBOTS) + 1, dtype=np.int32) * chunks
    return rev


def oracle_step(rs, rev, i, Rd):
    """Robot i's revolution through oracle/slam.py: (mask, models, measurement set)."""
    sco, cpo = rev["scan_chunk_off"], rev["chunk_pt_off"]
    c0, c1 = sco[i], sco[i + 1]
    meas = []
    mask, models = osl.map_step(rs, rev["xy"][cpo[c0]:cpo[c1]], cpo[c0:c1 + 1] - cpo[c0], U, Rd, meas_out=meas)
    return mask, models, meas


def exact_step(x_prev, P_prev, meas):
    """ukf_exact.step over the measurement set (predict alone if it is empty)."""
    if not meas:
        return ux.to_float(*ux.step(x_prev, P_prev, U, np.zeros(2), np.zeros((1, 2)), np.ones(2), update=False))
    z = np.concatenate([m[1] for m in meas])
    lmk = np.array([m[2] for m in meas])
    Rd = np.concatenate([m[3] for m in meas])
    return ux.to_float(*ux.step(x_prev, P_prev, U, z, lmk, Rd))


@pytest.fixture
def loose():
    orc.set_tolerances(LOOSE["tol_a"], LOOSE["tol_b"], LOOSE["tol_dist"])
    yield LOOSE
    orc.set_tolerances()


def check_conditions(slots, counts, top):
    """counts[k][i]: measurements of robot i at step k; top: the highest active slot seen."""
    if slots == 72:
        assert top >= 64, "no active measurement at slot >= 64"
        assert min(min(c) for c in counts) >= 10, counts
    else:
        assert sum(sum(c) for c in counts) >= 10, counts   # >= 20 over the 9- and 10-slot runs
    return sum(sum(c) for c in counts)


def test_workload_conditions_on_the_oracle(loose):
    """CPU: the float64 map oracle on its own states gives the measurement sets the GPU test needs,
    and stays within 2.5e-6 of the exact step over them (so 1e-5 judges the kernel)."""
    total = 0
    poses = synth.trajectory(ROBOTS, STEPS)
    for slots, chunks in RUNS:
        Rd = slot_R(slots)
        assert len(set(Rd)) == 2 * slots
        x0 = start_poses(poses)
        rs = [osl.RobotState(seed=s, x0=x0[i], P0=P0, cap=256) for i, s in enumerate(ROBOTS)]
        counts, top = [], -1
        for k in range(STEPS):
            rev = revolutions(poses, k, chunks)
            row = []
            for i in range(len(ROBOTS)):
                xp, Pp = rs[i].x.copy(), rs[i].P.copy()
                _, _, meas = oracle_step(rs[i], rev, i, Rd)
                row.append(len(meas))
                top = max([top] + [m[0] for m in meas])
                xe, Pe = exact_step(xp, Pp, meas)
                err = ux.component_errors(rs[i].x[None], rs[i].P[None], xe[None], Pe[None])
                assert max(err.values()) <= 2.5e-6, (slots, k, i, err)
            counts.append(row)
        n = check_conditions(slots, counts, top)
        assert chunks != 9 or top == 8   # the ninth slot carries a measurement
        total += n if chunks == 8 else 0
    assert total >= 20, total


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


@pytest.mark.gpu
@pytest.mark.parametrize("slots,chunks", RUNS)
def test_one_wave_ukf_vs_exact_step(ctx, loose, slots, chunks):
    from lidar_slam_amd.slam import LandmarkMap
    R = len(ROBOTS)
    poses = synth.trajectory(ROBOTS, STEPS)
    x0, Rd = start_poses(poses), slot_R(slots)
    lm = LandmarkMap(ctx, R, lmk_capacity=256, slots=slots, seeds=ROBOTS, x0=x0, P0=P0, R_diag=Rd, **loose)
    rs = [osl.RobotState(seed=s, x0=x0[i], P0=P0, cap=256) for i, s in enumerate(ROBOTS)]
    counts, top, worst = [], -1, {}
    for k in range(STEPS):
        rev = revolutions(poses, k, chunks)
        lm.step(rev["xy"], rev["scan_chunk_off"], rev["chunk_pt_off"], u=np.tile(U, (R, 1)))
        res = lm.results()
        sco = rev["scan_chunk_off"]
        row = []
        for i in range(R):
            xp, Pp = rs[i].x.copy(), rs[i].P.copy()
            _, models, meas = oracle_step(rs[i], rev, i, Rd)
            dm = res["models"][sco[i]:sco[i + 1]]
            assert list(dm["flags"]) == [m["flags"] for m in models], (slots, k, i)
            assert list(dm["match_index"]) == [m["match_index"] for m in models], (slots, k, i)
            row.append(len(meas))
            top = max([top] + [m[0] for m in meas])
            xe, Pe = exact_step(xp, Pp, meas)
            err = ux.component_errors(res["x"][i:i + 1], res["P"][i:i + 1], xe[None], Pe[None])
            print("map_exact slots=%d/%d step=%d robot=%d meas=%d %s" % (slots, chunks, k, i, len(meas), err))
            for key, v in err.items():
                worst[key] = max(worst.get(key, 0.0), v)
                assert v <= TOL, (slots, k, i, len(meas), err)
            # the next step starts oracle and exact step from the device's state (no drift)
            rs[i].x, rs[i].P = res["x"][i].copy(), res["P"][i].copy()
        counts.append(row)
    print("map_exact slots=%d worst %s" % (slots, worst))
    check_conditions(slots, counts, top)
    assert chunks != 9 or top == 8
