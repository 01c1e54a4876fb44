"""The field read under a revolution (include/lidarslam.h, lslam_field_score) on the CPU: hand-made
cases of tests/fieldscore_ref.py, and what the field is worth physically on the five-revolution room
of test_occgrid_ref.  tests/test_gpu_fieldscore.py holds the kernel to the reference bit for bit and
repeats the room's caps on the device's own grid.

The room.  Robots 200-207, ROOM_KW, ROOM_ORIGIN, the map built at the true poses; occ_min 85,
d_max 128, trunc2 625, near2 4; the fifth revolution.  Measured on the reference, per robot:
  * clearance_mm() at the true step-4 poses against the analytic distance to the nearest of the
    room's four walls: -16.9 .. -0.3 mm; cap |error| <= 40 mm (half a cell diagonal for the robot
    cell, one cell of wall thickness, 5 mm of range noise);
  * near share at the true poses 0.972 .. 0.983, cap >= 0.95 (the revolutions carry 3 % outliers); at
    the poses moved by (700, -600) mm and 0.5 rad 0.018 .. 0.086, cap <= 0.25;
  * mean of min(v, 625) at the true poses 9.8 .. 16.6, at the moved poses 251 .. 507; cap: moved
    >= 5 x true, per robot.
With occ_min 1 the figures move by less than 1 % (n_src 1148 .. 1236 against 975 .. 1066).  In
NOT_FREE mode every robot's clearance equals its OCC clearance (robot 200: 960 mm), so it is asserted
to be at most that plus one cell.
"""
import numpy as np
import pytest

import dist_ref as dr
import fieldscore_ref as fr
from lidar_slam_amd import synth
from test_occgrid_ref import ROOM_KW, ROOM_ORIGIN, ROOM_ROBOTS, build_room, room_run

ROOM_DIST = dict(occ_min=85, d_max=128)
ROOM_SCORE = dict(trunc2=625, near2=4, off2=128 * 128)
KW = dict(grid_w=32, cell=100.0, max_range=3000.0)


def far_moved(poses):
    out = np.array(poses, np.float64)
    out[:, 0] += 700.0
    out[:, 1] -= 600.0
    out[:, 2] += 0.5
    return out


def wall_distance(poses):
    x, y = poses[:, 0], poses[:, 1]
    return np.minimum(np.minimum(x, synth.ROOM_W - x), np.minimum(y, synth.ROOM_H - y))


def assert_room_caps(score_fn, poses_true):
    """score_fn(poses) -> (stats [R, 4], clear2 [R]), the reference here and the device in
    test_gpu_fieldscore.  The caps of the module's docstring."""
    s0, c0 = score_fn(poses_true)
    s1, _ = score_fn(far_moved(poses_true))
    err = fr.clearance_mm(c0, 20.0) - wall_distance(poses_true)
    n0, n1, m0, m1 = fr.near_share(s0), fr.near_share(s1), fr.mean_d2(s0), fr.mean_d2(s1)
    print("clearance error mm", err.round(1), "\nnear share true", n0.round(3), "moved", n1.round(3),
          "\nmean d2 true", m0.round(1), "moved", m1.round(1))
    assert np.all(np.abs(err) <= 40.0), err
    assert np.all(n0 >= 0.95) and np.all(n1 <= 0.25), (n0, n1)
    assert np.all(m1 >= 5.0 * m0) and np.all(m0 > 0.0), (m0, m1)
    return s0, c0


@pytest.fixture(scope="module")
def room():
    poses, revs = room_run()
    return poses, revs, build_room(poses, revs)


def ref_score_fn(room, d2):
    poses, revs, _ = room
    rev = revs[4]
    off = rev["chunk_pt_off"][rev["scan_chunk_off"]]
    origin = np.tile(ROOM_ORIGIN, (len(ROOM_ROBOTS), 1))

    def score_fn(p):
        rot = np.stack([np.cos(p[:, 2]), np.sin(p[:, 2])], -1)
        stats, clear2, flags = fr.score_batch(d2, rev["xy"], off, p, rot, origin, ROOM_KW, **ROOM_SCORE)
        assert not flags.any() and np.all(stats[:, 1] > 700)
        return stats, clear2
    return score_fn


def test_room_caps(room):
    poses, revs, L = room
    d2, n_src, flags = dr.field_batch(L, **ROOM_DIST)
    assert not flags.any() and n_src.min() >= 975 and n_src.max() <= 1066
    s0, c0 = assert_room_caps(ref_score_fn(room, d2), poses[4])
    # occ_min 1: the figures move by less than 1 %
    d21, n1, _ = dr.field_batch(L, occ_min=1, d_max=128)
    assert n1.min() >= 1148 and n1.max() <= 1236
    s1, c1 = assert_room_caps(ref_score_fn(room, d21), poses[4])
    assert np.all(np.abs(fr.near_share(s1) - fr.near_share(s0)) < 0.01) and np.array_equal(c0, c1)
    # NOT_FREE: unknown space and the border are obstacles too
    d2n, _, _ = dr.field_batch(L, mode=dr.NOT_FREE, d_max=128)
    _, cn = ref_score_fn(room, d2n)(poses[4])
    print("NOT_FREE clearance mm", fr.clearance_mm(cn, 20.0), "OCC", fr.clearance_mm(c0, 20.0))
    assert np.all(fr.clearance_mm(cn, 20.0) <= fr.clearance_mm(c0, 20.0) + 20.0)
    assert np.all(d2n <= d2)


def test_hand_made_scores():
    d2 = np.arange(32 * 32, dtype=np.uint16).reshape(32, 32)  # d2[Y][X] = 32 Y + X
    pose = (1050.0, 1050.0, 0.0)  # robot cell (10, 10), heading +x
    pts = np.array([[500.0, 0.0],       # (15, 10): 335
                    [-1000.0, -1000.0], # (0, 0): 0
                    [0.0, 300.0],       # (10, 13): 426
                    [-1100.0, 0.0],     # off the map: off2
                    [2950.0, 0.0],      # off the map (cell 40)
                    [3100.0, 0.0],      # beyond max_range: ignored
                    [np.nan, 1.0], [0.0, 0.0]])
    stats, clear2, flags = fr.score(d2, pts, pose, (1.0, 0.0), (0.0, 0.0), KW, trunc2=400, near2=335, off2=77)
    assert flags == 0 and clear2 == 32 * 10 + 10
    assert stats.tolist() == [335 + 0 + 400 + 77 + 77, 5, 4, 2]
    # near2 at an exact value; off2 above near2
    stats, _, _ = fr.score(d2, pts, pose, (1.0, 0.0), (0.0, 0.0), KW, trunc2=65025, near2=76, off2=77)
    assert stats.tolist() == [335 + 0 + 426 + 154, 5, 1, 2]
    # the robot off the map: clear2 is off2; a bad pose: nothing
    _, clear2, flags = fr.score(d2, pts, (-50.0, 1050.0, 0.0), (1.0, 0.0), (0.0, 0.0), KW, off2=9)
    assert (clear2, flags) == (9, 0)
    stats, clear2, flags = fr.score(d2, pts, (np.nan, 0.0, 0.0), (1.0, 0.0), (0.0, 0.0), KW)
    assert (stats.tolist(), clear2, flags) == ([0, 0, 0, 0], 0, fr.BAD_POSE)
    stats, clear2, flags = fr.score(d2, np.zeros((0, 2)), pose, (1.0, 0.0), (0.0, 0.0), KW)
    assert (stats.tolist(), clear2, flags) == ([0, 0, 0, 0], 330, 0)


def test_helpers():
    stats = np.array([[100, 10, 4, 1], [0, 0, 0, 0]], np.int64)
    assert fr.near_share(stats).tolist() == [0.4, 0.0] and fr.mean_d2(stats).tolist() == [10.0, 0.0]
    assert fr.clearance_mm([0, 4, 4096], 20.0).tolist() == [0.0, 40.0, 1280.0]
    assert fr.DEFAULTS == dict(trunc2=625, near2=4, off2=4096)
