"""The CSR arguments of a revolution -> per-robot point offsets (lidar_slam_amd/staging.py,
``point_offsets``): a pure function, no context and no library."""
import numpy as np
import pytest

from lidar_slam_amd.slam import MapInput
from lidar_slam_amd.staging import point_offsets

XY = np.arange(40.0).reshape(20, 2)
CPO = [0, 7, 12, 12, 18, 20]  # a chunk of seven points before the robots', one of two behind them


def test_a_slice_gives_absolute_offsets():
    xy, off = point_offsets(XY, [1, 2, 4], CPO, 2)
    assert xy is XY and off.dtype == np.int64 and off.tolist() == [7, 12, 18]
    _, off = point_offsets(XY, np.array([0, 3, 5], np.int32), np.array(CPO, np.int32), 2)  # chunks 0..2 and 3..4
    assert off.dtype == np.int64 and off.tolist() == [0, 12, 20]


def test_a_robot_without_points():
    assert point_offsets(XY, [1, 2, 3], CPO, 2)[1].tolist() == [7, 12, 12]  # chunk 2 is empty
    assert point_offsets(XY, [1, 1, 4], CPO, 2)[1].tolist() == [7, 7, 18]   # no chunk at all
    assert point_offsets(XY, [0, 0, 0], [0], 2)[1].tolist() == [0, 0, 0]


def test_a_map_input_is_unpacked():
    inp = MapInput()
    inp.xy, inp.sco, inp.cpo = XY, np.array([1, 2, 4], np.int32), np.array(CPO, np.int32)
    for others in ((None, None), ([0, 1, 2], [0, 1, 2])):  # (the input's own offsets count)
        xy, off = point_offsets(inp, *others, 2)
        assert xy is XY and off.tolist() == [7, 12, 18]


@pytest.mark.parametrize("sco", [[1, 2], [1, 2, 3, 4], []])
def test_scan_chunk_off_of_a_wrong_length(sco):
    with pytest.raises(ValueError, match=r"^one revolution per robot: scan_chunk_off needs n_robots \+ 1 entries$"):
        point_offsets(XY, sco, CPO, 2)


@pytest.mark.parametrize("sco,cpo,R", [([4, 2, 4], CPO, 2),                # a decreasing offset
                                       ([1, 4, 2], CPO, 2),                # the last one below the one before
                                       ([0, 1, 2], [-1, 7, 12], 2),        # a negative first offset
                                       ([0, 1], [0, 2 ** 31], 1),          # the last offset does not fit an int32
                                       ([1, 1], [0, 2 ** 31], 1)],
                         ids=["decreasing", "decreasing last", "negative", "2^31", "2^31 and no points"])
def test_inconsistent_offsets(sco, cpo, R):
    with pytest.raises(ValueError, match="^inconsistent CSR offsets$"):
        point_offsets(XY, sco, cpo, R)  # (nothing of that size is allocated: the offsets alone are read)


def test_the_largest_offsets_pass():
    assert point_offsets(XY, [0, 1], [0, 2 ** 31 - 1], 1)[1].tolist() == [0, 2 ** 31 - 1]
