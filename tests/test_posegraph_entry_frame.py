"""lslam_pose_graph's checks before it needs a device, in the map side's order: params, batch, negative size,
missing input, missing output, context (tests/test_map_entry_frame.py's table and helpers, with this entry's
row).  No device is used: every call passes ctx = NULL and reads lslam_last_error()."""
import ctypes as C

import pytest

import test_map_entry_frame as frame
from lidar_slam_amd import _lib

ROW = (_lib.PoseGraphBatch, (("posegraph", _lib.posegraph_params),), "n_graphs", set(),
       b"posegraph: missing input (n_nodes, n_edges, pose, edge_ij, edge_z, edge_info)",
       b"posegraph: missing output (pose_out, trace, chi2, edge_chi2, iters, flags)")


@pytest.fixture()
def entry(monkeypatch):
    monkeypatch.setitem(frame.ENTRIES, "lslam_pose_graph", ROW)
    return "lslam_pose_graph"


def test_params_batch_and_size_come_before_the_context(entry):
    frame.test_params_batch_and_size_come_before_the_context(entry)


def test_every_pointer_is_required_or_optional(entry):
    frame.test_every_pointer_is_required_or_optional(entry)


@pytest.mark.parametrize("field,value,text", [
    ("max_nodes", 1, b"posegraph: max_nodes must be in [2, 64]"), ("max_nodes", 65, b"posegraph: max_nodes must be in [2, 64]"),
    ("max_edges", 0, b"posegraph: max_edges must be in [1, 1024]"), ("max_edges", 1025, b"posegraph: max_edges must be in [1, 1024]"),
    ("n_iter", -1, b"posegraph: n_iter must be in [0, 32]"), ("n_iter", 33, b"posegraph: n_iter must be in [0, 32]"),
    ("damp_t", -1.0, b"posegraph: damp_t must be >= 0 and finite"), ("damp_r", float("nan"), b"posegraph: damp_r must be >= 0 and finite"),
    ("eps_t", float("inf"), b"posegraph: eps_t must be >= 0 and finite"), ("eps_r", -1e-9, b"posegraph: eps_r must be >= 0 and finite")])
def test_params_ranges(field, value, text):
    p = _lib.posegraph_params(**{field: value})
    assert frame.call("lslam_pose_graph", frame.full_batch(_lib.PoseGraphBatch, "n_graphs"), [p])[1] == text


def test_defaults_and_sizes():
    p = _lib.posegraph_params()
    assert (p.max_nodes, p.max_edges, p.n_iter) == (48, 256, 10)
    assert (p.damp_t, p.damp_r, p.eps_t, p.eps_r) == (1e-6, 1e-3, 0.01, 1e-5)
    assert C.sizeof(_lib.PoseGraphParams) == 48 and C.sizeof(_lib.PoseGraphBatch) == 104
    assert _lib.ABI_VERSION == 6
