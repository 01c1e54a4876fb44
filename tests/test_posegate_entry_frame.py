"""lslam_pose_graph_gate's checks before it needs a device, in the map side's order: params, batch, negative size,
missing input, missing output, context (tests/test_map_entry_frame.py's table and helpers, with this entry's
row).  No device is used: every call passes ctx = NULL and reads lslam_last_error()."""
import ctypes as C

import pytest

import test_map_entry_frame as frame
from lidar_slam_amd import _lib

ROW = (_lib.PoseGateBatch, (("posegate", _lib.posegate_params),), "n_graphs", set(),
       b"posegate: missing input (n_nodes, n_edges, pose, edge_ij, edge_z, edge_info, n_cand, cand_ij, cand_z, cand_info)",
       b"posegate: missing output (trace, chi2, cand_nis, cand_err, cand_cov, cand_flags, flags)")


@pytest.fixture()
def entry(monkeypatch):
    monkeypatch.setitem(frame.ENTRIES, "lslam_pose_graph_gate", ROW)
    return "lslam_pose_graph_gate"


def test_params_batch_and_size_come_before_the_context(entry):
    frame.test_params_batch_and_size_come_before_the_context(entry)


def test_every_pointer_is_required_or_optional(entry):
    frame.test_every_pointer_is_required_or_optional(entry)


@pytest.mark.parametrize("field,value,text", [
    ("max_nodes", 1, b"posegate: max_nodes must be in [2, 64]"), ("max_nodes", 65, b"posegate: max_nodes must be in [2, 64]"),
    ("max_edges", 0, b"posegate: max_edges must be in [1, 1024]"), ("max_edges", 1025, b"posegate: max_edges must be in [1, 1024]"),
    ("max_cand", 0, b"posegate: max_cand must be in [1, 64]"), ("max_cand", 65, b"posegate: max_cand must be in [1, 64]"),
    ("damp_t", -1.0, b"posegate: damp_t must be >= 0 and finite"), ("damp_r", float("nan"), b"posegate: damp_r must be >= 0 and finite"),
    ("damp_t", float("inf"), b"posegate: damp_t must be >= 0 and finite"),
    ("nis_max", 0.0, b"posegate: nis_max must be > 0 (+inf: no gate)"), ("nis_max", float("nan"), b"posegate: nis_max must be > 0 (+inf: no gate)"),
    ("append", 2, b"posegate: append must be 0 or 1"), ("append", -1, b"posegate: append must be 0 or 1")])
def test_params_ranges(field, value, text):
    p = _lib.posegate_params(**{field: value})
    assert frame.call("lslam_pose_graph_gate", frame.full_batch(_lib.PoseGateBatch, "n_graphs"), [p])[1] == text


def test_an_infinite_gate_and_the_largest_shape_pass_the_params_check():
    p = _lib.posegate_params(nis_max=float("inf"), max_nodes=64, max_edges=1024, max_cand=64, append=1)
    assert frame.call("lslam_pose_graph_gate", frame.full_batch(_lib.PoseGateBatch, "n_graphs"), [p])[1] == b"posegate: ctx is NULL"


def test_defaults_and_sizes():
    p = _lib.posegate_params()
    assert (p.max_nodes, p.max_edges, p.max_cand, p.append) == (48, 256, 16, 0)
    assert (p.damp_t, p.damp_r, p.nis_max) == (1e-6, 1e-3, 16.27)
    g = _lib.posegraph_params()
    assert (p.damp_t, p.damp_r, p.max_nodes, p.max_edges) == (g.damp_t, g.damp_r, g.max_nodes, g.max_edges)
    assert C.sizeof(_lib.PoseGateParams) == 40 and C.sizeof(_lib.PoseGateBatch) == 144
    assert _lib.ABI_VERSION == 6


def test_the_largest_shape_fits_the_lds():
    """(64 nodes, 1024 edges, 64 candidates) with one candidate solved at a time fits the kernel's 160 KiB; the
    package's figure is the header's (the budget is what the launcher compares with)."""
    from lidar_slam_amd import posegraph
    assert posegraph.gate_lds_bytes(64, 1024, 64, 1) <= 160 * 1024 < posegraph.gate_lds_bytes(64, 1024, 64, 2)
    assert posegraph.gate_lds_bytes(24, 256, 16, 8) < 40 * 1024
    assert posegraph.gate_slots(64, 1024, 64) == 1 and posegraph.gate_slots(24, 256, 16) == 8 and posegraph.gate_slots(24, 256, 3) == 3
