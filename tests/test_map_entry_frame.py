"""The checks every map-side entry point makes before it needs a device, in their order: params, batch,
negative size, missing input, missing output, context.  One table of the eleven entries; the 22 "missing"
lines are literals, so the texts are pinned and not only the names in them.  No device is used: every call
passes ctx = NULL and reads lslam_last_error()."""
import ctypes as C
import re

import pytest

from lidar_slam_amd import _lib

# name: (batch class, the params in the C argument order as (prefix of "params is NULL", factory) with None
# for an optional params pointer that the test leaves NULL, the batch's size field, its optional pointers,
# the "missing input" line, the "missing output" line)
ENTRIES = {
    "lslam_scan_match": (
        _lib.MatchBatch, (("match", _lib.match_params), None), "n_scans", {"scores", "ukf_u"},
        b"match: missing input (ref_xy, ref_off, cur_xy, cur_off, rot)",
        b"match: missing output (delta, best, n_valid, flags)"),
    "lslam_grid_update": (
        _lib.GridBatch, (("grid", _lib.grid_params),), "n_robots", set(),
        b"grid: missing input (xy, pt_off, pose, origin)",
        b"grid: missing output (logodds, rot, n_used, flags)"),
    "lslam_map_match": (
        _lib.MapMatchBatch, (("grid", _lib.grid_params), ("mapmatch", _lib.mapmatch_params)), "n_robots", {"scores"},
        b"mapmatch: missing input (xy, pt_off, pose, origin, logodds, rot)",
        b"mapmatch: missing output (pose_out, delta, best, n_valid, rot0, flags)"),
    "lslam_map_fuse": (
        _lib.MapFuseBatch,
        (("grid", _lib.grid_params), ("mapmatch", _lib.mapmatch_params), ("mapfuse", _lib.mapfuse_params)),
        "m.n_robots", {"m.scores", "moments"},
        b"mapfuse: missing input (xy, pt_off, pose, origin, logodds, rot, P)",
        b"mapfuse: missing output (pose_out, delta, best, n_valid, rot0, flags, P_out, z, Rm, nis)"),
    "lslam_map_relocalize": (
        _lib.RelocBatch,
        (("grid", _lib.grid_params), ("mapmatch", _lib.mapmatch_params), ("reloc", _lib.reloc_params)),
        "n_robots", {"P_out", "coarse_scores"},
        b"reloc: missing input (xy, pt_off, origin, logodds, rot, head_rot)",
        b"reloc: missing output (n_occ, n_used, cand, cand_pose, fine_pose, fine_delta, fine_best, "
        b"fine_nvalid, fine_rot0, fine_flags, result, flags, pose_out)"),
    "lslam_grid_raycast": (
        _lib.RaycastBatch, (("grid", _lib.grid_params), ("raycast", _lib.raycast_params)), "n_robots", {"stop"},
        b"raycast: missing input (xy, pt_off, pose, origin, logodds)",
        b"raycast: missing output (cls, counts, rot, flags)"),
    "lslam_grid_recentre": (
        _lib.RecentreBatch, (("grid", _lib.grid_params), ("recentre", _lib.recentre_params)), "n_robots", set(),
        b"recentre: missing input (pose, origin, logodds)",
        b"recentre: missing output (shift, flags)"),
    "lslam_grid_distance": (
        _lib.DistBatch, (("grid", _lib.grid_params), ("dist", _lib.dist_params)), "n_robots", set(),
        b"dist: missing input (logodds)",
        b"dist: missing output (d2, n_src, flags)"),
    "lslam_field_score": (
        _lib.FieldScoreBatch, (("grid", _lib.grid_params), ("fieldscore", _lib.fieldscore_params)), "n_robots", set(),
        b"fieldscore: missing input (xy, pt_off, pose, origin, d2)",
        b"fieldscore: missing output (rot, stats, clear2, flags)"),
    "lslam_field_align": (
        _lib.FieldAlignBatch, (("grid", _lib.grid_params), ("fieldalign", _lib.fieldalign_params)), "n_robots", set(),
        b"fieldalign: missing input (xy, pt_off, pose, origin, d2)",
        b"fieldalign: missing output (pose_out, trace, normal, n_used, iters, flags)"),
    "lslam_field_fuse": (
        _lib.FieldFuseBatch,
        (("grid", _lib.grid_params), ("fieldalign", _lib.fieldalign_params), ("fieldfuse", _lib.fieldfuse_params)),
        "a.n_robots", set(),
        b"fieldfuse: missing input (xy, pt_off, pose, origin, d2, P)",
        b"fieldfuse: missing output (pose_out, trace, normal, n_used, iters, flags, P_out, z, info, info_f, s2, nis)"),
}


def pointer_paths(cls, prefix=""):
    """Dotted paths of every pointer field of a batch Structure, the embedded batch's included."""
    out = []
    for name, typ in cls._fields_:
        if typ is C.c_void_p:
            out.append(prefix + name)
        elif issubclass(typ, C.Structure):
            out += pointer_paths(typ, prefix + name + ".")
    return out


def put(b, path, value):
    *owners, leaf = path.split(".")
    for o in owners:
        b = getattr(b, o)
    setattr(b, leaf, value)


def full_batch(cls, n_field, n=1):
    """Every pointer a dummy address of its own, 4 GiB apart (nothing is dereferenced without a context)."""
    b = cls()
    put(b, n_field, n)
    for i, path in enumerate(pointer_paths(cls)):
        put(b, path, (i + 1) << 32)
    return b


def call(name, b, params):
    """(status, message): the message is lslam_last_error(), and the text that _lib.check raises carries it."""
    L = _lib.load()
    st = getattr(L, name)(None, None if b is None else C.byref(b), *[None if p is None else C.byref(p) for p in params])
    msg = L.lslam_last_error()
    assert st == _lib.LSLAM_ERR_ARG  # (no context: no call here can succeed)
    with pytest.raises(ValueError) as e:
        _lib.check(st, name)
    assert "(%s)" % msg.decode() in str(e.value) and msg == L.lslam_last_error()
    return st, msg


def make_params(spec):
    return [None if s is None else s[1]() for s in spec]


@pytest.mark.parametrize("name", list(ENTRIES))
def test_params_batch_and_size_come_before_the_context(name):
    cls, spec, n_field, optional, _, _ = ENTRIES[name]
    for i, s in enumerate(spec):
        if s is None:
            continue
        params = make_params(spec)
        params[i] = None
        assert call(name, full_batch(cls, n_field), params)[1] == ("%s: params is NULL" % s[0]).encode()
    prefix = ENTRIES[name][4].split(b":")[0]
    assert call(name, None, make_params(spec))[1] == prefix + b": batch is NULL"
    msg = call(name, full_batch(cls, n_field, -1), make_params(spec))[1]
    assert msg == prefix + b": negative " + n_field.split(".")[-1].encode()
    assert call(name, full_batch(cls, n_field), make_params(spec))[1] == prefix + b": ctx is NULL"
    # an empty batch needs no pointer, and the context is asked for before the batch is found empty
    assert call(name, cls(), make_params(spec))[1] == prefix + b": ctx is NULL"


@pytest.mark.parametrize("name", list(ENTRIES))
def test_every_pointer_is_required_or_optional(name):
    cls, spec, n_field, optional, missing_in, missing_out = ENTRIES[name]
    prefix = missing_in.split(b":")[0]
    names = {line: re.fullmatch(rb"\w+: missing (?:in|out)put \((.*)\)", line).group(1).decode().split(", ")
             for line in (missing_in, missing_out)}
    paths = pointer_paths(cls)
    leaves = [p.split(".")[-1] for p in paths]
    assert len(set(leaves)) == len(leaves)  # (the lines name leaves: they must tell the fields apart)
    assert optional <= set(paths)
    # the two lines name every pointer that is not optional, each once, and nothing else
    assert sorted(names[missing_in] + names[missing_out]) == sorted(p.split(".")[-1] for p in paths if p not in optional)
    for path in paths:
        b = full_batch(cls, n_field)
        put(b, path, None)
        msg = call(name, b, make_params(spec))[1]
        if path in optional:
            assert msg == prefix + b": ctx is NULL", path
        else:
            assert msg == (missing_in if path.split(".")[-1] in names[missing_in] else missing_out), path
