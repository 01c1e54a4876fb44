"""The 3 x 3 algebra of lslam_field_fuse (lidar_slam_amd/csrc/lslam_fieldfuse_core.h), compiled with g++
on the CPU: the text the kernel compiles.  The program has its own main and is built with
-fsanitize=address,undefined when the compiler here can link an empty program with them, and with
-ffp-contract=off as the library is.  Nothing sanitised is loaded into Python.

It is fed rows of (the alignment's ten sums, n_last, x, P, z, cell and the five parameters) and its
outputs (flags, s2, info, info_f, nis, the updated mean and covariance or the input bits) are held to
tests/fieldfuse_ref.fuse_steps bit for bit: the room's alignments under seven priors and both floors, and
the rule cases (the gate at its edge, every cause of BAD_COV, floors that overflow, no point used, sums at
the ends of int64, a NaN's payload in P and in x).

What the GPU tests alone cover is the kernel around these functions: step 5, the loads and stores, the
flag word.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fieldalign_ref as far
import fieldfuse_ref as ffr
from test_fieldalign_ref import ROOM_DISPLACEMENTS, room  # noqa: F401
from test_fieldfuse_ref import CELL, CORRIDOR_POSE, CORRIDOR_PTS, P_CORRIDOR, P_ROOM, TIGHT, corridor_fuse, room_aligns
from test_mapfuse_ref import CORR, SCALES, nan_payload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_slam_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
PARAMS = ("sigma_min", "r_scale", "floor_t", "floor_r", "nis_max")

PROG = r"""
#include "lslam_fieldfuse_core.h"
#include <cstdio>
#include <cstring>
#include <vector>

// in: rows of 32 words: int64 N[10], n_last, then doubles x[3], P[9], z[3], cell, sigma_min, r_scale, floor_t,
//     floor_r, nis_max
// out: rows of 33 words: flags, then the bits of s2, info[9], info_f[9], nis, pose_out[3], P_out[9]
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb"), *g = std::fopen(argv[2], "wb");
    if (!f || !g) return 2;
    int64_t row[32];
    while (std::fread(row, 8, 32, f) == 32) {
        double d[21];
        std::memcpy(d, row + 11, sizeof(d));
        double x[3], P[9], z[3];
        std::memcpy(x, d, 24);
        std::memcpy(P, d + 3, 72);
        std::memcpy(z, d + 12, 24);
        const FieldFuseConsts k = fieldfuse_consts(d[15], d[16], d[17], d[18], d[19], d[20]);
        double s2, nis, info[9], info_f[9], xo[3], Po[9];
        const int fl = fieldfuse_steps(row, (int)row[10], k, x, P, z, s2, info, info_f, nis, xo, Po);
        int64_t o[33];
        o[0] = fl;
        std::memcpy(o + 1, &s2, 8);
        std::memcpy(o + 2, info, 72);
        std::memcpy(o + 11, info_f, 72);
        std::memcpy(o + 20, &nis, 8);
        std::memcpy(o + 21, fl ? x : xo, 24);  // (as the kernel: the input bits unless updated)
        std::memcpy(o + 24, fl ? P : Po, 72);
        if (std::fwrite(o, 8, 33, g) != 33) return 2;
    }
    std::fclose(f);
    return std::fclose(g) ? 2 : 0;
}
"""


def _compiles(cmd, src, exe):
    return subprocess.run(cmd + [str(src), "-o", str(exe)], capture_output=True).returncode == 0


@pytest.fixture(scope="module")
def core(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("fieldfuse_core")
    empty = d / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", CSRC]
    san = SAN if _compiles(["g++", "-std=c++17"] + SAN, empty, d / "empty") else []
    src = d / "t.cpp"
    src.write_text(PROG)
    exe = d / "t"
    subprocess.check_call(base + san + [str(src), "-o", str(exe)])
    return str(exe), d


def run_rows(core, rows):
    """rows: (al, x, P, cell, fp) with al an alignment that was accepted.  Every output against fuse_steps."""
    exe, d = core
    buf = np.zeros((len(rows), 32), np.int64)
    for i, (al, x, P, cell, fp) in enumerate(rows):
        buf[i, :10] = al["normal"]
        buf[i, 10] = al["n_used"][1]
        dbl = np.concatenate([np.asarray(x, np.float64), np.asarray(P, np.float64).reshape(9), np.asarray(al["pose_out"], np.float64),
                              [cell], [fp[k] for k in PARAMS]])
        buf[i, 11:] = dbl.view(np.int64)
    buf.tofile(str(d / "in.bin"))
    out = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(str(d / "out.bin"), np.int64).reshape(len(rows), 33)
    flags = []
    for i, (al, x, P, cell, fp) in enumerate(rows):
        assert not al["flags"] & far.KEEP
        w = ffr.fuse_steps(al, x, P, cell, fp)
        want = np.concatenate([[w["s2"]], w["info"].reshape(9), w["info_f"].reshape(9), [w["nis"]], w["pose_out"], w["P_out"].reshape(9)])
        assert got[i, 0] == w["flags"] & (ffr.OUTLIER | ffr.BAD_COV), (i, got[i, 0], w["flags"])
        assert got[i, 1:].tolist() == np.asarray(want, np.float64).view(np.int64).tolist(), (i, np.flatnonzero(got[i, 1:] != want.view(np.int64)))
        flags.append(int(got[i, 0]))
    return np.array(flags)


def test_room(core, room):
    rows = []
    priors = [P_ROOM, np.diag([25.0, 25.0, 1e-6])]
    for scale in [tuple(np.diag(P_ROOM))] + SCALES:
        d = np.sqrt(np.array(scale))
        priors.append(CORR * d[:, None] * d[None, :])
    for disp in ROOM_DISPLACEMENTS:
        guess, als = room_aligns(room, 4, disp)
        for r, al in enumerate(als):
            for P in priors:
                for over in ({}, TIGHT, dict(r_scale=3.0, sigma_min=1.25, nis_max=np.inf)):
                    rows.append((al, guess[r], P, CELL, dict(ffr.DEFAULTS, **over)))
    flags = run_rows(core, rows)
    assert len(rows) == 2 * 8 * 7 * 3 and (flags == 0).sum() > 200 and (flags == ffr.OUTLIER).sum() >= 16 and not (flags & ffr.BAD_COV).any()


def hand(normal, n_last, z):
    return dict(flags=far.CONVERGED, pose_out=np.array(z, np.float64), n_used=np.array([n_last, n_last, n_last], np.int32),
                normal=np.array(normal, np.int64))


def test_rules(core):
    fp = dict(ffr.DEFAULTS)
    al = corridor_fuse()
    nis = float(al["nis"])
    al = dict(al, pose_out=al["z"])  # back to the alignment's own dict: pose_out is the aligned pose
    x = CORRIDOR_POSE
    rows = [(al, x, P_CORRIDOR, 100.0, fp), (al, x, P_CORRIDOR, 100.0, dict(fp, nis_max=nis)),
            (al, x, P_CORRIDOR, 100.0, dict(fp, nis_max=float(np.nextafter(nis, 0.0)))), (al, x, P_CORRIDOR, 100.0, dict(fp, nis_max=5e-324)),
            (al, x, np.zeros((3, 3)), 100.0, fp), (al, x, P_CORRIDOR, 100.0, dict(fp, floor_t=1e-160)),
            (al, x, P_CORRIDOR, 100.0, dict(fp, floor_r=1e-170)), (al, x, P_CORRIDOR, 100.0, dict(fp, r_scale=1e308, sigma_min=1e10)),
            (al, x, P_CORRIDOR, 100.0, dict(fp, r_scale=5e-324)), (al, x, P_CORRIDOR * 1e-300, 100.0, fp),
            (al, x, P_CORRIDOR * 1e290, 100.0, fp), (al, np.array([1600.0, nan_payload(), 0.0]), P_CORRIDOR, 100.0, fp)]
    for at, value in (((0, 1), np.nan), ((2, 2), nan_payload()), ((1, 1), np.inf), ((0, 2), -np.inf), ((0, 0), -1e4), ((1, 1), -1e4),
                      ((2, 2), -1.0), ((0, 1), 150.0 ** 2), ((0, 1), 2e4)):
        P = np.array(P_CORRIDOR)
        P[at] = value
        rows.append((al, x, P, 100.0, fp))
    big = 2 ** 62
    sums = [[0] * 10, [4 << 20, 1 << 20, 0, 6 << 20, 0, 900 << 20, 0, 0, 0, 3 << 20], [1, 0, 0, 0, 0, 0, 1, 1, 1, 1],
            [big, 0, 0, big, 0, big, -big, big, -big, big], [big] * 6 + [-big, big, -big, big], [2 ** 63 - 1] * 10, [-2 ** 63] * 10,
            [-5, 0, 0, 7, 0, 9, 1, 2, 3, 4], [4 << 20, 2 << 21, 0, 4 << 20, 0, 9 << 20, 1, 2, 3, -4]]
    for N in sums:
        for n_last in (0, 1, 700):
            rows.append((hand(N, n_last, [12.0, -7.0, 0.004]), np.array([10.0, -5.0, 0.001]), P_ROOM, 20.0, fp))
            rows.append((hand(N, n_last, [12.0, -7.0, 0.004]), np.array([10.0, -5.0, 0.001]), P_ROOM, 1000.0 / 3.0, dict(fp, **TIGHT)))
    flags = run_rows(core, rows)
    assert flags[:4].tolist() == [0, 0, ffr.OUTLIER, ffr.OUTLIER] and flags[4:7].tolist() == [ffr.BAD_COV] * 3
    assert (flags[12:19] == ffr.BAD_COV).all() and (flags == 0).sum() > 20 and (flags & ffr.BAD_COV).sum() > 12
