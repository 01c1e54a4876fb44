"""The argument forms of the map-side wrappers and of ``LidarOdometry.step`` (lidar_slam_amd/staging.py).

Every method that takes a revolution accepts it as host arrays, as a ``DeviceArray`` read in place and as
a ``MapInput`` from ``LandmarkMap.upload``; every method that takes a pose accepts a host array, a float64
``DeviceArray`` and a ``LandmarkMap``.  Whatever the form, ``results()`` must hold the same bytes.  What
the kernels compute is held to the NumPy definitions elsewhere; here only the staging is under test, so
two robots of 37 and 64 points do.  The revolution is a slice of a longer ``xy``: seven points lie before
it and five behind it, so a form that lost the first point offset (or read past the last) reads others.
Each wrapper's parameters are those of the smallest case of its own GPU test file, named beside them.
"""
import numpy as np
import pytest

from test_gpu_mapfuse import MKW
from test_gpu_occgrid import nasty_points
from test_gpu_raycast import random_map
from test_gpu_reloc import fine_kw

pytestmark = pytest.mark.gpu

R, SIZES, BEFORE, BEHIND = 2, (37, 64), 7, 5
P_PRIOR = np.tile(np.diag([400.0 ** 2, 400.0 ** 2, 0.02 ** 2]), (R, 1, 1))  # a filter that any match may move


@pytest.fixture(scope="module")
def ctx():
    from lidar_slam_amd.device import Context
    if Context.device_count() < 1:
        pytest.skip("no HIP device")
    return Context(0)


def revolution(rng, W, cell, max_range):
    """(xy, scan_chunk_off, chunk_pt_off): one chunk per robot between a chunk of BEFORE points and one
    of BEHIND points that belong to no robot, all of them points that would count if they were read."""
    parts = [nasty_points(rng, n, W, cell, max_range) for n in (BEFORE,) + SIZES + (BEHIND,)]
    cpo = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
    return np.concatenate(parts), np.arange(1, R + 2, dtype=np.int32), cpo


def poses_in(rng, W, cell, origin=None):
    """[R, 3]: poses in the middle half of a grid of W cells (centred on (0, 0) unless origin is given)."""
    lo = -0.5 * W * cell if origin is None else origin
    return np.concatenate([lo + rng.uniform(0.25, 0.75, (R, 2)) * W * cell, rng.uniform(-3.0, 3.0, (R, 1))], 1)


class Case:
    """One method of one wrapper.  ``fresh()`` makes the wrapper (and what it reads) anew, ``call(obj,
    rev, pose)`` runs the method on a revolution (the positional arguments) and a pose, ``read(obj)``
    gives the dictionary to compare."""

    takes_revolution = takes_pose = True

    def __init__(self, ctx):
        self.ctx, self.rng = ctx, np.random.default_rng(sum(map(ord, type(self).__name__)))
        self.setup()

    def grid(self, L0=None, origin=None):
        from lidar_slam_amd.mapping import OccupancyGrid
        g = OccupancyGrid(self.ctx, R, origin=origin, **self.GKW)
        if L0 is not None:
            g.upload(L0)
        return g

    def scene(self, origin=None, occupied=0.1):
        """A random map, a revolution and poses for the grid parameters GKW."""
        W, cell = self.GKW["grid_w"], self.GKW["cell"]
        self.L0 = random_map(self.rng, R, W, occupied=occupied)
        self.rev = revolution(self.rng, W, cell, self.GKW.get("max_range", 8000.0))
        self.poses = poses_in(self.rng, W, cell, origin)


class GridStep(Case):
    GKW = dict(grid_w=16, cell=10.0, max_range=40960.0)  # test_gpu_occgrid.test_tile_seams

    def setup(self):
        self.scene(origin=0.0)

    def fresh(self):
        return self.grid(origin=(0.0, 0.0))

    def call(self, g, rev, pose):
        g.step(*rev, pose=pose)

    def read(self, g):
        return g.results()


class GridRecentre(Case):
    GKW = dict(grid_w=52, cell=20.0)  # test_gpu_recentre.test_every_shift_class
    takes_revolution = False

    def setup(self):
        self.scene()
        self.poses[:, :2] = [[-400.0, 250.0], [90.0, -515.0]]  # off the middle: both grids roll

    def fresh(self):
        return self.grid(self.L0)

    def call(self, g, rev, pose):
        g.recentre(pose, margin=26, quantum=1)

    def read(self, g):
        return dict(g.recentre_results(), logodds=g.logodds.download())


class CasterStep(Case):
    GKW = dict(grid_w=52, cell=100.0, max_range=3000.0)  # test_gpu_raycast.test_width_52

    def setup(self):
        self.scene()

    def fresh(self):
        from lidar_slam_amd.mapping import GridRayCaster
        return GridRayCaster(self.grid(self.L0))

    def call(self, rc, rev, pose):
        rc.step(*rev, pose=pose)

    def read(self, rc):
        return rc.results()


class FieldScore(Case):
    GKW = dict(grid_w=64, cell=100.0, max_range=3000.0)  # test_gpu_fieldscore.test_long_revolution_and_many_robots
    DKW = dict(d_max=12)

    def setup(self):
        self.scene(occupied=0.05)

    def fresh(self):
        from lidar_slam_amd.mapping import DistanceField
        f = DistanceField(self.grid(self.L0), **self.DKW)
        f.step()
        return f

    def call(self, f, rev, pose):
        f.score(*rev, pose=pose)

    def read(self, f):
        return f.score_results()


class FieldAlign(FieldScore):
    GKW = dict(grid_w=16, cell=500.0, max_range=3000.0)  # test_gpu_fieldalign.test_small_and_nasty
    DKW = dict(d_max=4, min_points=3)

    def call(self, f, rev, pose):
        f.align(*rev, pose=pose)

    def read(self, f):
        return f.align_results()


class FieldFuse(FieldScore):
    """The pose forms of a fuse are the filter's: a ``LandmarkMap``, or x and P on the device."""
    GKW = dict(grid_w=16, cell=500.0, max_range=3500.0)  # test_gpu_fieldfuse.test_shapes
    DKW = dict(d_max=4, trunc=4.0, min_points=3, min_permille=0, max_shift=np.inf, max_turn=np.inf)
    filter_only = True

    def call(self, f, rev, filt):
        f.fuse(*rev, write_back=False, **filt)

    def read(self, f):
        return f.fuse_results()


class LocStep(Case):
    GKW = dict(grid_w=16, cell=100.0)  # test_gpu_mapmatch.test_overhang
    MKW = dict(win_w=16, k_trans=4, k_theta=2, min_permille=100)

    def setup(self):
        self.scene(occupied=0.3)

    def fresh(self):
        from lidar_slam_amd.localize import GridLocalizer
        return GridLocalizer(self.ctx, R, **self.MKW), self.grid(self.L0)

    def call(self, o, rev, pose):
        o[0].step(*rev, grid=o[1], pose=pose, want_scores=True)

    def read(self, o):
        return o[0].results()


class LocFuse(LocStep):
    GKW = dict(grid_w=32, cell=100.0)  # test_gpu_mapfuse.test_batch_sizes
    MKW = dict(MKW, smear=2, min_permille=100)
    filter_only = True

    def call(self, o, rev, filt):
        o[0].fuse(*rev, grid=o[1], write_back=False, want_scores=True, **filt)


class Relocalize(Case):
    GKW = dict(grid_w=32, cell=100.0)  # test_gpu_reloc.test_ties_and_few_peaks
    MKW, QKW = fine_kw(4, smear=0, min_permille=0)
    QKW = dict(QKW, factor=4, n_cand=3)
    takes_pose = False

    def setup(self):
        self.scene(occupied=0.3)

    def fresh(self):
        from lidar_slam_amd.localize import GridRelocalizer
        return GridRelocalizer(self.ctx, R, **self.MKW, **self.QKW), self.grid(self.L0)

    def call(self, o, rev, pose):
        o[0].relocalize(*rev, grid=o[1], want_coarse=True)

    def read(self, o):
        return o[0].results()


class RelocalizePrior(Relocalize):
    """With the field and a window: the pose forms are the window's."""
    GKW = dict(grid_w=36, cell=50.0)  # test_gpu_relocprior.test_odd_widths
    MKW, QKW = fine_kw(4)
    QKW = dict(QKW, factor=4, n_cand=6, half_xy=600.0, half_theta=2.0)
    takes_pose = True

    def fresh(self):
        from lidar_slam_amd import _lib
        from lidar_slam_amd.mapping import DistanceField
        rel, g = Relocalize.fresh(self)
        field = DistanceField(g, mode=_lib.DIST_NOT_FREE, d_max=255)
        field.step()
        return rel, g, field

    def call(self, o, rev, pose):
        o[0].relocalize(*rev, grid=o[1], want_coarse=True, field=o[2], window=pose)


class OdometryStep(Case):
    """Two steps: the first stores the revolution, the second matches the next one against it."""
    GKW = dict(grid_w=64, cell=100.0)  # test_gpu_scanmatch.test_small_and_nasty
    takes_pose = False

    def setup(self):
        self.scene()
        self.rev2 = revolution(self.rng, 64, 100.0, 3000.0)

    def fresh(self):
        from lidar_slam_amd.odometry import LidarOdometry
        from lidar_slam_amd.slam import LandmarkMap
        return LidarOdometry(self.ctx, R, smear=1, k_trans=2, k_theta=2, **self.GKW), LandmarkMap(self.ctx, R)

    def call(self, o, rev, pose):
        o[0].step(*rev, lm=o[1])

    def read(self, o):
        return dict(o[0].results() or {}, lm_u=o[1].u.download())


CASES = [GridStep, GridRecentre, CasterStep, FieldScore, FieldAlign, FieldFuse, LocStep, LocFuse, Relocalize, RelocalizePrior,
         OdometryStep]


def revolution_forms(ctx, lm, xy, sco, cpo):
    return {"host": (xy, sco, cpo), "device": (ctx.to_device(xy), sco, cpo), "staged": (lm.upload(xy, sco, cpo),)}


def pose_forms(ctx, case):
    """The forms of a pose; of the filter (``lm``, or ``x`` and ``P``) where the method fuses."""
    from lidar_slam_amd.slam import LandmarkMap
    lm = LandmarkMap(ctx, R, x0=case.poses, P0=P_PRIOR)
    if getattr(case, "filter_only", False):
        x, P = ctx.to_device(case.poses), ctx.to_device(P_PRIOR.reshape(R, 9))
        return {"x and P": dict(x=x, P=P), "lm": dict(lm=lm)}
    return {"host": case.poses, "device": ctx.to_device(case.poses), "lm": lm}


def assert_same_bytes(got, what):
    """Every dictionary of ``got`` {form: results} holds the keys and the bytes of the first."""
    (first, want), *others = got.items()
    assert want and any(np.asarray(v).any() for v in want.values() if v is not None), (what, "nothing was computed")
    for form, res in others:
        assert res.keys() == want.keys(), (what, form)
        for key, w in want.items():
            g = res[key]
            if w is None or g is None:
                assert w is None and g is None, (what, form, key)
                continue
            g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, form, "against " + first, key)


@pytest.mark.parametrize("case", [c for c in CASES if c.takes_revolution], ids=lambda c: c.__name__)
def test_revolution_forms(ctx, case):
    from lidar_slam_amd.slam import LandmarkMap
    c = case(ctx)
    pose = next(iter(pose_forms(ctx, c).values()))
    revs = [c.rev] + ([c.rev2] if hasattr(c, "rev2") else [])
    forms = [revolution_forms(ctx, LandmarkMap(ctx, R), *rev) for rev in revs]
    got = {}
    for form in forms[0]:
        obj = c.fresh()
        for f in forms:
            c.call(obj, f[form], pose)
        got[form] = c.read(obj)
    assert_same_bytes(got, case.__name__)


@pytest.mark.parametrize("case", [c for c in CASES if c.takes_pose], ids=lambda c: c.__name__)
def test_pose_forms(ctx, case):
    c = case(ctx)
    got = {}
    for form, pose in pose_forms(ctx, c).items():
        obj = c.fresh()
        c.call(obj, c.rev, pose)
        got[form] = c.read(obj)
    assert_same_bytes(got, case.__name__)
