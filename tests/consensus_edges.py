"""Cases that hold the large-chunk consensus (model_kernel -> count_kernel<PPL> -> select_kernel,
launch_chunks_large in lidar_slam_amd/csrc/lslam_launch.h) to the CPU oracle at the edge of every
count form.  NumPy only: tests/test_consensus_edges.py proves from the oracle alone that each case
can see the class of error it is there for, tests/test_gpu_consensus_edges.py runs them on the GPU.

A batch is a list of chunks, each of one point family at a requested size, with explicit
hypotheses (T + 1 seeded pairs per chunk, some overwritten by planted pairs) so that the consensus
is isolated from the draw side.  Everything is deterministic: a batch depends on its key only.

Point families (threshold 20 unless a test says otherwise)
  band_axis    test_gpu_parity._border_batch chunk 1 at any size: points on y = 0 at x = 1.5 i, every
               fourth one at +-{20, nextafter(20, 0), nextafter(20, 40), 19.999999999999996,
               20.000000000000004} from it.
  band_rot     the same turned by 90 degrees and shifted (line x = 1000).
  band_slant   the same on y = 2 x, distances scaled by sqrt(5) (chunk 4's form).
  float_axis   points on y = 0, every second one at 20 (1 + k 2^-24) from it, on both sides, k over
  float_slant  FLOAT_K; the same along the normal of y = 2 x.  The count kernels test the HIGH dword
               of |r| against cutoffs two high-dword units either side of sqrt(ecut): a unit is 2^-16
               in [16, 32), so `sure in` is |r| < 20 - 2^-15 (k < -25.6) and `maybe in` is
               |r| < 20 + 3 2^-16 (k < 38.4).  FLOAT_K holds k = -27, -26, -25 and 38, 39, 40 around
               those, values far inside and outside, and k = -0.5, 0, +0.5 for float32's own ulp (the
               controls of test_consensus_edges.py).
  off_band     a slanted band at (3e5, -2e5), rebuilt there: the line through that point along
               (4, 3) / 5, every fourth point stepped off it by +-20 (-3, 4) / 5 = +-(-12, 16), which is
               exact at these coordinates (no point of y = 2 x + c can be: its distances are
               multiples of ulp / sqrt(5)), then moved by k ulps OF THE y COORDINATE, k over
               ULP_STEPS.  Every second such point is at 20 exactly, so only the rounding of the
               residual decides it; the others are whole ulps (2.9e-11) away.
  off_float    float_axis at (3e5, -2e5).
  off_wide     band_slant at (3e5, -2e5) with the x spacing stretched to a span >= 1.2e5 and the
               off-line points at line value +- 20 sqrt(5) + k ulps of the coordinate: E2 dominates
               the margin, and the residuals' own rounding (~1e-11) is as large as those steps.
  dups3, dups4 _border_batch chunks 3 and 4 grown: duplicate points, degenerate hypotheses.
  line         every point on y = 0.5 x + 3: all trials tie at M = N, sums ~1e-30, no stop.
  flat         every point on y = 7: the sum is exactly zero, the first trial stops.
  twin         two walls of equal point count, y = n_i and y = 100 - n_i at the same x (n_i a
               multiple of 1/8 in [-1, 1]): a pair far apart on one wall counts exactly that wall, so
               such hypotheses tie on the count with sums that differ, and a hypothesis and its mirror
               image have mirrored residuals.  Wall A first, then wall B.
  twin_ulp     the same with wall B stored back to front: the mirror image's squared residuals are
               the same numbers in another order of the pairwise sum, so its sum differs in the last
               ulps (about every second one) or not at all.  (Interleaving the walls point by point
               or in runs of 2 or 4 would not do: numpy's eight accumulators and their tree are
               symmetric under those swaps, and the sums come out equal.)
  cloud        uniform random points in [-3000, 3000]^2 (no ties).
  nan, inf     a cloud with one NaN coordinate; a cloud with one +-inf coordinate.
Sizes below MIN_FAMILY_N cannot carry most families' structure; they cycle through line, flat and
cloud.  A chunk of fewer than 3 points is two cloud points (no trials).

Planted hypotheses (plants(): where they sit)
  main     trials 0, 4, 8, ... (but 4): two points far apart on one of the family's lines.  Consecutive
           plants cycle through the lines with the same positions along them (twin: a hypothesis
           and then its mirror image).
  dup      trials 2, 66 and 1026: two copies of a duplicated point (a zero direction).
  twice    trials 3 and 4: the same pair.
  reverse  trial 7 and trial T - 1: a pair and its reverse.  T - 1 lies in another 64-trial flush
           group when T > 64 and in another hypothesis block when T > 1024.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

THRESHOLD = 20.0
OFFSET = (3.0e5, -2.0e5)
MIN_FAMILY_N = 16
SMALL_FAMILIES = ("line", "flat", "cloud")   # a line this short may hit a zero sum and stop

# ---- the kernel's constants, restated.  If one changes, these cases no longer sit on its edges ----
# launch_chunks_large (lslam_launch.h): count_kernel<PPL> by the batch's LARGEST chunk,
#   N <= 256 -> 1, <= 512 -> 2, <= 1024 -> 4, <= 2048 -> 8, else 16; a tile is CNT_TPB * PPL points.
# lidarslam.hip: CNT_TPB = 256, CNT_HYP_BLOCK = 1024 hypotheses per count workgroup, lane
#   accumulators flushed every 64 trials ((t & 63) == 63 || t == nt - 1); chunks of <= 128 points
#   alone take chunk_kernel (launch_chunks).
# layout_select (lslam_launch.h): select_kernel's LDS, at most 160 KiB.
CNT_TPB = 256
CNT_HYP_BLOCK = 1024
FLUSH_GROUP = 64
SMALL_CHUNK_MAX = 128
PPL_LIMITS = ((256, 1), (512, 2), (1024, 4), (2048, 8))
PPL_MAX = 16
LDS_LIMIT = 160 * 1024

# name -> (chunk sizes in the batch, T, PPL of the form the largest chunk selects)
MATRIX = {
    "n256": ((129, 130, 191, 192, 193, 255, 256, 128, 64, 3, 2), 65, 1),
    "n512": ((257, 320, 511, 512, 129, 5), 64, 2),
    "n1024": ((513, 700, 1023, 1024, 130), 127, 4),
    "n2048": ((1025, 1537, 2047, 2048, 200), 63, 8),
    "n4096": ((2049, 3000, 4095, 4096, 257), 128, 16),
    "n8200": ((4097, 8191, 8192, 8200, 300), 70, 16),
}
# times the size list is repeated: every size meets that many families
REPEATS = {"n256": 2, "n512": 3, "n1024": 4, "n2048": 4, "n4096": 4, "n8200": 4}

# hypothesis-block and flush-group edges, each at two largest chunks
HYP_EDGE_T = (0, 1, 63, 64, 65, 1023, 1024, 1025, 1087, 1088, 2049)
HYP_EDGE_SIZES = {300: (300, 299, 257, 300, 131, 200), 1025: (1025, 1025, 600, 1025, 1025, 129)}
HYP_EDGE_VARIANTS = ("band_slant", "twin", "dups4", "line", "twin_ulp", "band_axis")

THR_VARIANTS = ("band_axis", "band_rot", "band_slant", "line", "flat", "cloud")

# scans of the MT19937 batch: several chunks per scan, a flat chunk (an early stop, whose unused draws
# the following chunks replay) in the middle of three of them
MT_SCANS = (("cloud", "band_slant", "flat", "twin", "line"),
            ("float_axis", "flat", "cloud", "dups4", "band_axis"),
            ("line", "cloud", "off_band", "flat", "cloud"),
            ("twin_ulp", "dups3", "cloud", "float_slant", "band_rot"))

VARIANTS = ("band_axis", "band_rot", "band_slant", "float_axis", "float_slant", "off_band", "off_float",
            "off_wide", "dups3", "dups4", "line", "flat", "twin", "twin_ulp", "cloud", "nan", "inf")

THR5 = (20.0, float(np.nextafter(20.0, 0)), float(np.nextafter(20.0, 40)), 19.999999999999996,
        20.000000000000004)
# ordered by importance: a small chunk holds the head of the list only
FLOAT_K = (-0.5, 0.0, 0.5, -26.0, -25.0, 38.0, 39.0, -27.0, 40.0, -1.0, 1.0, -12.0, 12.0, -2.0, 2.0, -24.0,
           37.0, -3.0, 3.0, -4.0, 4.0, -5.0, 5.0, -6.0, 6.0, -7.0, 7.0, -8.0, 8.0, -9.0, 9.0, -10.0, 10.0,
           -11.0, 11.0, -16.0, 16.0, -20.0, 24.0, -32.0, 32.0, -48.0, 48.0, 56.0, -64.0, 64.0)
ULP_STEPS = (0, -1, 0, 1, 0, -2, 0, 2, 0, -3, 3)
SQRT5 = float(np.sqrt(5.0))


def ppl_of(n_max):
    """Points per lane of the count_kernel form that a batch whose largest chunk is n_max selects."""
    for lim, ppl in PPL_LIMITS:
        if n_max <= lim:
            return ppl
    return PPL_MAX


def select_lds_bytes(n_max, trials):
    """layout_select (lslam_launch.h): select_kernel's dynamic LDS for the batch's largest chunk."""
    a16 = lambda v: (v + 15) & ~15
    n, t = max(n_max, 1), max(trials, 1)
    return a16(16 * n) + 2 * a16(4 * t) + a16(8 * t) + a16(n) + a16(8 * 24) + a16(4 * 72) + a16(8 * 128)


@dataclass
class Chunk:
    variant: str
    xy: np.ndarray
    lines: list = field(default_factory=list)   # index arrays, each ordered along its line
    dups: list = field(default_factory=list)    # index arrays of identical points

    @property
    def n(self):
        return len(self.xy)

    @property
    def family(self):
        return family_of(self.variant)


def family_of(variant):
    for f in ("band", "float", "off", "dups", "twin"):
        if variant.startswith(f):
            return {"float": "float-band", "off": "offset"}.get(f, f)
    return "nonfinite" if variant in ("nan", "inf") else variant


def _step_ulps(v, k):
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def _band(n, form):
    i = np.arange(n)
    xs = 1.5 * i
    off = i % 4 == 1
    k = np.arange(int(off.sum()))
    d = np.array(THR5)[k % 5] * np.where(k % 2 == 1, 1.0, -1.0)
    ys = np.zeros(n)
    if form == "slant":
        ys = 2.0 * xs
        ys[off] = 2.0 * xs[off] + d * SQRT5
        xy = np.stack([xs, ys], 1)
    else:
        ys[off] = d
        xy = np.stack([xs, ys], 1) if form == "axis" else np.stack([ys + 1000.0, xs - 500.0], 1)
    return Chunk("band_" + form, xy, lines=[np.nonzero(~off)[0]])


def _float_dist(n_off):
    """Signed distances 20 (1 + k 2^-24) of the off-line points: k cycles through FLOAT_K, the side
    alternates with the position in the list and flips every full cycle."""
    j = np.arange(n_off)
    k = np.array(FLOAT_K)[j % len(FLOAT_K)]
    side = np.where((j + j // len(FLOAT_K)) % 2 == 0, 1.0, -1.0)
    return side * (20.0 * (1.0 + k * 2.0 ** -24))


def _float(n, form, origin=(0.0, 0.0)):
    i = np.arange(n)
    xs = 1.5 * i
    off = i % 2 == 1
    d = _float_dist(int(off.sum()))
    if form == "slant":
        x, y = xs.copy(), 2.0 * xs
        x[off] = xs[off] - 2.0 * d / SQRT5
        y[off] = 2.0 * xs[off] + d / SQRT5
    else:
        x, y = xs.copy(), np.zeros(n)
        y[off] = d
    x, y = x + origin[0], y + origin[1]   # axis: origin + d is within an ulp of the coordinate of d
    name = "float_" + form if origin == (0.0, 0.0) else "off_float"
    return Chunk(name, np.stack([x, y], 1), lines=[np.nonzero(~off)[0]])


def _off_band(n, wide):
    i = np.arange(n)
    off = i % 4 == 1
    if wide:    # slope 2, x spacing stretched; off-line points at line value +- 20 sqrt(5), moved by ulps
        lx = i * float(int(np.ceil(1.2e5 / max(n - 1, 1))))
        x, y = OFFSET[0] + lx, OFFSET[1] + 2.0 * lx          # exact at these sizes
        for j, p in enumerate(np.nonzero(off)[0]):
            side = 1.0 if j % 2 else -1.0
            y[p] = _step_ulps(y[p] + side * 20.0 * SQRT5, ULP_STEPS[j % len(ULP_STEPS)])
    else:       # direction (4, 3) / 5: the normal step 20 (-3, 4) / 5 = (-12, 16) is exact
        x, y = OFFSET[0] + 2.0 * i, OFFSET[1] + 1.5 * i
        for j, p in enumerate(np.nonzero(off)[0]):
            side = 1.0 if j % 2 else -1.0
            x[p] -= 12.0 * side
            y[p] = _step_ulps(y[p] + 16.0 * side, ULP_STEPS[j % len(ULP_STEPS)])
    return Chunk("off_wide" if wide else "off_band", np.stack([x, y], 1), lines=[np.nonzero(~off)[0]])


def _parts(n, weights):
    w = np.array(weights, float)
    c = np.floor(n * w / w.sum()).astype(int)
    c[0] += n - c.sum()
    return c


def _dups3(n):
    c = _parts(n, (30, 10, 10, 5))
    pts = ((3.0, 4.0), (3.0, 24.0), (23.0, 4.0), (100.0, 100.0))
    xy = np.concatenate([np.repeat([p], k, 0) for p, k in zip(pts, c)])
    o = np.concatenate([[0], np.cumsum(c)])
    return Chunk("dups3", xy, dups=[np.arange(o[k], o[k + 1]) for k in range(4) if c[k] >= 2])


def _dups4(n):
    c = _parts(n, (20, 15, 12))
    xa, xb = 1.5 * np.arange(c[0]), 1.5 * np.arange(c[2])
    xy = np.concatenate([np.stack([xa, 2.0 * xa], 1), np.repeat([[7.0, 14.0]], c[1], 0),
                         np.stack([xb, 2.0 * xb + 20.0 * SQRT5], 1)])
    ch = Chunk("dups4", xy, lines=[np.arange(c[0])])
    if c[1] >= 2:
        ch.dups = [np.arange(c[0], c[0] + c[1])]
    return ch


def _twin(n, interleave):
    h = n // 2
    i = np.arange(h)
    xs = 1.5 * i
    noise = ((i * 37) % 17 - 8) / 8.0
    a = np.stack([xs, noise], 1)
    b = np.stack([xs, 100.0 - noise], 1)     # exact: the mirror image in y = 50
    xy = np.empty((n, 2))
    if interleave:   # wall A, then wall B back to front
        lines = [np.arange(h), np.arange(2 * h - 1, h - 1, -1)]
        xy[lines[0]], xy[lines[1]] = a, b
    else:
        xy[:h], xy[h:2 * h] = a, b
        lines = [np.arange(h), np.arange(h, 2 * h)]
    if n % 2:   # the odd point: on the mirror axis, 50 from both walls
        xy[-1] = (1.5 * (h // 2), 50.0)
    return Chunk("twin_ulp" if interleave else "twin", xy, lines=lines)


def _cloud(n, rng, name="cloud"):
    return Chunk(name, rng.uniform(-3000.0, 3000.0, (n, 2)))


def make_chunk(variant, n, seed=0):
    """One chunk of the variant's family at n points (n >= 3; smaller: cloud points)."""
    rng = np.random.default_rng([seed, n, VARIANTS.index(variant)])
    if n < 3:
        return _cloud(n, rng)
    x = 1.5 * np.arange(n)
    if variant.startswith("band_"):
        return _band(n, variant[5:])
    if variant.startswith("float_"):
        return _float(n, variant[6:])
    if variant == "off_float":
        return _float(n, "axis", OFFSET)
    if variant in ("off_band", "off_wide"):
        return _off_band(n, variant == "off_wide")
    if variant == "dups3":
        return _dups3(n)
    if variant == "dups4":
        return _dups4(n)
    if variant == "line":
        return Chunk("line", np.stack([x, 0.5 * x + 3.0], 1), lines=[np.arange(n)])
    if variant == "flat":
        return Chunk("flat", np.stack([x, np.full(n, 7.0)], 1), lines=[np.arange(n)])
    if variant in ("twin", "twin_ulp"):
        return _twin(n, variant == "twin_ulp")
    ch = _cloud(n, rng, variant)
    if variant == "nan":
        ch.xy[n // 3, n % 2] = np.nan
    elif variant == "inf":
        ch.xy[n // 2, n % 2] = np.inf if n % 4 < 2 else -np.inf
    elif variant != "cloud":
        raise KeyError(variant)
    return ch


def plant_trials(trials):
    """Where the planted pairs sit for T trials (module docstring); later kinds overwrite earlier."""
    T = trials
    p = {"main": [t for t in range(0, T, 4)], "dup": [t for t in (2, 66, 1026) if t < T],
         "twice": (3, 4) if T >= 5 else None, "reverse": (7, T - 1) if T >= 9 else None}
    taken = set(p["dup"]) | set(p["twice"] or ()) | set(p["reverse"] or ())
    p["main"] = [t for t in p["main"] if t not in taken]
    return p


def hypotheses(ch, trials, seed):
    """draws [T + 1][2] for the chunk (distinct indices in range) and the plants that hold in it:
    {"main": [(trial, line)], "dup": [trial], "twice": (t, t') or None, "reverse": (t, t') or None}."""
    n, T = ch.n, trials
    rng = np.random.default_rng([seed, n, T, VARIANTS.index(ch.variant)])
    d = np.zeros((T + 1, 2), np.int32)
    held = {"main": [], "dup": [], "twice": None, "reverse": None}
    if n < 3:
        return d, held
    d[:, 0] = rng.integers(0, n, T + 1)
    d[:, 1] = (d[:, 0] + rng.integers(1, n, T + 1)) % n
    where = plant_trials(T)

    def far_pair(j):
        """Pair j: positions (from the first and the last quarter) shared by len(lines) consecutive
        j, each on its own line."""
        nl = len(ch.lines)
        ln = ch.lines[j % nl]
        q = np.random.default_rng([seed, n, j // nl])
        span = max(1, min(len(l) for l in ch.lines) // 4)
        a, b = int(q.integers(0, span)), int(q.integers(0, span))
        return int(ln[a]), int(ln[len(ln) - 1 - b])

    usable = [l for l in ch.lines if len(l) >= 2]
    if usable and len(usable) == len(ch.lines):
        for j, t in enumerate(where["main"]):
            d[t] = far_pair(j)
            held["main"].append((t, j % len(ch.lines)))
    for k, t in enumerate(where["dup"]):
        if ch.dups:
            g = ch.dups[k % len(ch.dups)]
            d[t] = (int(g[0]), int(g[-1]))
            held["dup"].append(t)
    if where["twice"]:
        t0, t1 = where["twice"]
        if usable and len(usable) == len(ch.lines):
            d[t0] = far_pair(10007)
        d[t1] = d[t0]
        held["twice"] = (t0, t1)
    if where["reverse"]:
        t0, t1 = where["reverse"]
        if usable and len(usable) == len(ch.lines):
            d[t0] = far_pair(10009)
        d[t1] = d[t0][::-1]
        held["reverse"] = (t0, t1)
    return d, held


@dataclass
class Batch:
    name: str
    chunks: list
    trials: int
    scan_chunk_off: np.ndarray
    draws: np.ndarray            # [C][T + 1][2]
    plants: list                 # per chunk, hypotheses()'s second value

    @property
    def sizes(self):
        return [c.n for c in self.chunks]

    @property
    def chunk_pt_off(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)

    @property
    def xy(self):
        return np.concatenate([c.xy for c in self.chunks])

    def label(self, c):
        ch = self.chunks[c]
        return "batch %s chunk %d: N = %d, family %s (%s), T = %d" % (self.name, c, ch.n, ch.family, ch.variant,
                                                                    self.trials)


def _assemble(name, sized_variants, trials, per_scan, seed, as_given=False):
    chunks, small = [], 0
    for n, v in sized_variants:
        if 3 <= n < MIN_FAMILY_N and not as_given:   # the batch's k-th small chunk: line, flat, cloud in turn
            v = SMALL_FAMILIES[small % len(SMALL_FAMILIES)]
            small += 1
        chunks.append(make_chunk(v, n, seed))
    C = len(chunks)
    hyp = [hypotheses(ch, trials, seed + 1000 * c) for c, ch in enumerate(chunks)]
    if isinstance(per_scan, int):
        sco = np.append(np.arange(0, C, per_scan), C)
    else:
        sco = np.concatenate([[0], np.cumsum(per_scan)])
    return Batch(name, chunks, trials, sco.astype(np.int32), np.stack([h[0] for h in hyp]), [h[1] for h in hyp])


@functools.lru_cache(maxsize=None)
def matrix_batch(name, variants=VARIANTS):
    """The shape-matrix entry `name`: its size list REPEATS[name] times, chunk j of the batch taking
    variant (j + its position in MATRIX) of `variants` in turn (17 variants, a prime, so every size
    meets different families in every repeat and in every entry); scans of three chunks."""
    sizes, T, _ = MATRIX[name]
    k = list(MATRIX).index(name)
    sv = [(n, variants[(r * len(sizes) + i + k) % len(variants)]) for r in range(REPEATS[name])
          for i, n in enumerate(sizes)]
    tag = name if variants is VARIANTS else name + "/" + "+".join(sorted(set(variants)))
    return _assemble(tag, sv, T, 3, 100 + k)


@functools.lru_cache(maxsize=None)
def hyp_edge_batch(n_max, trials):
    """Largest chunk n_max (300: PPL 2; 1025: PPL 8) with T at a flush-group or hypothesis-block edge."""
    sv = list(zip(HYP_EDGE_SIZES[n_max], HYP_EDGE_VARIANTS))
    return _assemble("hyp%d/T%d" % (n_max, trials), sv, trials, 2, 200 + n_max)


@functools.lru_cache(maxsize=None)
def mt_batch():
    """The n1024 sizes, one scan per repeat, with MT_SCANS' families (the draws come from the kernel's
    MT19937 streams here: `draws` and `plants` are unused)."""
    sizes, T, _ = MATRIX["n1024"]
    sv = [(n, v) for scan in MT_SCANS for n, v in zip(sizes, scan)]
    return _assemble("n1024/mt19937", sv, T, len(sizes), 300)


# MT19937 replays over ragged scans.  A scan with an early stop is replayed whole by the fix-up kernel,
# each chunk through mt_draws with its own slot count (mt_nslot, lslam_rng.h: 64 slots at 3 points, 8
# from 17 to 512, 2 above 512), in tables that build_args sizes once per batch: every entry starts with a
# flat chunk (the stop) and mixes sizes from several of those regimes under one largest chunk.
# name -> ((variant, size) per chunk of the one scan, T)
MT_RAGGED = {
    "n100": ((("flat", 40), ("cloud", 10), ("cloud", 3), ("cloud", 5), ("cloud", 100), ("cloud", 17)), 100),
    "n513": ((("flat", 64), ("cloud", 513), ("cloud", 130), ("cloud", 512), ("cloud", 9)), 127),
    "n1024": ((("flat", 64), ("cloud", 1024), ("cloud", 130)), 40),
}


@functools.lru_cache(maxsize=None)
def mt_ragged_batch(name):
    """MT_RAGGED[name] as two scans of the same chunks (other seeds, other stream positions)."""
    spec, T = MT_RAGGED[name]
    sv = [(n, v) for _ in range(2) for v, n in spec]
    return _assemble("ragged-" + name + "/mt19937", sv, T, len(spec), 400, as_given=True)


def all_explicit_batches():
    """Every batch the GPU file runs with explicit hypotheses at threshold 20."""
    out = [matrix_batch(k) for k in MATRIX]
    out += [hyp_edge_batch(n, t) for n in HYP_EDGE_SIZES for t in HYP_EDGE_T]
    return out


@functools.lru_cache(maxsize=None)
def oracle_batch(batch_fn, *args, thr=THRESHOLD):
    """oracle.cpu.ransac(want_trials=True) on every chunk of batch_fn(*args) with its explicit
    hypotheses: a list of (mask, model dict, cnt [T], sum [T]).  Cached: computed once, shared."""
    from oracle import cpu
    b = batch_fn(*args)
    out = []
    for c, ch in enumerate(b.chunks):
        mask, md, ex = cpu.ransac(ch.xy, thr, b.trials, hyp=b.draws[c], want_trials=True)
        out.append((mask, md, ex["cnt"].copy(), ex["sum"].copy()))
    return out


# ---- wrong counts, restated in plain float64 NumPy (controls of the band families) ----
def _models(P, draws):
    A, B = P[draws[:, 0]], P[draws[:, 1]]
    o = (A + B) / 2
    d = (B - o) - (A - o)
    nrm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(nrm[:, None] != 0, d / nrm[:, None], d)
    return o, u


def _cross(P, draws):
    o, u = _models(P, draws)
    with np.errstate(invalid="ignore", over="ignore"):
        return (P[None, :, 0] - o[:, None, 0]) * u[:, None, 1] - (P[None, :, 1] - o[:, None, 1]) * u[:, None, 0]


def control_counts(P, draws, ecut, which):
    """Per-trial counts [T] of a WRONG inlier test:
      a  r = (x - ox) uy - (y - oy) ux;  r^2 < ecut, no deferral to the reference's residual
      b  float32(|r|) <  float32(sqrt(ecut))
      c  float32(|r|) <= float32(sqrt(ecut))"""
    r = _cross(np.asarray(P, np.float64), np.asarray(draws)[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        if which == "a":
            return np.sum(r * r < ecut, axis=1)
        a32, c32 = np.abs(r).astype(np.float32), np.float32(np.sqrt(ecut))
        return np.sum(a32 < c32 if which == "b" else a32 <= c32, axis=1)


# the variants each control must disagree with the oracle on.  (a) needs a line that is not
# axis-parallel: on y = c or x = c the direction is (+-1, 0) or (0, +-1) exactly and both the cross
# product and the reference's projection reduce to fl(d^2) of the same exact d, so band_axis,
# band_rot, float_axis and off_float cannot tell them apart.  (b), (c) apply to the float-band chunks.
CONTROL_VARIANTS = {"a": ("band_slant", "off_band", "off_wide"),
                    "b": ("float_axis", "float_slant", "off_float"),
                    "c": ("float_axis", "float_slant", "off_float")}
