"""The cases of farthest-point sampling on a cell grid (``geometry.fps(method="grid")``, csrc/fps_grid.hip), seeded; shared by the
host and the GPU tests.  Every case of tests/fps_euclid_cases.py, plus the clouds where the box rule, the cell keys or the block
keys can go wrong.  A case has the form of that module's (``clouds``, one of ``ratio`` / ``n_samples``, ``start``); every case
runs at the three ``TARGETS``.  ``expected(case, target)`` -> per cloud (picks, stats) of the numpy restatement, computed once."""
import functools

import numpy as np

from tests import fps_euclid_cases as E
from tests import fps_grid_restate as R

case, normal = E.case, E.normal
ONE_CELL = 1e9                                # a target so large that every grid is one cell
# the default, one cell, 0.5 (2 n cells: the largest tables) -- the measured default IS 0.5, so 1.0 keeps a third grid in the set
TARGETS = tuple(dict.fromkeys((R.DEFAULT_TARGET, ONE_CELL, 0.5, 1.0)))


def sphere(seed, n, scale=1.0, shift=0.0):
    p = np.random.default_rng(seed).standard_normal((n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True) * scale + shift).astype(np.float32)


def _cube64():                                # 64 points, equal extents: 4 x 4 x 4 = 64 cells at target 1
    p = np.random.default_rng(400).random((64, 3)).astype(np.float32)
    p[0], p[1] = 0.0, 1.0
    return p


def _plane70():                               # 70 points, extents 1 : 0.38 : 0 -> 13 x 5 x 1 = 65 cells at target 1
    p = np.random.default_rng(401).random((70, 3)).astype(np.float32) * np.float32([1.0, 0.38, 0.0])
    p[0], p[1] = (0.0, 0.0, 0.0), (1.0, 0.38, 0.0)
    return p


def _heavy_cell():                            # 300 coincident points inside one cell of a 2 000-point cloud
    p = normal(410, 2000)
    rows = np.random.default_rng(411).choice(2000, 300, replace=False)
    p[rows] = p[rows[0]]
    return p


def _outlier():
    p = sphere(420, 1500)
    p[700] = (1000.0, 0.0, 0.0)
    return p


def _clumps():
    p = normal(430, 1200, 0.5)
    p[::2, 0] += 1000.0
    return p


def _line():
    t = np.random.default_rng(440).random(900).astype(np.float32)
    return np.stack([t, np.zeros_like(t), np.zeros_like(t)], 1)


def _nonfinite_row0():
    p = normal(450, 400)
    p[0, 2] = np.nan
    p[123, 0] = -np.inf
    p[399, 1] = np.inf
    return p


def _duplicates():
    p = normal(460, 150)
    return np.concatenate([p, p[:90], p[:30]])[np.random.default_rng(461).permutation(270)]


NEW = [
    case("coincident_50", [np.full((50, 3), 0.25, np.float32)], ratio=1),
    case("zero_extent_two_axes", [_line()], ratio=3),
    case("cells_64", [_cube64()], ratio=2),
    case("cells_65", [_plane70()], ratio=2),
    case("short_rows_2000", [normal(402, 2000)], ratio=4),
    case("heavy_cell_300_of_2000", [_heavy_cell()], ratio=4),
    case("sphere_3000", [sphere(403, 3000)], ratio=8),
    case("sphere_shifted_4096", [sphere(404, 2000, 1.0, 4096.0)], ratio=8),
    case("sphere_scaled_1e-17", [sphere(405, 1000, 1e-17)], ratio=4),
    case("coordinates_1e19", [normal(406, 600, 1e19)], ratio=4),
    case("outlier_at_1000", [_outlier()], ratio=6),
    case("two_clumps", [_clumps()], ratio=4),
    case("nonfinite_row0", [_nonfinite_row0()], ratio=1),
    case("nonfinite_row0_start_inf", [_nonfinite_row0()], ratio=3, start=[399]),
    case("nonfinite_row0_start_finite", [_nonfinite_row0()], ratio=1, start=[200]),
    case("no_finite_point", [np.full((37, 3), np.nan, np.float32)], ratio=2, start=[5]),
    case("no_finite_point_mixed", [np.where(np.arange(120)[:, None] % 2 == 0, np.nan, np.inf).astype(np.float32).repeat(3, 1)], ratio=1),
    case("full_order_duplicates", [_duplicates()], ratio=1, start=[17]),
    case("ragged_with_specials", [normal(470, 1), _nonfinite_row0(), sphere(471, 700), np.full((3, 3), 2.0, np.float32), _plane70()],
         ratio=2, start=[0, 123, 699, 2, 69]),
]
CASES = list(E.CASES) + NEW
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
assert len(NAMES) == len(CASES)
picks_of, start_of, ptr_of = E.picks_of, E.start_of, E.ptr_of


@functools.lru_cache(maxsize=None)
def _expected(name, target):
    c = BY_NAME[name]
    return tuple(R.sample(pos, picks_of(c, b), start_of(c, b), target) for b, pos in enumerate(c["clouds"]))


def expected(c, target):
    """-> per cloud (int64 local picks, int64 [2] stats) of the restatement (shared: do not write to them)."""
    return _expected(c["name"], float(target))


@functools.lru_cache(maxsize=None)
def big_sphere():
    """The pruning condition's cloud: a sphere of 20 000 points sampled to 5 000 at the default target -> (pos, picks, stats, history);
    history[r - 2] is the stats of the r-pick sample, whose picks are picks[:r]."""
    pos, history = sphere(480, 20000), []
    picks, stats = R.sample(pos, 5000, 0, R.DEFAULT_TARGET, history=history)
    return pos, picks, stats, history
