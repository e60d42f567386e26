"""The cases of voxel-grid subsampling (``geometry.voxel_subsample``, csrc/voxel.hip), seeded; shared by the host and the GPU
tests.  A case: ``clouds`` (float32 [n,3] arrays of one call), ``size`` (a float or three), ``origin`` (None, [3] or [B,3]),
``pick``; ``count``: the output rows it must give where that is known in advance; ``overflow``: the cloud the call must name.
``expected(name)`` -> the restatement's (rows, optr, cluster, overflow), computed once per case.

The smallest shapes at which each part can go wrong: one slot that every insert meets, a table at its design load (every point its
own cell: n cells in 2 n + 1 slots) whose rows span more than one 1 024-row scan block, points ON cell faces (where a product with
a reciprocal would round differently), negative cells, clouds of 1 / 65 / 1 025 rows and an empty one, rows and whole clouds that
are not finite, and the range check from both sides."""
import functools

import numpy as np

from tests import voxel_restate as R

F = np.float32


def uniform(seed, n, lo=0.0, hi=1.0, shift=0.0):
    return (np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F) + F(shift)).astype(F)


def lattice():
    g = np.arange(8, dtype=F) * F(0.125)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).copy()


def _nonfinite():
    a = uniform(40, 200)
    a[17, 1] = np.nan
    a[90, 0] = np.inf
    a[91, 2] = -np.inf
    b = uniform(41, 70)
    b[0] = [np.nan, 0.5, 0.5]                              # a cloud's first row
    c = np.full((5, 3), np.nan, F)                         # no finite point at all
    c[2] = [np.inf, 0.0, 0.0]
    d = uniform(42, 33)
    d[0, 0] = np.inf
    d[32, 2] = np.nan
    return [a, b, c, d]


RAGGED_SIZES = (1, 65, 1025, 0, 300)


def case(name, clouds, size, origin=None, pick="centre", count=None, overflow=-1):
    return dict(name=name, clouds=[np.ascontiguousarray(c, dtype=F).reshape(-1, 3) for c in clouds], size=size, origin=origin,
                pick=pick, count=count, overflow=overflow)


def both(name, clouds, size, **kw):
    return [case(name, clouds, size, pick="centre", **kw), case(name + "_first", clouds, size, pick="first", **kw)]


FAR = np.array([[0.25, 0.5, 0.75], [2e6, 0.5, 0.5], [0.5, 0.5, 0.5]], F)
CASES = (
    both("one_point", [uniform(1, 1)], 0.1, count=1)
    + both("two_coincident", [np.repeat(uniform(2, 1), 2, 0)], 0.1, count=1)
    + both("one_cell_300", [uniform(3, 300)], 2.0, count=1)
    + both("cells_64_of_2000", [uniform(4, 2000)], 0.25, count=64)
    + both("own_cell_5000", [uniform(5, 5000)], 1e-3, count=5000)
    + both("lattice_faces_512", [lattice()], 0.125, count=512)
    + both("lattice_faces_64", [lattice()], 0.25, count=64)
    + both("shifted_4096", [uniform(6, 700, shift=4096.0)], 0.125)
    + both("origin_zero_negative_cells", [uniform(7, 1500, -0.5, 0.5)], 0.25, origin=[0.0, 0.0, 0.0], count=64)
    + both("origin_per_cloud", [uniform(8, 400), uniform(9, 90, -2.0, 2.0)], 0.2, origin=[[0.05, -0.1, 0.3], [-7.0, 1.5, 0.0]])
    + both("anisotropic", [uniform(10, 1200)], [0.5, 0.125, 0.3])
    + both("ragged", [uniform(20 + i, n) for i, n in enumerate(RAGGED_SIZES)], 0.15)
    + both("nonfinite_rows", _nonfinite(), 0.2)
    + [case("overflow_size_1", [uniform(30, 50), FAR], 1.0, overflow=1),
       case("far_point_size_4", [uniform(30, 50), FAR], 4.0, count=int(R.batch([uniform(30, 50)], 4.0)[1][-1]) + 2),
       case("overflow_given_origin", [uniform(31, 20)], 0.5, origin=[-6e5, 0.0, 0.0], overflow=0)]
)
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
# continuous draws: no two members of a cell at the same fp32 distance from its centre (asserted in tests/test_voxel_host.py)
TIE_FREE = ("cells_64_of_2000", "shifted_4096", "origin_zero_negative_cells", "anisotropic")


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (rows, optr, cluster, first overflowing cloud or -1) of the restatement (shared: do not write to them)."""
    c = BY_NAME[name]
    return R.batch(c["clouds"], c["size"], c["origin"], c["pick"])


def ptr_of(c):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in c["clouds"]])]).astype(np.int64)
