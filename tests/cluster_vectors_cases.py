"""The cases of the vector pooling over cluster cells (``geometry.cluster_*_vectors``, csrc/cluster_vectors.hip), seeded; shared by
the host and the GPU tests.  A case: ``cluster`` (int64 [n]), ``m`` (cells), ``v`` (float32 [2n,C], possibly a strided view: the
values that are pooled, and the gradient the un-pooling's backward is fed), ``g`` (float32 [2m,C]: the gradient the pooling's
backward is fed, and the values that are un-pooled), ``fine`` / ``coarse`` (the frames (normal, x, y), float32 [n,3] / [m,3] each)
and ``non_oriented``.  ``expected(name)`` -> the restatement's results, computed once per case.

The smallest shapes at which each part can go wrong, on the cluster vectors of tests/cluster_cases.py where they fit: one row; one
cell of 300 rows at C = 3 and of 5 000 at C = 5 (a long walk, the four-in-flight tail, a scalar channel tail); 5 000 cells of one
row at C = 1; i % 7 at C = 64; 3 000 rows into 200 cells at C = 130; ids without a cell and cells without a member; no row, no
cell; a 16-byte aligned and an unaligned strided view; what the strict comparison of the maximum has to get right; cells of at
most 16 members (the search form of tests/pool_vectors_restate.py covers them too).  Frames: random ones (normals on both
hemispheres, so about half of the entries are reflections under non_oriented, and the same case with non_oriented off); cells whose
frame is a member's bit for bit (entry (1, -0, 0, 1)); parallel normals with different x-axes (the axis fallback); and two
clusterings of the voxel grid with frames from the points' normals and frames_coarse = frames_fine[rows]."""
import functools

import numpy as np

from tests import cluster_cases as CC
from tests import cluster_vectors_restate as R
from tests import connection_restate as CR

F = np.float32
REDUCES = ("max", "sum", "mean")


def _unit(a):
    a = np.asarray(a, dtype=F)
    return (a / np.maximum(CR.norm3(a), F(1e-6))[:, None]).astype(F)


def random_frames(rows, rng):
    """Unit normals anywhere on the sphere with tangent_basis frames -> (normal, x, y)."""
    n = _unit(rng.standard_normal((rows, 3)))
    x, y = CR.tangent_basis(n)
    return n, x, y


def frames_of_normals(n):
    n = _unit(n)
    x, y = CR.tangent_basis(n)
    return n, x, y


def parallel_frames(rows, rng):
    """The normal (0, 0, 1) everywhere, the x-axis turned by a random angle: the cross product of two normals has no direction."""
    a = rng.uniform(0, 2 * np.pi, rows)
    n = np.tile(np.array([[0, 0, 1]], F), (rows, 1))
    x = np.stack([np.cos(a), np.sin(a), np.zeros(rows)], 1).astype(F)
    y = np.stack([-np.sin(a), np.cos(a), np.zeros(rows)], 1).astype(F)
    return n, x, y


def first_member_frames(cluster, m, fine, rng):
    """Every cell takes the frame of its LOWEST member bit for bit (an empty cell a random one) -> coarse frames."""
    coarse = [a.copy() for a in random_frames(m, rng)]
    cptr, members = R.CL.lists(cluster, m)
    full = np.flatnonzero(np.diff(cptr) > 0)
    for a, b in zip(coarse, fine):
        a[full] = b[members[cptr[full]]]
    return tuple(coarse)


def case(name, cluster, m, c=4, seed=0, v=None, frames="random", non_oriented=True, fine=None, coarse=None):
    cluster = np.ascontiguousarray(cluster, dtype=np.int64).reshape(-1)
    n = cluster.size
    rng = np.random.default_rng(2000 + seed)
    if v is None:
        v = rng.standard_normal((2 * n, c)).astype(F)
    g = rng.standard_normal((2 * m, v.shape[1])).astype(F)
    if fine is None:
        fine = parallel_frames(n, rng) if frames == "parallel" else random_frames(n, rng)
    if coarse is None:
        if frames == "members":
            coarse = first_member_frames(cluster, m, fine, rng)
        else:
            coarse = parallel_frames(m, rng) if frames == "parallel" else random_frames(m, rng)
    return dict(name=name, cluster=cluster, m=int(m), v=v, g=g, fine=fine, coarse=coarse, non_oriented=bool(non_oriented))


def _special():
    """Cell 0 of four rows, cell 1 of two; one scenario per channel.  Rows 2i, 2i+1 are the vector at point i."""
    nan, inf = np.nan, np.inf
    #                 equal norms        NaN key first   NaN key later   infinite key
    vectors = [[(3, 4), (nan, 1), (1, 1), (1, 1)],           # point 0
               [(5, 0), (2, 2), (nan, 0), (inf, 0)],         # point 1
               [(-5, 0), (9, 9), (2, 2), (3, 3)],            # point 2
               [(1, 1), (1, 1), (0, nan), (inf, 1)],         # point 3
               [(5, 0), (0, 0), (-0.0, 0), (1, 0)],          # point 4 (cell 1)
               [(3, 4), (0, -0.0), (0, 0), (0, 1)]]          # point 5 (cell 1): equal norms again, zero keys, equal keys
    v = np.zeros((12, 4), F)
    for i, row in enumerate(vectors):
        for ch, (a, b) in enumerate(row):
            v[2 * i, ch], v[2 * i + 1, ch] = a, b
    return v, np.array([0, 0, 0, 0, 1, 1])


def _voxel(name, c, seed):
    """A clustering of the voxel grid: normals point away from the cube's centre, frames_coarse = frames_fine[rows]."""
    from tests import voxel_cases as V
    rows, _, cluster, _ = V.expected(name)
    pos = np.concatenate(V.BY_NAME[name]["clouds"])
    fine = frames_of_normals(pos - F(0.5) + F(1e-3))
    return case("voxel_" + name, cluster, rows.size, c=c, seed=seed, fine=fine, coarse=tuple(a[rows] for a in fine))


def _cases():
    cc = lambda name: (CC.BY_NAME[name]["cluster"], CC.BY_NAME[name]["m"])
    rng = np.random.default_rng(78)
    wide = rng.standard_normal((600, 12)).astype(F)
    small = rng.permutation(np.concatenate([np.arange(700) % 97, np.full(20, -1)]))     # cells of 7 or 8 rows
    sv, sc = _special()
    return [
        case("one_row", *cc("one_row"), c=4, seed=1, frames="members"),
        case("one_cell_300", *cc("one_cell_300"), c=3, seed=2),
        case("one_cell_5000_c5", *cc("one_cell_5000_c5"), c=5, seed=3),
        case("own_cell_5000", *cc("own_cell_5000"), c=1, seed=4, frames="members"),
        case("mod7_1000_c64", *cc("mod7_1000_c64"), c=64, seed=5),
        case("random_3000_200_c130", *cc("random_3000_200_c130"), c=130, seed=6),
        case("ids_without_a_cell", *cc("ids_without_a_cell"), c=4, seed=7, frames="members"),
        case("no_row", *cc("no_row"), c=3, seed=8),
        case("no_cell", *cc("no_cell"), c=2, seed=9),
        case("strided_view_c4", np.arange(300) % 11, 11, v=wide[:, 4:8], seed=12),
        case("strided_view_c3_unaligned", np.arange(300) % 11, 11, v=wide[:, 1:4], seed=13),
        case("special_max", sc, 2, v=sv, seed=14),
        case("small_cells_oriented", small, 97, c=6, seed=15, non_oriented=False),
        case("small_cells", small, 97, c=6, seed=15),
        case("parallel_normals", np.arange(200) % 9, 9, c=4, seed=16, frames="parallel"),
        _voxel("cells_64_of_2000", 5, 17),
        _voxel("lattice_faces_512", 4, 18),
    ]


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
FINITE = [n for n in NAMES if np.isfinite(BY_NAME[n]["v"]).all()]
SMALL = [n for n in NAMES if BY_NAME[n]["cluster"].size and BY_NAME[n]["m"]
         and np.bincount(BY_NAME[n]["cluster"][R.CL.valid(BY_NAME[n]["cluster"], BY_NAME[n]["m"])], minlength=1).max() <= 16]


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> dict(cptr, members, rdown, rup, out / arg / dv per reduce, up, dup) of the restatement (shared: do not write to them)."""
    c = BY_NAME[name]
    cptr, members = R.CL.lists(c["cluster"], c["m"])
    e = dict(cptr=cptr, members=members)
    for direction in ("down", "up"):
        e["r" + direction] = R.table(c["cluster"], c["m"], c["fine"], c["coarse"], direction, c["non_oriented"])
    for r in REDUCES:
        e["out", r], e["arg", r] = R.pool(c["v"], cptr, members, e["rdown"], r)
        e["dv", r] = R.pool_backward(c["g"], c["cluster"], cptr, e["rdown"], e["arg", r], r)
    e["up"] = R.unpool(c["g"], c["cluster"], e["rup"])                           # un-pooling of the [2m,C] rows g
    e["dup"] = R.unpool_backward(c["v"], cptr, members, e["rup"])                # its backward, fed the [2n,C] rows v
    return e
