"""The cases of the pooling over cluster cells (``geometry.cluster_*``, csrc/cluster.hip), seeded; shared by the host and the GPU
tests.  A case: ``cluster`` (int64 [n]), ``m`` (cells), ``x`` (float32 [n,C], possibly a strided view), ``g`` (float32 [m,C], the
gradient the backward is fed), ``pos`` / ``norm`` (float32 [n,3]), ``labels`` (int64 [n]) and ``classes``.  ``expected(name)`` ->
the restatement's results, computed once per case.

The smallest shapes at which each part can go wrong: a list of one row, a list longer than a scan block (1 024) or a rank block
(256) with a channel tail, more cells than one scan block, lists whose fill order the atomics scramble, ids that name no cell and
cells without a member, no row and no cell at all, ties / signed zeros / NaN first and later / infinities for the selection,
every vector-width path of the channels (C = 1, 3, 4, 5, 64, 130, a strided view), a cloud far from the origin for the barycentre,
label ties and labels out of range, and two clusterings that come from the voxel grid."""
import functools

import numpy as np

from tests import cluster_restate as R

F = np.float32
REDUCES = ("max", "min", "sum", "mean")


def case(name, cluster, m, c=4, seed=0, x=None, shift=0.0, labels=None, classes=7, pos=None):
    cluster = np.ascontiguousarray(cluster, dtype=np.int64).reshape(-1)
    n = cluster.size
    rng = np.random.default_rng(1000 + seed)
    if x is None:
        x = rng.standard_normal((n, c)).astype(F)
    if pos is None:
        pos = (rng.uniform(0, 1, (n, 3)).astype(F) + F(shift)).astype(F)
    norm = rng.standard_normal((n, 3)).astype(F)
    norm = (norm / np.maximum(np.linalg.norm(norm, axis=1, keepdims=True), 1e-6)).astype(F)
    if labels is None:
        labels = rng.integers(-1, classes + 1, n)               # -1 and `classes` are out of range
    g = rng.standard_normal((m, x.shape[1])).astype(F)
    return dict(name=name, cluster=cluster, m=int(m), x=x, g=g, pos=np.ascontiguousarray(pos, dtype=F), norm=norm,
                labels=np.ascontiguousarray(labels, dtype=np.int64), classes=int(classes))


def _special():
    """Two cells of four rows each, three channels: what the strict comparison has to get right."""
    nan, inf = np.nan, np.inf
    x = np.array([[nan, 1.0, -inf], [2.0, nan, 5.0], [3.0, 7.0, inf], [1.0, 7.0, inf],          # cell 0: NaN first | NaN later | infs
                  [0.0, -0.0, 4.0], [-0.0, 0.0, 4.0], [0.0, -0.0, -inf], [-0.0, 0.0, 4.0]], F)    # cell 1: signed zeros | equal values
    return x, np.array([0, 0, 0, 0, 1, 1, 1, 1])


def _voxel(name):
    from tests import voxel_cases as V
    rows, _, cluster, _ = V.expected(name)
    return cluster, rows.size, np.concatenate(V.BY_NAME[name]["clouds"])


def _cases():
    rng = np.random.default_rng(77)
    some = rng.integers(-3, 53, 800)
    some[np.isin(some, (5, 17, 49))] = -1                       # cells 5, 17 and the last one stay empty
    wide = rng.standard_normal((300, 12)).astype(F)
    sx, sc = _special()
    tie_labels = np.array([2, 1, 1, 2, 9, -4, 0, 0, 3, 3, 3, 0, 8, -1, 9, 8])      # cells of 4: tie 1|2 -> 1; only 0 valid; 3; none valid
    vc, vm, vpos = _voxel("cells_64_of_2000")
    lc, lm, lpos = _voxel("lattice_faces_64")
    return [
        case("one_row", [0], 1, c=4, seed=1),
        case("one_cell_300", np.zeros(300), 1, c=3, seed=2),
        case("one_cell_5000_c5", np.zeros(5000), 1, c=5, seed=3),
        case("own_cell_5000", np.random.default_rng(4).permutation(5000), 5000, c=1, seed=4),
        case("mod7_1000_c64", np.arange(1000) % 7, 7, c=64, seed=5),
        case("random_3000_200_c130", rng.integers(0, 200, 3000), 200, c=130, seed=6),
        case("ids_without_a_cell", some, 50, c=4, seed=7),
        case("no_row", np.zeros(0), 5, c=3, seed=8),
        case("no_cell", rng.integers(-2, 4, 40), 0, c=2, seed=9),
        case("all_equal", np.arange(100) % 5, 5, x=np.full((100, 4), 1.5, F), seed=10),
        case("nan_inf_signed_zero", sc, 2, x=sx, seed=11),
        case("strided_view_c4", np.arange(300) % 11, 11, x=wide[:, 4:8], seed=12),
        case("strided_view_c3_unaligned", np.arange(300) % 11, 11, x=wide[:, 1:4], seed=13),
        case("shifted_4096", rng.integers(0, 20, 500), 20, c=3, shift=4096.0, seed=14),
        case("label_ties", np.repeat(np.arange(4), 4), 4, c=1, labels=tie_labels, classes=8, seed=15),
        case("voxel_cells_64_of_2000", vc, vm, c=5, pos=vpos, seed=16),
        case("voxel_lattice_faces_64", lc, lm, c=4, pos=lpos, seed=17),
        case("voxel_lattice_faces_512", *_voxel("lattice_faces_512")[:2], c=3, pos=lpos, seed=18),
    ]


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
FINITE = [n for n in NAMES if np.isfinite(BY_NAME[n]["x"]).all()]


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> dict(cptr, members, out / arg / dx per reduce, up, dup, bary, nbar, label) of the restatement (shared: do not write to
    them)."""
    c = BY_NAME[name]
    cptr, members = R.lists(c["cluster"], c["m"])
    e = dict(cptr=cptr, members=members)
    for r in REDUCES:
        e["out", r], e["arg", r] = R.pool(c["x"], cptr, members, r)
        e["dx", r] = R.pool_backward(c["g"], c["cluster"], cptr, e["arg", r], r)
    e["up"] = R.gather(c["g"], c["cluster"])                                    # un-pooling of the [m,C] rows g
    e["dup"] = R.gather_backward(c["x"], cptr, members)                         # its backward, fed the [n,C] rows x
    e["bary"] = R.mean3(c["pos"], c["cluster"], c["m"])
    e["nbar"] = R.mean3(c["norm"], c["cluster"], c["m"], normalize=True)
    e["label"] = R.majority(c["labels"], c["cluster"], c["m"], c["classes"])
    return e
