"""Host side of the exact grid search (csrc/knn_grid_math.h), without a GPU: a g++ build of the header (tests/hostcheck_knn_grid)
against the numpy restatement (tests/knn_grid_restate.py) bit for bit in the grid parameters, the cells and the bounds; its search
against the order oracle (``oracle.geometry.knn``) for the self form and against a lexsort by (d2 bits, id) for the cross form, on
every case of tests/knn_grid_cases.py at the three grid shapes; and the property the stopping rule rests on.  Everything here
is an equality: there is no tolerance in this change."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import geometry as geo
from tests import knn_grid_cases as C
from tests import knn_grid_restate as R
from tests.helpers import ROOT

HG_DIR = os.path.join(ROOT, "tests", "hostcheck_knn_grid")
P = lambda a: ctypes.c_void_p(a.ctypes.data)
HEADER = open(os.path.join(ROOT, "deltaconv_amd", "csrc", "knn_grid_math.h")).read()
DEFAULT_TARGET = float(re.search(r"DEFAULT_TARGET = ([0-9.]+)f;", HEADER).group(1))
TARGETS = [DEFAULT_TARGET if t is None else t for t in C.TARGETS]
f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


@pytest.fixture(scope="module")
def hg():
    subprocess.run(["make", "-s", "-C", HG_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HG_DIR, "libhostcheck_knn_grid.so"))
    vp, i32, i64, fl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.hg_make_grid.argtypes, lib.hg_make_grid.restype = [i64, vp, vp, fl, vp], None
    lib.hg_grid_of.argtypes, lib.hg_grid_of.restype = [vp, i64, fl, vp], None
    lib.hg_cells.argtypes, lib.hg_cells.restype = [vp, vp, i64, vp], None
    lib.hg_bound2.argtypes, lib.hg_bound2.restype = [vp, i64, fl, vp], None
    lib.hg_search.argtypes, lib.hg_search.restype = [vp, i64, vp, i64, i32, fl, i32, i32, vp, vp], ctypes.c_int
    return lib


def host_search(hg, qry, ref, k, target, self_form, rev=0):
    qry, ref = f32(qry).reshape(-1, 3), f32(ref).reshape(-1, 3)
    idx, d2 = np.full((qry.shape[0], k), -7, np.int32), np.full((qry.shape[0], k), -7, np.float32)
    assert hg.hg_search(P(qry), qry.shape[0], P(ref), ref.shape[0], k, target, int(self_form), rev, P(idx), P(d2)) == 0
    return idx, d2


def clouds(pos, sizes):
    ptr = C.ptr_of(sizes)
    return [f32(pos[ptr[b]:ptr[b + 1]]) for b in range(len(sizes))]


def lexsort_knn(qry, ref, k):
    """The cross form's definition: the k smallest (d2 bits, id) among the candidates with d2 below +inf."""
    idx, d2 = np.full((qry.shape[0], k), -1, np.int32), np.full((qry.shape[0], k), np.inf, np.float32)
    for q in range(qry.shape[0]):
        d = R.dist2(qry[q], ref)
        cand = np.nonzero(d < np.inf)[0]
        order = cand[np.lexsort((cand, d[cand].view(np.uint32)))][:k]
        idx[q, :order.size], d2[q, :order.size] = order, d[order]
    return idx, d2


_oracle = {}


def oracle_nbr(name):
    if name not in _oracle:
        pos, sizes, k = C.SELF[name]()
        _oracle[name] = geo.knn(pos, k, torch.from_numpy(C.ptr_of(sizes))).numpy()
    return _oracle[name]


# ---- grid parameters, cells and bounds: the g++ build = the restatement, bit for bit -----------------------------------------
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", list(C.SELF))
def test_grid_cells_and_bounds_equal_the_restatement_bitwise(hg, name, target):
    pos, sizes, _ = C.SELF[name]()
    for ref in clouds(pos, sizes):
        G = R.grid_of(ref, target)
        got = np.zeros(12, np.uint32)
        hg.hg_grid_of(P(ref), ref.shape[0], target, P(got))
        assert np.array_equal(got, R.words(G)), (got, R.words(G))
        assert G["cells"] <= max(1, 2 * ref.shape[0]) and G["g"].max() <= R.MAX_AXIS
        if target == 1e9:
            assert G["cells"] == 1
        cells = np.zeros((ref.shape[0], 3), np.int32)
        hg.hg_cells(P(got), P(ref), ref.shape[0], P(cells))
        assert np.array_equal(cells, R.cells(G, ref))
        r = np.concatenate([np.arange(0, 40), [255, 1023, 1024]]).astype(np.int32)
        b2 = np.zeros(r.size, np.float32)
        hg.hg_bound2(P(r), r.size, G["min_h"], P(b2))
        assert np.array_equal(b2.view(np.uint32), R.bound2(r, G["min_h"]).view(np.uint32)) and b2[0] == 0


def test_grid_rule_degenerate_boxes(hg):
    """One cell and inv_h = 0 on an axis whose extent is zero, not finite, or whose inverse cell size is not finite / not normal."""
    big = np.float32(3e38)
    boxes = [((0, 0, 0), (1, 0, 1)), ((-big, 0, 0), (big, 1, 1)), ((0, 0, 0), (1e-42, 1, 1)), ((0, 0, 0), (1e38, 1e-3, 1)),
             ((5, 5, 5), (5, 5, 5)), ((0, 0, 0), (1, 2, 4)), ((-1, -1, -1), (1, 1e-6, 1))]
    for lo, hi in boxes:
        for m, target in ((1, 2.0), (1000, 2.0), (5000, 0.25), (5000, 1e9), (100000, 1.0)):
            lo32, hi32 = f32(lo), f32(hi)
            got = np.zeros(12, np.uint32)
            hg.hg_make_grid(m, P(lo32), P(hi32), target, P(got))
            G = R.make_grid(m, lo32, hi32, target)
            assert np.array_equal(got, R.words(G)), (lo, hi, m, target, got, R.words(G))
            assert G["cells"] <= max(1, 2 * m) and all((G["inv_h"][a] == 0) == (G["g"][a] == 1) for a in range(3))
            with np.errstate(all="ignore"):
                ext = hi32 - lo32
            assert all(G["g"][a] == 1 for a in range(3) if not (np.isfinite(ext[a]) and ext[a] > 0))
    got = np.zeros(12, np.uint32)
    hg.hg_make_grid(0, P(f32([0, 0, 0])), P(f32([0, 0, 0])), 2.0, P(got))
    assert np.array_equal(got, R.words(R.make_grid(0, None, None, 2.0)))


# ---- the search: the self form against the order oracle, the cross form against the lexsort -------------------------------------
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", list(C.SELF))
def test_self_search_equals_the_oracle(hg, name, target):
    pos, sizes, k = C.SELF[name]()
    want, ptr = oracle_nbr(name), C.ptr_of(sizes)
    for b, ref in enumerate(clouds(pos, sizes)):
        for rev in ((0, 1) if target == DEFAULT_TARGET else (0,)):              # the order inside a cell cannot reach the result
            idx, _ = host_search(hg, ref, ref, k, target, True, rev)
            assert np.array_equal(idx.astype(np.int64) + ptr[b], want[ptr[b]:ptr[b + 1]]), (name, b, rev)


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", list(C.CROSS) + ["self:" + n for n in C.SELF])
def test_cross_search_equals_the_lexsort(hg, name, target):
    qry, qsizes, ref, rsizes, k = C.self_as_cross(name[5:]) if name.startswith("self:") else C.CROSS[name]()
    for q, r in zip(clouds(qry, qsizes), clouds(ref, rsizes)):
        idx, d2 = host_search(hg, q, r, k, target, False)
        widx, wd2 = lexsort_knn(q, r, k)
        assert np.array_equal(idx, widx) and np.array_equal(d2.view(np.uint32), wd2.view(np.uint32)), name
        bad = ~np.isfinite(q).all(1)
        assert (idx[bad] == -1).all() and np.isinf(d2[bad]).all()
        assert not np.isin(idx, np.nonzero(~np.isfinite(r).all(1))[0]).any()


def test_restated_search_equals_the_host_build(hg):
    for name in ("outside_k3", "few_and_empty_k3", "non_finite_k16"):
        qry, qsizes, ref, rsizes, k = C.CROSS[name]()
        for q, r in zip(clouds(qry, qsizes), clouds(ref, rsizes)):
            for target in TARGETS:
                a, b = host_search(hg, q[:40], r, k, target, False), R.search(q[:40], r, k, target)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_search_argument_range(hg):
    assert hg.hg_search(None, 0, None, 0, 65, 2.0, 1, 0, None, None) == -1
    assert hg.hg_search(None, 0, None, 0, 17, 2.0, 0, 0, None, None) == -1
    assert hg.hg_search(None, 0, None, 0, 0, 2.0, 0, 0, None, None) == -1


# ---- the property the stopping rule rests on --------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("name", list(C.SELF) + ["cross:" + n for n in C.CROSS])
def test_bound_is_below_every_unvisited_distance(name, target):
    """A reference point whose cell lies more than r rings from the query's cell never has computed d2 below bound2(r): for
    sampled (query, point) pairs, with D the Chebyshev distance of their cells, d2 >= bound2(D - 1) (the largest r it is unvisited
    after; bound2 grows with r) -- and strictly above, so the point cannot tie the k-th key either."""
    if name.startswith("cross:"):
        qry, qsizes, ref, rsizes, _ = C.CROSS[name[6:]]()
        pairs = list(zip(clouds(qry, qsizes), clouds(ref, rsizes)))
    else:
        pos, sizes, _ = C.SELF[name]()
        pairs = [(c, c) for c in clouds(pos, sizes)]
    rng = np.random.default_rng(3)
    for qry, ref in pairs:
        qry, ref = qry[R.finite_rows(qry)], ref[R.finite_rows(ref)]
        if not len(qry) or not len(ref):
            continue
        G = R.grid_of(ref, target)
        qi, ri = rng.integers(0, len(qry), 20000), rng.integers(0, len(ref), 20000)
        dist = np.abs(R.cells(G, qry)[qi] - R.cells(G, ref)[ri]).max(1)
        with np.errstate(all="ignore"):
            d = (qry[qi] - ref[ri]).astype(np.float32)
            sq = (d * d).astype(np.float32)
            d2 = ((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32)
        far = dist >= 2                                                         # (bound2(0) = 0 says nothing)
        b2 = R.bound2(dist[far] - 1, G["min_h"])
        assert (d2[far] > b2).all() or not far.any()
        assert not far.any() or (b2 > 0).all() or G["min_h"] ** 2 < 1e-29
