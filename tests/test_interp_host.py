"""Host side of the propagation stage (csrc/interp_math.h: two-set nearest neighbours + inverse-squared-distance interpolation),
without a GPU: a g++ build of interp_math.h (tests/hostcheck_interp) against the numpy restatement (tests/interp_restate.py)
bit for bit; the restatement's neighbours against fp64 (``cKDTree`` on the widened points), its interpolation against the PyG
formula in fp64 within (2k + 4) * 2^-24 * max|x over the row's neighbours|; the edge cases.

The interpolation bound: the weights are positive, so the exact quotient is a convex combination of the neighbours' values and
relative perturbations of its terms move it by that fraction of max|x| at most.  A term of the numerator passes through its
product and at most k - 1 additions (k roundings), a term of the denominator through at most k - 1 additions; the reciprocal
behind a weight is rounded once and enters both sums (2 in all); one division: k + (k - 1) + 2 + 1 = 2k + 2 roundings of 2^-24
at most, held to the 2k + 4 the stage's specification states.  Measured on the restatement: 0.09 .. 0.22 of the bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import interp_restate as R
from tests.helpers import ROOT

HI_DIR = os.path.join(ROOT, "tests", "hostcheck_interp")
P = lambda a: ctypes.c_void_p(a.ctypes.data)
EPS = 2.0 ** -24
SHAPES = [(2049, 700, 16), (2049, 700, 3), (300, 257, 8), (5, 257, 3)]          # (Nr, Nq, k)


@pytest.fixture(scope="module")
def hi():
    subprocess.run(["make", "-s", "-C", HI_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HI_DIR, "libhostcheck_interp.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hi_knn_cross.argtypes, lib.hi_knn_cross.restype = [vp, i64, vp, i64, i32, vp, vp], ctypes.c_int
    lib.hi_interpolate.argtypes, lib.hi_interpolate.restype = [vp, i64, i32, i64, i64, i32, vp, vp, i32, vp, i64], None
    return lib


def host_knn(hi, q, r, k):
    q, r = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 3)
    idx, d2 = np.full((q.shape[0], k), -7, dtype=np.int32), np.full((q.shape[0], k), -7, dtype=np.float32)
    assert hi.hi_knn_cross(P(q), q.shape[0], P(r), r.shape[0], k, P(idx), P(d2)) == 0
    return idx, d2


def host_interp(hi, x, idx, d2, pad=0, vec=False):
    """x [Nr,C] laid out with a leading dimension of C + pad (the gap holds NaN)."""
    nr, c = x.shape
    ldx = c + pad
    if vec:
        ldx = (ldx + 3) // 4 * 4
    raw = np.full(nr * ldx + 4, np.nan, dtype=np.float32)
    off = (-(raw.ctypes.data // 4)) % 4 if vec else 0                           # a 16-byte aligned base for the 16-byte loads
    wide = raw[off:off + nr * ldx].reshape(nr, ldx)
    wide[:, :c] = x
    idx, d2 = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(d2, dtype=np.float32)
    out = np.full((idx.shape[0], c + 2), -7, dtype=np.float32)
    hi.hi_interpolate(P(wide), ldx, c, nr, idx.shape[0], idx.shape[1], P(idx), P(d2), int(vec), P(out), c + 2)
    assert (out[:, c:] == -7).all()
    return np.ascontiguousarray(out[:, :c])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cube(nr, nq, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((nr, 3), dtype=np.float32), rng.random((nq, 3), dtype=np.float32)


# ---- g++ build of interp_math.h = the restatement, bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("nr,nq,k", SHAPES + [(40, 33, 1), (17, 9, 4), (3, 20, 16)])
def test_hostcheck_equals_the_restatement_bitwise(hi, nr, nq, k):
    ref, qry = cube(nr, nq, seed=nr + k)
    ref[nr // 2:nr // 2 + min(3, nr - nr // 2)] = ref[0]                        # duplicated reference points: ties
    qry[0] = ref[0]
    idx, d2 = host_knn(hi, qry, ref, k)
    widx, wd2 = R.knn_cross(qry, ref, k)
    assert np.array_equal(idx, widx) and np.array_equal(bits(d2), bits(wd2))
    rng = np.random.default_rng(1)
    for c in (1, 3, 50, 64, 65):
        x = rng.standard_normal((nr, c)).astype(np.float32)
        want = R.interpolate(x, idx, d2)
        for vec in (False, True):
            assert np.array_equal(bits(host_interp(hi, x, idx, d2, pad=3, vec=vec)), bits(want)), (c, vec)


# ---- the neighbours against fp64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nq,k", SHAPES)
def test_neighbours_match_fp64_where_fp64_separates_them(nr, nq, k):
    from scipy.spatial import cKDTree
    ref, qry = cube(nr, nq, seed=0)
    idx, d2 = R.knn_cross(qry, ref, k)
    kk = min(k + 1, nr)
    dist, want = cKDTree(ref.astype(np.float64)).query(qry.astype(np.float64), k=kk)
    dist, want = dist.reshape(nq, kk), want.reshape(nq, kk)
    sq = dist ** 2
    close = (np.diff(sq, axis=1) < 16 * EPS * 3).any(axis=1) if kk > 1 else np.zeros(nq, dtype=bool)
    share = float(close.mean())
    m = min(k, nr)
    mismatch = int((idx[~close, :m] != want[~close, :m]).any(axis=1).sum())
    print(f"(Nr, Nq, k) = ({nr}, {nq}, {k}): {100 * share:.1f} % of the rows left out, {mismatch} index mismatches, "
          f"max |d2 - fp64| = {np.abs(d2[:, :m].astype(np.float64) - sq[:, :m]).max():.3e}")
    assert share <= 0.10
    assert mismatch == 0
    assert (idx[:, m:] == -1).all() and np.isinf(d2[:, m:]).all()
    assert np.abs(d2[:, :m].astype(np.float64) - sq[:, :m]).max() <= 16 * EPS * 3


# ---- the interpolation against the PyG formula in fp64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nq,k", SHAPES)
def test_interpolation_is_within_the_fp32_bound_of_the_pyg_formula(nr, nq, k):
    ref, qry = cube(nr, nq, seed=0)
    idx, d2 = R.knn_cross(qry, ref, k)
    x = np.random.default_rng(2).standard_normal((nr, 50)).astype(np.float32) * 10
    got = R.interpolate(x, idx, d2).astype(np.float64)
    ok = idx >= 0
    j = np.where(ok, idx, 0)
    w = np.where(ok, 1.0 / np.maximum(d2.astype(np.float64), 1e-16), 0.0)                       # PyG: 1 / clamp(d2, min=1e-16)
    rows = x.astype(np.float64)[j]                                                               # [Nq, k, C]
    want = (w[:, :, None] * rows).sum(axis=1) / w.sum(axis=1, keepdims=True)
    scale = np.abs(np.where(ok[:, :, None], rows, 0.0)).max(axis=(1, 2))
    bound = (2 * k + 4) * EPS * scale
    err = np.abs(got - want).max(axis=1)
    print(f"(Nr, Nq, k) = ({nr}, {nq}, {k}): worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
def test_duplicates_pick_the_lower_index_and_zero_distance_takes_the_clamp(hi):
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]], dtype=np.float32)
    qry = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    for fn in (lambda: host_knn(hi, qry, ref, 4), lambda: R.knn_cross(qry, ref, 4)):
        idx, d2 = fn()
        assert idx.tolist() == [[0, 2, 4, 1], [1, 3, 0, 2]] and d2.tolist() == [[0, 0, 0, 1], [0, 0, 1, 1]]
    x = np.array([[1.0], [5.0], [2.0], [7.0], [3.0]], dtype=np.float32)
    idx, d2 = R.knn_cross(qry, ref, 4)
    w0, w1 = np.float32(1.0) / np.float32(1e-16), np.float32(1.0)
    num = ((w0 * x[0] + w0 * x[2]).astype(np.float32) + w0 * x[4]).astype(np.float32) + w1 * x[1]
    den = np.float32(np.float32(np.float32(w0 + w0) + w0) + w1)
    want = (num.astype(np.float32) / den).astype(np.float32)
    for got in (R.interpolate(x, idx, d2), host_interp(hi, x, idx, d2)):
        assert bits(got[0]) == bits(want) and abs(float(got[0, 0]) - 2.0) < 1e-6


def test_one_valid_slot_is_an_exact_copy_and_k1_is_a_gather(hi):
    rng = np.random.default_rng(3)
    ref, qry = cube(37, 50, seed=3)
    x = (rng.standard_normal((37, 7)) * 1e3).astype(np.float32)
    x[5, 2], x[6, 1] = -0.0, np.float32(1e-42)                                   # a negative zero and a denormal survive a copy
    idx, d2 = R.knn_cross(qry, ref, 1)
    for got in (R.interpolate(x, idx, d2), host_interp(hi, x, idx, d2), host_interp(hi, x, idx, d2, pad=1, vec=True)):
        assert np.array_equal(bits(got), bits(x[idx[:, 0]]))
    one = np.full((50, 3), -1, dtype=np.int32)
    one[:, 1] = idx[:, 0]                                                        # the one valid slot in the middle
    dd = np.full((50, 3), np.inf, dtype=np.float32)
    dd[:, 1] = d2[:, 0]
    for got in (R.interpolate(x, one, dd), host_interp(hi, x, one, dd)):
        assert np.array_equal(bits(got), bits(x[idx[:, 0]]))


def test_a_short_reference_cloud_pads_and_an_empty_one_gives_zeros(hi):
    ref, qry = cube(2, 9, seed=4)
    x = np.arange(6, dtype=np.float32).reshape(2, 3) + 1
    for fn in (lambda r: host_knn(hi, qry, r, 3), lambda r: R.knn_cross(qry, r, 3)):
        idx, d2 = fn(ref)
        assert (idx[:, 2] == -1).all() and np.isinf(d2[:, 2]).all() and (np.sort(idx[:, :2], axis=1) == [0, 1]).all()
        assert (d2[:, 0] <= d2[:, 1]).all()
        eidx, ed2 = fn(ref[:0])
        assert (eidx == -1).all() and np.isinf(ed2).all() and (ed2 > 0).all()
    idx, d2 = R.knn_cross(qry, ref, 3)
    got, want = host_interp(hi, x, idx, d2), R.interpolate(x, idx, d2)
    assert np.array_equal(bits(got), bits(want)) and (got >= 1).all() and (got <= 6).all()
    eidx, ed2 = R.knn_cross(qry, ref[:0], 3)
    assert not R.interpolate(x[:0], eidx, ed2).any() and not host_interp(hi, x[:0], eidx, ed2).any()
    # slots that point outside the reference cloud index nothing and count as invalid
    wild = np.array([[5, 0, -3]], dtype=np.int32)
    for got in (R.interpolate(x, wild, np.ones((1, 3), dtype=np.float32)), host_interp(hi, x, wild, np.ones((1, 3), dtype=np.float32))):
        assert np.array_equal(bits(got[0]), bits(x[0]))


def test_a_nan_coordinate_is_never_picked_and_nothing_is_indexed(hi):
    ref, qry = cube(20, 6, seed=5)
    ref[3, 1], ref[11, 0] = np.nan, np.nan
    qry[2, 2] = np.nan
    for fn in (lambda r, k: host_knn(hi, qry, r, k), lambda r, k: R.knn_cross(qry, r, k)):
        idx, d2 = fn(ref, 16)
        assert not np.isin(idx, [3, 11]).any() and np.isfinite(d2[idx >= 0]).all()
        assert (idx[2] == -1).all() and np.isinf(d2[2]).all()                   # the NaN query finds nothing
        live = np.delete(np.arange(6), 2)
        assert (idx[live, :16] >= 0).all() and not np.isnan(d2).any()
        idx, d2 = fn(ref, 4)
        assert (idx[live] >= 0).all() and (idx[2] == -1).all()
        idx, d2 = fn(ref[[3, 11]], 3)                                            # only NaN candidates: every slot stays empty
        assert (idx == -1).all() and np.isinf(d2).all()
    a, b = host_knn(hi, qry, ref, 16), R.knn_cross(qry, ref, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    x = np.ones((20, 4), dtype=np.float32)
    assert not R.interpolate(x, *b)[2].any() and not host_interp(hi, x, *b)[2].any()
    assert host_knn(hi, qry, ref, 1)[0].shape == (6, 1) and hi.hi_knn_cross(None, 0, None, 0, 17, None, None) == -1
