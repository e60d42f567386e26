"""Host side of the backward of the propagation stage (csrc/interp_math.h: coef / pick / bwd4), without a GPU: a g++ build of
those functions (tests/hostcheck_interp_grad) against the numpy restatement (tests/interp_grad_restate.py) bit for bit --
coefficients, transposed lists and dx; the restatement against the SAME lists and sum in fp64 (from the fp32 search result) within

    |dx - dx64| <= (L_j + k + 8) * 2^-24 * sum_e |c_e| |g_e|        (L_j the list length, the sum formed in fp64)

-- the first-order bound of an L-term sequential sum (a term passes through its product and at most L - 1 additions) whose
coefficients are built from at most k positive additions and two divisions (the reciprocal behind a weight, the quotient by
den); the slack of 8 covers the second-order terms; the adjoint identity <interp(x), g> = <x, backward(g)> in fp64 within the sum
of those bounds; the edge cases.  Measured on the restatement (the ragged call of interp_grad_restate.PAIRS): the worst
|dx - dx64| / bound is printed by test_restatement_is_within_the_fp64_bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import interp_grad_restate as G
from tests import interp_restate as R
from tests.helpers import ROOT

HG_DIR = os.path.join(ROOT, "tests", "hostcheck_interp_grad")
P = lambda a: ctypes.c_void_p(a.ctypes.data)
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def hg():
    subprocess.run(["make", "-s", "-C", HG_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HG_DIR, "libhostcheck_interp_grad.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hg_coef.argtypes, lib.hg_coef.restype = [i64, i64, i32, vp, vp, vp], None
    lib.hg_transpose.argtypes, lib.hg_transpose.restype = [vp, vp, i32, i64, i64, i32, vp, vp, vp, vp, vp], i64
    lib.hg_backward.argtypes, lib.hg_backward.restype = [vp, i64, i64, i32, vp, i32, i32, vp, vp, vp, i64, i32, vp, i64], None
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def host_transpose(hg, idx, d2, qptr, rptr, num_ref):
    idx, d2 = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(d2, dtype=F32)
    qptr, rptr = np.ascontiguousarray(qptr, dtype=np.int64), np.ascontiguousarray(rptr, dtype=np.int64)
    nq, k = idx.shape
    tptr = np.full(num_ref + 1, -7, dtype=np.int64)
    tedge, tcoef = np.full(nq * k + 1, -7, dtype=np.int64), np.full(nq * k + 1, -7, dtype=F32)
    n = hg.hg_transpose(P(qptr), P(rptr), len(qptr) - 1, nq, num_ref, k, P(idx), P(d2), P(tptr), P(tedge), P(tcoef))
    assert n == tptr[-1] and (tedge[n:] == -7).all() and (tcoef[n:] == -7).all()
    return tptr, tedge[:n].copy(), tcoef[:n].copy()


def host_backward(hg, g, rptr, k, tptr, tedge, tcoef, edge_base=0, vec=False, pad=3):
    """g [rows,C] laid out with a leading dimension of C + pad (the gap holds NaN); dx prefilled with NaN."""
    rows, c = g.shape
    ldg = c + pad
    if vec:
        ldg = (ldg + 3) // 4 * 4
    raw = np.full(rows * ldg + 4, np.nan, dtype=F32)
    off = (-(raw.ctypes.data // 4)) % 4 if vec else 0
    wide = raw[off:off + rows * ldg].reshape(rows, ldg)
    wide[:, :c] = g
    rptr = np.ascontiguousarray(rptr, dtype=np.int64)
    num_ref = len(tptr) - 1
    dx = np.full((num_ref, c + 2), np.nan, dtype=F32)
    dx[:, c:] = -7
    tedge, tcoef = np.ascontiguousarray(tedge, dtype=np.int64), np.ascontiguousarray(tcoef, dtype=F32)
    tptr = np.ascontiguousarray(tptr, dtype=np.int64)
    hg.hg_backward(P(wide), ldg, rows, c, P(rptr), len(rptr) - 1, k, P(tptr), P(tedge), P(tcoef), edge_base, int(vec), P(dx), c + 2)
    assert (dx[:, c:] == -7).all()
    return np.ascontiguousarray(dx[:, :c])


# ---- g++ build of interp_math.h = the restatement, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("k", G.KS)
def test_hostcheck_equals_the_restatement_bitwise(hg, k):
    _, qptr, _, rptr = G.ragged_clouds()
    idx, d2 = G.ragged_search(k)
    num_ref = int(rptr[-1])
    for b, (nq, nr) in enumerate(G.PAIRS):                                      # the coefficients, pair by pair
        rows = slice(qptr[b], qptr[b + 1])
        want, ok = G.coefficients(idx[rows], d2[rows], nr)
        got = np.full((nq, k), -7, dtype=F32)
        hg.hg_coef(nq, nr, k, P(np.ascontiguousarray(idx[rows])), P(np.ascontiguousarray(d2[rows])), P(got))
        assert np.array_equal(bits(got), bits(want)), (b, k)
        assert (want[~ok] == 0).all() and (want[ok] > 0).all()
    tptr, tedge, tcoef = host_transpose(hg, idx, d2, qptr, rptr, num_ref)
    wptr, wedge, wcoef = G.ragged_lists(k)
    assert np.array_equal(tptr, wptr) and np.array_equal(tedge, wedge) and np.array_equal(bits(tcoef), bits(wcoef))
    for j in range(num_ref):                                                    # ascending within every list
        assert (np.diff(wedge[wptr[j]:wptr[j + 1]]) > 0).all()
    assert wptr[-1] == ((idx >= 0)).sum()
    for c in G.CHANNELS:
        g = G.ragged_gradient(c)
        want = G.backward(g, wptr, wedge, wcoef, k)
        for vec in (False, True):
            got = host_backward(hg, g, rptr, k, tptr, tedge, tcoef, vec=vec)
            assert not np.isnan(got).any(), "a reference row of a pair was not written"
            assert np.array_equal(bits(got), bits(want)), (k, c, vec)


def test_a_cloud_range_against_the_lists_of_the_whole_call(hg):
    """edge_base: pairs 1 .. 3 run with their own rows of g, their slice of tptr and offsets relative to the range."""
    k, c = 3, 50
    _, qptr, _, rptr = G.ragged_clouds()
    tptr, tedge, tcoef = G.ragged_lists(k)
    g = G.ragged_gradient(c)
    whole = G.backward(g, tptr, tedge, tcoef, k)
    lo, hi = 1, 4
    q0, q1, r0, r1 = qptr[lo], qptr[hi], rptr[lo], rptr[hi]
    part = G.backward(g[q0:q1], tptr[r0:r1 + 1], tedge, tcoef, k, edge_base=q0)
    assert np.array_equal(bits(part), bits(whole[r0:r1]))
    got = host_backward(hg, g[q0:q1], rptr[lo:hi + 1] - r0, k, tptr[r0:r1 + 1], tedge, tcoef, edge_base=int(q0))
    assert np.array_equal(bits(got), bits(whole[r0:r1]))


# ---- the restatement against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.KS)
def test_restatement_is_within_the_fp64_bound(k):
    _, qptr, _, rptr = G.ragged_clouds()
    tptr, tedge, tcoef = G.ragged_lists(k)
    ptr64, edge64, coef64 = G.ragged_lists(k, F64)
    assert np.array_equal(tptr, ptr64) and np.array_equal(tedge, edge64)
    worst = 0.0
    for c in G.CHANNELS:
        g = G.ragged_gradient(c)
        dx = G.backward(g, tptr, tedge, tcoef, k).astype(F64)
        dx64 = G.backward(g, tptr, tedge, coef64, k, dtype=F64)
        bound = G.bound(g, tptr, tedge, coef64, k)
        err = np.abs(dx - dx64)
        assert (err <= bound).all(), (k, c, float((err - bound).max()))
        live = bound > 0
        worst = max(worst, float((err[live] / bound[live]).max()))
        assert not dx[~live.any(axis=1)].any()
    print(f"k = {k}: worst |dx - dx64| / bound = {worst:.3f}")


@pytest.mark.parametrize("k", G.KS)
def test_adjoint_identity_in_fp64(k):
    """<interp(x), g> = <x, backward(g)>: the fp32 forward and backward restatements, the inner products in fp64, within the sum
    of the entrywise bounds of both sides (the forward's: (2k + 4) * 2^-24 * max|x over the row's neighbours|, test_interp_host)."""
    _, qptr, _, rptr = G.ragged_clouds()
    idx, d2 = G.ragged_search(k)
    tptr, tedge, tcoef = G.ragged_lists(k)
    _, _, coef64 = G.ragged_lists(k, F64)
    c = 50
    x = (np.random.default_rng(7).standard_normal((int(rptr[-1]), c)) * 10).astype(F32)
    g = G.ragged_gradient(c)
    out = R.interpolate_batched(x, qptr, rptr, idx, d2).astype(F64)
    dx = G.backward(g, tptr, tedge, tcoef, k).astype(F64)
    lhs, rhs = float((out * g.astype(F64)).sum()), float((x.astype(F64) * dx).sum())
    # the slack of each side: |g| . (bound of out) and |x| . (bound of dx)
    scale = np.zeros(int(qptr[-1]))
    for b in range(len(G.PAIRS)):
        rows = slice(qptr[b], qptr[b + 1])
        ok = (idx[rows] >= 0) & (idx[rows] < G.PAIRS[b][1])
        near = np.abs(x[rptr[b]:rptr[b + 1]].astype(F64))[np.where(ok, idx[rows], 0)] if G.PAIRS[b][1] else np.zeros((G.PAIRS[b][0], k, c))
        scale[rows] = np.where(ok[:, :, None], near, 0.0).max(axis=(1, 2)) if G.PAIRS[b][0] else 0
    slack = float((np.abs(g.astype(F64)) * ((2 * k + 4) * G.EPS * scale)[:, None]).sum())
    slack += float((np.abs(x.astype(F64)) * G.bound(g, tptr, tedge, coef64, k)).sum())
    print(f"k = {k}: <interp(x), g> - <x, backward(g)> = {lhs - rhs:.3e}, allowed {slack:.3e}")
    assert abs(lhs - rhs) <= slack


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_one_valid_slot_has_coefficient_one_and_dx_is_the_ordered_sum_of_g(hg):
    rng = np.random.default_rng(3)
    nq, nr, k, c = 300, 1, 4, 5
    idx, d2 = np.full((nq, k), -1, dtype=np.int32), np.full((nq, k), np.inf, dtype=F32)
    idx[:, 2], d2[:, 2] = 0, rng.random(nq, dtype=F32)                          # the one valid slot in the middle
    qptr, rptr = np.array([0, nq]), np.array([0, nr])
    g = (rng.standard_normal((nq, c)) * 1e3).astype(F32)
    want = np.zeros(c, dtype=F32)
    for q in range(nq):
        want = (want + g[q]).astype(F32)
    for tptr, tedge, tcoef in (G.transpose(idx, d2, qptr, rptr, nr), host_transpose(hg, idx, d2, qptr, rptr, nr)):
        assert tptr.tolist() == [0, nq] and np.array_equal(tedge, np.arange(nq) * k + 2) and (bits(tcoef) == bits(F32(1))).all()
        for dx in (G.backward(g, tptr, tedge, tcoef, k), host_backward(hg, g, rptr, k, tptr, tedge, tcoef)):
            assert np.array_equal(bits(dx[0]), bits(want))


def test_no_valid_slot_and_an_unpicked_row_give_zeros(hg):
    ref = np.array([[0, 0, 0], [9, 9, 9], [0.1, 0, 0]], dtype=F32)              # nobody picks row 1 at k = 2
    qry = np.random.default_rng(4).random((20, 3), dtype=F32) * 0.1
    idx, d2 = R.knn_cross(qry, ref, 2)
    assert not (idx == 1).any()
    g = np.ones((20, 3), dtype=F32)
    qptr, rptr = np.array([0, 20]), np.array([0, 3])
    for tptr, tedge, tcoef in (G.transpose(idx, d2, qptr, rptr, 3), host_transpose(hg, idx, d2, qptr, rptr, 3)):
        assert tptr[1] == tptr[2] and tptr[-1] == 40
        for dx in (G.backward(g, tptr, tedge, tcoef, 2), host_backward(hg, g, rptr, 2, tptr, tedge, tcoef)):
            assert not dx[1].any() and (dx[[0, 2]] > 0).all()
            assert abs(float(dx.astype(F64).sum()) - 60.0) < 1e-3               # the coefficients of a query sum to 1
    # an empty reference cloud, and slots that point outside the cloud: no in-edge, zeros
    eidx, ed2 = R.knn_cross(qry, ref[:0], 3)
    wild = np.array([[5, -3, 3]] * 20, dtype=np.int32)
    for i, d, nr in ((eidx, ed2, 0), (wild, np.ones((20, 3), dtype=F32), 3)):
        for tptr, tedge, tcoef in (G.transpose(i, d, qptr, np.array([0, nr]), nr), host_transpose(hg, i, d, qptr, [0, nr], nr)):
            assert not tptr.any() and tedge.size == 0 and tcoef.size == 0
            assert not G.backward(g, tptr, tedge, tcoef, 3).any()
    assert hg.hg_transpose(None, None, 0, 0, 0, 17, None, None, None, None, None) == -1


def test_duplicated_reference_points_send_every_in_edge_to_the_lower_id(hg):
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0]], dtype=F32)
    qry = np.array([[0, 0, 0], [1, 0, 0], [0.1, 0, 0], [0.9, 0, 0]], dtype=F32)
    idx, d2 = R.knn_cross(qry, ref, 1)
    assert idx[:, 0].tolist() == [0, 1, 0, 1]
    qptr, rptr = np.array([0, 4]), np.array([0, 4])
    for tptr, tedge, tcoef in (G.transpose(idx, d2, qptr, rptr, 4), host_transpose(hg, idx, d2, qptr, rptr, 4)):
        assert tptr.tolist() == [0, 2, 4, 4, 4] and tedge.tolist() == [0, 2, 1, 3] and (tcoef == 1).all()


def test_a_nan_distance_takes_the_clamp(hg):
    idx = np.array([[0, 1]], dtype=np.int32)
    d2 = np.array([[np.nan, 1e-16]], dtype=F32)
    for c in (G.coefficients(idx, d2, 2)[0], ):
        assert np.array_equal(bits(c), bits(np.array([[0.5, 0.5]])))
    got = np.zeros((1, 2), dtype=F32)
    hg.hg_coef(1, 2, 2, P(idx), P(d2), P(got))
    assert np.array_equal(bits(got), bits(np.array([[0.5, 0.5]])))
    tptr, tedge, tcoef = host_transpose(hg, idx, d2, [0, 1], [0, 2], 2)
    assert tptr.tolist() == [0, 1, 2] and tedge.tolist() == [0, 1] and tcoef.tolist() == [0.5, 0.5]
