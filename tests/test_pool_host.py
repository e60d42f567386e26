"""Host side of the cross-cloud pooling (csrc/pool_math.h: fwd4 / store_arg4 / load_arg4 / bwd4), without a GPU: a g++ build of
those functions (tests/hostcheck_pool) against the numpy restatement (tests/pool_restate.py) bit for bit -- values, ``arg`` and
``cnt``, forward and backward, on both load paths and both ``arg`` paths; the restatement against its fp64 form within

    max / min   out and arg EQUAL the fp64 selection on the same fp32 inputs (a selection rounds nothing; ties: the lowest slot)
    sum         |out - out64| <= cnt * 2^-24 * sum_s |x_s|
    mean        |out - out64| <= (cnt + 1) * 2^-24 * sum_s |x_s| / cnt
    backward    |dx - dx64| <= (L_j + 2) * 2^-24 * sum_e |term_e|          (L_j the terms added, the sum formed in fp64)

-- a value of an n-term sequential sum passes through at most n - 1 additions, each within 2^-24 relative of a partial sum that
is itself at most sum |terms| (first order: (n - 1) * 2^-24 * sum |terms|); the mean's division and the term's division of the
mean's backward add one rounding each; the remaining 1 (forward) and 2 (backward) cover the second order.  The adjoint identity
<pool(x), g> = <x, backward(g)> in fp64 for sum and mean within the sum of those bounds; the edge cases.  The worst ratio to every
bound is printed by the tests that hold it."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import pool_restate as P
from tests.helpers import ROOT

HP_DIR = os.path.join(ROOT, "tests", "hostcheck_pool")
PTR = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
F32, F64 = np.float32, np.float64
CHANNELS = (1, 3, 4, 5, 8, 67)
MODES = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def hp():
    subprocess.run(["make", "-s", "-C", HP_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HP_DIR, "libhostcheck_pool.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hp_forward.argtypes, lib.hp_forward.restype = [vp, i64, i32, vp, vp, i32, i32, vp, i32, i32, vp, i64, vp, i64, i32, vp], i32
    lib.hp_backward.argtypes, lib.hp_backward.restype = [vp, i64, i64, i32, vp, i32, i32, vp, vp, i32, vp, i64, i32, vp, i32, vp, i64], i32
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def laid_out(a, vec, pad=3):
    """a [rows,C] fp32 with a leading dimension of C + pad whose gap holds NaN; vec: 16-byte aligned rows (ld a multiple of 4),
    otherwise a base one float off alignment."""
    rows, c = a.shape
    ld = c + pad
    if vec:
        ld = (ld + 3) // 4 * 4
    raw = np.full(max(rows, 1) * ld + 8, np.nan, dtype=F32)
    off = (-(raw.ctypes.data // 4)) % 4
    off = off if vec else off + 1
    wide = raw[off:off + rows * ld].reshape(rows, ld)
    wide[:, :c] = a
    assert (wide.ctypes.data % 16 == 0) == vec or rows == 0
    return wide, ld


def arg_buffer(rows, c, word):
    """uint8 [rows, ld] prefilled with 77: ld a multiple of 4 on a 4-byte aligned base (word stores), or odd on an odd base."""
    ld = (c + 4) // 4 * 4 if word else (c + 1) | 1
    raw = np.full(max(rows, 1) * ld + 8, 77, dtype=np.uint8)
    off = (-raw.ctypes.data) % 4
    off = off if word else off + 1
    return raw[off:off + rows * ld].reshape(rows, ld), ld


def host_forward(hp, x, qptr, rptr, idx, mode, vec=False, word=False, with_arg=True):
    """-> (out, arg or None, cnt) of hp_forward on padded layouts: x's gaps hold NaN, out is prefilled with NaN beside two guard
    columns, arg with 77 (its gap must keep it), cnt with 99."""
    nq, c = idx.shape[0], x.shape[1]
    wide, ldx = laid_out(x, vec)
    qptr, rptr = np.ascontiguousarray(qptr, dtype=np.int64), np.ascontiguousarray(rptr, dtype=np.int64)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    out = np.full((nq, c + 2), np.nan, dtype=F32)
    out[:, c:] = -7
    arg, ldarg = arg_buffer(nq, c, word) if with_arg else (None, 0)
    cnt = np.full(nq, 99, dtype=np.uint8)
    rc = hp.hp_forward(PTR(wide), ldx, c, PTR(qptr), PTR(rptr), len(qptr) - 1, idx.shape[1], PTR(idx), mode, int(vec), PTR(out), c + 2,
                       PTR(arg), ldarg, int(word), PTR(cnt))
    assert rc == 0
    assert (out[:, c:] == -7).all(), "the guard columns of out were written"
    if arg is not None:
        assert (arg[:, c:] == 77).all(), "the gap of arg was written"
        if mode >= 2:
            assert (arg == 77).all(), "sum / mean wrote arg"
    return np.ascontiguousarray(out[:, :c]), (None if arg is None else np.ascontiguousarray(arg[:, :c])), cnt


def host_backward(hp, g, rptr, k, tptr, tedge, mode, arg, cnt, vec=False, word=False):
    """g and arg on padded layouts (the gaps hold NaN / 77), dx prefilled with NaN beside two guard columns."""
    rows, c = g.shape
    wide, ldg = laid_out(g, vec)
    rptr, tptr = np.ascontiguousarray(rptr, dtype=np.int64), np.ascontiguousarray(tptr, dtype=np.int64)
    tedge = np.ascontiguousarray(tedge, dtype=np.int64)
    abuf, ldarg = (None, 0)
    if arg is not None:
        abuf, ldarg = arg_buffer(rows, c, word)
        abuf[:, :c] = arg
    num_ref = len(tptr) - 1
    dx = np.full((num_ref, c + 2), np.nan, dtype=F32)
    dx[:, c:] = -7
    cnt = np.ascontiguousarray(cnt, dtype=np.uint8)
    rc = hp.hp_backward(PTR(wide), ldg, rows, c, PTR(rptr), len(rptr) - 1, k, PTR(tptr), PTR(tedge), mode, PTR(abuf), ldarg, int(word),
                        PTR(cnt), int(vec), PTR(dx), c + 2)
    assert rc == 0 and (dx[:, c:] == -7).all()
    return np.ascontiguousarray(dx[:, :c])


# ---- g++ build of pool_math.h = the restatement, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("k", P.KS)
def test_hostcheck_equals_the_restatement_bitwise(hp, k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    tptr, tedge, _ = P.ragged_lists(k)
    for mode in MODES:
        x, g, out, arg, cnt, dx = P.ragged_case(k, mode)
        assert (cnt == (idx >= 0).sum(axis=1)).all() and cnt.max() == k and (cnt == 0).any()    # a pair without reference points
        assert k == 1 or ((cnt > 0) & (cnt < k)).any()                            # and reference clouds smaller than k
        for c in CHANNELS:
            for vec, word in ((False, False), (True, True), (True, False)):
                got, garg, gcnt = host_forward(hp, x[:, :c], qptr, rptr, idx, mode, vec, word)
                assert not np.isnan(got).any(), "a query row of a pair was not written"
                assert np.array_equal(bits(got), bits(out[:, :c])), (k, mode, c, vec)
                assert np.array_equal(gcnt, cnt)
                if mode <= 1:
                    assert np.array_equal(garg, arg[:, :c]), (k, mode, c, word)
                back = host_backward(hp, g[:, :c], rptr, k, tptr, tedge, mode, arg[:, :c] if mode <= 1 else None, cnt, vec, word)
                assert not np.isnan(back).any(), "a reference row of a pair was not written"
                assert np.array_equal(bits(back), bits(dx[:, :c])), (k, mode, c, vec, word)
        if mode >= 2:                                                             # sum / mean take no arg at all
            got, garg, gcnt = host_forward(hp, x[:, :5], qptr, rptr, idx, mode, with_arg=False)
            assert garg is None and np.array_equal(bits(got), bits(out[:, :5])) and np.array_equal(gcnt, cnt)
    assert hp.hp_forward(None, 0, 1, None, None, 0, 17, None, 0, 0, None, 0, None, 0, 0, None) == -1
    assert hp.hp_forward(None, 0, 1, None, None, 0, 3, None, 4, 0, None, 0, None, 0, 0, None) == -1


# ---- the restatement against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", P.KS)
def test_selection_equals_the_fp64_selection_and_ties_go_to_the_lowest_slot(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    for mode in (0, 1):
        for kind in ("ties", "distinct"):
            x, _, out, arg, cnt, _ = P.ragged_case(k, mode, kind)
            out64, arg64, cnt64, _ = P.forward64(x, qptr, rptr, idx, mode)
            assert np.array_equal(out.astype(F64), out64) and np.array_equal(arg, arg64) and np.array_equal(cnt, cnt64)
        x, _, out, arg, cnt, _ = P.ragged_case(k, mode)
        if k > 1:                                                                # the ties are there, and the lowest slot has them
            rows, ok = P._gathered(x, qptr, rptr, idx)
            near = np.where(ok[:, :, None], x[rows], np.nan)
            tied = (near == out[:, None, :]).sum(axis=1)
            assert (tied[cnt > 0] >= 1).all() and (tied > 1).sum() > 1000        # thousands of ties at every k > 1
            first = (near == out[:, None, :]).argmax(axis=1)
            assert np.array_equal(first[cnt > 0], arg[cnt > 0])


@pytest.mark.parametrize("k", P.KS)
def test_sum_and_mean_are_within_the_fp64_bound(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    for mode, name in ((2, "sum"), (3, "mean")):
        x, _, out, _, cnt, _ = P.ragged_case(k, mode, "gauss")
        out64, _, cnt64, mag = P.forward64(x, qptr, rptr, idx, mode)
        assert np.array_equal(cnt, cnt64)
        bound = P.forward_bound(mode, cnt, mag)
        err = np.abs(out.astype(F64) - out64)
        assert (err <= bound).all(), (k, mode, float((err - bound).max()))
        live = bound > 0
        assert not out[cnt == 0].any()
        print(f"k = {k}, {name}: worst |out - out64| / bound = {float((err[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("k", P.KS)
def test_backward_is_within_the_fp64_bound(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    num_ref = int(rptr[-1])
    for mode, name in enumerate(("max", "min", "sum", "mean")):
        # max / min on tie-free x: the gradient of the fp64 selection (its own arg) is the yardstick
        x, g, _, arg, cnt, dx = P.ragged_case(k, mode, "distinct" if mode <= 1 else "gauss")
        arg64 = P.forward64(x, qptr, rptr, idx, mode)[1]
        dx64, mag, terms = P.backward64(g, qptr, rptr, idx, mode, arg64, cnt, num_ref)
        bound = P.backward_bound(mag, terms)
        err = np.abs(dx.astype(F64) - dx64)
        assert (err <= bound).all(), (k, mode, float((err - bound).max()))
        live = bound > 0
        assert not dx[~live].any()
        if mode >= 2:
            assert np.array_equal(terms[:, 0], np.diff(P.ragged_lists(k)[0]))
        else:
            assert np.array_equal(terms.sum(axis=0), np.full(P.WIDTH, int((cnt > 0).sum())))   # one winner per query and channel
        print(f"k = {k}, {name}: worst |dx - dx64| / bound = {float((err[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("k", P.KS)
def test_adjoint_identity_in_fp64(k):
    """<pool(x), g> = <x, backward(g)> for the two linear modes: the fp32 restatements, the inner products in fp64, within
    |g| . (bound of out) + |x| . (bound of dx)."""
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    for mode, name in ((2, "sum"), (3, "mean")):
        x, g, out, arg, cnt, dx = P.ragged_case(k, mode, "gauss")
        _, _, _, xmag = P.forward64(x, qptr, rptr, idx, mode)
        _, gmag, terms = P.backward64(g, qptr, rptr, idx, mode, arg, cnt, int(rptr[-1]))
        x64, g64 = x.astype(F64), g.astype(F64)
        lhs, rhs = float((out.astype(F64) * g64).sum()), float((x64 * dx.astype(F64)).sum())
        slack = float((np.abs(g64) * P.forward_bound(mode, cnt, xmag)).sum() + (np.abs(x64) * P.backward_bound(gmag, terms)).sum())
        print(f"k = {k}, {name}: <pool(x), g> - <x, backward(g)> = {lhs - rhs:.3e}, allowed {slack:.3e}")
        assert abs(lhs - rhs) <= slack


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_k_1_is_an_exact_gather_and_its_backward_an_exact_scatter_sum(hp):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(1)
    tptr, tedge, _ = P.ragged_lists(1)
    x, g = P.ragged_features("gauss")[:, :5].copy(), P.ragged_gradient()[:, :5]
    x[::7, 0] = -0.0                                                            # copied bit for bit: the sign of a zero too
    rows, ok = P._gathered(x, qptr, rptr, idx)
    want = np.where(ok[:, 0, None], x[rows[:, 0]], F32(0))
    scatter = np.zeros_like(x)
    for q in np.nonzero(ok[:, 0])[0]:                                            # ascending query row = ascending edge id at k = 1
        scatter[rows[q, 0]] = (scatter[rows[q, 0]] + g[q]).astype(F32)
    for mode in MODES:
        for out, arg, cnt in (P.forward(x, qptr, rptr, idx, mode), host_forward(hp, x, qptr, rptr, idx, mode)):
            assert np.array_equal(bits(out), bits(want)) and np.array_equal(cnt, ok[:, 0])
            if mode <= 1:
                assert np.array_equal(arg, np.where(ok[:, 0, None], 0, 255) * np.ones_like(arg))
        _, arg, cnt = P.forward(x, qptr, rptr, idx, mode)
        for dx in (P.backward(g, tptr, tedge, 1, mode, arg, cnt), host_backward(hp, g, rptr, 1, tptr, tedge, mode, arg, cnt)):
            assert np.array_equal(bits(dx), bits(scatter))


def test_a_query_without_a_valid_slot_gives_zeros_and_feeds_nothing_back(hp):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 5)).astype(F32)
    idx = np.array([[0, 2, 1], [-1, 7, 3], [2, -1, 9]], dtype=np.int32)         # query 1: every slot outside [0, 3)
    qptr, rptr = np.array([0, 3]), np.array([0, 3])
    g = np.ones((3, 5), dtype=F32)
    tptr, tedge = np.array([0, 1, 2, 4]), np.array([0, 2, 1, 6])               # the valid slots only: (0,0) (0,2) (0,1) (2,0)
    for mode in MODES:
        for out, arg, cnt in (P.forward(x, qptr, rptr, idx, mode), host_forward(hp, x, qptr, rptr, idx, mode)):
            assert not out[1].any() and cnt.tolist() == [3, 0, 1] and np.array_equal(bits(out[2]), bits(x[2]))
            if mode <= 1:
                assert (arg[1] == 255).all() and (arg[2] == 0).all()
        _, arg, cnt = P.forward(x, qptr, rptr, idx, mode)
        want = P.backward64(g, qptr, rptr, idx, mode, arg, cnt, 3)[0]
        for dx in (P.backward(g, tptr, tedge, 3, mode, arg, cnt), host_backward(hp, g, rptr, 3, tptr, tedge, mode, arg, cnt)):
            assert np.allclose(dx, want, rtol=1e-6, atol=0) and abs(float(dx.sum()) - 5 * (2 if mode <= 1 else (4 if mode == 2 else 2))) < 1e-5
    # an empty reference cloud: nothing is indexed (x has no row at all)
    for mode in MODES:
        out, arg, cnt = host_forward(hp, np.zeros((0, 5), dtype=F32), qptr, np.array([0, 0]), idx, mode)
        assert not out.any() and not cnt.any() and (mode >= 2 or (arg == 255).all())


def test_a_nan_in_a_later_slot_is_dropped_and_one_in_the_first_valid_slot_stays(hp):
    x = np.array([[1.0], [np.nan], [3.0], [2.0]], dtype=F32)
    idx = np.array([[0, 1, 2, 3],                                               # later NaN: max 3 from slot 2, min 1 from slot 0
                    [1, 0, 2, 3],                                               # first NaN: stays
                    [-1, 1, 2, 0]], dtype=np.int32)                             # first VALID slot (1) is the NaN: stays
    qptr, rptr = np.array([0, 3]), np.array([0, 4])
    for fwd in (lambda m: P.forward(x, qptr, rptr, idx, m), lambda m: host_forward(hp, x, qptr, rptr, idx, m)):
        out, arg, cnt = fwd(0)
        assert out[0, 0] == 3 and arg[0, 0] == 2 and np.isnan(out[1, 0]) and arg[1, 0] == 0 and np.isnan(out[2, 0]) and arg[2, 0] == 1
        assert cnt.tolist() == [4, 4, 3]
        out, arg, _ = fwd(1)
        assert out[0, 0] == 1 and arg[0, 0] == 0 and np.isnan(out[1, 0]) and arg[1, 0] == 0 and np.isnan(out[2, 0]) and arg[2, 0] == 1
        assert np.isnan(fwd(2)[0]).all() and np.isnan(fwd(3)[0]).all()           # a sum keeps every NaN


def test_rows_outside_every_pair_are_untouched(hp):
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal((9, 4)).astype(F32), rng.standard_normal((8, 4)).astype(F32)
    idx = rng.integers(0, 3, (8, 2)).astype(np.int32)
    qptr, rptr = np.array([2, 5, 7]), np.array([1, 4, 8])                       # query rows 0, 1, 7 and reference rows 0, 8: no pair
    for mode in MODES:
        for vec in (False, True):
            wide, ldx = laid_out(x, vec)
            out, cnt = np.full((8, 4), np.nan, dtype=F32), np.full(8, 99, dtype=np.uint8)
            arg, ldarg = arg_buffer(8, 4, vec)
            i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
            assert hp.hp_forward(PTR(wide), ldx, 4, PTR(i64(qptr)), PTR(i64(rptr)), 2, 2, PTR(idx), mode, int(vec), PTR(out), 4, PTR(arg),
                                 ldarg, int(vec), PTR(cnt)) == 0
            want, warg, wcnt = P.forward(x, qptr, rptr, idx, mode)
            assert np.isnan(out[[0, 1, 7]]).all() and (cnt[[0, 1, 7]] == 99).all() and (arg[[0, 1, 7]] == 77).all()
            assert np.array_equal(bits(out[2:7]), bits(want[2:7])) and np.array_equal(cnt[2:7], wcnt[2:7])
            # the lists of the two pairs, from the restated slots
            es = [(int(rptr[b]) + idx[q, s], q * 2 + s) for b in range(2) for q in range(qptr[b], qptr[b + 1]) for s in range(2)]
            tptr = np.zeros(10, dtype=np.int64)
            for r, _ in es:
                tptr[r + 1:] += 1
            tedge = np.array([e for _, e in sorted(es)], dtype=np.int64)
            dx = np.full((9, 4), np.nan, dtype=F32)
            gw, ldg = laid_out(g, vec)
            abuf, lda = arg_buffer(8, 4, vec)
            abuf[:, :4] = warg
            assert hp.hp_backward(PTR(gw), ldg, 8, 4, PTR(i64(rptr)), 2, 2, PTR(tptr), PTR(tedge), mode, PTR(abuf), lda, int(vec),
                                  PTR(wcnt), int(vec), PTR(dx), 4) == 0
            assert np.isnan(dx[[0, 8]]).all() and not np.isnan(dx[1:8]).any()
            assert np.array_equal(bits(dx[1:8]), bits(P.backward(g, tptr, tedge, 2, mode, warg, wcnt)[1:8]))
    # an edge whose query row lies outside g is skipped: g cut to its first 5 rows
    want = P.backward(g[:5], tptr, tedge, 2, 2, warg[:5], wcnt[:5])
    got = host_backward(hp, g[:5], np.array([0, 9]), 2, tptr, tedge, 2, None, wcnt[:5])
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(want), bits(P.backward(g, tptr, tedge, 2, 2, warg, wcnt)))
