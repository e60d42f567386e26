"""Host side of the cross-cloud pooling of tangent-vector features (csrc/pool_vectors_math.h: rotation / fwd4 / bwd4), without a
GPU: a g++ build of those functions (tests/hostcheck_pool_vectors) against the numpy restatement (tests/pool_vectors_restate.py)
bit for bit -- table, values, ``arg`` and ``cnt``, forward and the three backwards, on both load paths and both ``arg`` paths;
the restatement against its fp64 form, taking the fp32 table as given (the table against the reference's connection is
tests/test_connection_host.py's), with u = 2^-24 and S = sum_s (|R00 v0| + |R01 v1|) per component:

    sum         |out - out64| <= 2 cnt u S          (per slot two product roundings and two additions, no partial sum above S)
    mean        |out - out64| <= (2 cnt + 1) u S / cnt                                  (one more rounding: the division)
    backward    the same form over the L terms of a list, T = sum_e (|R00 g0| + |R10 g1|): 2 L u T; mean (2 L + 1) u T
    max         arg EQUALS the fp64 selection where the keys are exact (ties: the lowest slot); on random inputs the chosen
                slot's exact squared norm is >= (1 - 2^-22) of the largest (three roundings on non-negative terms); the value
                is within 3 u (|R00 v0| + |R01 v1|) of the fp64 transport of that slot

-- derived in the header's comment; the worst ratio to every bound is printed.  In fp64 the 3-D vector max and mean return does
not depend on the choice of frames; the adjoint identity holds for sum and mean; on a coarse cloud that is a SUBSET of the fine
one the transported interpolation is a gather of the coarse points' own vectors, which is what the pooling is for."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import connection_restate as CR
from tests import interp_restate as IR
from tests import pool_vectors_restate as P
from tests import vector_interp_restate as V
from tests.helpers import ROOT

HP_DIR = os.path.join(ROOT, "tests", "hostcheck_pool_vectors")
F32, F64 = np.float32, np.float64
I64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
PTR = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None


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


def orthonormal64(frames):
    n, x = (np.asarray(a, dtype=F64) for a in frames[:2])
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    x = x - n * (x * n).sum(1, keepdims=True)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return n, x, np.cross(n, x)


def turned(frames, theta):
    """Every frame turned about its normal by its angle."""
    n, x, y = frames
    c, s = np.cos(theta)[:, None], np.sin(theta)[:, None]
    return n, c * x + s * y, -s * x + c * y


@pytest.fixture(scope="module")
def hp():
    subprocess.run(["make", "-s", "-C", HP_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HP_DIR, "libhostcheck_pool_vectors.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hpv_rotation.argtypes, lib.hpv_rotation.restype = [vp, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, i32, vp], i32
    lib.hpv_forward.argtypes, lib.hpv_forward.restype = [vp, i64, i32, vp, vp, i32, i32, vp, vp, i32, i32, vp, i64, vp, i64, i32, vp], i32
    lib.hpv_backward.argtypes = [vp, i64, i64, i32, vp, i32, i32, vp, vp, vp, i32, vp, i64, i32, vp, i32, vp, i64]
    lib.hpv_backward.restype = i32
    return lib


def host_table(hp, idx, qptr, rptr, tframes, sframes, non_oriented=True):
    nq, k = idx.shape
    raw = np.full(4 * nq * k + 8, np.nan, dtype=F32)
    off = (-(raw.ctypes.data // 4)) % 4
    rmat = raw[off:off + 4 * nq * k]
    c = lambda a: np.ascontiguousarray(a, dtype=F32)
    tn, tx, ty, sn, sx = c(tframes[0]), c(tframes[1]), c(tframes[2]), c(sframes[0]), c(sframes[1])
    qptr, rptr, idx = I64(qptr), I64(rptr), np.ascontiguousarray(idx, dtype=np.int32)
    assert hp.hpv_rotation(PTR(qptr), PTR(rptr), len(qptr) - 1, nq, k, PTR(idx), PTR(tn), PTR(tx), PTR(ty), PTR(sn), PTR(sx),
                           int(non_oriented), PTR(rmat)) == 0
    return rmat.reshape(-1, 4)


def host_forward(hp, v, qptr, rptr, idx, rmat, mode, vec=False, word=False, with_arg=True):
    """-> (out, arg or None, cnt) of hpv_forward on padded layouts: v's gaps hold NaN, out is prefilled with NaN beside two guard
    columns, arg with 77 (its gap must keep it), cnt with 99."""
    nq, c = idx.shape[0], v.shape[1]
    wide, ldv = laid_out(v, vec)
    qptr, rptr, idx = I64(qptr), I64(rptr), np.ascontiguousarray(idx, dtype=np.int32)
    rmat = host_aligned(rmat)
    out = np.full((2 * nq, c + 2), np.nan, dtype=F32)
    out[:, c:] = -7
    arg, ldarg = arg_buffer(nq, c, word) if with_arg else (None, 0)
    cnt = np.full(nq, 99, dtype=np.uint8)
    rc = hp.hpv_forward(PTR(wide), ldv, c, PTR(qptr), PTR(rptr), len(qptr) - 1, idx.shape[1], PTR(idx), PTR(rmat), mode, int(vec),
                        PTR(out), c + 2, PTR(arg), ldarg, int(word), PTR(cnt))
    assert rc == 0
    assert (out[:, c:] == -7).all(), "the guard columns of out were written"
    if arg is not None:
        assert (arg[:, c:] == 77).all(), "the gap of arg was written"
        if mode >= 2:
            assert (arg == 77).all(), "sum / mean wrote arg"
    return np.ascontiguousarray(out[:, :c]), (None if arg is None else np.ascontiguousarray(arg[:, :c])), cnt


def host_aligned(rmat):
    rmat = np.asarray(rmat, dtype=F32).reshape(-1)
    raw = np.zeros(rmat.size + 8, dtype=F32)
    off = (-(raw.ctypes.data // 4)) % 4
    raw[off:off + rmat.size] = rmat
    return raw[off:off + rmat.size]


def host_backward(hp, g, rptr, k, tptr, tedge, rmat, mode, arg, cnt, vec=False, word=False):
    """g and arg on padded layouts (the gaps hold NaN / 77), dv prefilled with NaN beside two guard columns."""
    c = g.shape[1]
    rows = g.shape[0] // 2
    wide, ldg = laid_out(g, vec)
    rptr, tptr, tedge = I64(rptr), I64(tptr), I64(tedge)
    rmat = host_aligned(rmat)
    abuf, ldarg = (None, 0)
    if arg is not None:
        abuf, ldarg = arg_buffer(rows, c, word)
        abuf[:, :c] = arg
    num_ref = len(tptr) - 1
    dv = np.full((2 * num_ref, c + 2), np.nan, dtype=F32)
    dv[:, c:] = -7
    cnt = np.ascontiguousarray(cnt, dtype=np.uint8)
    rc = hp.hpv_backward(PTR(wide), ldg, rows, c, PTR(rptr), len(rptr) - 1, k, PTR(tptr), PTR(tedge), PTR(rmat), mode, PTR(abuf),
                         ldarg, int(word), PTR(cnt), int(vec), PTR(dv), c + 2)
    assert rc == 0 and (dv[:, c:] == -7).all()
    return np.ascontiguousarray(dv[:, :c])


# ---- g++ build of pool_vectors_math.h = the restatement, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("k", P.KS)
def test_hostcheck_equals_the_restatement_bitwise(hp, k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    tptr, tedge, _ = P.ragged_lists(k)
    tf, sf = P.ragged_frames()
    assert np.diff(tptr).max() >= 2000                                          # one in-edge list of about 2 100
    for non_oriented in (True, False):
        rmat = P.ragged_table(k, non_oriented)
        assert np.array_equal(bits(host_table(hp, idx, qptr, rptr, tf, sf, non_oriented)), bits(rmat)), (k, non_oriented)
    ok, _ = P.slots(idx, qptr, rptr)
    assert not rmat.reshape(-1, k, 4)[~ok].any() and not np.signbit(rmat.reshape(-1, k, 4)[~ok]).any()   # four +0.0f
    for mode in P.MODE_CODES:
        v, g, rmat, out, arg, cnt, dv = P.ragged_case(k, mode)
        assert (cnt == ok.sum(axis=1)).all() and cnt.max() == k and (cnt == 0).any()        # a pair without reference points
        assert k == 1 or ((cnt > 0) & (cnt < k)).any()                                      # and reference clouds smaller than k
        for c in P.CHANNELS:
            for vec, word in ((False, False), (True, True), (True, False)):
                got, garg, gcnt = host_forward(hp, v[:, :c], qptr, rptr, idx, rmat, mode, vec, word)
                assert not np.isnan(got).any(), "a query row of a pair was not written"
                assert np.array_equal(bits(got), bits(out[:, :c])), (k, mode, c, vec)
                assert np.array_equal(gcnt, cnt)
                if mode == 0:
                    assert np.array_equal(garg, arg[:, :c]), (k, mode, c, word)
                back = host_backward(hp, g[:, :c], rptr, k, tptr, tedge, rmat, mode, arg[:, :c] if mode == 0 else None, cnt, vec, word)
                assert not np.isnan(back).any(), "a reference row of a pair was not written"
                assert np.array_equal(bits(back), bits(dv[:, :c])), (k, mode, c, vec, word)
        if mode >= 2:                                                            # sum / mean take no arg at all
            got, garg, gcnt = host_forward(hp, v[:, :6], qptr, rptr, idx, rmat, mode, with_arg=False)
            assert garg is None and np.array_equal(bits(got), bits(out[:, :6])) and np.array_equal(gcnt, cnt)
    # sum IS the transported interpolation on the rotation table, forward and backward
    v, g, rmat, out, _, _, dv = P.ragged_case(k, 2)
    d2 = P.ragged_search(k)[1]
    assert np.array_equal(bits(V.forward(v[:, :6], idx, d2, qptr, rptr, rmat)), bits(out[:, :6]))
    assert np.array_equal(bits(V.backward(g[:, :6], tptr, tedge, rmat, k)), bits(dv[:, :6]))
    assert hp.hpv_forward(None, 0, 1, None, None, 0, 17, None, None, 0, 0, None, 0, None, 0, 0, None) == -1
    assert hp.hpv_forward(None, 0, 1, None, None, 0, 3, None, None, 1, 0, None, 0, None, 0, 0, None) == -1     # min is refused


# ---- the restatement against fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", P.KS)
def test_max_selects_what_fp64_selects_and_ties_go_to_the_lowest_slot(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    v, _, rmat, out, arg, cnt, _ = P.ragged_case(k, 0, "ties")
    _, arg64, cnt64, _ = P.forward64(v, idx, qptr, rptr, rmat, 0)
    assert np.array_equal(arg, arg64) and np.array_equal(cnt, cnt64)
    key = P.transported64(v, idx, qptr, rptr, rmat)[4]
    if k > 1:
        tied = (key == key.max(axis=1, keepdims=True)).sum(axis=1)[cnt > 0]
        assert (tied > 1).sum() > 1000                                           # thousands of ties at every k > 1
    # random inputs: the chosen slot's exact squared norm is within three roundings of the largest, the value within 3 u S
    v, _, rmat, out, arg, cnt, _ = P.ragged_case(k, 0, "gauss")
    key = P.transported64(v, idx, qptr, rptr, rmat)[4]
    some = cnt > 0
    chosen = np.take_along_axis(key, np.where(arg == 255, 0, arg).astype(np.int64)[:, None, :], axis=1)[:, 0, :]
    assert (chosen[some] >= (1 - 2.0 ** -22) * key.max(axis=1)[some]).all()
    out64, _, _, mag = P.forward64(v, idx, qptr, rptr, rmat, 0, arg=arg)
    bound = P.forward_bound(0, cnt, mag)
    err = np.abs(out.astype(F64) - out64)
    assert (err <= bound).all(), (k, float((err - bound).max()))
    assert not out[np.repeat(~some, 2)].any() and (arg[~some] == 255).all()
    live = bound > 0
    print(f"k = {k}, max: worst |out - out64| / bound = {float((err[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("k", P.KS)
def test_sum_and_mean_are_within_the_fp64_bound(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    for mode, name in ((2, "sum"), (3, "mean")):
        v, _, rmat, out, _, cnt, _ = P.ragged_case(k, mode, "gauss")
        out64, _, cnt64, mag = P.forward64(v, idx, qptr, rptr, rmat, mode)
        assert np.array_equal(cnt, cnt64)
        bound = P.forward_bound(mode, cnt, mag)
        err = np.abs(out.astype(F64) - out64)
        assert (err <= bound).all(), (k, mode, float((err - bound).max()))
        live = bound > 0
        assert not out[np.repeat(cnt == 0, 2)].any()
        print(f"k = {k}, {name}: worst |out - out64| / bound = {float((err[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("k", P.KS)
def test_backward_is_within_the_fp64_bound(k):
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    num_ref = int(rptr[-1])
    for mode, name in ((0, "max"), (2, "sum"), (3, "mean")):
        v, g, rmat, _, arg, cnt, dv = P.ragged_case(k, mode, "gauss")
        dv64, mag, terms = P.backward64(g, idx, qptr, rptr, rmat, mode, arg, cnt, num_ref)
        bound = P.backward_bound(mode, mag, terms)
        err = np.abs(dv.astype(F64) - dv64)
        assert (err <= bound).all(), (k, mode, float((err - bound).max()))
        live = bound > 0
        assert not dv[~live].any()
        if mode >= 2:
            assert np.array_equal(terms[:, 0], np.diff(P.ragged_lists(k)[0]))
        else:
            assert np.array_equal(terms.sum(axis=0), np.full(P.WIDTH, int((cnt > 0).sum())))   # one winner per query and channel
        print(f"k = {k}, {name}: worst |dv - dv64| / bound = {float((err[live] / bound[live]).max()):.3f}")


@pytest.mark.parametrize("k", P.KS)
def test_adjoint_identity_in_fp64(k):
    """<pool(v), g> = <v, backward(g)> for the two linear modes: the fp32 restatements, the inner products in fp64, within
    |g| . (bound of out) + |v| . (bound of dv)."""
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    for mode, name in ((2, "sum"), (3, "mean")):
        v, g, rmat, out, arg, cnt, dv = P.ragged_case(k, mode, "gauss")
        vmag = P.forward64(v, idx, qptr, rptr, rmat, mode)[3]
        _, gmag, terms = P.backward64(g, idx, qptr, rptr, rmat, mode, arg, cnt, int(rptr[-1]))
        v64, g64 = v.astype(F64), g.astype(F64)
        lhs, rhs = float((out.astype(F64) * g64).sum()), float((v64 * dv.astype(F64)).sum())
        slack = float((np.abs(g64) * P.forward_bound(mode, cnt, vmag)).sum() +
                      (np.abs(v64) * P.backward_bound(mode, gmag, terms)).sum())
        print(f"k = {k}, {name}: <pool(v), g> - <v, backward(g)> = {lhs - rhs:.3e}, allowed {slack:.3e}")
        assert abs(lhs - rhs) <= slack


# ---- frame independence ----------------------------------------------------------------------------------------------------------------
def _subset_pair(n, m, k, seed):
    """A bumpy sphere of n points and a sorted random subset of m of them with the SAME frames, the subset the QUERY (the way
    down) -> dict(tframes, sframes, keep, qptr, rptr, idx, d2)."""
    pos, nrm, xb, yb = CR.cloud(n, seed)
    keep = np.sort(np.random.default_rng(1000 + seed).permutation(n)[:m])
    qptr, rptr = np.array([0, m], dtype=np.int64), np.array([0, n], dtype=np.int64)
    idx, d2 = IR.knn_cross_batched(pos[keep], qptr, pos, rptr, k)
    return dict(tframes=(nrm[keep], xb[keep], yb[keep]), sframes=(nrm, xb, yb), keep=keep, qptr=qptr, rptr=rptr, idx=idx, d2=d2)


def test_max_and_mean_do_not_depend_on_the_choice_of_frames():
    worst = 0.0
    for seed, n, m, k in ((1, 600, 150, 16), (2, 500, 90, 5)):
        S = _subset_pair(n, m, k, seed)
        rng = np.random.default_rng(60 + seed)
        tf, sf = orthonormal64(S["tframes"]), orthonormal64(S["sframes"])
        v = rng.standard_normal((2 * n, 3)) * 3
        args = (S["idx"], S["qptr"], S["rptr"])
        size = np.sqrt(v[0::2] ** 2 + v[1::2] ** 2)
        ok, src = P.slots(*args)
        tol = 2.0 ** -40 * (size[src] * ok[:, :, None]).sum(axis=1)[:, None, :]
        theta = rng.uniform(-np.pi, np.pi, n)                                   # every source frame turned about its normal
        cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
        v_turned = np.empty_like(v)
        v_turned[0::2], v_turned[1::2] = cs * v[0::2] + sn * v[1::2], -sn * v[0::2] + cs * v[1::2]
        phi = rng.uniform(-np.pi, np.pi, m)                                     # separately, every target frame
        for mode in (0, 3):
            def in_space(tframes, sframes, vals):
                out = P.forward(vals, *args, P.table(*args, tframes, sframes, True, F64), mode, F64)[0]
                return out[0::2, None, :] * tframes[1][:, :, None] + out[1::2, None, :] * tframes[2][:, :, None]    # [Nq, 3, C]

            base = in_space(tf, sf, v)
            for label, got in (("source", in_space(tf, turned(sf, theta), v_turned)), ("target", in_space(turned(tf, phi), sf, v))):
                err = np.abs(got - base)
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (seed, mode, label, float(err.max()))
            assert float(np.abs(base).max()) > 1
    print(f"gauge invariance of max and mean: largest change of the 3-D result {worst:.1e}")


# ---- why the pooling exists ---------------------------------------------------------------------------------------------------------
def test_on_a_subset_the_interpolation_is_a_gather_and_the_pooling_is_not():
    S = _subset_pair(600, 150, 16, 3)
    n, m, c = 600, 150, 8
    v = V.values(2 * n, c, 91)
    args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
    assert (S["idx"][:, 0] == S["keep"]).all() and not S["d2"][:, 0].any()       # the coincident fine point, at d2 = 0
    down = V.forward(v, *args, V.table(*args, S["tframes"], S["sframes"]))
    own = np.empty((2 * m, c), dtype=F32)
    own[0::2], own[1::2] = v[2 * S["keep"]], v[2 * S["keep"] + 1]
    assert np.array_equal(bits(down), bits(own))                                 # "interpolate" down: the other 15 contribute nothing
    rmat = P.table(S["idx"], S["qptr"], S["rptr"], S["tframes"], S["sframes"])
    for mode in (0, 3):
        out = P.forward(v, S["idx"], S["qptr"], S["rptr"], rmat, mode)[0]
        differs = (out != own).reshape(m, 2, c).any(axis=(1, 2))
        assert differs.mean() > 0.5, (mode, float(differs.mean()))


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
def test_a_query_without_a_valid_slot_and_nan_keys(hp):
    tf, sf = P._frames(3, 7), P._frames(4, 8)
    idx = np.array([[0, 1, 2, 3],                                               # later NaN key: never taken
                    [1, 0, 2, 3],                                               # first NaN key: stays
                    [-1, 9, 4, -5]], dtype=np.int32)                            # no valid slot
    qptr, rptr = np.array([0, 3]), np.array([0, 4])
    v = np.array([[1.0], [0.0], [np.nan], [0.0], [3.0], [0.0], [2.0], [0.0]], dtype=F32)
    rmat = P.table(idx, qptr, rptr, tf, sf)
    for out, arg, cnt in (P.forward(v, idx, qptr, rptr, rmat, 0), host_forward(hp, v, qptr, rptr, idx, rmat, 0)):
        assert arg[:, 0].tolist() == [2, 0, 255] and cnt.tolist() == [4, 4, 0]
        assert not np.isnan(out[0:2]).any() and np.isnan(out[2:4]).all() and not out[4:6].any()
    for mode in (2, 3):
        out, _, cnt = host_forward(hp, v, qptr, rptr, idx, rmat, mode)
        assert np.isnan(out[0:4]).all() and not out[4:6].any() and cnt.tolist() == [4, 4, 0]
        assert np.array_equal(bits(out), bits(P.forward(v, idx, qptr, rptr, rmat, mode)[0]))
    # an empty reference cloud: nothing is indexed (v has no row at all)
    for mode in P.MODE_CODES:
        out, arg, cnt = host_forward(hp, np.zeros((0, 5), dtype=F32), qptr, np.array([0, 0]), idx, np.zeros((12, 4), dtype=F32), mode)
        assert not out.any() and not cnt.any() and (mode >= 2 or (arg == 255).all())
