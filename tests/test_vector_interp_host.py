"""Host side of the transported interpolation of tangent-vector features (csrc/interp_transport_math.h), without a GPU: a g++
build of the header (tests/hostcheck_vector_interp) against the numpy restatement (tests/vector_interp_restate.py) bit for bit
-- uint32 views, so -0.0 counts -- and the restatement against fp64.

The bounds are derived, not tuned (d = 2^-24, c64 the fp64 coefficients, R32 the fp32 restatement's connection promoted):

    table      |M - c64 R32| <= (k + 3) d |c64 R32|: k roundings in den, the weight, the division, the product
    forward    |out - sum c64 R32 v| <= (3k + 4) d sum_s sum_b |c64 R32_ab| |v_b|: the table's k + 3, one product, up to 2k additions
    backward   against the fp64 sum with the fp32 table promoted: (2L + 1) d sum |M| |g|, L the list length

Against the reference: the fp64 yardstick is connection_restate.transport(dtype=float64), which tests/test_connection_host.py
holds to the real reference's fp64 output in tests/golden/connection.npz; out64 = sum c64 R64 v.  The fp32 restatement stays within
the forward bound plus E_R sum_s c64_s (|v0| + |v1|), E_R = 2 e_ref with e_ref the reference's own fp32 error read from that file
as that test computes it (the allowance the restatement already has there).  Slots where fp64 cannot decide a branch are left
out by the kept_cases rule of that test; at most 1 % of a set.  The worst ratios are printed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import connection_restate as CR
from tests import test_connection_host as TC
from tests import vector_interp_restate as V
from tests.helpers import ROOT

HC_DIR = os.path.join(ROOT, "tests", "hostcheck_vector_interp")
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
F32, F64 = np.float32, np.float64
EPS = V.EPS
CHANNELS = (1, 3, 4, 5)


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-s", "-C", HC_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HC_DIR, "libhostcheck_vector_interp.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hv_table.argtypes, lib.hv_table.restype = [vp, vp, i32, i64, i32] + [vp] * 7 + [i32, vp], None
    lib.hv_forward.argtypes, lib.hv_forward.restype = [vp, i64, i32, vp, vp, i32, i32, vp, vp, i32, vp, i64], None
    lib.hv_backward.argtypes, lib.hv_backward.restype = [vp, i64, i64, i32, vp, i32, i32, vp, vp, i64, vp, i64, i32, vp, i64], None
    return lib


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def cases():
    """-> [(label, set dict, non_oriented)]: the four input sets and the edge cases of the issue."""
    out = [(f"set{s[0]}", V.input_set(*s), True) for s in V.SETS]
    apart = dict(V.input_set(*V.SETS[0]))
    sn, sx, sy = apart["sframes"]
    flip = (np.arange(len(sn)) % 2 == 0)[:, None]
    apart["sframes"] = (np.where(flip, -sn, sn), sx, sy)                        # normals pointing apart for half the sources
    out += [("apart/T", apart, True), ("apart/F", apart, False), ("set2/F", V.input_set(*V.SETS[1]), False)]
    out += [(name, V.batch_set(name), True) for name in V.BATCHES]              # fewer than k sources; an empty query cloud
    outside = dict(V.input_set(*V.SETS[3]))
    outside["qptr"] = np.array([5, 500], dtype=np.int64)                        # query rows 0 .. 4 and 500 .. 512 lie in no pair
    out.append(("outside", outside, True))
    out.append(("hub", V.hub_set(), True))                                     # in-lists of 14 entries and of none
    return out


CASES = cases()


def host_table(hc, S, flag):
    nq, k = S["idx"].shape
    tmat = np.full((nq * k + 1, 4), -7, dtype=F32)
    fr = [np.ascontiguousarray(a, dtype=F32) for a in S["tframes"] + S["sframes"][:2]]
    hc.hv_table(P(S["qptr"]), P(S["rptr"]), len(S["qptr"]) - 1, nq, k, P(S["idx"]), P(S["d2"]), *[P(a) for a in fr], int(flag),
                P(tmat))
    assert (tmat[-1] == -7).all()
    return tmat[:-1].copy()


def in_pairs(ptr, n):
    mask = np.zeros(n, dtype=bool)
    for b in range(len(ptr) - 1):
        mask[int(ptr[b]):int(ptr[b + 1])] = True
    return mask


# ---- 1. the g++ build of interp_transport_math.h = the restatement, bit for bit ------------------------------------------------
@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_hostcheck_equals_the_restatement_bitwise(hc, case):
    label, S, flag = CASES[case]
    nq, k = S["idx"].shape
    nr = len(S["pos_s"])
    want_m = V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], S["tframes"], S["sframes"], flag)
    tmat = host_table(hc, S, flag)
    assert np.array_equal(bits(tmat), bits(want_m)), label
    _, ok, _ = V.slots(S["idx"], S["d2"], S["qptr"], S["rptr"])
    assert not bits(want_m.reshape(nq, k, 4)[~ok]).any()                        # invalid slots and rows in no pair: four +0.0f
    tptr, tedge = V.lists(S["idx"], S["d2"], S["qptr"], S["rptr"], nr)
    qin, rin = np.repeat(in_pairs(S["qptr"], nq), 2), np.repeat(in_pairs(S["rptr"], nr), 2)
    b = len(S["qptr"]) - 1
    for c in CHANNELS:
        v, g = V.values(2 * nr, c, 10 + c), V.values(2 * nq, c, 20 + c)
        want_f = V.forward(v, S["idx"], S["d2"], S["qptr"], S["rptr"], want_m)
        want_b = V.backward(g, tptr, tedge, want_m, k)
        for vec in (True, False):              # strided rows either way (ld > C); vec with C = 5: a whole group beside a partial one
            vin, ldv = TC.laid_out(v, vec)
            out, ldo = TC.laid_out(np.full((2 * nq, c), np.nan, dtype=F32), vec)
            hc.hv_forward(P(vin), ldv, c, P(S["qptr"]), P(S["rptr"]), b, k, P(S["idx"]), P(tmat), int(vec), P(out), ldo)
            assert np.array_equal(bits(out[qin, :c]), bits(want_f[qin])) and np.isnan(out[:, c:]).all(), (label, c, vec)
            assert np.isnan(out[~qin, :c]).all() and not want_f[~qin].any()     # rows in no pair: not written / zeros
            gin, ldg = TC.laid_out(g, vec)
            dv, ldd = TC.laid_out(np.full((2 * nr, c), np.nan, dtype=F32), vec)
            hc.hv_backward(P(gin), ldg, nq, c, P(S["rptr"]), b, k, P(tptr), P(tedge), 0, P(tmat), nq * k, int(vec), P(dv), ldd)
            assert np.array_equal(bits(dv[rin, :c]), bits(want_b[rin])) and np.isnan(dv[:, c:]).all(), (label, c, vec)


def test_a_range_of_pairs_runs_against_the_lists_of_the_whole_call(hc):
    """edge_base != 0: pairs 1 .. 2 of the three-pair batch with their own rows of g and their slice of the table."""
    S = V.batch_set("three_pairs")
    k, c = S["k"], 5
    nq, nr = len(S["pos_t"]), len(S["pos_s"])
    M = V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], S["tframes"], S["sframes"])
    tptr, tedge = V.lists(S["idx"], S["d2"], S["qptr"], S["rptr"], nr)
    g = V.values(2 * nq, c, 3)
    whole = V.backward(g, tptr, tedge, M, k)
    q0, r0 = int(S["qptr"][1]), int(S["rptr"][1])
    part = V.backward(g[2 * q0:], tptr[r0:], tedge, M[q0 * k:], k, edge_base=q0)
    assert np.array_equal(bits(part), bits(whole[2 * r0:]))
    rel = np.ascontiguousarray(S["rptr"][1:] - r0)
    dv = np.full((2 * (nr - r0), c), np.nan, dtype=F32)
    gp, mp, tp = np.ascontiguousarray(g[2 * q0:]), np.ascontiguousarray(M[q0 * k:]), np.ascontiguousarray(tptr[r0:])
    hc.hv_backward(P(gp), c, nq - q0, c, P(rel), 2, k, P(tp), P(tedge), q0, P(mp), (nq - q0) * k, 0, P(dv), c)
    assert np.array_equal(bits(dv), bits(whole[2 * r0:]))


# ---- 2. rounding bounds -----------------------------------------------------------------------------------------------------------
def fp64_pieces(S, flag=True):
    """-> (c64 [Nq,k], R32 promoted [Nq,k,4], ok, src)"""
    c64, ok, src = V.slots(S["idx"], S["d2"], S["qptr"], S["rptr"], F64)
    R32 = V.connection(ok, src, S["tframes"], S["sframes"], flag, F32).astype(F64)
    return c64, R32, ok, src


def test_table_and_sums_are_within_the_derived_bounds():
    worst = dict(table=0.0, forward=0.0, backward=0.0)
    for spec in V.SETS:
        S = V.input_set(*spec)
        nq, k = S["idx"].shape
        nr = len(S["pos_s"])
        c64, R32, ok, _ = fp64_pieces(S)
        exact = c64[:, :, None] * R32
        M = V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], S["tframes"], S["sframes"])
        err, bound = np.abs(M.reshape(nq, k, 4).astype(F64) - exact), (k + 3) * EPS * np.abs(exact)
        assert (err <= bound).all(), (spec, float((err - bound).max()))
        worst["table"] = max(worst["table"], float((err[bound > 0] / bound[bound > 0]).max()))
        v, g = V.values(2 * nr, 7, spec[0]), V.values(2 * nq, 7, 50 + spec[0])
        args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
        err = np.abs(V.forward(v, *args, M).astype(F64) - V.forward(v, *args, exact.reshape(-1, 4), F64))
        bound = (3 * k + 4) * EPS * V.forward(np.abs(v), *args, np.abs(exact).reshape(-1, 4), F64)
        assert (err <= bound).all(), (spec, float((err - bound).max()))
        worst["forward"] = max(worst["forward"], float((err[bound > 0] / bound[bound > 0]).max()))
        tptr, tedge = V.lists(*args, nr)
        L = np.repeat(np.diff(tptr), 2).astype(F64)[:, None]
        err = np.abs(V.backward(g, tptr, tedge, M, k).astype(F64) - V.backward(g, tptr, tedge, M.astype(F64), k, dtype=F64))
        bound = (2 * L + 1) * EPS * V.backward(np.abs(g), tptr, tedge, np.abs(M.astype(F64)), k, dtype=F64)
        assert (err <= bound).all(), (spec, float((err - bound).max()))
        worst["backward"] = max(worst["backward"], float((err[bound > 0] / bound[bound > 0]).max()))
    print("worst error / bound: " + ", ".join(f"{name} {r:.3f}" for name, r in worst.items()))


# ---- 3. against the reference ----------------------------------------------------------------------------------------------------
def reference_fp32_error():
    """e_ref: the reference's own fp32 error max |ref32 - ref64| over the kept cases of the pair sets of tests/golden/connection.npz,
    as tests/test_connection_host.py computes it."""
    gold = np.load(os.path.join(TC.GOLDEN, "connection.npz"))
    e_ref = 0.0
    for tag, flags in (("a", "TF"), ("b", "T")):
        ins = [gold[f"{tag}_{n}"] for n in TC.NAMES]
        for f in flags:
            keep = TC.kept_cases(ins, f == "T")
            e_ref = max(e_ref, float(np.abs(gold[f"{tag}_out32_{f}"].astype(F64) - gold[f"{tag}_out64_{f}"])[keep].max()))
    return e_ref


def test_restatement_is_within_the_reference_allowance_of_the_fp64_composition():
    E_R = 2 * reference_fp32_error()
    assert 0 < E_R < 2e-6
    for spec in V.SETS:
        S = V.input_set(*spec)
        nq, k = S["idx"].shape
        nr = len(S["pos_s"])
        c64, R32, ok, src = fp64_pieces(S)
        R64, (d, an, l), (q, s) = V.connection(ok, src, S["tframes"], S["sframes"], True, F64, details=True)
        near = lambda x: (x > 0.5e-6) & (x < 2e-6)
        undecided = np.zeros(ok.shape, dtype=bool)
        undecided[q, s] = (np.abs(d) <= 1e-6) | near(an) | near(l)              # the kept_cases rule, slot by slot
        keep = ~undecided.any(axis=1)
        assert (~keep).sum() <= 0.01 * nq, (spec, int((~keep).sum()))
        own = float(np.abs(R32 - R64)[keep].max())
        args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
        v = V.values(2 * nr, 7, spec[0])
        M = V.table(*args, S["tframes"], S["sframes"])
        out64 = V.forward(v, *args, (c64[:, :, None] * R64).reshape(-1, 4), F64)
        rounding = (3 * k + 4) * EPS * V.forward(np.abs(v), *args, np.abs(c64[:, :, None] * R32).reshape(-1, 4), F64)
        ones = np.ones((nq, k, 4)) * c64[:, :, None]
        allowance = E_R * V.forward(np.abs(v), *args, ones.reshape(-1, 4), F64)   # E_R sum_s c64_s (|v0| + |v1|), both rows
        err, bound = np.abs(V.forward(v, *args, M).astype(F64) - out64), rounding + allowance
        rows = np.repeat(keep, 2)
        print(f"set {spec}: left out {int((~keep).sum())} of {nq}; max |R32 - R64| {own:.2e}, E_R {E_R:.2e}; worst error / bound "
              f"{float((err[rows] / bound[rows]).max()):.3f}")
        assert (err[rows] <= bound[rows]).all(), (spec, float((err - bound)[rows].max()))


# ---- 4. gauge invariance: the property the feature exists for ----------------------------------------------------------------------
def orthonormal64(frames):
    n, x = (np.asarray(a, dtype=F64) for a in frames[:2])
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    x = x - n * (x * n).sum(1, keepdims=True)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return n, x, np.cross(n, x)


def turned(frames, theta):
    n, x, y = frames
    c, s = np.cos(theta)[:, None], np.sin(theta)[:, None]
    return n, c * x + s * y, -s * x + c * y


def test_the_result_does_not_depend_on_the_choice_of_frames():
    worst = 0.0
    for spec in V.SETS:
        S = V.input_set(*spec)
        nq, k = S["idx"].shape
        nr = len(S["pos_s"])
        rng = np.random.default_rng(60 + spec[0])
        tf, sf = orthonormal64(S["tframes"]), orthonormal64(S["sframes"])
        v = rng.standard_normal((2 * nr, 3)) * 3
        args = (S["idx"], S["d2"], S["qptr"], S["rptr"])

        def in_space(tframes, sframes, vals):
            out = V.forward(vals, *args, V.table(*args, tframes, sframes, True, F64), F64)
            return out[0::2, None, :] * tframes[1][:, :, None] + out[1::2, None, :] * tframes[2][:, :, None]    # [Nq, 3, C]

        base = in_space(tf, sf, v)
        c64, ok, src = V.slots(*args, F64)
        size = np.sqrt(v[0::2] ** 2 + v[1::2] ** 2)                             # |v_s| per source point and channel
        tol = 2.0 ** -40 * (c64[:, :, None] * size[src] * ok[:, :, None]).sum(axis=1)[:, None, :]
        theta = rng.uniform(-np.pi, np.pi, nr)                                  # every source frame turned about its normal
        cs, sn = np.cos(theta)[:, None], np.sin(theta)[:, None]
        v_turned = np.empty_like(v)
        v_turned[0::2], v_turned[1::2] = cs * v[0::2] + sn * v[1::2], -sn * v[0::2] + cs * v[1::2]
        phi = rng.uniform(-np.pi, np.pi, nq)                                    # separately, every target frame
        for label, got in (("source", in_space(tf, turned(sf, theta), v_turned)), ("target", in_space(turned(tf, phi), sf, v))):
            err = np.abs(got - base)
            worst = max(worst, float(err.max()))
            assert (err <= tol).all(), (spec, label, float(err.max()))
        assert float(np.abs(base).max()) > 1
    print(f"gauge invariance: largest change of the 3-D result {worst:.1e}")


# ---- 5. exact copy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(3, 700, 700, 1), (1, 2048, 256, 1)])
def test_k1_on_shared_frames_copies_the_source_vector_exactly(hc, spec):
    S = V.input_set(*spec)
    nq, nr, c = len(S["pos_t"]), len(S["pos_s"]), 5
    v = V.values(2 * nr, c, 77)
    args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
    M = V.table(*args, S["tframes"], S["sframes"])
    tmat = host_table(hc, S, True)
    out = np.full((2 * nq, c), np.nan, dtype=F32)
    hc.hv_forward(P(v), c, c, P(S["qptr"]), P(S["rptr"]), 1, 1, P(S["idx"]), P(tmat), 0, P(out), c)
    keep = S["keep"]                                                            # target row keep[i] IS source point i
    assert (S["idx"][keep, 0] == np.arange(nr)).all()
    for got in (V.forward(v, *args, M), out):
        assert (got[2 * keep] == v[0::2]).all() and (got[2 * keep + 1] == v[1::2]).all()
