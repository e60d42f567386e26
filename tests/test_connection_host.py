"""Host side of the parallel-transport module (csrc/connection_math.h), without a GPU: a g++ build of the header
(tests/hostcheck_connection) against the numpy restatement (tests/connection_restate.py) bit for bit -- uint32 views, so -0.0
counts -- and the restatement against the reference's own fp64 output on the same inputs (tests/golden/connection.npz).

The connection.  The reference's fp32 evaluation and the restatement round differently (libm trig against two more
divisions); neither is privileged, so the yardstick is the reference's own fp32 error e_ref = max |ref32 - ref64| over the kept
cases of a set, computed here from the file, and the restatement must stay within 2 * e_ref.  (A frame seen from itself is the identity by
rule, connection_math.h: the reference's fp64 output differs from it by the frame's own tx . ty, 2.7e-08 at most on set (c).)  A case is left out only where
fp64 cannot decide a branch (|sn . tn| <= 1e-6, or the axis length or the projected length within a factor 2 of 1e-6); at most
1 % of a set.  The committed file gives (max |. - ref64|, reference fp32 / restatement, none of any set left out):

    (a) random pairs, both non_oriented    1.53e-07 / 1.73e-07
    (b) source normal 5 % off the target   1.21e-07 / 1.15e-07
    (c) the golden graph scene, 5 120 edges 1.41e-07 / 1.71e-07
    (d) rotate_around (g++ build)          9.20e-08 / 1.21e-07        angle_in_plane (g++ build)  1.77e-07 / 2.43e-07

The sums.  out[2i+a] = scale * acc_a is a sequential sum of 2k terms c * v.  A term passes through its product (one rounding),
at most 2k additions, the product with scale and, for the mean, the rounding of 1/k itself: (1 + d)^(2k+3) - 1 with |d| <= 2^-24,
to first order

    |out - out64| <= (2k + 3) * 2^-24 * |scale| * sum_s sum_b |coef_ab| |v_b|        (+ 1 when weights are folded in: coef = fl(w R))

and the same for the transpose with the in-list length L_j in place of k.  The second-order terms are below 2^-24 of the first
for every list here (L <= 301); the observed worst ratio is printed (forward 0.29, backward 0.34 of the bound)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import connection_restate as R
from tests.helpers import ROOT

HC_DIR = os.path.join(ROOT, "tests", "hostcheck_connection")
GOLDEN = os.path.join(ROOT, "tests", "golden")
P = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
F32, F64 = np.float32, np.float64
NAMES = ("tn", "tx", "ty", "sn", "sx")
IDENTITY = np.array([1, 0, 0, 1], dtype=F32)


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-s", "-C", HC_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HC_DIR, "libhostcheck_connection.so"))
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.hc_build_transport.argtypes, lib.hc_build_transport.restype = [vp] * 6 + [i32, i64, i32, vp], None
    lib.hc_angle_in_plane.argtypes, lib.hc_angle_in_plane.restype = [vp, vp, vp, i64, vp], None
    lib.hc_rotate_around.argtypes, lib.hc_rotate_around.restype = [vp, vp, vp, i64, vp], None
    lib.hc_transport_sum.argtypes, lib.hc_transport_sum.restype = [vp, i32, i32, vp, vp, i32, i64, f32, i32, vp, i64], None
    lib.hc_transport_sum_backward.argtypes = [vp, vp, i32, i32, vp, vp, i32, i64, f32, i32, vp, i64, i32]
    lib.hc_transport_sum_backward.restype = None
    return lib


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "connection.npz"))


@pytest.fixture(scope="module")
def scene():
    s = np.load(os.path.join(GOLDEN, "geom_normals_B2_N128_k20.npz"))
    n = s["normal_f32"].shape[0]
    row, col = s["edge_index"]
    k = len(row) // n
    assert np.array_equal(row, np.repeat(np.arange(n), k))
    return s["normal_f32"], s["x_basis_f32"], s["y_basis_f32"], col.reshape(n, k).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def host_transport(hc, tn, tx, ty, sn, sx, non_oriented=True, nbr=None):
    arrs = [np.ascontiguousarray(a, dtype=F32) for a in (tn, tx, ty, sn, sx)]
    m = arrs[0].shape[0] if nbr is None else nbr.size
    out = np.full((m + 2, 4), -7, dtype=F32)
    nbr = None if nbr is None else np.ascontiguousarray(nbr, dtype=np.int32)
    hc.hc_build_transport(*[P(a) for a in arrs], P(nbr), 1 if nbr is None else nbr.shape[1], m, int(non_oriented), P(out))
    assert (out[m:] == -7).all()
    return out[:m].copy()


def golden_sets(gold, scene):
    """-> [(label, the five inputs, non_oriented, ref32, ref64)]"""
    sets = []
    for tag, flags in (("a", "TF"), ("b", "T")):
        ins = [gold[f"{tag}_{n}"] for n in NAMES]
        sets += [(f"{tag}/{f}", ins, f == "T", gold[f"{tag}_out32_{f}"], gold[f"{tag}_out64_{f}"]) for f in flags]
    nrm, xb, yb, nbr = scene
    t, s = np.repeat(np.arange(nbr.shape[0]), nbr.shape[1]), nbr.reshape(-1)
    sets.append(("c", [nrm[t], xb[t], yb[t], nrm[s], xb[s]], True, gold["c_out32"], gold["c_out64"]))
    return sets


def kept_cases(ins, non_oriented):
    """the cases fp64 decides: not |sn . tn| <= 1e-6, axis length and projected length not within a factor 2 of 1e-6"""
    _, (d, an, l) = R.transport(*ins, non_oriented, dtype=F64, details=True)
    near = lambda x: (x > 0.5e-6) & (x < 2e-6)
    return ~((np.abs(d) <= 1e-6) | near(an) | near(l))


# ---- the g++ build of connection_math.h = the restatement, bit for bit --------------------------------------------------------
def test_hostcheck_transport_equals_the_restatement_bitwise(hc, gold, scene):
    for label, ins, flag, _, _ in golden_sets(gold, scene):
        assert np.array_equal(bits(host_transport(hc, *ins, flag)), bits(R.transport(*ins, flag))), label
    nrm, xb, yb, nbr = scene                                                   # the graph form = the pair form on expanded rows
    for flag in (True, False):
        got = host_transport(hc, nrm, xb, yb, nrm, xb, flag, nbr=nbr)
        assert np.array_equal(bits(got), bits(R.graph_transport(nrm, xb, yb, nbr, flag)))
    for seed in (1, 2):                                                          # normals apart, reflected frames, tiny inputs
        tn, tx, ty, sn, sx = R.random_pairs(1025, seed)
        for ins in ((tn, tx, ty, -tn, tx), (tn, tx, -ty, sn, sx), (tn, tx, ty, tn, sx), (tn * F32(1e-7), tx, ty, sn, sx),
                    (tn, tx * F32(1e-9), ty * F32(1e-9), sn, sx * F32(1e-9))):
            for flag in (True, False):
                assert np.array_equal(bits(host_transport(hc, *ins, flag)), bits(R.transport(*ins, flag)))


# ---- the restatement against the reference's fp64 output ----------------------------------------------------------------------
def test_restatement_is_within_twice_the_reference_fp32_error(gold, scene):
    for label, ins, flag, ref32, ref64 in golden_sets(gold, scene):
        keep = kept_cases(ins, flag)
        assert (~keep).sum() <= 0.01 * len(keep), (label, int((~keep).sum()))
        e_ref = float(np.abs(ref32.astype(F64) - ref64)[keep].max())
        e_own = float(np.abs(R.transport(*ins, flag).astype(F64) - ref64)[keep].max())
        own = (ins[3] == ins[0]).all(axis=1) & (ins[4] == ins[1]).all(axis=1)   # a frame seen from itself: the identity by rule
        same64 = float(np.abs(R.transport(*ins, flag, dtype=F64) - ref64)[keep & ~own].max())
        print(f"{label}: left out {int((~keep).sum())} of {len(keep)}; |ref32 - ref64| {e_ref:.3e}, |restatement - ref64| {e_own:.3e}, "
              f"fp64 restatement - ref64 {same64:.1e}")
        assert 0 < e_ref < 1e-6 and e_own <= 2 * e_ref, label
        assert same64 < 1e-12, label                                            # the formulas ARE the reference's, in fp64


def test_helpers_are_within_twice_the_reference_fp32_error(hc, gold):
    v, axis, angle = (np.ascontiguousarray(gold[f"d_rot_{n}"]) for n in ("v", "axis", "angle"))
    got = np.full((len(v) + 1, 3), -7, dtype=F32)
    hc.hc_rotate_around(P(v), P(axis), P(angle), len(v), P(got))
    assert (got[-1] == -7).all()
    e_ref = float(np.abs(gold["d_rot_out32"].astype(F64) - gold["d_rot_out64"]).max())
    e_own = float(np.abs(got[:-1].astype(F64) - gold["d_rot_out64"]).max())
    print(f"rotate_around: |ref32 - ref64| {e_ref:.3e}, |g++ - ref64| {e_own:.3e}")
    assert 0 < e_ref < 1e-6 and e_own <= 2 * e_ref
    assert np.abs(R.rotate_around(v, axis, angle) - gold["d_rot_out64"]).max() < 1e-12
    u, w, normal = (np.ascontiguousarray(gold[f"d_ang_{n}"]) for n in ("u", "v", "normal"))
    got = np.full(len(u) + 1, -7, dtype=F32)
    hc.hc_angle_in_plane(P(u), P(w), P(normal), len(u), P(got))
    assert got[-1] == -7
    ref64 = gold["d_ang_out64"].reshape(-1)
    e_ref = float(np.abs(gold["d_ang_out32"].reshape(-1).astype(F64) - ref64).max())
    e_own = float(np.abs(got[:-1].astype(F64) - ref64).max())
    print(f"angle_in_plane: |ref32 - ref64| {e_ref:.3e}, |g++ - ref64| {e_own:.3e}")
    assert 0 < e_ref < 1e-5 and e_own <= 2 * e_ref
    assert np.abs(R.angle_in_plane(u, w, normal) - ref64).max() < 1e-12
    assert np.abs(ref64 - gold["d_ang_angle"].reshape(-1)).max() < 1e-5         # and the angle the inputs were built from


# ---- edge cases with exact expectations ---------------------------------------------------------------------------------------
def test_a_frame_seen_from_itself_is_the_identity(hc, gold, scene):
    tn, tx, ty, _, _ = R.random_pairs(1025, 5)
    for flag in (True, False):
        for out in (R.transport(tn, tx, ty, tn, tx, flag), host_transport(hc, tn, tx, ty, tn, tx, flag)):
            assert (out == IDENTITY).all()
    nrm, xb, yb, nbr = scene
    own = nbr == np.arange(nbr.shape[0])[:, None]
    assert own.sum() == nbr.shape[0]                                            # every point of the scene is its own neighbour once
    for out in (R.graph_transport(nrm, xb, yb, nbr), host_transport(hc, nrm, xb, yb, nrm, xb, nbr=nbr)):
        assert (out[own.reshape(-1)] == IDENTITY).all()
    # the reference's fp32 output is the identity there only up to the frames' own orthogonality
    assert np.abs(gold["c_out32"][own.reshape(-1)] - IDENTITY).max() < 1e-7


def test_equal_normals_give_the_in_plane_rotation(hc, gold):
    e_ref = float(np.abs(gold["a_out32_T"].astype(F64) - gold["a_out64_T"]).max())
    tn, tx, ty, _, _ = R.random_pairs(1025, 6)
    phi = np.random.default_rng(6).uniform(-np.pi, np.pi, len(tn))
    sx = (np.cos(phi)[:, None] * tx.astype(F64) + np.sin(phi)[:, None] * ty.astype(F64)).astype(F32)
    want = np.stack([np.cos(phi), -np.sin(phi), np.sin(phi), np.cos(phi)], axis=1)
    for out in (R.transport(tn, tx, ty, tn, sx), host_transport(hc, tn, tx, ty, tn, sx)):
        err = float(np.abs(out.astype(F64) - want).max())
        print(f"in-plane rotation: max error {err:.3e}, allowed {2 * e_ref:.3e}")
        assert err <= 2 * e_ref


def test_opposite_normals_reflect_or_rotate(hc):
    tn, tx, ty, _, sx = R.random_pairs(1025, 7)
    ulp = 2.0 ** -23
    for flag, det in ((True, -1.0), (False, 1.0)):
        for out in (R.transport(tn, tx, ty, -tn, sx, flag), host_transport(hc, tn, tx, ty, -tn, sx, flag)):
            m = out.astype(F64).reshape(-1, 2, 2)
            assert np.abs(m @ m.transpose(0, 2, 1) - np.eye(2)).max() <= 4 * ulp
            assert np.abs(np.linalg.det(m) - det).max() <= 4 * ulp


def test_zero_inputs_are_finite_and_fall_back(hc):
    z = np.zeros((3, 3), dtype=F32)
    e = np.tile(np.array([[1, 0, 0]], dtype=F32), (3, 1))
    want = np.tile(np.array([[1, -0.0, 0, 1]], dtype=F32), (3, 1))
    for ins in ((z, z, z, z, z), (z, e, z, z, z), (z, z, z, z, e), (z, z, e, e, z)):    # the frame rule, and the clamps of the steps
        for flag in (True, False):
            for out in (R.transport(*ins, flag), host_transport(hc, *ins, flag)):
                assert np.isfinite(out).all() and np.array_equal(bits(out), bits(want)), (ins, out)


# ---- the sums ----------------------------------------------------------------------------------------------------------------------
def knn(pos, k):
    d = ((pos[:, None, :].astype(F64) - pos[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k].astype(np.int32)


def graphs(scene):
    out = []
    for n, seed in ((37, 21), (300, 22)):
        pos, nrm, xb, yb = R.cloud(n, seed)
        out += [(f"knn{n}k{k}", nrm, xb, yb, knn(pos, k)) for k in (5, 20)]
    _, nrm, xb, yb = R.cloud(300, 23)
    out.append(("hand", nrm, xb, yb, R.hand_table()))
    out.append(("scene",) + tuple(scene))
    return out


def laid_out(a, vec, fill=np.nan):
    """a [rows,C] inside a buffer with a leading dimension above C: 16-byte aligned rows (vec) or an odd leading dimension"""
    rows, c = a.shape
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    raw = np.full(rows * ld + 8, fill, dtype=F32)
    off = (-(raw.ctypes.data // 4)) % 4 if vec else 0
    wide = raw[off:off + rows * ld].reshape(rows, ld)
    wide[:, :c] = a
    return wide, ld


@pytest.mark.parametrize("c", [1, 3, 64, 65])
def test_hostcheck_sums_equal_the_restatement_bitwise(hc, scene, c):
    rng = np.random.default_rng(30 + c)
    for label, nrm, xb, yb, nbr in graphs(scene):
        n, k = nbr.shape
        conn = R.graph_transport(nrm, xb, yb, nbr)
        w = rng.random(n * k, dtype=F32)
        v, g = rng.standard_normal((2 * n, c)).astype(F32), rng.standard_normal((2 * n, c)).astype(F32)
        tptr, tedge = R.csc(nbr)
        assert tptr[-1] == n * k and all((np.diff(tedge[tptr[j]:tptr[j + 1]]) > 0).all() for j in range(n))
        for coef, scale in ((conn, 1.0), (R.fold_weights(conn, w), F32(1.0 / k))):
            want, want_b = R.transport_sum(v, coef, nbr, scale), R.transport_sum_backward(g, coef, nbr, scale)
            for vec in ((True, False) if c % 4 == 0 else (False,)):
                vin, ldv = laid_out(v, vec)
                out, ldo = laid_out(np.full((2 * n, c), -7, dtype=F32), vec)
                hc.hc_transport_sum(P(nbr), n, k, P(coef), P(vin), c, ldv, float(scale), int(vec), P(out), ldo)
                assert np.array_equal(bits(out[:, :c]), bits(want)) and np.isnan(out[:, c:]).all(), (label, c, vec)
                gin, ldg = laid_out(g, vec)
                dv, ldd = laid_out(np.full((2 * n, c), -7, dtype=F32), vec)
                hc.hc_transport_sum_backward(P(tptr), P(tedge), n, k, P(coef), P(gin), c, ldg, float(scale), int(vec), P(dv), ldd, 0)
                assert np.array_equal(bits(dv[:, :c]), bits(want_b)) and np.isnan(dv[:, c:]).all(), (label, c, vec)
                dv[:, :c] = v                                                   # accumulate = 1 adds onto what is there
                hc.hc_transport_sum_backward(P(tptr), P(tedge), n, k, P(coef), P(gin), c, ldg, float(scale), int(vec), P(dv), ldd, 1)
                assert np.array_equal(bits(dv[:, :c]), bits(R.transport_sum_backward(g, coef, nbr, scale, into=v)))


def test_the_hand_table_has_one_long_list_and_a_point_with_its_self_edge_only():
    nbr = R.hand_table()
    deg = np.diff(R.csc(nbr)[0])
    assert deg[0] >= 300 and deg[-1] == 1 and (nbr[:, 0] == np.arange(300)).all()
    g = np.ones((600, 2), dtype=F32)
    coef = np.tile(IDENTITY, (nbr.size, 1))
    dv = R.transport_sum_backward(g, coef, nbr)
    assert (dv[0] == deg[0]).all() and (dv[-1] == 1).all() and (dv[-2] == 1).all()


def test_sum_restatements_are_within_the_fp64_bound(scene):
    rng = np.random.default_rng(40)
    worst_f = worst_b = 0.0
    for label, nrm, xb, yb, nbr in graphs(scene):
        n, k = nbr.shape
        conn = R.graph_transport(nrm, xb, yb, nbr)
        w = rng.random(n * k, dtype=F32)
        v, g = (rng.standard_normal((2 * n, 7)) * 10).astype(F32), (rng.standard_normal((2 * n, 7)) * 10).astype(F32)
        for weights, reduce in ((None, "sum"), (w, "mean"), (w, "sum")):
            coef, extra = R.fold_weights(conn, weights), 0 if weights is None else 1
            coef64 = conn.astype(F64) if weights is None else w.astype(F64)[:, None] * conn.astype(F64)
            s32, s64 = (F32(1.0 / k), 1.0 / k) if reduce == "mean" else (1.0, 1.0)
            err = np.abs(R.transport_sum(v, coef, nbr, s32).astype(F64) - R.transport_sum(v, coef64, nbr, s64, F64))
            bound = R.sum_bound(v, coef64, nbr, s64, extra)
            assert (err <= bound).all(), (label, reduce, float((err - bound).max()))
            worst_f = max(worst_f, float((err[bound > 0] / bound[bound > 0]).max()))
            err = np.abs(R.transport_sum_backward(g, coef, nbr, s32).astype(F64) - R.transport_sum_backward(g, coef64, nbr, s64, F64))
            bound = R.backward_bound(g, coef64, nbr, s64, extra)
            assert (err <= bound).all(), (label, reduce, float((err - bound).max()))
            worst_b = max(worst_b, float((err[bound > 0] / bound[bound > 0]).max()))
    print(f"worst |out - out64| / bound: forward {worst_f:.3f}, backward {worst_b:.3f}")


def test_the_two_fp64_forms_are_adjoint(scene):
    rng = np.random.default_rng(41)
    for label, nrm, xb, yb, nbr in graphs(scene):
        n, k = nbr.shape
        coef = rng.random(n * k)[:, None] * R.graph_transport(nrm, xb, yb, nbr, dtype=F64)
        v, g = rng.standard_normal((2 * n, 5)), rng.standard_normal((2 * n, 5))
        lhs = float((R.transport_sum(v, coef, nbr, 1.0 / k, F64) * g).sum())
        rhs = float((v * R.transport_sum_backward(g, coef, nbr, 1.0 / k, F64)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (label, lhs, rhs)
