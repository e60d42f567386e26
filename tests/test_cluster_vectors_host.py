"""Host side of the vector pooling over cluster cells (csrc/cluster_vectors_math.h), without a GPU: a g++ build of the header with
serial drivers (tests/hostcheck_cluster_vectors) equals the numpy restatement (tests/cluster_vectors_restate.py) BIT FOR BIT on
every case of tests/cluster_vectors_cases.py -- both tables, out, arg, both backwards, the un-pooling and its backward; the
restatement lies inside the bounds the header derives against the same formulas in fp64; the maximum selects what fp64 selects
outside the derived margin; the search form of tests/pool_vectors_restate.py gives the same bits on cells of at most 16 members;
and the properties the op promises.  Run with ``-s`` to see the worst observed fraction of every bound (the table of DESIGN.md
section 3.4r)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import cluster_vectors_cases as C
from tests import cluster_vectors_restate as R
from tests import connection_restate as CR
from tests import pool_vectors_restate as PR
from tests.helpers import ROOT

HC_DIR = os.path.join(ROOT, "tests", "hostcheck_cluster_vectors")
F, F64 = np.float32, np.float64
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
bits = lambda a: np.ascontiguousarray(a).view(np.int32) if a.dtype == F else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-s", "-C", HC_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HC_DIR, "libhostcheck_cluster_vectors.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hcv_mode_ok.argtypes, lib.hcv_mode_ok.restype = [i32], i32
    lib.hcv_rotation.argtypes, lib.hcv_rotation.restype = [vp, i64, i64, vp, vp, vp, vp, vp, vp, i32, i32, vp], None
    lib.hcv_pool.argtypes, lib.hcv_pool.restype = [vp, i64, i64, i32, vp, vp, i64, vp, i32, vp, i64, vp, i64], None
    lib.hcv_pool_backward.argtypes, lib.hcv_pool_backward.restype = [vp, i64, i64, i32, vp, i64, vp, vp, vp, i64, i32, vp, i64], None
    lib.hcv_unpool.argtypes, lib.hcv_unpool.restype = [vp, i64, i64, i32, vp, i64, vp, vp, i64], None
    lib.hcv_unpool_backward.argtypes, lib.hcv_unpool_backward.restype = [vp, i64, i64, i32, vp, vp, i64, vp, vp, i64], None
    return lib


def ld_of(a):
    """The leading dimension of a [rows, C] fp32 array with unit stride along the channels."""
    assert a.ndim == 2 and (a.shape[1] == 1 or a.shape[0] == 0 or a.strides[1] == 4)
    return a.strides[0] // 4 if a.shape[0] > 1 else a.shape[1]


def aligned(rows, cols=4, fill=7.0):
    """A float32 [rows, cols] array whose data is 16-byte aligned (the tables are read 16 bytes at a time)."""
    raw = np.full(rows * cols + 4, fill, F)
    off = (-raw.ctypes.data % 16) // 4
    return raw[off:off + rows * cols].reshape(rows, cols)


def host_table(hc, c, direction):
    n = c["cluster"].size
    out = aligned(n)
    fr = [np.ascontiguousarray(a, dtype=F) for a in (*c["fine"], *c["coarse"])]
    hc.hcv_rotation(P(c["cluster"]), n, c["m"], *(P(a) for a in fr), 1 if direction == "down" else 0, int(c["non_oriented"]), P(out))
    return out


def as_table(r):
    out = aligned(r.shape[0])
    out[...] = r
    return out


def host_pool(hc, v, cptr, members, rmat, reduce):
    m, c = cptr.size - 1, v.shape[1]
    out, arg, rmat = np.full((2 * m, c), 7, F), np.full((m, c), -7, np.int32), as_table(rmat)      # (held: P keeps no reference)
    hc.hcv_pool(P(v), ld_of(v), v.shape[0] // 2, c, P(cptr), P(members), m, P(rmat), R.MODES[reduce], P(out), c,
                P(arg) if reduce == "max" else None, c)
    return out, (arg if reduce == "max" else None)


def host_pool_backward(hc, g, cluster, cptr, rmat, arg, reduce):
    dv, rmat = np.full((2 * cluster.size, g.shape[1]), 7, F), as_table(rmat)
    hc.hcv_pool_backward(P(g), ld_of(g), g.shape[0] // 2, g.shape[1], P(cluster), cluster.size, P(cptr), P(rmat), P(arg),
                         g.shape[1], R.MODES[reduce], P(dv), g.shape[1])
    return dv


def test_the_modes_are_declared_the_same_everywhere(hc):
    from deltaconv_amd.geometry import cluster_vectors as G
    from deltaconv_amd.geometry.pool_vectors import _MODES
    assert all(_MODES[k] == v and hc.hcv_mode_ok(v) for k, v in R.MODES.items()) and not hc.hcv_mode_ok(1) and not hc.hcv_mode_ok(4)
    assert set(G.__all__) >= {"cluster_rotation", "cluster_pool_vectors", "cluster_unpool_vectors", "ClusterPair"}
    from deltaconv_amd import geometry
    assert all(hasattr(geometry, name) for name in G.__all__)


@pytest.mark.parametrize("name", C.NAMES)
def test_host_tables_equal_the_restatement(hc, name):
    c, e = C.BY_NAME[name], C.expected(name)
    ok = R.CL.valid(c["cluster"], c["m"])
    for direction in ("down", "up"):
        got = host_table(hc, c, direction)
        assert same(np.ascontiguousarray(got), e["r" + direction]), direction
        assert (bits(np.ascontiguousarray(got[~ok])) == 0).all()                 # four +0.0f without a cell
        if ok.any():                                                             # orthogonal up to rounding, determinant +-1
            det = got[ok, 0].astype(F64) * got[ok, 3] - got[ok, 1].astype(F64) * got[ok, 2]
            assert np.allclose(np.abs(det), 1, atol=1e-5)


@pytest.mark.parametrize("reduce", C.REDUCES)
@pytest.mark.parametrize("name", C.NAMES)
def test_host_pool_and_its_backward_equal_the_restatement(hc, name, reduce):
    c, e = C.BY_NAME[name], C.expected(name)
    out, arg = host_pool(hc, c["v"], e["cptr"], e["members"], e["rdown"], reduce)
    assert same(out, e["out", reduce])
    assert (arg is None and e["arg", reduce] is None) or same(arg, e["arg", reduce])
    assert same(host_pool_backward(hc, c["g"], c["cluster"], e["cptr"], e["rdown"], arg, reduce), e["dv", reduce])
    empty = np.repeat(np.diff(e["cptr"]) == 0, 2)
    assert (bits(out[empty]) == 0).all() and (arg is None or (arg[empty[::2]] == -1).all())


@pytest.mark.parametrize("name", C.NAMES)
def test_host_unpool_and_its_backward_equal_the_restatement(hc, name):
    c, e = C.BY_NAME[name], C.expected(name)
    n, m, ch = c["cluster"].size, c["m"], c["g"].shape[1]
    up, rup = np.full((2 * n, ch), 7, F), as_table(e["rup"])
    hc.hcv_unpool(P(c["g"]), ld_of(c["g"]), m, ch, P(c["cluster"]), n, P(rup), P(up), ch)
    assert same(up, e["up"])
    dup = np.full((2 * m, ch), 7, F)
    hc.hcv_unpool_backward(P(c["v"]), ld_of(c["v"]), n, ch, P(e["cptr"]), P(e["members"]), m, P(rup), P(dup), ch)
    assert same(dup, e["dup"])
    assert (bits(up[np.repeat(~R.CL.valid(c["cluster"], m), 2)]) == 0).all()


def test_foreign_members_are_skipped_and_not_counted(hc):
    """Lists that do not belong: members outside [0, N) take no part, in the restatement and in the header alike."""
    c, e = C.BY_NAME["small_cells"], C.expected("small_cells")
    members = e["members"].copy()
    members[::5] = np.where(np.arange(members[::5].size) % 2 == 0, -3, c["cluster"].size + 2)
    for reduce in C.REDUCES:
        want, warg = R.pool(c["v"], e["cptr"], members, e["rdown"], reduce)
        out, arg = host_pool(hc, c["v"], e["cptr"], members, e["rdown"], reduce)
        assert same(out, want) and (arg is None or same(arg, warg))
    kept = np.array([np.sum((members[a:b] >= 0) & (members[a:b] < c["cluster"].size)) for a, b in zip(e["cptr"][:-1], e["cptr"][1:])])
    total = R.pool(np.ones_like(c["v"]), e["cptr"], members, np.tile(np.array([[1, 0, 0, 1]], F), (c["cluster"].size, 1)), "sum")[0]
    assert np.array_equal(total[0::2, 0], kept.astype(F))


def test_the_selection_rules_on_the_special_values():
    e = C.expected("special_max")
    out, arg = e["out", "max"], e["arg", "max"]
    assert arg[0].tolist() == [0, 0, 2, 1]          # equal norms: the lower row | a first NaN stays | a later NaN is never taken | inf
    assert np.isnan(out[0, 1]) and np.isinf(e["out", "max"][0:2, 3]).any()
    assert arg[1].tolist() == [4, 4, 4, 4]          # equal norms again, zero keys and equal keys: the lower row
    e = C.expected("ids_without_a_cell")
    c = C.BY_NAME["ids_without_a_cell"]
    assert all(e["cptr"][j] == e["cptr"][j + 1] for j in (5, 17, 49))
    assert (e["dv", "sum"][np.repeat(~R.CL.valid(c["cluster"], 50), 2)] == 0).all()


def test_members_whose_frame_is_the_cells_hold_the_identity():
    for name in ("one_row", "own_cell_5000", "ids_without_a_cell", "voxel_cells_64_of_2000", "voxel_lattice_faces_512"):
        c, e = C.BY_NAME[name], C.expected(name)
        same_frame = np.zeros(c["cluster"].size, bool)
        ok = R.CL.valid(c["cluster"], c["m"])
        cl = c["cluster"][ok]
        same_frame[ok] = (c["fine"][0][ok] == c["coarse"][0][cl]).all(1) & (c["fine"][1][ok] == c["coarse"][1][cl]).all(1)
        assert same_frame.sum() >= np.count_nonzero(np.diff(e["cptr"])) > 0, name
        ident = np.array([1, -0.0, 0, 1], F)
        for key in ("rdown", "rup"):
            assert (bits(e[key][same_frame]) == bits(ident)[None, :]).all(), (name, key)


@pytest.mark.parametrize("name", ["one_row", "own_cell_5000"])
def test_a_cell_of_one_member_with_a_coincident_frame_returns_that_members_vector(name):
    c, e = C.BY_NAME[name], C.expected(name)
    order = np.argsort(c["cluster"])                                              # the member of cell j
    want = np.empty_like(c["v"])
    want[0::2], want[1::2] = c["v"][0::2][order], c["v"][1::2][order]
    for reduce in C.REDUCES:
        assert np.array_equal(e["out", reduce], want), reduce
    assert np.array_equal(e["arg", "max"][:, 0], order.astype(np.int32))


# ---- the search form cross-checks the cluster form ------------------------------------------------------------------------------------
def test_enough_cases_have_small_cells():
    assert {"one_row", "own_cell_5000", "special_max", "small_cells", "small_cells_oriented", "voxel_lattice_faces_512"} <= set(C.SMALL)


@pytest.mark.parametrize("reduce", C.REDUCES)
@pytest.mark.parametrize("name", C.SMALL)
def test_cells_of_at_most_16_members_equal_the_search_form(name, reduce):
    c, e = C.BY_NAME[name], C.expected(name)
    n, m, k = c["cluster"].size, c["m"], 16
    cptr, members = e["cptr"], e["members"]
    idx = np.full((m, k), -1, np.int32)
    for j in range(m):
        idx[j, :cptr[j + 1] - cptr[j]] = members[cptr[j]:cptr[j + 1]]
    qptr, rptr = np.array([0, m]), np.array([0, n])
    rmat = PR.table(idx, qptr, rptr, c["coarse"], c["fine"], c["non_oriented"])   # slot-wise: target = the cell, source = the member
    out, slot, cnt = PR.forward(c["v"], idx, qptr, rptr, rmat, R.MODES[reduce])
    assert same(out, e["out", reduce])
    assert np.array_equal(cnt, np.diff(cptr).astype(np.uint8))
    if reduce == "max":
        rows = np.where(slot == PR.NO_ARG, -1, np.take_along_axis(idx, np.minimum(slot, k - 1).astype(np.int64), axis=1))
        assert np.array_equal(rows, e["arg", "max"])


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------------
WORST = {}
SLACK = 1 + 2.0 ** -20          # the fp64 yardstick's own roundings (2^-53 per operation) against bounds in units of 2^-24


def note(key, err, bound):
    """The worst err / bound of a check -> WORST, after asserting err <= bound everywhere."""
    assert (err <= bound * SLACK).all(), (key, float((err - bound).max()))
    frac = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), frac)


@pytest.mark.parametrize("name", C.FINITE)
def test_the_restatement_lies_inside_the_derived_bounds_of_fp64(name):
    c, e = C.BY_NAME[name], C.expected(name)
    v, g, cluster, cptr, members, rdown, rup = c["v"], c["g"], c["cluster"], e["cptr"], e["members"], e["rdown"], e["rup"]
    S, cnt = R.pool_magnitude(v, cptr, members, rdown)
    k = np.repeat(cnt, 2).astype(F64)[:, None]
    note("sum", np.abs(e["out", "sum"] - R.pool(v, cptr, members, rdown, "sum", F64)[0]), R.gamma(2 * k) * S)
    note("mean", np.abs(e["out", "mean"] - R.pool(v, cptr, members, rdown, "mean", F64)[0]), R.gamma(2 * k + 1) * S / np.maximum(k, 1))
    T = R.gather_magnitude(g, cluster, rdown, True)
    note("sum backward", np.abs(e["dv", "sum"] - R.pool_backward(g, cluster, cptr, rdown, None, "sum", F64)), R.gamma(2) * T)
    note("max backward", np.abs(e["dv", "max"] - R.pool_backward(g, cluster, cptr, rdown, e["arg", "max"], "max", F64)), R.gamma(2) * T)
    Tm = R.gather_magnitude(g, cluster, rdown, True, cptr, mean=True)
    note("mean backward", np.abs(e["dv", "mean"] - R.pool_backward(g, cluster, cptr, rdown, None, "mean", F64)), R.gamma(3) * Tm)
    note("unpool", np.abs(e["up"] - R.unpool(g, cluster, rup, F64)), R.gamma(2) * R.gather_magnitude(g, cluster, rup, False))
    Tu, L = R.pool_magnitude(v, cptr, members, rup, transposed=True)
    note("unpool backward", np.abs(e["dup"] - R.unpool_backward(v, cptr, members, rup, F64)),
         R.gamma(2 * np.repeat(L, 2).astype(F64)[:, None]) * Tu)
    # max: the value against the fp64 transport of the member fp32 chose
    arg = e["arg", "max"]
    full = arg[:, 0] >= 0
    if full.any():
        rows, ch = arg[full].astype(np.int64), np.arange(v.shape[1])[None, :]
        v64, r64 = np.asarray(v, dtype=F).astype(F64), rdown.astype(F64)
        a, b = v64[2 * rows, ch], v64[2 * rows + 1, ch]
        want = np.stack([r64[rows, 0] * a + r64[rows, 1] * b, r64[rows, 2] * a + r64[rows, 3] * b], 1)
        mag = np.stack([np.abs(r64[rows, 0] * a) + np.abs(r64[rows, 1] * b), np.abs(r64[rows, 2] * a) + np.abs(r64[rows, 3] * b)], 1)
        got = np.stack([e["out", "max"][0::2][full], e["out", "max"][1::2][full]], 1)
        note("max value", np.abs(got - want), R.gamma(2) * mag)
    print(f"\n{name}: worst fraction of the bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


@pytest.mark.parametrize("name", C.FINITE)
def test_the_maximum_selects_what_fp64_selects_outside_the_margin(name):
    c, e = C.BY_NAME[name], C.expected(name)
    keys, arg, cptr, members = R.exact_keys(c["v"]), e["arg", "max"], e["cptr"], e["members"]
    checked = 0
    for j in np.flatnonzero(np.diff(cptr) > 0):
        rows = members[cptr[j]:cptr[j + 1]]
        kk = keys[rows]                                                           # [members, C]
        best = kk.argmax(0)                                                       # the LOWEST row of the largest exact key
        top = kk.max(0)
        rest = np.where(np.arange(rows.size)[:, None] == best[None, :], -np.inf, kk).max(0) if rows.size > 1 else np.full_like(top, -np.inf)
        clear = rest < top * R.MARGIN * (1 - 2.0 ** -50)
        assert np.array_equal(arg[j][clear], rows[best][clear].astype(np.int32)), (name, j)
        # and inside the margin the winner is still within it of the largest
        chosen = keys[arg[j].astype(np.int64), np.arange(kk.shape[1])]
        assert (chosen >= top * R.MARGIN * (1 - 2.0 ** -50)).all()
        checked += int(clear.sum())
    assert checked > 0 or not c["cluster"].size or not c["m"]


# ---- properties, in fp64 ------------------------------------------------------------------------------------------------------------
def frames64(frames, angle=None):
    """The fp32 frames made orthonormal in fp64; the x-axes turned about the normals by `angle` (radians per row) where given."""
    n, x = (np.asarray(a, dtype=F64) for a in frames[:2])
    n = n / CR.norm3(n)[:, None]
    x = x - n * CR.dot3(x, n)[:, None]
    x = x / CR.norm3(x)[:, None]
    y = CR.cross3(n, x)
    if angle is not None:
        cs, sn = np.cos(angle)[:, None], np.sin(angle)[:, None]
        x, y = cs * x + sn * y, cs * y - sn * x
    return n, x, y


def embed(out, frames):
    """[2m,C] coefficients in `frames` -> [m,C,3] vectors of space."""
    return out[0::2, :, None] * frames[1][:, None, :] + out[1::2, :, None] * frames[2][:, None, :]


@pytest.mark.parametrize("name", ["small_cells", "mod7_1000_c64", "ids_without_a_cell"])
def test_the_pooled_vector_of_space_does_not_depend_on_any_x_axis(name):
    c, e = C.BY_NAME[name], C.expected(name)
    rng = np.random.default_rng(5)
    n, m = c["cluster"].size, c["m"]
    fine, coarse = frames64(c["fine"]), frames64(c["coarse"])
    fine_t, coarse_t = frames64(c["fine"], rng.uniform(0, 2 * np.pi, n)), frames64(c["coarse"], rng.uniform(0, 2 * np.pi, m))
    space = embed(np.asarray(c["v"], dtype=F64), fine)                           # the same vectors of space in the turned fine frames
    v_t = np.empty(c["v"].shape, F64)
    v_t[0::2], v_t[1::2] = (space * fine_t[1][:, None, :]).sum(2), (space * fine_t[2][:, None, :]).sum(2)
    for reduce in ("sum", "mean"):
        a = R.pool(np.asarray(c["v"], dtype=F64), e["cptr"], e["members"], R.table(c["cluster"], m, fine, coarse, "down", True, F64), reduce, F64)[0]
        b = R.pool(v_t, e["cptr"], e["members"], R.table(c["cluster"], m, fine_t, coarse_t, "down", True, F64), reduce, F64)[0]
        va, vb = embed(a, coarse), embed(b, coarse_t)
        assert np.abs(va - vb).max() <= 1e-9 * max(1.0, np.abs(va).max()), reduce


@pytest.mark.parametrize("name", ["small_cells", "mod7_1000_c64", "ids_without_a_cell"])
def test_unpool_then_sum_pool_returns_the_count_times_the_input(name):
    """Under non_oriented (the default) an entry holds the coordinates of the rotated vector itself, so up and down are inverse
    to each other.  With it off, a pair of normals that point apart carries the vector in the frame of the FLIPPED normal (the
    reference's connection does), and the two directions compose to a reflection there: not a property of that setting."""
    c, e = C.BY_NAME[name], C.expected(name)
    non_oriented = True
    m = c["m"]
    fine, coarse = frames64(c["fine"]), frames64(c["coarse"])
    x = np.asarray(c["g"], dtype=F64)
    up = R.unpool(x, c["cluster"], R.table(c["cluster"], m, fine, coarse, "up", non_oriented, F64), F64)
    back = R.pool(up, e["cptr"], e["members"], R.table(c["cluster"], m, fine, coarse, "down", non_oriented, F64), "sum", F64)[0]
    cnt = np.repeat(np.diff(e["cptr"]), 2).astype(F64)[:, None]
    assert np.abs(back - cnt * x).max() <= 1e-9 * cnt.max() * np.abs(x).max()


@pytest.mark.parametrize("name", ["small_cells", "random_3000_200_c130", "ids_without_a_cell", "voxel_cells_64_of_2000"])
def test_the_backwards_are_the_adjoints_of_the_forwards(name):
    c, e = C.BY_NAME[name], C.expected(name)
    rng = np.random.default_rng(6)
    dv, g = rng.standard_normal(c["v"].shape), rng.standard_normal(c["g"].shape)
    for reduce in ("sum", "mean"):
        lhs = (dv * R.pool_backward(g, c["cluster"], e["cptr"], e["rdown"], None, reduce, F64)).sum()
        rhs = (R.pool(dv, e["cptr"], e["members"], e["rdown"], reduce, F64)[0] * g).sum()
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs)), reduce
    lhs = (g * R.unpool_backward(dv, e["cptr"], e["members"], e["rup"], F64)).sum()
    rhs = (R.unpool(g, c["cluster"], e["rup"], F64) * dv).sum()
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_the_python_layer_refuses_what_the_host_can_see():
    from deltaconv_amd import geometry as G
    v, cl = torch.zeros(16, 3), torch.zeros(8, dtype=torch.int64)
    fr = (torch.zeros(8, 3),) * 3
    ptr, rot = torch.tensor([0, 8]), torch.zeros(8, 4)
    for call in (lambda: G.cluster_rotation(cl, 1, fr, fr), lambda: G.cluster_pool_vectors(v, cl, fr, fr, 1),
                 lambda: G.cluster_unpool_vectors(v[:2], cl, fr, fr), lambda: G.cluster_pool_vectors_rows(v, ptr, cl, rot),
                 lambda: G.cluster_pool_vectors_rows_backward(v[:2], cl, ptr, rot, None, "sum"),
                 lambda: G.cluster_unpool_vectors_rows(v[:2], cl, rot), lambda: G.cluster_unpool_vectors_rows_backward(v, ptr, cl, rot),
                 lambda: G.ClusterPair(cl, 1)):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    for bad in ("min", "median", None):
        with pytest.raises(ValueError, match="reduce"):
            G.cluster_pool_vectors(v, cl, fr, fr, 1, reduce=bad)
    with pytest.raises(RuntimeError, match="requires grad"):
        G.cluster_pool_vectors(v.clone().requires_grad_(), cl, fr, fr, 1)
    with pytest.raises(RuntimeError, match="requires grad"):
        G.cluster_unpool_vectors(v[:2].clone().requires_grad_(), cl, fr, fr)
