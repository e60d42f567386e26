"""Host side of the pooling over cluster cells (csrc/cluster_math.h), without a GPU: a g++ build of the header with serial drivers
(tests/hostcheck_cluster) equals the numpy restatement (tests/cluster_restate.py) BIT FOR BIT on every case of
tests/cluster_cases.py -- lists, out, arg, both gradients, barycentres, majority labels; the restatement is held to fp64
(math.fsum) inside bounds derived in cluster_restate.bounds; and the properties the op promises.  Run with ``-s`` to see the worst
observed fraction of every bound (the table of DESIGN.md section 3.4q)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import cluster_cases as C
from tests import cluster_restate as R
from tests.helpers import ROOT

HC_DIR = os.path.join(ROOT, "tests", "hostcheck_cluster")
F = np.float32
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
bits = lambda a: np.ascontiguousarray(a).view(np.int32) if a.dtype == F else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def hc():
    subprocess.run(["make", "-s", "-C", HC_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HC_DIR, "libhostcheck_cluster.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hcl_max_classes.argtypes, lib.hcl_max_classes.restype = [], i32
    lib.hcl_mode.argtypes, lib.hcl_mode.restype = [i32], i32
    lib.hcl_lists.argtypes, lib.hcl_lists.restype = [vp, i64, i64, vp, vp], None
    lib.hcl_pool.argtypes, lib.hcl_pool.restype = [vp, i64, i64, i32, vp, vp, i64, i32, vp, i64, vp, i64], None
    lib.hcl_pool_backward.argtypes, lib.hcl_pool_backward.restype = [vp, i64, i64, i32, vp, i64, vp, vp, i64, i32, vp, i64], None
    lib.hcl_mean3.argtypes, lib.hcl_mean3.restype = [vp, i64, vp, vp, i64, i32, vp], None
    lib.hcl_majority.argtypes, lib.hcl_majority.restype = [vp, i64, vp, vp, i64, i32, vp], None
    return lib


def ld_of(a):
    """The leading dimension of a [rows, C] fp32 array with unit stride along the channels."""
    assert a.ndim == 2 and (a.shape[1] == 1 or a.shape[0] == 0 or a.strides[1] == 4)
    return a.strides[0] // 4 if a.shape[0] > 1 else a.shape[1]


def host_lists(hc, cluster, m):
    cptr, members = np.full(m + 1, -7, np.int64), np.full(cluster.size, -7, np.int64)
    hc.hcl_lists(P(cluster), cluster.size, m, P(cptr), P(members))
    return cptr, members


def host_pool(hc, x, cptr, members, reduce):
    m, c = cptr.size - 1, x.shape[1]
    out, arg = np.full((m, c), 7, F), np.full((m, c), -7, np.int32)
    hc.hcl_pool(P(x), ld_of(x), x.shape[0], c, P(cptr), P(members), m, R.MODES[reduce], P(out), c,
                P(arg) if reduce in ("max", "min") else None, c)
    return out, (arg if reduce in ("max", "min") else None)


def host_backward(hc, g, cluster, cptr, arg, reduce):
    dx = np.full((cluster.size, g.shape[1]), 7, F)
    hc.hcl_pool_backward(P(g), ld_of(g), g.shape[0], g.shape[1], P(cluster), cluster.size, P(cptr), P(arg), g.shape[1],
                         R.MODES[reduce], P(dx), g.shape[1])
    return dx


def test_the_constants_are_declared_the_same_everywhere(hc):
    from deltaconv_amd.geometry import cluster as G
    from deltaconv_amd.geometry.pool import _MODES
    assert hc.hcl_max_classes() == G.MAX_CLASSES == 1024 and G.MAX_ROWS == 2 ** 31 - 1
    assert all(hc.hcl_mode(v) == v == _MODES[k] for k, v in R.MODES.items())


@pytest.mark.parametrize("name", C.NAMES)
def test_host_lists_equal_the_restatement_and_hold_every_valid_row_once(hc, name):
    c, e = C.BY_NAME[name], C.expected(name)
    cptr, members = host_lists(hc, c["cluster"], c["m"])
    assert same(cptr, e["cptr"]) and same(members, e["members"])
    ok = R.valid(c["cluster"], c["m"])
    assert cptr[0] == 0 and cptr[-1] == ok.sum() and (np.diff(cptr) >= 0).all()
    assert np.array_equal(np.sort(members[:cptr[-1]]), np.flatnonzero(ok)) and (members[cptr[-1]:] == -1).all()
    for j in range(c["m"]):
        mine = members[cptr[j]:cptr[j + 1]]
        assert (np.diff(mine) > 0).all() and (c["cluster"][mine] == j).all()


@pytest.mark.parametrize("reduce", C.REDUCES)
@pytest.mark.parametrize("name", C.NAMES)
def test_host_pool_and_its_backward_equal_the_restatement(hc, name, reduce):
    c, e = C.BY_NAME[name], C.expected(name)
    out, arg = host_pool(hc, c["x"], e["cptr"], e["members"], reduce)
    assert same(out, e["out", reduce])
    assert (arg is None and e["arg", reduce] is None) or same(arg, e["arg", reduce])
    assert same(host_backward(hc, c["g"], c["cluster"], e["cptr"], arg, reduce), e["dx", reduce])
    empty = np.diff(e["cptr"]) == 0
    assert (out[empty] == 0).all() and (arg is None or (arg[empty] == -1).all())


@pytest.mark.parametrize("name", C.NAMES)
def test_host_unpool_barycentres_and_labels_equal_the_restatement(hc, name):
    c, e = C.BY_NAME[name], C.expected(name)
    assert same(host_backward(hc, c["g"], c["cluster"], None, None, "sum"), e["up"])
    assert same(host_pool(hc, c["x"], e["cptr"], e["members"], "sum")[0], e["dup"])
    for key, p, normalize in (("bary", c["pos"], 0), ("nbar", c["norm"], 1)):
        out = np.full((c["m"], 3), 7, F)
        hc.hcl_mean3(P(p), p.shape[0], P(e["cptr"]), P(e["members"]), c["m"], normalize, P(out))
        assert same(out, e[key]), key
    lab = np.full(c["m"], -7, np.int64)
    hc.hcl_majority(P(c["labels"]), c["labels"].size, P(e["cptr"]), P(e["members"]), c["m"], c["classes"], P(lab))
    assert same(lab, e["label"])


def test_the_selection_rules_on_the_special_values():
    e = C.expected("nan_inf_signed_zero")
    hi, lo, amax, amin = e["out", "max"], e["out", "min"], e["arg", "max"], e["arg", "min"]
    assert np.isnan(hi[0, 0]) and np.isnan(lo[0, 0]) and amax[0, 0] == amin[0, 0] == 0         # a first NaN stays
    assert hi[0, 1] == 7 and amax[0, 1] == 2 and lo[0, 1] == 1 and amin[0, 1] == 0             # a later NaN is never taken; tie: lower row
    assert hi[0, 2] == np.inf and amax[0, 2] == 2 and lo[0, 2] == -np.inf and amin[0, 2] == 0
    for ch, first in ((0, 0.0), (1, -0.0)):                                                    # +0.0 against -0.0 is a tie
        for out, arg in ((hi, amax), (lo, amin)):
            assert arg[1, ch] == 4 and np.signbit(out[1, ch]) == np.signbit(F(first))
    assert hi[1, 2] == 4 and amax[1, 2] == 4 and lo[1, 2] == -np.inf and amin[1, 2] == 6
    e = C.expected("all_equal")
    assert (e["out", "max"] == 1.5).all() and np.array_equal(e["arg", "max"], np.repeat(np.arange(5, dtype=np.int32)[:, None], 4, 1))
    assert same(e["arg", "max"], e["arg", "min"])
    e = C.expected("label_ties")
    assert e["label"].tolist() == [1, 0, 3, -1]
    c, e = C.BY_NAME["ids_without_a_cell"], C.expected("ids_without_a_cell")
    assert all(e["cptr"][j] == e["cptr"][j + 1] for j in (5, 17, 49)) and (e["dx", "sum"][~R.valid(c["cluster"], 50)] == 0).all()


WORST = {}


def note(key, err, bound):
    """The worst err / bound of a check -> WORST, after asserting err <= bound everywhere."""
    assert (err <= bound).all(), (key, float((err - bound).max()))
    frac = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), frac)


@pytest.mark.parametrize("name", C.FINITE)
def test_the_restatement_lies_inside_the_derived_bounds_of_fp64(name):
    c, e = C.BY_NAME[name], C.expected(name)
    x = np.asarray(c["x"], dtype=np.float64)
    full = np.diff(e["cptr"]) > 0
    for reduce, pick in (("max", np.max), ("min", np.min)):                        # the fp64 selection, and the LOWEST row that holds it
        for j in np.flatnonzero(full):
            rows = e["members"][e["cptr"][j]:e["cptr"][j + 1]]
            want = pick(x[rows], axis=0)
            assert np.array_equal(e["out", reduce][j].astype(np.float64), want)
            assert np.array_equal(e["arg", reduce][j], rows[(x[rows] == want[None, :]).argmax(0)])
    b = R.bounds(c["x"], e["cptr"], e["members"])
    note("sum", np.abs(e["out", "sum"] - b["true_sum"]), b["sum"])
    note("mean", np.abs(e["out", "mean"] - b["true_mean"]), b["mean"])
    note("unpool backward", np.abs(e["dup"] - b["true_sum"]), b["sum"])             # a sum over L terms: L * 2^-24 * sum |g|
    bp = R.bounds(c["pos"], e["cptr"], e["members"])
    note("barycentre", np.abs(e["bary"] - bp["true_mean"]), bp["bary"])
    print(f"\n{name}: worst fraction of the bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in WORST.items()))


def test_the_fp32_barycentre_would_lose_the_shifted_cloud():
    """Why dc_cluster_mean3 sums in fp64: at a shift of 4 096 the fp32 chain leaves the fp64-held bound, the fp64 chain does not."""
    c, e = C.BY_NAME["shifted_4096"], C.expected("shifted_4096")
    bp = R.bounds(c["pos"], e["cptr"], e["members"])
    chain = R.pool(c["pos"], e["cptr"], e["members"], "mean")[0]
    assert (np.abs(chain - bp["true_mean"]) > bp["bary"]).any() and (np.abs(e["bary"] - bp["true_mean"]) <= bp["bary"]).all()


@pytest.mark.parametrize("reduce", C.REDUCES)
def test_a_batch_equals_its_clouds_one_by_one(hc, reduce):
    a, b = C.BY_NAME["random_3000_200_c130"], C.BY_NAME["mod7_1000_c64"]
    xa, xb = a["x"][:, :64], b["x"]
    cluster = np.concatenate([a["cluster"], b["cluster"] + a["m"]])
    cptr, members = host_lists(hc, cluster, a["m"] + b["m"])
    out, arg = host_pool(hc, np.ascontiguousarray(np.concatenate([xa, xb])), cptr, members, reduce)
    oa, aa = host_pool(hc, xa, *R.lists(a["cluster"], a["m"]), reduce)
    ob, ab = host_pool(hc, xb, *R.lists(b["cluster"], b["m"]), reduce)
    assert same(out, np.concatenate([oa, ob]))
    assert arg is None or same(arg, np.concatenate([aa, ab + np.int32(3000)]))


@pytest.mark.parametrize("name", ["random_3000_200_c130", "ids_without_a_cell", "voxel_cells_64_of_2000"])
def test_permuting_the_rows_keeps_the_maxima_and_minima(hc, name):
    c, e = C.BY_NAME[name], C.expected(name)
    perm = np.random.default_rng(3).permutation(c["cluster"].size)
    cluster, x = np.ascontiguousarray(c["cluster"][perm]), np.ascontiguousarray(c["x"][perm])
    cptr, members = host_lists(hc, cluster, c["m"])
    for reduce in ("max", "min"):
        out, arg = host_pool(hc, x, cptr, members, reduce)
        assert same(out, e["out", reduce])
        full = arg[:, 0] >= 0
        assert same(x[arg[full], np.arange(x.shape[1])[None, :]], out[full])      # arg names a row that holds the value


def test_the_python_layer_refuses_what_the_host_can_see():
    from deltaconv_amd import geometry as G
    x, cl = torch.zeros(8, 3), torch.zeros(8, dtype=torch.int64)
    ptr = torch.tensor([0, 8])
    for call in (lambda: G.cluster_lists(cl, 1), lambda: G.cluster_pool(x, cl, 1), lambda: G.cluster_unpool(x[:1], cl),
                 lambda: G.cluster_pool_rows(x, ptr, cl), lambda: G.cluster_pool_rows_backward(x[:1], cl, ptr, None, "sum"),
                 lambda: G.cluster_mean_pos(x, ptr, cl), lambda: G.cluster_majority(cl, ptr, cl, 3)):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    with pytest.raises(ValueError, match="reduce"):
        G.cluster_pool(x, cl, 1, reduce="median")
    with pytest.raises(RuntimeError, match="requires grad"):
        G.cluster_pool(x.clone().requires_grad_(), cl, 1)
