"""Host side of voxel-grid subsampling (csrc/voxel_math.h), without a GPU: a g++ build of the header with a serial driver
(tests/hostcheck_voxel) equals the numpy restatement (tests/voxel_restate.py) on every case of tests/voxel_cases.py -- rows, optr,
cluster and the overflow flag -- and the properties the op promises.  Every check is an equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import voxel_cases as C
from tests import voxel_restate as R
from tests.helpers import ROOT

HV_DIR = os.path.join(ROOT, "tests", "hostcheck_voxel")
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
PICK = {"centre": 0, "first": 1}
F = np.float32


@pytest.fixture(scope="module")
def hv():
    subprocess.run(["make", "-s", "-C", HV_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HV_DIR, "libhostcheck_voxel.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hv_axis_limit.argtypes, lib.hv_axis_limit.restype = [], i32
    lib.hv_keys.argtypes, lib.hv_keys.restype = [vp, vp, i64, vp], None
    lib.hv_bids.argtypes, lib.hv_bids.restype = [vp, i64, vp, vp, i32, vp, vp, vp], None
    lib.hv_subsample.argtypes, lib.hv_subsample.restype = [vp, vp, i32, vp, vp, i32, vp, vp, vp], i64
    return lib


def host_batch(hv, clouds, size, origin=None, pick="centre"):
    """-> (rows, optr, cluster, first overflowing cloud or -1) of the g++ build."""
    b = len(clouds)
    pos = np.ascontiguousarray(np.concatenate(clouds) if b else np.zeros((0, 3)), dtype=F).reshape(-1, 3)
    ptr = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    n = pos.shape[0]
    rows, cluster, optr = np.full(n, -7, np.int64), np.full(n, -7, np.int64), np.full(b + 1, -7, np.int64)
    if origin is not None:
        origin = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=F).reshape(-1, 3), (b, 3)))
    over = hv.hv_subsample(P(pos), P(ptr), b, P(R.edges(size)), P(origin), PICK[pick], P(rows), P(optr), P(cluster))
    assert over >= -1
    return rows[:optr[-1]], optr, cluster, int(over)


def host_case(hv, c):
    return host_batch(hv, c["clouds"], c["size"], c["origin"], c["pick"])


def test_the_range_is_declared_the_same_everywhere(hv):
    from deltaconv_amd.geometry.voxel import CELL_LIMIT, PICKS
    assert hv.hv_axis_limit() == CELL_LIMIT == int(R.LIMIT) == R.BIAS == 1 << 20 and PICKS == PICK


@pytest.mark.parametrize("name", C.NAMES)
def test_host_build_equals_the_restatement(hv, name):
    c = C.BY_NAME[name]
    rows, optr, cluster, over = host_case(hv, c)
    want_rows, want_optr, want_cluster, want_over = C.expected(name)
    assert over == want_over == c["overflow"]
    if over >= 0:
        return                                              # the call raises: the outputs are not to be used
    assert np.array_equal(optr, want_optr) and np.array_equal(rows, want_rows) and np.array_equal(cluster, want_cluster)
    if c["count"] is not None:
        assert rows.size == c["count"], (name, rows.size)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_bids_equal_the_restatement_point_by_point(hv, name):
    c = C.BY_NAME[name]
    b = len(c["clouds"])
    origin = None if c["origin"] is None else np.broadcast_to(np.asarray(c["origin"], dtype=F).reshape(-1, 3), (b, 3))
    for i, pos in enumerate(c["clouds"]):
        n = pos.shape[0]
        o = R.origin_of(pos) if origin is None else np.ascontiguousarray(origin[i])
        cell, key, flags = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
        hv.hv_bids(P(pos), n, P(o), P(R.edges(c["size"])), PICK[c["pick"]], P(cell), P(key), P(flags))
        want = R.cloud(pos, c["size"], o, c["pick"])
        assert np.array_equal(cell, want["cell"]) and np.array_equal(key, want["key"]), (name, i)
        assert np.array_equal((flags & 1) == 1, R.finite_rows(pos)) and bool((flags & 2).any()) == want["overflow"]


def test_the_key_orders_by_d2_then_the_lower_index(hv):
    d2 = np.array([0.0, 0.0, 1e-45, 1e-45, 1e-38, 0.5, 1.0, 1.0, 3e38, np.inf, np.inf], F)
    ids = np.array([7, 3, 9, 2, 0, 11, 6, 5, 1, 10, 8], np.uint32)
    keys = np.zeros(d2.size, np.uint64)
    hv.hv_keys(P(d2), P(ids), d2.size, P(keys))
    assert np.array_equal(keys, R.key(d2, ids))
    want = sorted(range(d2.size), key=lambda i: (float(d2[i]), int(ids[i])))
    assert list(np.argsort(keys, kind="stable")) == want and np.unique(keys).size == keys.size
    assert int(np.argmax(keys)) == 9 and int(np.argmin(keys)) == 1            # +inf sorts last; of two equal d2 the lower index
    assert int(keys.max()) < 2 ** 64 - 1                                      # all ones stays free for "no representative"


def cells_of(c, b):
    """The restatement's per-axis cells of cloud b (fp32 [n,3]) and which rows take part."""
    pos = c["clouds"][b]
    origin = None if c["origin"] is None else np.broadcast_to(np.asarray(c["origin"], dtype=F).reshape(-1, 3), (len(c["clouds"]), 3))
    o = R.origin_of(pos) if origin is None else origin[b]
    return R.cells(pos, o, R.edges(c["size"])), R.finite_rows(pos)


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.BY_NAME[n]["overflow"] < 0])
def test_one_representative_per_occupied_cell_in_row_order(hv, name):
    c = C.BY_NAME[name]
    rows, optr, cluster, _ = host_case(hv, c)
    ptr = C.ptr_of(c)
    assert np.unique(rows).size == rows.size                                  # pairwise distinct
    for b, pos in enumerate(c["clouds"]):
        t, fin = cells_of(c, b)
        mine = rows[optr[b]:optr[b + 1]] - ptr[b]
        assert (np.diff(mine) > 0).all() and (mine.size == 0 or (mine.min() >= 0 and mine.max() < pos.shape[0]))
        assert mine.size == np.unique(t[fin], axis=0).shape[0]                # one per occupied cell
        assert np.unique(t[mine], axis=0).shape[0] == mine.size and fin[mine].all()
        cl = cluster[ptr[b]:ptr[b + 1]]
        assert (cl[~fin] == -1).all() and (cl[fin] >= optr[b]).all() and (cl[fin] < optr[b + 1]).all()
        rep = rows[cl[fin]] - ptr[b]                                          # every point's representative lies in its own cell
        assert np.array_equal(t[rep], t[fin])
        assert np.array_equal(cluster[rows[optr[b]:optr[b + 1]]], np.arange(optr[b], optr[b + 1]))   # a representative stands for itself


def test_centre_and_first_differ_where_cells_hold_many(hv):
    a, b = host_case(hv, C.BY_NAME["cells_64_of_2000"]), host_case(hv, C.BY_NAME["cells_64_of_2000_first"])
    assert a[0].size == b[0].size == 64 and not np.array_equal(a[0], b[0])
    pos = C.BY_NAME["cells_64_of_2000"]["clouds"][0]
    t, _ = cells_of(C.BY_NAME["cells_64_of_2000"], 0)
    _, first = np.unique(t, axis=0, return_index=True)                        # the first member of every cell
    assert np.array_equal(b[0], np.sort(first))
    assert np.array_equal(np.unique(t[a[0]], axis=0), np.unique(t[b[0]], axis=0)) and pos.shape[0] == 2000


@pytest.mark.parametrize("name", ["ragged", "ragged_first", "nonfinite_rows", "origin_per_cloud"])
def test_a_batch_equals_the_per_cloud_calls(hv, name):
    """The default origin is a cloud's own minimum: its batch-mates cannot reach it."""
    c = C.BY_NAME[name]
    rows, optr, cluster, _ = host_case(hv, c)
    ptr = C.ptr_of(c)
    origin = None if c["origin"] is None else np.asarray(c["origin"], dtype=F).reshape(-1, 3)
    for b, pos in enumerate(c["clouds"]):
        r1, o1, c1, _ = host_batch(hv, [pos], c["size"], None if origin is None else origin[b], c["pick"])
        assert np.array_equal(r1 + ptr[b], rows[optr[b]:optr[b + 1]]) and o1[1] == optr[b + 1] - optr[b]
        assert np.array_equal(np.where(c1 >= 0, c1 + optr[b], -1), cluster[ptr[b]:ptr[b + 1]])
    order = [2, 0, 4, 1, 3][:len(c["clouds"])] if len(c["clouds"]) == 5 else list(range(len(c["clouds"])))[::-1]
    r2, o2, _, _ = host_batch(hv, [c["clouds"][i] for i in order], c["size"], None if origin is None else origin[order], c["pick"])
    ptr2 = np.concatenate([[0], np.cumsum([c["clouds"][i].shape[0] for i in order])])
    for j, i in enumerate(order):                                             # the same clouds in another batch order
        assert np.array_equal(r2[o2[j]:o2[j + 1]] - ptr2[j], rows[optr[i]:optr[i + 1]] - ptr[i])


@pytest.mark.parametrize("name", C.TIE_FREE)
def test_permuting_the_rows_keeps_the_set_of_picked_positions(hv, name):
    c = C.BY_NAME[name]
    assert c["pick"] == "centre" and len(c["clouds"]) == 1
    pos = c["clouds"][0]
    want = R.cloud(pos, c["size"], None if c["origin"] is None else c["origin"], "centre")
    d2 = (want["key"] >> np.uint64(32)).astype(np.int64)
    pairs = np.stack([want["cell"].astype(np.int64), d2], 1)                   # no two members of a cell at one distance
    assert np.unique(pairs, axis=0).shape[0] == pos.shape[0]
    rows = host_case(hv, c)[0]
    perm = np.random.default_rng(9).permutation(pos.shape[0])
    got = host_batch(hv, [pos[perm]], c["size"], c["origin"], "centre")[0]
    assert np.array_equal(np.sort(perm[got]), rows)
    first = host_batch(hv, [pos[perm]], c["size"], c["origin"], "first")[0]    # the first pick follows the order instead
    assert not np.array_equal(np.sort(perm[first]), host_batch(hv, [pos], c["size"], c["origin"], "first")[0])


def test_voxel_subsample_refuses_what_the_host_can_see():
    from deltaconv_amd.geometry import voxel_subsample
    with pytest.raises(ValueError, match="HIP device"):
        voxel_subsample(torch.zeros(8, 3), 0.1)
    with pytest.raises(ValueError, match="HIP device"):
        voxel_subsample(np.zeros((8, 3), np.float32), 0.1)
