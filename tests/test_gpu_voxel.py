"""``geometry.voxel_subsample`` (csrc/voxel.hip behind ``dc_voxel_subsample``) and ``DeviceDataset.voxel_subsample`` on the MI355X.
Every comparison is an equality: the device against the numpy restatement (tests/voxel_restate.py) on every case of
tests/voxel_cases.py -- both picks, both given-origin forms -- a second run against the first, a ragged batch against the per-cloud
calls and against the same clouds in another batch order; the thinned store against the parent's rows, and through
``geodesic_subsample``, a ``DeviceLoader`` batch and ``Propagator`` against a store built by hand from the same rows."""
import numpy as np
import pytest
import torch

from tests import voxel_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def on_device(c):
    clouds = c["clouds"]
    pos = torch.from_numpy(np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32)).to(DEV)
    return pos, torch.from_numpy(C.ptr_of(c)).to(DEV)


def run(c, pos=None, ptr=None, **kw):
    from deltaconv_amd.geometry import voxel_subsample
    if pos is None:
        pos, ptr = on_device(c)
    return voxel_subsample(pos, c["size"], ptr=ptr, origin=c["origin"], pick=c["pick"], **kw)


@pytest.mark.parametrize("name", [n for n in C.NAMES if C.BY_NAME[n]["overflow"] < 0])
def test_device_equals_the_restatement_and_a_second_run(name):
    c = C.BY_NAME[name]
    rows, optr, cluster = run(c)
    want_rows, want_optr, want_cluster, _ = C.expected(name)
    assert rows.dtype == optr.dtype == cluster.dtype == torch.int64 and rows.is_cuda and optr.is_cuda and cluster.is_cuda
    assert torch.equal(optr.cpu(), torch.from_numpy(want_optr))
    assert torch.equal(rows.cpu(), torch.from_numpy(want_rows))
    assert torch.equal(cluster.cpu(), torch.from_numpy(want_cluster))
    if c["count"] is not None:
        assert rows.numel() == c["count"]
    again = run(c)
    assert all(torch.equal(a, b) for a, b in zip((rows, optr, cluster), again))


def test_the_origin_as_a_device_tensor_and_the_batch_vector_and_ptr_info_forms():
    from deltaconv_amd.geometry import voxel_subsample
    from deltaconv_amd.geometry.graph import PtrInfo
    c = C.BY_NAME["origin_per_cloud"]
    pos, ptr = on_device(c)
    want = run(c, pos, ptr)
    origin = torch.tensor(c["origin"], dtype=torch.float32, device=DEV)
    got = voxel_subsample(pos, c["size"], ptr=ptr, origin=origin)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    c = C.BY_NAME["origin_zero_negative_cells"]
    pos, ptr = on_device(c)
    assert all(torch.equal(a, b) for a, b in zip(run(c, pos, ptr), voxel_subsample(pos, c["size"], origin=torch.zeros(3, device=DEV))))
    c = C.BY_NAME["nonfinite_rows"]                                            # no empty cloud: a batch vector can state it
    pos, ptr = on_device(c)
    want = run(c, pos, ptr)
    batch = torch.repeat_interleave(torch.arange(len(c["clouds"]), device=DEV), ptr[1:] - ptr[:-1])
    sizes = [p.shape[0] for p in c["clouds"]]
    info = PtrInfo(ptr.to(torch.int32), len(sizes), max(sizes), min(sizes))
    for got in (voxel_subsample(pos, c["size"], batch=batch), voxel_subsample(pos, c["size"], ptr_info=info),
                voxel_subsample(pos, [c["size"]] * 3, ptr=ptr.cpu())):
        assert all(torch.equal(a, b) for a, b in zip(want, got))


@pytest.mark.parametrize("name", ["ragged", "ragged_first", "nonfinite_rows"])
def test_the_ragged_batch_equals_the_per_cloud_calls_and_another_batch_order(name):
    from deltaconv_amd.geometry import voxel_subsample
    c = C.BY_NAME[name]
    pos, ptr = on_device(c)
    rows, optr, cluster = run(c, pos, ptr)
    hp, ho = C.ptr_of(c), optr.tolist()
    for b in range(len(c["clouds"])):
        r1, o1, c1 = voxel_subsample(pos[hp[b]:hp[b + 1]], c["size"], pick=c["pick"])
        assert torch.equal(r1 + int(hp[b]), rows[ho[b]:ho[b + 1]]) and o1.tolist() == [0, ho[b + 1] - ho[b]]
        assert torch.equal(torch.where(c1 >= 0, c1 + ho[b], c1), cluster[hp[b]:hp[b + 1]])
    order = list(range(len(c["clouds"])))[::-1]
    other = dict(c, clouds=[c["clouds"][i] for i in order])
    r2, o2, _ = run(other)
    hp2, ho2 = C.ptr_of(other), o2.tolist()
    for j, i in enumerate(order):
        assert torch.equal(r2[ho2[j]:ho2[j + 1]] - int(hp2[j]), rows[ho[i]:ho[i + 1]] - int(hp[i]))
    # the offsets may cover a part of `pos`: rows outside every cloud belong to no cell
    lo, hi = int(hp[1]), int(hp[-2])
    r3, o3, c3 = voxel_subsample(pos, c["size"], ptr=ptr[1:-1], pick=c["pick"])
    assert torch.equal(r3, rows[ho[1]:ho[-2]]) and torch.equal(o3, optr[1:-1] - ho[1])
    assert bool((c3[:lo] == -1).all()) and bool((c3[hi:] == -1).all())
    assert torch.equal(c3[lo:hi], torch.where(cluster[lo:hi] >= 0, cluster[lo:hi] - ho[1], cluster[lo:hi]))


def test_the_overflow_error_names_the_cloud_and_the_edge_length():
    for name in ("overflow_size_1", "overflow_given_origin"):
        c = C.BY_NAME[name]
        with pytest.raises(ValueError, match=rf"cloud {c['overflow']} .*2\^20.*\({c['size']:g}, "):
            run(c)
    assert run(C.BY_NAME["far_point_size_4"])[0].numel() == C.BY_NAME["far_point_size_4"]["count"]


def test_the_argument_errors_raise():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import voxel_subsample
    pos = torch.from_numpy(C.uniform(1, 40)).to(DEV)
    ptr = torch.tensor([0, 40], device=DEV)
    for size in (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, [0.1, 0.2], [0.1, 0.2, 0.0], "x", None, [[0.1, 0.1, 0.1]]):
        with pytest.raises(ValueError, match="size"):
            voxel_subsample(pos, size)
    for kw in (dict(pick="mean"), dict(ptr=ptr, batch=torch.zeros(40, dtype=torch.long, device=DEV)), dict(ptr=torch.tensor([0, 41])),
               dict(ptr=torch.tensor([0, 30, 20, 40])), dict(ptr=torch.tensor([-1, 40])), dict(ptr=torch.zeros((2, 2), dtype=torch.long)),
               dict(batch=torch.zeros(39, dtype=torch.long, device=DEV)), dict(origin=[0.0, 0.0]), dict(origin=torch.zeros(2, 3)),
               dict(origin=[0.0, float("nan"), 0.0])):
        with pytest.raises(ValueError):
            voxel_subsample(pos, 0.1, **kw)
    for bad_pos in (pos.double(), pos.reshape(-1), pos[:, :2], pos.cpu()):
        with pytest.raises(ValueError):
            voxel_subsample(bad_pos, 0.1)
    with pytest.raises(RuntimeError, match="requires grad"):
        voxel_subsample(pos.clone().requires_grad_(), 0.1)
    with torch.no_grad():
        assert voxel_subsample(pos.clone().requires_grad_(), 0.1)[2].shape == (40,)
    rows, optr, cluster = voxel_subsample(pos[:0], 0.1)                         # an empty cloud: zero rows
    assert rows.numel() == 0 and optr.tolist() == [0, 0] and cluster.numel() == 0
    raw, need = lib.raw("dc_voxel_subsample"), int(lib.raw("dc_voxel_subsample_workspace_bytes")(40, 1))
    assert need >= 40 * 40 and lib.raw("dc_voxel_subsample_workspace_bytes")(-1, 1) == 0
    ws = torch.zeros(need // 8 + 1, dtype=torch.int64, device=DEV)
    out = [torch.zeros(40, dtype=torch.int64, device=DEV) for _ in range(2)]
    optr, info = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    args = lambda **kw: tuple({**dict(pos=pos.data_ptr(), ptr=ptr.data_ptr(), B=1, n=40, sx=0.1, sy=0.1, sz=0.1, origin=None, pick=0,
                                     rows=out[0].data_ptr(), optr=optr.data_ptr(), cluster=out[1].data_ptr(), info=info.data_ptr(),
                                     ws=ws.data_ptr(), bytes=need, stream=None), **kw}.values())
    for bad in (dict(pos=None), dict(ptr=None), dict(rows=None), dict(optr=None), dict(cluster=None), dict(info=None), dict(ws=None),
                dict(ws=ws.data_ptr() + 8), dict(bytes=need - 16), dict(B=-1), dict(n=-1), dict(sx=0.0), dict(sz=float("inf")),
                dict(pick=2)):
        assert raw(*args(**bad)) == -1 and "dc_voxel_subsample" in lib.last_error(), bad


# ---- the store ----------------------------------------------------------------------------------------------------------------------------
SIZES = (700, 1, 1300, 400)


@pytest.fixture(scope="module")
def stores():
    from deltaconv_amd.loader import DeviceDataset
    n = sum(SIZES)
    g = torch.Generator().manual_seed(5)
    pos = torch.from_numpy(np.concatenate([C.uniform(60 + i, s) for i, s in enumerate(SIZES)]))
    norm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64)
    parent = DeviceDataset(pos.to(DEV), ptr.to(DEV), SIZES, norm.to(DEV), torch.randn(n, 5, generator=g).to(DEV),
                           torch.randint(0, 7, (n,), generator=g).to(DEV), None, torch.randn(len(SIZES), 4, generator=g).to(DEV))
    sub = parent.voxel_subsample(0.2)
    rows = sub.source_rows
    take = lambda t: t[rows].contiguous()
    by_hand = DeviceDataset(take(parent.pos), sub.ptr.clone(), sub.sizes.copy(), take(parent.norm), take(parent.x),
                            take(parent.y_point), parent.y_cloud, parent.category)
    return parent, sub, by_hand


def test_the_thinned_store_gathers_the_parent_by_source_rows(stores):
    from deltaconv_amd.geometry import voxel_subsample
    parent, sub, _ = stores
    rows, optr, cluster = voxel_subsample(parent.pos, 0.2, ptr=parent.ptr)
    assert torch.equal(sub.source_rows, rows) and torch.equal(sub.ptr, optr) and torch.equal(sub.cluster, cluster)
    for name in ("pos", "norm", "x", "y_point"):
        assert torch.equal(getattr(sub, name), getattr(parent, name)[rows]), name
    assert sub.y_cloud is None and sub.category is parent.category
    from deltaconv_amd.loader import DeviceDataset
    labelled = DeviceDataset(parent.pos, parent.ptr, SIZES, y_cloud=torch.arange(len(SIZES), device=DEV))     # one label a cloud: shared
    thin = labelled.voxel_subsample(0.2)
    assert thin.y_cloud is labelled.y_cloud and thin.y_point is None and thin.norm is None and torch.equal(thin.pos, sub.pos)
    assert sub.sizes.dtype == np.int64 and sub.sizes.tolist() == (optr[1:] - optr[:-1]).tolist() and len(sub) == len(parent)
    assert sub.sizes[1] == 1 and all(1 <= m <= n for m, n in zip(sub.sizes, SIZES)) and sub.sizes.sum() < sum(SIZES) // 2
    assert torch.equal(sub.pos[cluster], parent.pos[rows[cluster]]) and int(cluster.min()) >= 0
    first = parent.voxel_subsample([0.2, 0.2, 0.2], origin=[0.0, 0.0, 0.0], pick="first")
    assert torch.equal(first.source_rows, voxel_subsample(parent.pos, 0.2, ptr=parent.ptr, origin=torch.zeros(3), pick="first")[0])


def test_the_thinned_store_is_a_store_like_any_other(stores):
    from deltaconv_amd.loader import DeviceLoader
    from deltaconv_amd.propagate import Propagator
    parent, sub, by_hand = stores
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t     # the one-point cloud normalises to NaN: compare bits
    same = lambda a, b: all((getattr(a, n) is None and getattr(b, n) is None) or torch.equal(bits(getattr(a, n)), bits(getattr(b, n)))
                            for n in ("pos", "norm", "x", "y_point", "y_cloud", "category", "ptr")) and np.array_equal(a.sizes, b.sizes)
    assert same(sub.subset([2, 0]), by_hand.subset([2, 0])) and sub.subset([3]).sizes.tolist() == [int(sub.sizes[3])]
    from deltaconv_amd import transforms as T
    assert same(sub.normalize(T.NormalizeScale()), by_hand.normalize(T.NormalizeScale()))
    assert same(sub.geodesic_subsample(32, seed=3), by_hand.geodesic_subsample(32, seed=3))
    assert sub.geodesic_subsample(32, seed=3).pos.shape == (4 * 32, 3)
    a, b = next(iter(DeviceLoader(sub, 3))), next(iter(DeviceLoader(by_hand, 3)))
    assert a.pos.shape[0] == int(sub.sizes[:3].sum()) and a.num_graphs == 3
    for name in ("pos", "batch", "norm", "x", "y", "category"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    prop, ref = Propagator(sub, parent, k=1), Propagator(by_hand, parent, k=1)
    up = prop.apply(sub.x)
    assert up.shape == (parent.pos.shape[0], 5) and torch.equal(up, ref.apply(by_hand.x))
    ids = torch.arange(sub.pos.shape[0], device=DEV)
    back = prop.labels(ids)
    assert torch.equal(back[sub.source_rows], ids)                              # a kept row's nearest kept row is itself
    assert torch.equal(prop.labels(sub.y_point)[sub.source_rows], parent.y_point[sub.source_rows])
