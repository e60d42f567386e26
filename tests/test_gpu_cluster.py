"""``geometry.cluster_*`` (csrc/cluster.hip) and ``DeviceDataset.voxel_subsample(reduce=...)`` on the MI355X.  The device against the
numpy restatement (tests/cluster_restate.py) on every case of tests/cluster_cases.py by ``torch.equal`` on the bits -- lists,
forward, arg, both backwards, barycentres, majority labels -- and a second run against the first; the autograd nodes through
``backward()``; the pool / un-pool composition against fp64 inside the derived bounds; a captured lists + pool + backward replayed
on data written in place; ``voxel_subsample`` -> ``cluster_pool`` end to end; the store in both modes; the argument errors."""
import numpy as np
import pytest
import torch

from tests import cluster_cases as C
from tests import cluster_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    """A numpy array on the device, with its strides (a strided view stays one)."""
    if a.size == 0:
        return torch.zeros(a.shape, dtype=torch.from_numpy(a).dtype, device=DEV)
    if a.flags["C_CONTIGUOUS"]:
        return torch.from_numpy(a).to(DEV)
    base = a.base
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // a.itemsize
    return torch.from_numpy(base).to(DEV).as_strided(a.shape, [s // a.itemsize for s in a.strides], off)


def same(t, a):
    """A device tensor equals a numpy array bit for bit (NaN and signed zeros included)."""
    if a is None:
        return t is None
    w = torch.from_numpy(np.ascontiguousarray(a))
    t = t.cpu()
    view = (lambda v: v.contiguous().view(torch.int32)) if w.dtype == torch.float32 else (lambda v: v)
    return t.dtype == w.dtype and t.shape == w.shape and torch.equal(view(t), view(w))


def run_case(name):
    from deltaconv_amd import geometry as G
    c = C.BY_NAME[name]
    cluster, x, g = dev(c["cluster"]), dev(c["x"]), dev(c["g"])
    res = dict(lists=G.cluster_lists(cluster, c["m"]))
    cptr, members = res["lists"]
    for r in C.REDUCES:
        res["fwd", r] = G.cluster_pool_rows(x, cptr, members, r)
        res["dx", r] = G.cluster_pool_rows_backward(g, cluster, cptr, res["fwd", r][1], r)
    res["up"] = G.cluster_unpool(g, cluster)
    res["dup"] = G.cluster_pool_rows(x, cptr, members, "sum")[0]
    res["bary"] = G.cluster_mean_pos(dev(c["pos"]), cptr, members)
    res["nbar"] = G.cluster_mean_pos(dev(c["norm"]), cptr, members, normalize=True)
    res["label"] = G.cluster_majority(dev(c["labels"]), cptr, members, c["classes"])
    return res


def flat(res):
    return [t for v in res.values() for t in (v if isinstance(v, tuple) else (v,)) if t is not None]


@pytest.mark.parametrize("name", C.NAMES)
def test_device_equals_the_restatement_and_a_second_run(name):
    c, e = C.BY_NAME[name], C.expected(name)
    res = run_case(name)
    assert same(res["lists"][0], e["cptr"]) and same(res["lists"][1], e["members"])
    if not (c["x"].flags["C_CONTIGUOUS"] or c["x"].size == 0):
        assert not dev(c["x"]).is_contiguous()                                  # the strided view reaches the kernel as one
    for r in C.REDUCES:
        assert same(res["fwd", r][0], e["out", r]), r
        assert same(res["fwd", r][1], e["arg", r]), r
        assert same(res["dx", r], e["dx", r]), r
    for key in ("up", "dup", "bary", "nbar", "label"):
        assert same(res[key], e[key]), key
    again = flat(run_case(name))
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(res), again))


@pytest.mark.parametrize("reduce", C.REDUCES)
@pytest.mark.parametrize("name", ["random_3000_200_c130", "ids_without_a_cell", "one_cell_5000_c5"])
def test_the_autograd_nodes_give_the_restated_gradients(name, reduce):
    from deltaconv_amd import geometry as G
    c, e = C.BY_NAME[name], C.expected(name)
    cluster, g = dev(c["cluster"]), dev(c["g"])
    x = dev(c["x"]).requires_grad_()
    out = G.cluster_pool(x, cluster, c["m"], reduce, differentiable=True)
    assert out.requires_grad and same(out.detach(), e["out", reduce])
    out.backward(g)
    assert same(x.grad, e["dx", reduce])
    with torch.no_grad():
        assert same(G.cluster_pool(x, cluster, c["m"], reduce), e["out", reduce])
    lists = G.cluster_lists(cluster, c["m"])
    assert same(G.cluster_pool(x.detach(), cluster, reduce=reduce, lists=lists), e["out", reduce])
    if reduce == "sum":                                                         # the un-pooling, its backward fed the [n,C] rows x
        y = g.clone().requires_grad_()
        up = G.cluster_unpool(y, cluster, differentiable=True)
        assert up.requires_grad and same(up.detach(), e["up"])
        up.backward(x.detach())
        assert same(y.grad, e["dup"])
        y.grad = None
        G.cluster_unpool(y, cluster, lists=lists, differentiable=True).backward(x.detach())
        assert same(y.grad, e["dup"])
        if int(c["cluster"].max()) + 1 == c["m"]:                               # M read from the device
            assert same(G.cluster_pool(x.detach(), cluster, None, "sum"), e["out", "sum"])


def test_unpool_of_the_mean_pool_lies_inside_the_bounds_of_an_fp64_composition():
    from deltaconv_amd import geometry as G
    c, e = C.BY_NAME["random_3000_200_c130"], C.expected("random_3000_200_c130")
    cluster = dev(c["cluster"])
    x = dev(c["x"]).requires_grad_()
    up = G.cluster_unpool(G.cluster_pool(x, cluster, c["m"], "mean", differentiable=True), cluster, differentiable=True)
    w = dev(c["x"][::-1].copy())                                                 # any cotangent
    up.backward(w)
    x64 = x.detach().double().requires_grad_()
    cnt = torch.bincount(cluster, minlength=c["m"]).double()[:, None]
    mean64 = torch.zeros(c["m"], x.shape[1], dtype=torch.float64, device=DEV).index_add_(0, cluster, x64) / cnt
    up64 = mean64[cluster]
    up64.backward(w.double())
    b = R.bounds(c["x"], e["cptr"], e["members"])
    bound = torch.from_numpy(b["mean"]).to(DEV)[cluster]                         # un-pooling is exact: the mean's bound, per point
    err = (up.detach().double() - up64.detach()).abs()
    # the fp64 composition itself: index_add_ in fp64, (cnt + 1) * 2^-53 of the magnitudes -- 2^-29 of the fp32 bound
    assert bool((err <= bound * (1 + 2.0 ** -20)).all()), float((err / bound).max())
    # gradient: dx[i] = (sum over i's cell of w) / cnt: the ordered fp32 sum of L terms (L * 2^-24 * sum |w|), then one quotient
    bw = R.bounds(w.cpu().numpy(), e["cptr"], e["members"])
    gbound = torch.from_numpy(bw["mean"]).to(DEV)[cluster]
    gerr = (x.grad.double() - x64.grad).abs()
    assert bool((gerr <= gbound * (1 + 2.0 ** -20)).all()), float((gerr / gbound).max())
    print(f"\ncomposition: worst fraction of the bound: forward {float((err / bound).max()):.3f}, gradient {float((gerr / gbound).max()):.3f}")


def test_a_captured_lists_pool_backward_replays_on_data_written_in_place():
    from deltaconv_amd import geometry as G
    a, b = C.BY_NAME["random_3000_200_c130"], C.BY_NAME["ids_without_a_cell"]
    n, m, ch = 3000, 200, 130
    pad = lambda c: (np.concatenate([c["cluster"], np.full(n - c["cluster"].size, -1)]),
                     np.random.default_rng(5).standard_normal((n, ch)).astype(np.float32))
    cluster, x, g = dev(a["cluster"]).clone(), dev(a["x"]).clone(), dev(a["g"]).clone()

    def step():
        cptr, members = G.cluster_lists(cluster, m)
        out, arg = G.cluster_pool_rows(x, cptr, members, "max")
        mean = G.cluster_pool_rows(x, cptr, members, "mean")[0]
        return out, arg, mean, G.cluster_pool_rows_backward(g, cluster, cptr, arg, "max"), \
            G.cluster_pool_rows_backward(g, cluster, cptr, None, "mean")

    step()                                                                       # warm: the library is loaded, the allocator has blocks
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    graph.replay()
    e = C.expected("random_3000_200_c130")
    assert same(held[0], e["out", "max"]) and same(held[3], e["dx", "max"]) and same(held[4], e["dx", "mean"])
    new_cluster, new_x = pad(b)
    cluster.copy_(torch.from_numpy(new_cluster))
    x.copy_(torch.from_numpy(new_x))
    graph.replay()
    eager = step()
    assert all(torch.equal(p, q) for p, q in zip(held, eager))
    cptr, members = R.lists(new_cluster, m)
    assert same(held[0], R.pool(new_x, cptr, members, "max")[0]) and same(held[2], R.pool(new_x, cptr, members, "mean")[0])


def test_voxel_subsample_then_cluster_pool_equals_pooling_by_the_restated_clusters():
    from deltaconv_amd import geometry as G
    from tests import voxel_cases as V
    from tests import voxel_restate as VR
    clouds = [V.uniform(70, 2000), V.uniform(71, 2000)]
    pos = torch.from_numpy(np.concatenate(clouds)).to(DEV)
    ptr = torch.tensor([0, 2000, 4000], device=DEV)
    rows, optr, cluster = G.voxel_subsample(pos, 0.1, ptr=ptr)
    want_rows, _, want_cluster, _ = VR.batch(clouds, 0.1)
    assert same(rows, want_rows) and same(cluster, want_cluster)
    x = np.random.default_rng(72).standard_normal((4000, 6)).astype(np.float32)
    cptr, members = R.lists(want_cluster, want_rows.size)
    for r in C.REDUCES:
        assert same(G.cluster_pool(torch.from_numpy(x).to(DEV), cluster, rows.numel(), r), R.pool(x, cptr, members, r)[0]), r
    assert same(G.cluster_mean_pos(pos, *G.cluster_lists(cluster, rows.numel())), R.mean3(np.concatenate(clouds), want_cluster, want_rows.size))


# ---- the store ----------------------------------------------------------------------------------------------------------------------------
SIZES = (700, 1, 1300, 400)


@pytest.fixture(scope="module")
def parent():
    from deltaconv_amd.loader import DeviceDataset
    from tests import voxel_cases as V
    n = sum(SIZES)
    g = torch.Generator().manual_seed(5)
    pos = torch.from_numpy(np.concatenate([V.uniform(60 + i, s) for i, s in enumerate(SIZES)]))
    pos[-3:] = 5.0                                                              # three coincident points far off: a cell of their own ...
    norm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    norm[-3:] = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.0]])      # ... whose normals cancel
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(SIZES)]), dtype=torch.int64)
    return DeviceDataset(pos.to(DEV), ptr.to(DEV), SIZES, norm.to(DEV), torch.randn(n, 5, generator=g).to(DEV),
                         torch.randint(0, 7, (n,), generator=g).to(DEV), None, torch.randn(len(SIZES), 4, generator=g).to(DEV))


def test_the_default_store_did_not_move(parent):
    from deltaconv_amd.geometry import voxel_subsample
    rows, optr, cluster = voxel_subsample(parent.pos, 0.2, ptr=parent.ptr)
    for sub in (parent.voxel_subsample(0.2), parent.voxel_subsample(0.2, reduce=None)):
        assert torch.equal(sub.source_rows, rows) and torch.equal(sub.ptr, optr) and torch.equal(sub.cluster, cluster)
        for name in ("pos", "norm", "x", "y_point"):
            assert torch.equal(getattr(sub, name), getattr(parent, name)[rows]), name
        assert sub.y_cloud is None and sub.category is parent.category and sub.sizes.tolist() == (optr[1:] - optr[:-1]).tolist()


def test_the_mean_store_is_assembled_from_the_tensor_level_calls(parent):
    from deltaconv_amd import geometry as G
    from deltaconv_amd.loader import DeviceDataset, DeviceLoader
    from deltaconv_amd.propagate import Propagator
    plain, sub = parent.voxel_subsample(0.2), parent.voxel_subsample(0.2, reduce="mean")
    assert torch.equal(sub.source_rows, plain.source_rows) and torch.equal(sub.cluster, plain.cluster) and torch.equal(sub.ptr, plain.ptr)
    assert np.array_equal(sub.sizes, plain.sizes)
    rows, cluster = sub.source_rows, sub.cluster
    cptr, members = G.cluster_lists(cluster, rows.numel())
    assert torch.equal(sub.pos, G.cluster_mean_pos(parent.pos, cptr, members))
    mean_normal = G.cluster_mean_pos(parent.norm, cptr, members, normalize=True)
    cancel = int(cluster[-1])                                                   # the cell of the three coincident points
    assert bool((mean_normal[cancel] == 0).all()) and torch.equal(sub.norm[cancel], parent.norm[rows[cancel]])
    keep = torch.ones(rows.numel(), dtype=torch.bool, device=DEV)
    keep[cancel] = False
    assert torch.equal(sub.norm[keep], mean_normal[keep]) and bool(((sub.norm[keep].norm(dim=1) - 1).abs() < 1e-6).all())
    assert torch.equal(sub.x, G.cluster_pool(parent.x, cluster, rows.numel(), "mean"))
    assert torch.equal(sub.y_point, G.cluster_majority(parent.y_point, cptr, members, 7))
    assert torch.equal(sub.y_point, parent.voxel_subsample(0.2, reduce="mean", num_classes=7).y_point)
    assert same(sub.y_point, R.majority(parent.y_point.cpu().numpy(), cluster.cpu().numpy(), rows.numel(), 7))
    assert not torch.equal(sub.pos, plain.pos) and not torch.equal(sub.x, plain.x)
    # a store like any other
    by_hand = DeviceDataset(sub.pos.clone(), sub.ptr.clone(), sub.sizes.copy(), sub.norm.clone(), sub.x.clone(), sub.y_point.clone(),
                            parent.y_cloud, parent.category)
    part = sub.subset([2, 0])
    assert torch.equal(part.pos, by_hand.subset([2, 0]).pos) and part.sizes.tolist() == [int(sub.sizes[2]), int(sub.sizes[0])]
    a, b = next(iter(DeviceLoader(sub, 3))), next(iter(DeviceLoader(by_hand, 3)))
    assert a.pos.shape[0] == int(sub.sizes[:3].sum()) and a.num_graphs == 3
    for name in ("pos", "batch", "norm", "x", "y", "category"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    up = Propagator(sub, parent, k=1).apply(sub.x)
    assert up.shape == (parent.pos.shape[0], 5) and torch.equal(up, Propagator(by_hand, parent, k=1).apply(by_hand.x))


def test_the_argument_errors_raise(parent):
    from deltaconv_amd import geometry as G
    from deltaconv_amd._lib import lib
    c = C.BY_NAME["ids_without_a_cell"]
    cluster, x, g = dev(c["cluster"]), dev(c["x"]), dev(c["g"])
    cptr, members = G.cluster_lists(cluster, c["m"])
    for call in (lambda: G.cluster_lists(cluster.cpu(), 50), lambda: G.cluster_pool(x.cpu(), cluster, 50),
                 lambda: G.cluster_pool(x, cluster.cpu(), 50), lambda: G.cluster_unpool(g.cpu(), cluster),
                 lambda: G.cluster_pool_rows(x, cptr.cpu(), members), lambda: G.cluster_mean_pos(x[:, :3].cpu(), cptr, members),
                 lambda: G.cluster_majority(cluster.cpu(), cptr, members, 3)):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    for call in (lambda: G.cluster_lists(cluster.int(), 50), lambda: G.cluster_lists(cluster[:, None], 50),
                 lambda: G.cluster_pool(x.long(), cluster, 50), lambda: G.cluster_pool(x, cluster[:-1], 50),
                 lambda: G.cluster_mean_pos(x[:, :3].double(), cptr, members), lambda: G.cluster_mean_pos(x, cptr, members),
                 lambda: G.cluster_majority(cluster.int(), cptr, members, 3),
                 lambda: G.cluster_pool_rows_backward(g, cluster, cptr[:-1], None, "sum")):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: G.cluster_lists(cluster, -1), lambda: G.cluster_pool(x[:, :0], cluster, 50),
                 lambda: G.cluster_pool(x, cluster, 50, lists=(cptr[:-1], members)), lambda: G.cluster_pool_rows(x[:-1], cptr, members),
                 lambda: G.cluster_mean_pos(x[:-1, :3].contiguous(), cptr, members),
                 lambda: G.cluster_majority(cluster[:-1], cptr, members, 3)):
        with pytest.raises(ValueError):
            call()
    for bad in ("median", None, 0):
        with pytest.raises(ValueError, match="reduce"):
            G.cluster_pool(x, cluster, 50, reduce=bad)
    for k in (0, -1, 1025):
        with pytest.raises(ValueError, match="num_classes"):
            G.cluster_majority(cluster, cptr, members, k)
    with pytest.raises(ValueError, match="num_classes"):
        parent.voxel_subsample(0.2, reduce="mean", num_classes=2000)
    with pytest.raises(ValueError, match="reduce"):
        parent.voxel_subsample(0.2, reduce="max")
    for call in (lambda: G.cluster_pool(x.clone().requires_grad_(), cluster, 50),
                 lambda: G.cluster_unpool(g.clone().requires_grad_(), cluster)):
        with pytest.raises(RuntimeError, match="requires grad"):
            call()
    with pytest.raises(RuntimeError, match="requires grad"):
        G.cluster_mean_pos(x[:, :3].contiguous().requires_grad_(), cptr, members)
    for r in ("max", "min"):
        with pytest.raises(ValueError, match="arg"):
            G.cluster_pool_rows_backward(g, cluster, cptr, None, r)
    assert G.cluster_majority(cluster, cptr, members, 1024).shape == (50,)
    # the ABI refuses what it is given, before anything touches the device
    out = torch.zeros((50, 4), device=DEV)
    arg = torch.zeros((50, 4), dtype=torch.int32, device=DEV)
    args = lambda **kw: tuple({**dict(x=x.data_ptr(), ldx=4, n=800, C=4, cptr=cptr.data_ptr(), members=members.data_ptr(), m=50, mode=0,
                                     out=out.data_ptr(), ldo=4, arg=arg.data_ptr(), ldarg=4, stream=None), **kw}.values())
    for bad in (dict(n=2 ** 31), dict(m=2 ** 31), dict(n=-1), dict(C=0), dict(mode=4), dict(ldx=3), dict(ldo=3), dict(arg=None),
                dict(ldarg=3), dict(x=None), dict(out=None), dict(cptr=None)):
        assert lib.raw("dc_cluster_pool")(*args(**bad)) == -1 and "dc_cluster_pool" in lib.last_error(), bad
    assert lib.raw("dc_cluster_lists_workspace_bytes")(2 ** 31, 1) == 0 and lib.raw("dc_cluster_lists_workspace_bytes")(-1, 1) == 0
    assert lib.raw("dc_cluster_lists")(cluster.data_ptr(), 800, 50, cptr.data_ptr(), members.data_ptr(), None, 0, None) == -1
    assert lib.raw("dc_cluster_majority")(cluster.data_ptr(), 800, cptr.data_ptr(), members.data_ptr(), 50, 1025, out.data_ptr(), None) == -1
