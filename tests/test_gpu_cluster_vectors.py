"""``geometry.cluster_*_vectors`` and ``ClusterPair`` (csrc/cluster_vectors.hip) on the MI355X.  The device against the numpy
restatement (tests/cluster_vectors_restate.py) on every case of tests/cluster_vectors_cases.py by ``torch.equal`` on the bits --
both tables, the pooling with ``arg``, its backward, the un-pooling and its backward -- and a second run against the first; the
autograd nodes through ``backward()``; lists + tables + both directions + their backwards captured in one graph and replayed on
data written in place; ``ClusterPair`` against the tensor-level calls; ``voxel_subsample`` -> ``ClusterPair`` end to end; the
argument errors."""
import numpy as np
import pytest
import torch

from tests import cluster_vectors_cases as C
from tests import cluster_vectors_restate as R
from tests import connection_restate as CR

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


def frames(fr):
    return tuple(dev(np.ascontiguousarray(a)) for a in fr)


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
    cluster, v, g = dev(c["cluster"]), dev(c["v"]), dev(c["g"])
    fine, coarse = frames(c["fine"]), frames(c["coarse"])
    cptr, members = G.cluster_lists(cluster, c["m"])
    res = {"r" + d: G.cluster_rotation(cluster, c["m"], fine, coarse, d, c["non_oriented"]) for d in ("down", "up")}
    for r in C.REDUCES:
        res["fwd", r] = G.cluster_pool_vectors_rows(v, cptr, members, res["rdown"], r)
        res["dv", r] = G.cluster_pool_vectors_rows_backward(g, cluster, cptr, res["rdown"], res["fwd", r][1], r)
    res["up"] = G.cluster_unpool_vectors_rows(g, cluster, res["rup"])
    res["dup"] = G.cluster_unpool_vectors_rows_backward(v, cptr, members, res["rup"])
    return res


def flat(res):
    return [t for v in res.values() for t in (v if isinstance(v, tuple) else (v,)) if t is not None]


@pytest.mark.parametrize("name", C.NAMES)
def test_device_equals_the_restatement_and_a_second_run(name):
    c, e = C.BY_NAME[name], C.expected(name)
    res = run_case(name)
    if not (c["v"].flags["C_CONTIGUOUS"] or c["v"].size == 0):
        assert not dev(c["v"]).is_contiguous()                                  # the strided view reaches the kernel as one
    assert same(res["rdown"], e["rdown"]) and same(res["rup"], e["rup"])
    for r in C.REDUCES:
        assert same(res["fwd", r][0], e["out", r]), r
        assert same(res["fwd", r][1], e["arg", r]), r
        assert same(res["dv", r], e["dv", r]), r
    assert same(res["up"], e["up"]) and same(res["dup"], e["dup"])
    again = flat(run_case(name))
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(flat(res), again))


@pytest.mark.parametrize("reduce", C.REDUCES + ("add",))
@pytest.mark.parametrize("name", ["random_3000_200_c130", "ids_without_a_cell", "strided_view_c3_unaligned"])
def test_the_autograd_nodes_give_the_restated_gradients(name, reduce):
    from deltaconv_amd import geometry as G
    c, e = C.BY_NAME[name], C.expected(name)
    key = "sum" if reduce == "add" else reduce
    cluster, g = dev(c["cluster"]), dev(c["g"])
    fine, coarse = frames(c["fine"]), frames(c["coarse"])
    v = dev(c["v"]).requires_grad_()
    out = G.cluster_pool_vectors(v, cluster, fine, coarse, c["m"], reduce, differentiable=True, non_oriented=c["non_oriented"])
    assert out.requires_grad and same(out.detach(), e["out", key])
    out.backward(g)
    assert same(v.grad, e["dv", key])
    with torch.no_grad():                                                       # M from the coarse frames, from the lists
        assert same(G.cluster_pool_vectors(v, cluster, fine, coarse, reduce=reduce, non_oriented=c["non_oriented"]), e["out", key])
    lists = G.cluster_lists(cluster, c["m"])
    rdown = G.cluster_rotation(cluster, c["m"], fine, coarse, "down", c["non_oriented"])
    assert same(G.cluster_pool_vectors(v.detach(), cluster, reduce=reduce, lists=lists, rotation=rdown), e["out", key])
    if reduce == "sum":                                                         # the un-pooling, its backward fed the [2n,C] rows v
        y = g.clone().requires_grad_()
        up = G.cluster_unpool_vectors(y, cluster, fine, coarse, differentiable=True, non_oriented=c["non_oriented"])
        assert up.requires_grad and same(up.detach(), e["up"])
        up.backward(v.detach())
        assert same(y.grad, e["dup"])
        y.grad = None
        rup = G.cluster_rotation(cluster, c["m"], fine, coarse, "up", c["non_oriented"])
        G.cluster_unpool_vectors(y, cluster, lists=lists, rotation=rup, differentiable=True).backward(v.detach())
        assert same(y.grad, e["dup"])
        assert same(G.cluster_unpool_vectors(y.detach(), cluster, rotation=rup), e["up"])


def test_what_is_not_differentiable_raises():
    from deltaconv_amd import geometry as G
    c = C.BY_NAME["ids_without_a_cell"]
    cluster, v, g = dev(c["cluster"]), dev(c["v"]), dev(c["g"])
    fine, coarse = frames(c["fine"]), frames(c["coarse"])
    for call in (lambda: G.cluster_pool_vectors(v.clone().requires_grad_(), cluster, fine, coarse, c["m"]),
                 lambda: G.cluster_unpool_vectors(g.clone().requires_grad_(), cluster, fine, coarse)):
        with pytest.raises(RuntimeError, match="requires grad"):
            call()
    for i in range(3):
        hot = tuple(t.clone().requires_grad_() if j == i else t for j, t in enumerate(fine))
        for call in (lambda: G.cluster_rotation(cluster, c["m"], hot, coarse), lambda: G.cluster_rotation(cluster, c["m"], hot, coarse, "up"),
                     lambda: G.cluster_pool_vectors(v, cluster, hot, coarse, c["m"], differentiable=True),
                     lambda: G.ClusterPair(cluster, c["m"], hot, coarse)):
            with pytest.raises(RuntimeError, match="requires grad"):
                call()
    hot = (coarse[0].clone().requires_grad_(),) + coarse[1:]
    with pytest.raises(RuntimeError, match="requires grad"):
        G.cluster_unpool_vectors(g, cluster, fine, hot, differentiable=True)
    with torch.no_grad():                                                       # grad mode off: nothing to cut
        assert G.cluster_rotation(cluster, c["m"], fine, hot).shape == (800, 4)


def test_a_captured_pair_replays_on_data_written_in_place():
    from deltaconv_amd import geometry as G
    a, b = C.BY_NAME["random_3000_200_c130"], C.BY_NAME["ids_without_a_cell"]
    n, m, ch = 3000, 200, 130
    rng = np.random.default_rng(5)
    cluster, v, g = dev(a["cluster"]).clone(), dev(a["v"]).clone(), dev(a["g"]).clone()
    fine, coarse = tuple(t.clone() for t in frames(a["fine"])), tuple(t.clone() for t in frames(a["coarse"]))

    def step():
        pair = G.ClusterPair(cluster, m, fine, coarse).prepare()
        vin, xin = v.detach().requires_grad_(), g.detach().requires_grad_()
        down, up = pair.down_vectors(vin, "max"), pair.up_vectors(xin)
        mean = pair.down_vectors(vin, "mean")
        dv, = torch.autograd.grad(down, vin, g)
        dmean, = torch.autograd.grad(mean, vin, g)
        dx, = torch.autograd.grad(up, xin, v)
        return (*pair.lists(), pair.rotation("down"), pair.rotation("up"), down.detach(), mean.detach(), up.detach(), dv, dmean, dx)

    step()                                                                       # warm: the library is loaded, the allocator has blocks
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    graph.replay()
    e = C.expected("random_3000_200_c130")
    for t, key in zip(held, ("cptr", "members", "rdown", "rup", ("out", "max"), ("out", "mean"), "up", ("dv", "max"), ("dv", "mean"), "dup")):
        assert same(t, e[key]), key
    new_cluster = np.concatenate([b["cluster"], np.full(n - b["cluster"].size, -1)])
    new_v = rng.standard_normal((2 * n, ch)).astype(np.float32)
    new_fine, new_coarse = C.random_frames(n, rng), C.random_frames(m, rng)
    cluster.copy_(torch.from_numpy(new_cluster))
    v.copy_(torch.from_numpy(new_v))
    for t, w in zip(fine + coarse, new_fine + new_coarse):
        t.copy_(torch.from_numpy(w))
    graph.replay()
    eager = step()
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    assert all(torch.equal(bits(p), bits(q)) for p, q in zip(held, eager))
    cptr, members = R.CL.lists(new_cluster, m)
    rdown, rup = (R.table(new_cluster, m, new_fine, new_coarse, d) for d in ("down", "up"))
    out, arg = R.pool(new_v, cptr, members, rdown, "max")
    assert same(held[2], rdown) and same(held[3], rup) and same(held[4], out)
    assert same(held[5], R.pool(new_v, cptr, members, rdown, "mean")[0]) and same(held[6], R.unpool(a["g"], new_cluster, rup))
    assert same(held[7], R.pool_backward(a["g"], new_cluster, cptr, rdown, arg, "max"))
    assert same(held[9], R.unpool_backward(new_v, cptr, members, rup))


def test_the_pair_equals_the_tensor_level_calls():
    from deltaconv_amd import geometry as G
    c, e = C.BY_NAME["random_3000_200_c130"], C.expected("random_3000_200_c130")
    cluster, v, g = dev(c["cluster"]), dev(c["v"]), dev(c["g"])
    fine, coarse = frames(c["fine"]), frames(c["coarse"])
    pair = G.ClusterPair(cluster, c["m"], fine, coarse)
    assert pair.lists() is pair.lists() and pair.rotation("down") is pair.rotation("down")         # built once
    assert same(pair.lists()[0], e["cptr"]) and same(pair.rotation("down"), e["rdown"]) and same(pair.rotation("up"), e["rup"])
    for r in C.REDUCES:
        assert torch.equal(pair.down_vectors(v, r), G.cluster_pool_vectors(v, cluster, fine, coarse, c["m"], r))
        vin = v.clone().requires_grad_()
        out = pair.down_vectors(vin, r)
        assert out.requires_grad and same(out.detach(), e["out", r])
        out.backward(g)
        assert same(vin.grad, e["dv", r])
    assert torch.equal(pair.up_vectors(g), G.cluster_unpool_vectors(g, cluster, fine, coarse)) and same(pair.up_vectors(g), e["up"])
    xin = g.clone().requires_grad_()
    pair.up_vectors(xin).backward(v)
    assert same(xin.grad, e["dup"])
    # the scalar stream is cluster_pool / cluster_unpool
    x, gx = v[: v.shape[0] // 2], g[: g.shape[0] // 2]
    for r in ("max", "min", "sum", "mean"):
        assert torch.equal(pair.down(x, r), G.cluster_pool(x, cluster, c["m"], r))
    assert torch.equal(pair.up(gx), G.cluster_unpool(gx, cluster))
    xin = x.clone().requires_grad_()
    pair.down(xin, "mean").backward(gx)
    want = x.clone().requires_grad_()
    G.cluster_pool(want, cluster, c["m"], "mean", differentiable=True).backward(gx)
    assert torch.equal(xin.grad, want.grad)
    yin, want = gx.clone().requires_grad_(), gx.clone().requires_grad_()
    pair.up(yin).backward(x)
    G.cluster_unpool(want, cluster, differentiable=True).backward(x)
    assert torch.equal(yin.grad, want.grad)
    # differentiable=False: nothing is recorded, the inference bits come back
    frozen = G.ClusterPair(cluster, c["m"], fine, coarse, differentiable=False)
    out = frozen.down_vectors(v.clone().requires_grad_(), "max")
    assert not out.requires_grad and same(out, e["out", "max"]) and not frozen.up_vectors(g.clone().requires_grad_()).requires_grad
    assert not frozen.down(x.clone().requires_grad_()).requires_grad and not frozen.up(gx.clone().requires_grad_()).requires_grad


def test_voxel_subsample_then_a_pair_on_a_sphere_like_cloud():
    from deltaconv_amd import geometry as G
    pos, nrm, xb, yb = CR.cloud(2000, 9)
    fine = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (nrm, xb, yb))
    rows, optr, cluster = G.voxel_subsample(torch.from_numpy(pos).to(DEV), 0.25)
    m = rows.numel()
    assert 1 < m < 2000 and torch.equal(cluster[rows], torch.arange(m, device=DEV))
    pair = G.ClusterPair(cluster, m, fine, tuple(t[rows] for t in fine)).prepare()
    ident = torch.tensor([1.0, -0.0, 0.0, 1.0], device=DEV).view(torch.int32)
    for d in ("down", "up"):                                                    # every representative sees its own frame
        assert bool((pair.rotation(d)[rows].view(torch.int32) == ident[None, :]).all()), d
    cl = cluster.cpu().numpy()
    fr = (nrm, xb, yb)
    coarse = tuple(a[rows.cpu().numpy()] for a in fr)
    assert same(pair.rotation("down"), R.table(cl, m, fr, coarse, "down")) and same(pair.rotation("up"), R.table(cl, m, fr, coarse, "up"))
    # vectors that live on the representatives alone come down unchanged, row j of the result belonging to rows[j]
    v = torch.zeros(4000, 3, device=DEV)
    own = torch.randn(2 * m, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    v[2 * rows], v[2 * rows + 1] = own[0::2], own[1::2]
    assert torch.equal(pair.down_vectors(v, "sum"), own) and torch.equal(pair.down_vectors(v, "max"), own)
    up = pair.up_vectors(own)
    assert torch.equal(up[2 * rows], own[0::2]) and torch.equal(up[2 * rows + 1], own[1::2])
    w = np.random.default_rng(4).standard_normal((4000, 3)).astype(np.float32)
    cptr, members = R.CL.lists(cl, m)
    assert same(pair.down_vectors(torch.from_numpy(w).to(DEV), "mean"), R.pool(w, cptr, members, R.table(cl, m, fr, coarse, "down"), "mean")[0])


def test_the_argument_errors_raise():
    from deltaconv_amd import geometry as G
    from deltaconv_amd._lib import lib
    c = C.BY_NAME["ids_without_a_cell"]
    n, m = 800, 50
    cluster, v, g = dev(c["cluster"]), dev(c["v"]), dev(c["g"])
    fine, coarse = frames(c["fine"]), frames(c["coarse"])
    cptr, members = G.cluster_lists(cluster, m)
    rdown, rup = (G.cluster_rotation(cluster, m, fine, coarse, d) for d in ("down", "up"))
    out, arg = G.cluster_pool_vectors_rows(v, cptr, members, rdown, "max")
    for call in (lambda: G.cluster_rotation(cluster.cpu(), m, fine, coarse), lambda: G.cluster_pool_vectors(v.cpu(), cluster, fine, coarse, m),
                 lambda: G.cluster_pool_vectors(v, cluster.cpu(), fine, coarse, m), lambda: G.cluster_unpool_vectors(g.cpu(), cluster, fine, coarse),
                 lambda: G.cluster_pool_vectors_rows(v, cptr.cpu(), members, rdown), lambda: G.cluster_pool_vectors_rows(v, cptr, members, rdown.cpu()),
                 lambda: G.cluster_unpool_vectors_rows(g, cluster, rup.cpu()), lambda: G.ClusterPair(cluster.cpu(), m)):
        with pytest.raises(ValueError, match="HIP device"):
            call()
    with pytest.raises(RuntimeError, match="HIP device"):                       # a frame off the device
        G.cluster_rotation(cluster, m, (fine[0].cpu(),) + fine[1:], coarse)
    for call in (lambda: G.cluster_rotation(cluster.int(), m, fine, coarse), lambda: G.cluster_pool_vectors(v.long(), cluster, fine, coarse, m),
                 lambda: G.cluster_pool_vectors(v, cluster[:-1], fine, coarse, m),
                 lambda: G.cluster_pool_vectors_rows_backward(g, cluster, cptr[:-1], rdown, None, "sum")):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: G.cluster_rotation(cluster, -1, fine, coarse), lambda: G.cluster_rotation(cluster, m, fine, coarse, "sideways"),
                 lambda: G.cluster_rotation(cluster, m, fine[:2], coarse, "up"), lambda: G.cluster_rotation(cluster, m, fine, coarse[:2], "down"),
                 lambda: G.cluster_rotation(cluster, m, tuple(t[:-1] for t in fine), coarse),          # frames of the wrong length
                 lambda: G.cluster_rotation(cluster, m + 1, fine, coarse), lambda: G.cluster_rotation(cluster, m, None, coarse),
                 lambda: G.cluster_pool_vectors(v[:-1], cluster, fine, coarse, m), lambda: G.cluster_pool_vectors(v[:, :0], cluster, fine, coarse, m),
                 lambda: G.cluster_pool_vectors(v, cluster, fine, coarse, m, lists=(cptr[:-1], members)),   # lists that do not belong
                 lambda: G.cluster_pool_vectors(v, cluster, fine, coarse, m, lists=(cptr, members[:-1])),
                 lambda: G.cluster_unpool_vectors(g.clone().requires_grad_(), cluster, fine, coarse, lists=(cptr[:-1], members), differentiable=True),
                 lambda: G.cluster_pool_vectors_rows(v[:-2], cptr, members, rdown), lambda: G.cluster_pool_vectors_rows(v, cptr, members, rdown[:-1]),
                 lambda: G.cluster_pool_vectors_rows(v, cptr, members, rdown.double()),
                 lambda: G.cluster_pool_vectors_rows_backward(g, cluster, cptr, rdown, arg.long(), "max"),
                 lambda: G.cluster_unpool_vectors_rows(g, cluster, rup[:, :3]), lambda: G.cluster_unpool_vectors_rows_backward(v[:-2], cptr, members, rup),
                 lambda: G.ClusterPair(cluster, m, fine[:2], coarse), lambda: G.ClusterPair(cluster, m, fine, tuple(t[:-1] for t in coarse))):
        with pytest.raises(ValueError):
            call()
    assert G.cluster_rotation(cluster, m, fine[:2], coarse, "down").shape == (n, 4)      # the source side needs no y-axis
    for bad in ("min", "median", None, 1):
        for call in (lambda: G.cluster_pool_vectors(v, cluster, fine, coarse, m, reduce=bad),
                     lambda: G.cluster_pool_vectors_rows(v, cptr, members, rdown, bad),
                     lambda: G.ClusterPair(cluster, m, fine, coarse).down_vectors(v, bad)):
            with pytest.raises(ValueError, match="reduce"):
                call()
    with pytest.raises(ValueError, match="arg"):
        G.cluster_pool_vectors_rows_backward(g, cluster, cptr, rdown, None, "max")
    bare = G.ClusterPair(cluster, m)
    for call in (lambda: bare.down_vectors(v), lambda: bare.up_vectors(g), lambda: bare.rotation("down")):
        with pytest.raises(ValueError, match="without frames"):
            call()
    assert torch.equal(bare.prepare().down(v[:n]), G.cluster_pool(v[:n], cluster, m))   # the scalar stream needs none
    with pytest.raises(ValueError):
        G.ClusterPair(cluster, m, fine, coarse).up_vectors(g[:-2])
    # the ABI refuses what it is given, before anything touches the device
    out = torch.zeros((2 * m, 4), device=DEV)
    args = lambda **kw: tuple({**dict(v=v.data_ptr(), ldv=4, n=n, C=4, cptr=cptr.data_ptr(), members=members.data_ptr(), m=m,
                                     rmat=rdown.data_ptr(), mode=0, out=out.data_ptr(), ldo=4, arg=arg.data_ptr(), ldarg=4, stream=None),
                                 **kw}.values())
    for bad in (dict(n=2 ** 31), dict(m=2 ** 31), dict(n=-1), dict(C=0), dict(mode=1), dict(mode=4), dict(ldv=3), dict(ldo=3), dict(arg=None),
                dict(ldarg=3), dict(v=None), dict(out=None), dict(cptr=None), dict(rmat=None), dict(rmat=rdown.data_ptr() + 4)):
        assert lib.raw("dc_cluster_pool_vectors")(*args(**bad)) == -1 and "dc_cluster_pool_vectors" in lib.last_error(), bad
    assert lib.raw("dc_cluster_pool_vectors")(*args(m=0)) == 0 and lib.raw("dc_cluster_pool_vectors")(*args(n=0, mode=2, arg=None)) == 0
    rot = lambda **kw: tuple({**dict(cluster=cluster.data_ptr(), n=n, m=m, fn=fine[0].data_ptr(), fx=fine[1].data_ptr(), fy=fine[2].data_ptr(),
                                    cn=coarse[0].data_ptr(), cx=coarse[1].data_ptr(), cy=coarse[2].data_ptr(), to_cell=1, non_oriented=1,
                                    rmat=rdown.data_ptr(), stream=None), **kw}.values())
    for bad in (dict(to_cell=2), dict(cy=None), dict(to_cell=0, fy=None), dict(cluster=None), dict(rmat=None), dict(n=2 ** 31), dict(m=-1)):
        assert lib.raw("dc_cluster_rotation")(*rot(**bad)) == -1 and "dc_cluster_rotation" in lib.last_error(), bad
    assert lib.raw("dc_cluster_rotation")(*rot(n=0)) == 0
    assert lib.raw("dc_cluster_pool_vectors_backward")(g.data_ptr(), 4, m, 4, cluster.data_ptr(), n, None, rdown.data_ptr(), None, 0, 3,
                                                       v.data_ptr(), 4, None) == -1 and "cptr" in lib.last_error()
    assert lib.raw("dc_cluster_unpool_vectors")(g.data_ptr(), 3, m, 4, cluster.data_ptr(), n, rup.data_ptr(), v.data_ptr(), 4, None) == -1
    assert lib.raw("dc_cluster_unpool_vectors_backward")(v.data_ptr(), 4, n, 4, cptr.data_ptr(), None, m, rup.data_ptr(), out.data_ptr(), 4,
                                                         None) == -1
    torch.cuda.synchronize()
    assert same(G.cluster_pool_vectors_rows(v, cptr, members, rdown, "max")[0], C.expected("ids_without_a_cell")["out", "max"])
