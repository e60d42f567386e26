"""The exact grid search on the MI355X (csrc/knn_grid.hip: ``dc_knn_grid``, ``dc_knn_cross_grid``; ``Graph.knn(method="grid")``,
``geometry.knn_cross(method="grid")``, ``CloudPair(search_method="grid")``, the ``KNN_METHOD`` switch): the brute-force kernels are
its complete oracle.  Every comparison is ``torch.equal`` on the index tables and on the bits of ``d2``; there is no tolerance in
this change.  The cases (tests/knn_grid_cases.py) are the smallest shapes at which each mechanism can fail, each at the default
grid target, at one cell (1e9) and at the cell cap (0.25)."""
import pytest
import torch

from tests import knn_grid_cases as C
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
GEOM = ["geom_normals_B2_N128_k20", "geom_ragged_dups_k30", "geom_nonormals_N200_k10"]
_brute = {}


def batch_of(sizes):
    return torch.arange(len(sizes)).repeat_interleave(torch.tensor(sizes)).to(DEV)


def ptr64(sizes):
    return torch.from_numpy(C.ptr_of(sizes)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def brute_self(name):
    from deltaconv_amd.geometry import Graph
    if name not in _brute:
        pos, sizes, k = C.SELF[name]()
        _brute[name] = Graph.knn(pos.to(DEV), k, batch_of(sizes), method="brute").nbr
    return _brute[name]


def cross_case(name):
    return C.self_as_cross(name[5:]) if name.startswith("self:") else C.CROSS[name]()


def brute_cross(name):
    from deltaconv_amd.geometry import knn_cross
    if name not in _brute:
        qry, qsizes, ref, rsizes, k = cross_case(name)
        _brute[name] = knn_cross(qry.to(DEV), ref.to(DEV), k, ptr_query=ptr64(qsizes), ptr_ref=ptr64(rsizes), method="brute")
    return _brute[name]


@pytest.mark.parametrize("target", C.TARGETS)
@pytest.mark.parametrize("name", list(C.SELF))
def test_graph_knn_grid_equals_brute(name, target):
    from deltaconv_amd.geometry import Graph
    pos, sizes, k = C.SELF[name]()
    want = brute_self(name)
    got = Graph.knn(pos.to(DEV), k, batch_of(sizes), method="grid", grid_target=target)
    assert got.nbr.dtype == torch.int32 and got.nbr.shape == want.shape
    bad = (got.nbr != want).any(1).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} rows differ, first {bad[:3].tolist()}: {got.nbr[bad[:1]].tolist()} vs {want[bad[:1]].tolist()}"
    assert torch.equal(got.nbr, want) and got.pos is not None and got.max_cloud == max(sizes)


@pytest.mark.parametrize("target", C.TARGETS)
@pytest.mark.parametrize("name", list(C.CROSS) + ["self:" + n for n in C.SELF])
def test_knn_cross_grid_equals_brute(name, target):
    from deltaconv_amd.geometry import knn_cross
    qry, qsizes, ref, rsizes, k = cross_case(name)
    widx, wd2 = brute_cross(name)
    idx, d2 = knn_cross(qry.to(DEV), ref.to(DEV), k, ptr_query=ptr64(qsizes), ptr_ref=ptr64(rsizes), method="grid", grid_target=target)
    assert torch.equal(idx, widx), f"{int((idx != widx).any(1).sum())} rows differ"
    assert torch.equal(bits(d2), bits(wd2))
    bad = ~torch.isfinite(qry).all(1).to(DEV)
    assert bool((idx[bad] == -1).all()) and bool(torch.isinf(d2[bad]).all())


def test_knn_cross_grid_offsets_that_are_a_slice_and_batch_vectors():
    """Absolute offsets that do not start at row 0 (a slice of a store's), and the ``batch_*`` form."""
    from deltaconv_amd.geometry import knn_cross
    qry, qsizes, ref, rsizes, k = C.CROSS["outside_k3"]()
    qp, rp = ptr64(qsizes), ptr64(rsizes)
    widx, wd2 = brute_cross("outside_k3")
    idx, d2 = knn_cross(qry.to(DEV), ref.to(DEV), k, ptr_query=qp[1:], ptr_ref=rp[1:], method="grid")
    lo = int(qp[1])
    assert torch.equal(idx[lo:], widx[lo:]) and torch.equal(bits(d2[lo:]), bits(wd2[lo:]))
    assert bool((idx[:lo] == -1).all()) and bool(torch.isinf(d2[:lo]).all())     # rows outside every pair keep the fill
    idx, d2 = knn_cross(qry.to(DEV), ref.to(DEV), k, batch_query=batch_of(qsizes), batch_ref=batch_of(rsizes), method="grid")
    assert torch.equal(idx, widx) and torch.equal(bits(d2), bits(wd2))
    with pytest.raises(ValueError, match="query clouds but"):                   # differing cloud counts
        knn_cross(qry.to(DEV), ref.to(DEV), k, ptr_query=qp, ptr_ref=rp[:-1], method="grid")


@pytest.mark.parametrize("name", GEOM)
def test_golden_fixtures_through_the_grid(name):
    from deltaconv_amd.geometry import Graph
    g = load_golden(name)
    gr = Graph.knn(g["pos"].to(DEV), g["k"], g["batch"].to(DEV), method="grid")
    assert torch.equal(gr.edge_index.cpu(), g["edge_index"])


def test_switch_and_keyword_rules():
    from deltaconv_amd.geometry import Graph, graph, knn_cross
    pos, sizes, k = C.SELF["whole_2x40_k40"]()
    dpos, batch = pos.to(DEV), batch_of(sizes)
    assert graph.KNN_METHOD[0] in graph.KNN_METHODS
    with pytest.raises(ValueError, match="lanes_per_query"):
        Graph.knn(dpos, k, batch, lanes_per_query=8, method="grid")
    with pytest.raises(ValueError, match="method"):
        Graph.knn(dpos, k, batch, method="tree")
    with pytest.raises(ValueError, match="method"):
        knn_cross(dpos, dpos, 3, method="tree")
    with pytest.raises(ValueError, match="at least k"):
        Graph.knn(dpos, 41, batch, method="grid")
    old = graph.KNN_METHOD[0]
    try:
        graph.KNN_METHOD[0] = "grid"
        with pytest.raises(ValueError, match="lanes_per_query"):                # None reads the switch
            Graph.knn(dpos, k, batch, lanes_per_query=8)
        assert torch.equal(Graph.knn(dpos, k, batch).nbr, brute_self("whole_2x40_k40"))
        assert torch.equal(Graph.knn(dpos, k, batch, lanes_per_query=8, method="brute").nbr, brute_self("whole_2x40_k40"))
    finally:
        graph.KNN_METHOD[0] = old


def test_capture_and_replay_on_new_positions():
    """The whole call inside a ``torch.cuda.graph``; replayed on a second cloud written in place (another box, other cells)."""
    from deltaconv_amd.geometry.graph import Graph, PtrInfo
    pos, sizes, k = C.SELF["ragged_64_1000_257_k20"]()
    n = pos.shape[0]
    gen = torch.Generator().manual_seed(44)
    second = (torch.randn(n, 3, generator=gen) * torch.tensor([3.0, 0.5, 1.0]) + 7.0).to(DEV)
    info = PtrInfo(torch.from_numpy(C.ptr_of(sizes)).to(torch.int32).to(DEV), len(sizes), max(sizes), min(sizes))
    static = pos.to(DEV).clone()
    Graph.knn(static, k, ptr_info=info, method="grid")                           # (library load and allocator warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = Graph.knn(static, k, ptr_info=info, method="grid").nbr
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, brute_self("ragged_64_1000_257_k20"))
    static.copy_(second)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, Graph.knn(second, k, ptr_info=info, method="brute").nbr)


def test_model_step_is_bitwise_the_same_with_the_switch_on():
    import deltaconv_amd as dc
    from deltaconv_amd.data import synthetic_batch
    from deltaconv_amd.geometry import graph
    from deltaconv_amd.utils import calc_loss
    b = synthetic_batch(2, 256, seed=1).to(DEV)
    torch.manual_seed(1)
    model = dc.models.DeltaNetClassification(3, 40, num_neighbors=20).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    state = {key: v.clone() for key, v in model.state_dict().items()}

    def step():
        model.load_state_dict(state)                                            # (the BatchNorm running statistics too)
        model.zero_grad(set_to_none=True)
        logits = model(b)
        calc_loss(logits, b.y).backward()
        return logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    old = graph.KNN_METHOD[0]
    try:
        graph.KNN_METHOD[0] = "brute"
        logits, grads = step()
        graph.KNN_METHOD[0] = "grid"
        glogits, ggrads = step()
    finally:
        graph.KNN_METHOD[0] = old
    assert torch.equal(logits, glogits) and grads.keys() == ggrads.keys() and len(grads) > 0
    for name in grads:
        assert torch.equal(grads[name], ggrads[name]), name


def test_cloud_pair_search_method():
    from deltaconv_amd.geometry import CloudPair
    pos, sizes, _ = C.SELF["ragged_64_1000_257_k20"]()
    fptr = C.ptr_of(sizes)
    keep = torch.cat([torch.arange(fptr[b], fptr[b + 1], 4) for b in range(len(sizes))])
    csizes = [len(range(0, s, 4)) for s in sizes]
    fine, coarse = pos.to(DEV), pos[keep].contiguous().to(DEV)
    kw = dict(k_down=16, k_up=3, max_fine_cloud=max(sizes), max_coarse_cloud=max(csizes))
    a = CloudPair(fine, coarse, ptr64(sizes), ptr64(csizes), **kw)
    b = CloudPair(fine, coarse, ptr64(sizes), ptr64(csizes), search_method="grid", **kw)
    gen = torch.Generator().manual_seed(2)
    xf, xc = torch.randn(fine.shape[0], 12, generator=gen).to(DEV), torch.randn(coarse.shape[0], 12, generator=gen).to(DEV)
    for direction in ("down", "up"):
        (ia, da), (ib, db) = a.search(direction), b.search(direction)
        assert torch.equal(ia, ib) and torch.equal(bits(da), bits(db))
    assert torch.equal(bits(a.down(xf)), bits(b.down(xf))) and torch.equal(bits(a.up(xc)), bits(b.up(xc)))


def test_non_finite_positions_stay_in_bounds():
    """dc_knn's output is meaningless on non-finite positions; the grid form still emits only ids inside the row's cloud, and equals
    brute force on every finite query whose brute-force list holds no non-finite point."""
    from deltaconv_amd.geometry import Graph
    pos, sizes, k = C.SELF["ragged_64_1000_257_k20"]()
    pos = pos.clone()
    ptr = C.ptr_of(sizes)
    poison = [3, 70, 71, 500, 1063, 1064 + 5, 1064 + 256]
    for j, i in enumerate(poison):
        pos[i, j % 3] = (float("nan"), float("inf"), -float("inf"))[j % 3]
    pos[1, :] = float("nan")
    dpos, batch = pos.to(DEV), batch_of(sizes)
    guard = torch.full((pos.shape[0] + 2, k), -12345, dtype=torch.int32, device=DEV)
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import graph
    work, nbytes = graph.grid_workspace(pos.shape[0], len(sizes), DEV)
    cptr = torch.from_numpy(ptr).to(torch.int32).to(DEV)
    lib.call("dc_knn_grid", dpos, cptr, len(sizes), max(sizes), k, 2.0, guard[1:-1], work, nbytes)
    got = guard[1:-1]
    assert bool((guard[0] == -12345).all()) and bool((guard[-1] == -12345).all())
    lo = torch.from_numpy(ptr[:-1]).to(DEV)[batch][:, None]
    hi = torch.from_numpy(ptr[1:]).to(DEV)[batch][:, None]
    assert bool(((got >= lo) & (got < hi)).all())
    finite = torch.isfinite(dpos).all(1)
    own = torch.arange(pos.shape[0], device=DEV, dtype=torch.int32)[:, None].expand(-1, k)
    assert torch.equal(got[~finite], own[~finite])                              # such a point's own row names itself
    assert not bool(torch.isin(got[finite], (~finite).nonzero().flatten().to(torch.int32)).any())
    want = Graph.knn(dpos, k, batch, method="brute").nbr
    ok = (want >= lo) & (want < hi)                                             # (brute force may emit anything on these inputs)
    clean = finite & ok.all(1) & finite[want.clamp(0, pos.shape[0] - 1).long()].all(1)
    assert int(clean.sum()) > 1000 and torch.equal(got[clean], want[clean])


def test_argument_errors():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import graph
    pos, sizes, k = C.SELF["whole_2x40_k40"]()
    n, nc, mx = pos.shape[0], len(sizes), max(sizes)
    dpos = pos.to(DEV)
    cptr = torch.from_numpy(C.ptr_of(sizes)).to(torch.int32).to(DEV)
    nbr = torch.empty(n, k, dtype=torch.int32, device=DEV)
    work, nbytes = graph.grid_workspace(n, nc, DEV)
    assert nbytes == lib.raw("dc_knn_grid_workspace_bytes")(n, nc) > 0 and nbytes <= 64 * n + 64 * nc + 64
    assert lib.raw("dc_knn_grid_workspace_bytes")(-1, 1) == 0 and lib.raw("dc_knn_grid_workspace_bytes")(1, -1) == 0
    assert lib.raw("dc_knn_grid_workspace_bytes")(2 ** 31, 1) == 0
    fn, s = lib.raw("dc_knn_grid"), torch.cuda.current_stream().cuda_stream
    base = dict(pos=dpos.data_ptr(), ptr=cptr.data_ptr(), nc=nc, mx=mx, k=k, t=2.0, nbr=nbr.data_ptr(), w=work.data_ptr(), wb=nbytes)

    def call(**kw):
        a = {**base, **kw}
        return fn(a["pos"], a["ptr"], a["nc"], a["mx"], a["k"], a["t"], a["nbr"], a["w"], a["wb"], s)

    assert call() == 0
    for kw, msg in ((dict(pos=None), "null"), (dict(ptr=None), "null"), (dict(nbr=None), "null"), (dict(w=None), "workspace"),
                    (dict(wb=lib.raw("dc_knn_grid_workspace_bytes")(mx - 1, nc)), "too small"), (dict(wb=0), "too small"),
                    (dict(w=work.data_ptr() + 8), "aligned"), (dict(k=0), "k=0"), (dict(k=65), "k=65"), (dict(t=0.0), "target"),
                    (dict(t=-1.0), "target"), (dict(t=float("inf")), "target"), (dict(t=float("nan")), "target"),
                    (dict(nc=-1), "num_clouds"), (dict(nc=65536), "num_clouds")):
        assert call(**kw) == -1 and msg in lib.last_error() and "dc_knn_grid:" in lib.last_error(), (kw, lib.last_error())
    assert call(nc=0, w=None) == 0 and call(mx=0, w=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(nbr, brute_self("whole_2x40_k40"))

    qptr = torch.from_numpy(C.ptr_of(sizes)).to(DEV)
    idx = torch.empty(n, 16, dtype=torch.int32, device=DEV)
    d2 = torch.empty(n, 16, dtype=torch.float32, device=DEV)
    cfn = lib.raw("dc_knn_cross_grid")
    cbase = dict(q=dpos.data_ptr(), qp=qptr.data_ptr(), r=dpos.data_ptr(), rp=qptr.data_ptr(), B=nc, mq=mx, k=16, t=2.0,
                 idx=idx.data_ptr(), d2=d2.data_ptr(), w=work.data_ptr(), wb=nbytes)

    def ccall(**kw):
        a = {**cbase, **kw}
        return cfn(a["q"], a["qp"], a["r"], a["rp"], a["B"], a["mq"], a["k"], a["t"], a["idx"], a["d2"], a["w"], a["wb"], s)

    assert ccall() == 0
    for kw, msg in ((dict(q=None), "null"), (dict(qp=None), "null"), (dict(r=None), "null"), (dict(rp=None), "null"),
                    (dict(idx=None), "null"), (dict(d2=None), "null"), (dict(w=None), "workspace"), (dict(wb=16), "too small"),
                    (dict(w=work.data_ptr() + 4), "aligned"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(t=0.0), "target"),
                    (dict(t=float("nan")), "target"), (dict(B=-1), "cloud pairs"), (dict(B=65536), "cloud pairs"),
                    (dict(mq=-1), "max_query_cloud")):
        assert ccall(**kw) == -1 and msg in lib.last_error() and "dc_knn_cross_grid:" in lib.last_error(), (kw, lib.last_error())
    assert ccall(B=0, w=None) == 0 and ccall(mq=0, w=None) == 0
    torch.cuda.synchronize()
