"""The backward of the propagation stage on the MI355X (csrc/interp.hip: ``dc_knn_cross_transpose``,
``dc_knn_interpolate_backward``; ``geometry.knn_cross_transpose`` / ``interpolate_rows_backward`` /
``knn_interpolate(differentiable=True)``; ``Propagator(differentiable=True)``) against the numpy restatement of the backward
rules of csrc/interp_math.h (tests/interp_grad_restate.py, itself held to a g++ build of that header and to fp64 by
tests/test_interp_grad_host.py): list offsets, edge ids, coefficients and gradients bit for bit.  The ragged call is the one of
tests/test_gpu_interp.py plus a one-point reference cloud (ONE list of 2 100 entries: past every 64- and 256-wide seam of the
ranking and of the sum, every coefficient 1) and a two-point one (two lists of about 65 k entries with true divisions).

The fp64 bound (tests/test_interp_grad_host.py derives it): |dx - dx64| <= (L_j + k + 8) * 2^-24 * sum_e |c_e| |g_e|."""
import ctypes

import numpy as np
import pytest
import torch

from tests import interp_grad_restate as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype, fill):
    whole = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + n], whole


def guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def restated_dx(k, c):
    if (k, c) not in _cache:
        _cache[k, c] = G.backward(G.ragged_gradient(c), *G.ragged_lists(k), k)
    return _cache[k, c]


def transposed(k):
    """dc_knn_cross_transpose of the restated search of the ragged call into guarded buffers -> (tptr, tedge, tcoef) on the
    device, tedge / tcoef cut to the in-edges."""
    from deltaconv_amd._lib import lib
    _, qptr, _, rptr = G.ragged_clouds()
    idx, d2 = G.ragged_search(k)
    nq, nr = int(qptr[-1]), int(rptr[-1])
    (tptr, pw), (tedge, ew), (tcoef, cw) = guarded(nr + 1, torch.int64, -9), guarded(nq * k, torch.int64, -9), \
        guarded(nq * k, torch.float32, -9.0)
    nbytes = lib.raw("dc_knn_cross_transpose_workspace_bytes")(nq, nr, k)
    assert nbytes >= 8 * (nr + nq * k)
    work, ww = guarded(nbytes // 8, torch.int64, -9)
    lib.call("dc_knn_cross_transpose", dev(qptr), dev(rptr), len(G.PAIRS), nq, nr, k, dev(idx), dev(d2), tptr, tedge, tcoef, work,
             nbytes)
    torch.cuda.synchronize()
    assert guards_intact(pw, nr + 1, -9) and guards_intact(ew, nq * k, -9) and guards_intact(cw, nq * k, -9.0) and \
        guards_intact(ww, nbytes // 8, -9), "guard words around tptr / tedge / tcoef / the workspace were written"
    n = int(tptr[-1])
    assert bool((tedge[n:] == -9).all()) and bool((tcoef[n:] == -9.0).all()), "entries past the last list were written"
    return tptr, tedge[:n], tcoef[:n]


def laid_out(g, vec):
    """g [n,C] on the device with a leading dimension above C: 16-byte aligned rows (vec) or an odd leading dimension on a base
    one float off alignment (the scalar path).  The gaps hold NaN."""
    n, c = g.shape
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    whole = torch.full((n * ld + 8,), float("nan"), device=DEV)
    off = 0 if vec else 1
    view = whole[off:off + n * ld].view(n, ld)[:, :c]
    view.copy_(dev(g))
    assert (view.data_ptr() % 16 == 0) == vec
    return view, ld


def guarded_rows(n, c, vec):
    """-> (out [n,c] view with NaN in it, whole buffer with -9 everywhere else, ld, the mask of the floats of `whole` out covers)."""
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    whole = torch.full((GUARD + n * ld + GUARD,), -9.0, device=DEV)
    start = GUARD if vec else GUARD + 1
    out = whole[start:start + (n - 1) * ld + c].as_strided((n, c), (ld, 1))
    out.fill_(float("nan"))
    touched = np.zeros(whole.numel(), dtype=bool)
    for r in range(n):
        touched[start + r * ld:start + r * ld + c] = True
    assert (out.data_ptr() % 16 == 0) == vec
    return out, whole, ld, touched


# ---- 1. the transposed lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.KS)
def test_transposed_lists_equal_the_restatement_bitwise(k):
    tptr, tedge, tcoef = transposed(k)
    wptr, wedge, wcoef = G.ragged_lists(k)
    assert np.array_equal(tptr.cpu().numpy(), wptr)
    assert np.array_equal(tedge.cpu().numpy(), wedge), np.argwhere(tedge.cpu().numpy() != wedge)[:5]
    assert np.array_equal(bits(tcoef), bits(wcoef))
    _, qptr, _, rptr = G.ragged_clouds()
    one = int(rptr[6])                                                          # the one-point cloud: ONE list of 2 100, all 1
    assert wptr[one + 1] - wptr[one] == 2100 and (wcoef[wptr[one]:wptr[one + 1]] == 1).all()
    again = transposed(k)                                                       # a second run: the same bits
    assert all(torch.equal(a, b) for a, b in zip(again, (tptr, tedge, tcoef)))


# ---- 2. the ordered sum -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.KS)
def test_gradient_equals_the_restatement_bitwise(k):
    from deltaconv_amd._lib import lib
    _, qptr, _, rptr = G.ragged_clouds()
    nq, nr, b = int(qptr[-1]), int(rptr[-1]), len(G.PAIRS)
    wptr, wedge, wcoef = G.ragged_lists(k)
    tptr, tedge, tcoef, drp = dev(wptr), dev(wedge), dev(wcoef), dev(rptr)
    mr = max(p[1] for p in G.PAIRS)

    def run(g, ldg, c, out, ldo, groups):
        for lo, hi in groups:
            lib.call("dc_knn_interpolate_backward", g, ldg, nq, c, drp[lo:hi + 1], hi - lo, max(p[1] for p in G.PAIRS[lo:hi]), k,
                     tptr, tedge, tcoef, int(tedge.numel()), 0, out, ldo)
        torch.cuda.synchronize()

    for c in G.CHANNELS + (1021,):                                              # 1021: 256 groups, one row a workgroup (rpb = 1)
        want = restated_dx(k, c)
        for vec in (True, False):
            g, ldg = laid_out(G.ragged_gradient(c), vec)
            out, whole, ldo, touched = guarded_rows(nr, c, vec)
            run(g, ldg, c, out, ldo, [(0, b)])
            assert not bool(torch.isnan(out).any()), "a reference row of a pair was not written"
            assert np.array_equal(bits(out), bits(want)), (k, c, vec)
            full = whole.cpu().numpy()
            assert (full[~touched] == -9.0).all(), "floats between the rows or around the gradient were written"
            # one launch per pair, two launches, and a second run of the one launch: the same bits, guards and gaps included
            for groups in ([(i, i + 1) for i in range(b)], [(0, 3), (3, b)], [(0, b)]):
                whole.fill_(-9.0)
                out.fill_(float("nan"))
                run(g, ldg, c, out, ldo, groups)
                assert np.array_equal(bits(whole), bits(full)), (groups, k, c, vec)
    assert mr == 2049


def test_a_cloud_range_runs_against_the_lists_of_the_whole_call():
    """edge_base != 0: pairs 1 .. 6 with their own rows of g, tptr from their first reference row on, offsets relative to it."""
    from deltaconv_amd.geometry import interpolate_rows_backward
    k, c, lo, hi = 3, 50, 1, 7
    _, qptr, _, rptr = G.ragged_clouds()
    wptr, wedge, wcoef = G.ragged_lists(k)
    q0, q1, r0, r1 = int(qptr[lo]), int(qptr[hi]), int(rptr[lo]), int(rptr[hi])
    g = dev(G.ragged_gradient(c))
    tptr, tedge, tcoef = dev(wptr), dev(wedge), dev(wcoef)
    rel = dev(rptr[lo:hi + 1] - r0)
    got = interpolate_rows_backward(g[q0:q1], rel, tptr[r0:r1 + 1], tedge, tcoef, k, 2048, n_ref=r1 - r0, edge_base=q0,
                                    out=torch.full((r1 - r0, c), float("nan"), device=DEV))
    assert np.array_equal(bits(got), bits(restated_dx(k, c)[r0:r1]))


# ---- 3. autograd ---------------------------------------------------------------------------------------------------------------------
def _fp64_autograd(x, g, k):
    """torch autograd of the fp64 restatement (the same lists in fp64 from the fp32 search) -> dx64 [Nr,C] numpy."""
    _, qptr, _, rptr = G.ragged_clouds()
    idx, d2 = G.ragged_search(k)
    coef = np.zeros(idx.shape, dtype=np.float64)
    rows = np.zeros(idx.shape, dtype=np.int64)
    for b, (_, nr) in enumerate(G.PAIRS):
        s = slice(qptr[b], qptr[b + 1])
        c64, ok = G.coefficients(idx[s], d2[s], nr, np.float64)
        coef[s], rows[s] = c64, np.where(ok, rptr[b] + idx[s], 0)
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    out = (torch.from_numpy(coef)[:, :, None] * x64[torch.from_numpy(rows)]).sum(dim=1)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return x64.grad.numpy()


@pytest.mark.parametrize("form", ["contiguous", "row_strided", "one_dimensional"])
def test_knn_interpolate_differentiable_gives_the_restated_gradient(form):
    from deltaconv_amd.geometry import knn_interpolate
    k = 3
    c = 1 if form == "one_dimensional" else 50
    qry, qptr, ref, rptr = G.ragged_clouds()
    nr = int(rptr[-1])
    x = (np.random.default_rng(5).standard_normal((nr, c)) * 10).astype(np.float32)
    g = G.ragged_gradient(c)
    if form == "contiguous":
        leaf = dev(x).requires_grad_(True)
        xin, grad_of = leaf, lambda: leaf.grad
    elif form == "row_strided":
        leaf = torch.zeros((nr, 64), device=DEV)
        leaf[:, 3:53] = dev(x)
        leaf.requires_grad_(True)
        xin, grad_of = leaf[:, 3:53], lambda: leaf.grad[:, 3:53]
    else:
        leaf = dev(x[:, 0]).requires_grad_(True)
        xin, grad_of = leaf, lambda: leaf.grad[:, None]
    args = dict(k=k, ptr_x=dev(rptr), ptr_y=dev(qptr))
    out = knn_interpolate(xin, dev(ref), dev(qry), differentiable=True, **args)
    assert out.requires_grad and out.shape == (int(qptr[-1]), c)
    plain = knn_interpolate(xin.detach(), dev(ref), dev(qry), **args)
    assert torch.equal(out.detach(), plain)                                     # the forward values: the inference path's bits
    out.backward(dev(g))
    got = grad_of()
    assert leaf.grad.dtype == torch.float32 and leaf.grad.shape == leaf.shape
    if form == "row_strided":
        assert not bool(leaf.grad[:, :3].any()) and not bool(leaf.grad[:, 53:].any())
    want = restated_dx(k, c)
    assert np.array_equal(bits(got), bits(want))
    err = np.abs(got.cpu().numpy().astype(np.float64) - _fp64_autograd(x, g, k))
    wptr, wedge, _ = G.ragged_lists(k)
    bound = G.bound(g, wptr, wedge, G.ragged_lists(k, np.float64)[2], k)
    live = bound > 0
    print(f"{form}: worst |dx - dx64| / bound = {(err[live] / bound[live]).max():.3f}")
    assert (err <= bound).all()
    with pytest.raises(RuntimeError, match="second time"):                      # once: the saved lists are freed
        out.backward(dev(g))
    with pytest.raises(RuntimeError, match="inference-only"):                   # the default refuses as before
        knn_interpolate(xin, dev(ref), dev(qry), **args)
    # a second forward + backward: the same bits
    leaf.grad = None
    knn_interpolate(xin, dev(ref), dev(qry), differentiable=True, **args).backward(dev(g))
    assert torch.equal(grad_of(), got)


def test_propagator_differentiable_apply_gives_the_same_gradient():
    from deltaconv_amd import Propagator
    from deltaconv_amd.loader import DeviceDataset
    k, c = 3, 50
    qry, qptr, ref, rptr = G.ragged_clouds()
    source = DeviceDataset(dev(ref), dev(rptr), np.diff(rptr))
    target = DeviceDataset(dev(qry), dev(qptr), np.diff(qptr))
    prop = Propagator(source, target, k=k, differentiable=True)
    wptr, wedge, wcoef = G.ragged_lists(k)
    n = int(wptr[-1])
    assert np.array_equal(prop.lists[0].cpu().numpy(), wptr) and np.array_equal(prop.lists[1][:n].cpu().numpy(), wedge)
    assert np.array_equal(bits(prop.lists[2][:n]), bits(wcoef))
    x = dev((np.random.default_rng(5).standard_normal((int(rptr[-1]), c)) * 10).astype(np.float32))
    g = dev(G.ragged_gradient(c))
    leaf = x.clone().requires_grad_(True)
    out = prop.apply(leaf)
    assert out.requires_grad and torch.equal(out.detach(), Propagator(source, target, k=k).apply(x))
    out.backward(g)
    assert np.array_equal(bits(leaf.grad), bits(restated_dx(k, c)))
    # a range of clouds against the store-wide lists (edge_base = the range's first target row)
    lo, hi = 1, 7
    q0, q1, r0, r1 = int(qptr[lo]), int(qptr[hi]), int(rptr[lo]), int(rptr[hi])
    part = x[r0:r1].clone().requires_grad_(True)
    sub = prop.apply(part, (lo, hi))
    assert torch.equal(sub.detach(), out.detach()[q0:q1])
    sub.backward(g[q0:q1])
    assert torch.equal(part.grad, leaf.grad[r0:r1])
    # nothing is recorded without the option, under no_grad, or for values that do not require grad
    assert not Propagator(source, target, k=k).apply(leaf).requires_grad and not prop.apply(x).requires_grad
    with torch.no_grad():
        assert not prop.apply(leaf).requires_grad
    with pytest.raises(ValueError, match="out="):
        prop.apply(leaf, out=torch.empty_like(out))


# ---- 4. graph capture -------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_are_capturable_in_one_graph():
    from deltaconv_amd.geometry import knn_interpolate
    k, c = 3, 50
    qry, qptr, ref, rptr = G.ragged_clouds()
    nq, nr = int(qptr[-1]), int(rptr[-1])
    rng = np.random.default_rng(8)
    pos_x, pos_y = dev(ref), dev(qry)
    args = dict(k=k, ptr_x=dev(rptr), ptr_y=dev(qptr), differentiable=True, max_query_cloud=max(p[0] for p in G.PAIRS),
                max_ref_cloud=max(p[1] for p in G.PAIRS))
    xs = torch.zeros((nr, c), device=DEV, requires_grad=True)
    gs = torch.zeros((nq, c), device=DEV)

    def step():
        out = knn_interpolate(xs, pos_x, pos_y, **args)
        return out, torch.autograd.grad(out, xs, gs)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dx = step()
    for seed in (1, 2):
        x, g = (rng.standard_normal((nr, c)) * 10).astype(np.float32), (rng.standard_normal((nq, c)) * 10).astype(np.float32)
        with torch.no_grad():
            xs.copy_(dev(x))
            gs.copy_(dev(g))
        graph.replay()
        torch.cuda.synchronize()
        got_out, got_dx = out.detach().clone(), dx.clone()
        eager_out, eager_dx = step()
        assert torch.equal(got_out, eager_out.detach()) and torch.equal(got_dx, eager_dx)
        assert np.array_equal(bits(got_dx), bits(G.backward(g, *G.ragged_lists(k), k)))


# ---- 5. a small end-to-end run ---------------------------------------------------------------------------------------------------
def test_a_loss_on_the_full_clouds_trains_a_layer_on_the_sampled_ones():
    from deltaconv_amd import Propagator
    from deltaconv_amd.loader import DeviceDataset
    rng = np.random.default_rng(12)
    sizes, picked = np.array([300, 257, 400, 64]), 48
    full = rng.random((int(sizes.sum()), 3), dtype=np.float32)
    fptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    keep = np.concatenate([fptr[b] + rng.permutation(sizes[b])[:picked] for b in range(4)])
    sptr = np.arange(5, dtype=np.int64) * picked
    y = dev((full[:, 0] > 0.5).astype(np.int64) + 2 * (full[:, 1] > 0.5).astype(np.int64))
    target = DeviceDataset(dev(full), dev(fptr), sizes)
    source = DeviceDataset(dev(full[keep]), dev(sptr), np.full(4, picked))
    prop = Propagator(source, target, k=3, differentiable=True)

    def run():
        torch.manual_seed(0)
        layer = torch.nn.Linear(3, 4).to(DEV)
        opt = torch.optim.SGD(layer.parameters(), lr=0.2)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(prop.apply(layer(source.pos)), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    first, second = run(), run()
    print("losses:", first)
    assert all(b < a for a, b in zip(first, first[1:])), first
    assert first == second


# ---- 6. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_dc_err_arg_without_a_launch():
    from deltaconv_amd._lib import lib
    _, qptr, _, rptr = G.ragged_clouds()
    k, b = 3, len(G.PAIRS)
    idx, d2 = G.ragged_search(k)
    nq, nr = int(qptr[-1]), int(rptr[-1])
    dqp, drp, didx, dd2 = dev(qptr), dev(rptr), dev(idx), dev(d2)
    tptr = torch.full((nr + 1,), -9, dtype=torch.int64, device=DEV)
    tedge = torch.full((nq * 16,), -9, dtype=torch.int64, device=DEV)
    tcoef = torch.full((nq * 16,), -9.0, device=DEV)
    nbytes = lib.raw("dc_knn_cross_transpose_workspace_bytes")(nq, nr, 16)
    work = torch.full((nbytes // 8,), -9, dtype=torch.int64, device=DEV)
    g, dx = torch.ones((nq, 4), device=DEV), torch.full((nr, 4), -9.0, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    trans, back = lib.raw("dc_knn_cross_transpose"), lib.raw("dc_knn_interpolate_backward")

    def call_trans(B=b, k=3, qp=dqp, rp=drp, i=didx, d=dd2, tp=tptr, te=tedge, tc=tcoef, w=work, wb=nbytes, n=nq):
        return trans(vp(qp), vp(rp), B, n, nr, k, vp(i), vp(d), vp(tp), vp(te), vp(tc), vp(w), wb, None)

    def call_back(B=b, k=3, gg=g, rp=drp, tp=tptr, te=tedge, tc=tcoef, o=dx, C=4, ldg=4, ldx=4, mr=2049):
        return back(vp(gg), ldg, nq, C, vp(rp), B, mr, k, vp(tp), vp(te), vp(tc), nq * 3, 0, vp(o), ldx, None)

    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=-1), "B = -1"), (dict(qp=None), "null"),
                    (dict(rp=None), "null"), (dict(i=None), "null"), (dict(d=None), "null"), (dict(tp=None), "null"),
                    (dict(te=None), "null"), (dict(tc=None), "null"), (dict(w=None), "workspace"), (dict(wb=lib.raw("dc_knn_cross_transpose_workspace_bytes")(nq, nr, 3) - 8), "workspace"),
                    (dict(n=-1), "num_query")):
        assert call_trans(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(gg=None), "null"),
                    (dict(rp=None), "null"), (dict(tp=None), "null"), (dict(te=None), "null"), (dict(tc=None), "null"),
                    (dict(o=None), "null"), (dict(C=0), "C = 0"), (dict(ldg=3), "ldg"), (dict(ldx=3), "ldx"),
                    (dict(mr=-1), "max_ref_cloud")):
        assert call_back(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    assert call_back(B=0) == 0 and call_back(mr=0) == 0
    assert lib.raw("dc_knn_cross_transpose_workspace_bytes")(nq, nr, 17) == 0
    torch.cuda.synchronize()
    assert bool((tptr == -9).all()) and bool((tedge == -9).all()) and bool((tcoef == -9).all()) and bool((dx == -9).all())
    assert bool((work == -9).all())
