"""The cross-cloud pooling on the MI355X (csrc/pool.hip: ``dc_knn_pool``, ``dc_knn_pool_backward``; ``geometry.pool_rows`` /
``pool_rows_backward`` / ``knn_pool``) against the numpy restatement of csrc/pool_math.h (tests/pool_restate.py, itself held to a
g++ build of that header and to fp64 by tests/test_pool_host.py): values, ``arg``, ``cnt`` and gradients bit for bit, on the
ragged call of tests/interp_grad_restate.py (a reference cloud smaller than k, an empty pair, query clouds of more than 256 rows).

The fp64 bounds (tests/test_pool_host.py derives them): max / min EQUAL the fp64 selection; sum |out - out64| <= cnt * 2^-24 *
sum|x_s|; mean (cnt + 1) * 2^-24 * sum|x_s| / cnt; every backward |dx - dx64| <= (L_j + 2) * 2^-24 * sum_e |term_e|."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pool_restate as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
MODES = ("max", "min", "sum", "mean")
MQ, MR = max(p[0] for p in P.PAIRS), max(p[1] for p in P.PAIRS)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def laid_out(a, aligned, dtype=torch.float32, fill=float("nan")):
    """a [n,C] on the device.  aligned: contiguous on an allocation's base (16-byte rows where C is a multiple of 4).  Otherwise a
    strided view with an odd leading dimension, one element off the base (no row is aligned); the gaps hold `fill`.
    -> (view, ld, whole buffer, the mask of the elements of `whole` the view covers)."""
    n, c = a.shape
    ld, off = (c, 0) if aligned else ((c + 1) | 1, 1)
    whole = torch.full((GUARD + off + max(n, 1) * ld + GUARD,), fill, dtype=dtype, device=DEV)
    view = whole[GUARD + off:].as_strided((n, c), (ld, 1))
    view.copy_(dev(a).to(dtype))
    covered = np.zeros(whole.numel(), dtype=bool)
    for r in range(n):
        covered[GUARD + off + r * ld:GUARD + off + r * ld + c] = True
    return view, ld, whole, covered


def untouched(whole, covered, fill):
    rest = whole.cpu().numpy()[~covered]
    return bool(np.isnan(rest).all()) if isinstance(fill, float) and np.isnan(fill) else bool((rest == fill).all())


# ---- 1. the two entry points against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3, 16))
def test_device_equals_the_restatement_bitwise(k):
    from deltaconv_amd._lib import lib
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    wptr, wedge, _ = P.ragged_lists(k)
    nq, nr, b = int(qptr[-1]), int(rptr[-1]), len(P.PAIRS)
    dqp, drp, didx, tptr, tedge = dev(qptr), dev(rptr), dev(idx), dev(wptr), dev(wedge)
    for mode, name in enumerate(MODES):
        x, g, out, arg, cnt, dx = P.ragged_case(k, mode)
        for c in (1, 4, 5, 64, 67):
            for aligned in (True, False):
                xin, ldx, _, _ = laid_out(x[:, :c], aligned)
                gin, ldg, _, _ = laid_out(g[:, :c], aligned)
                assert (xin.data_ptr() % 16 == 0 and ldx % 4 == 0) == (aligned and c % 4 == 0)

                def run():
                    o, ldo, ow, oc = laid_out(np.full((nq, c), -9.0, dtype=np.float32), aligned, fill=-9.0)
                    a, lda, aw, ac = laid_out(np.full((nq, c), 77, dtype=np.uint8), aligned, torch.uint8, 77)
                    n = torch.full((GUARD + nq + GUARD,), 99, dtype=torch.uint8, device=DEV)
                    d, ldd, dw, dc = laid_out(np.full((nr, c), -9.0, dtype=np.float32), aligned, fill=-9.0)
                    o.fill_(float("nan"))
                    d.fill_(float("nan"))
                    lib.call("dc_knn_pool", xin, ldx, c, dqp, drp, b, MQ, k, didx, mode, o, ldo, a, lda, n[GUARD:GUARD + nq])
                    lib.call("dc_knn_pool_backward", gin, ldg, nq, c, drp, b, MR, k, tptr, tedge, int(tedge.numel()), mode, a, lda,
                             n[GUARD:GUARD + nq], d, ldd)
                    torch.cuda.synchronize()
                    assert untouched(ow, oc, -9.0) and untouched(aw, ac, 77) and untouched(dw, dc, -9.0), \
                        "bytes between the rows or around out / arg / dx were written"
                    assert bool((n[:GUARD] == 99).all()) and bool((n[GUARD + nq:] == 99).all())
                    return o, a, n[GUARD:GUARD + nq], d

                o, a, n, d = run()
                assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(d).any()), "a row of a pair was not written"
                assert np.array_equal(bits(o), bits(out[:, :c])), (k, name, c, aligned)
                assert np.array_equal(n.cpu().numpy(), cnt)
                assert np.array_equal(a.cpu().numpy(), arg[:, :c] if mode <= 1 else np.full((nq, c), 77)), (k, name, c, aligned)
                assert np.array_equal(bits(d), bits(dx[:, :c])), (k, name, c, aligned)
                if c == 67:                                                        # a second run gives the same bits
                    again = run()
                    assert all(torch.equal(p, q) for p, q in zip(again, (o, a, n, d)))
        if mode >= 2:                                                             # sum / mean without an arg at all
            o = torch.full((nq, 5), float("nan"), device=DEV)
            n = torch.full((nq,), 99, dtype=torch.uint8, device=DEV)
            lib.call("dc_knn_pool", dev(x[:, :5]), 5, 5, dqp, drp, b, MQ, k, didx, mode, o, 5, None, 0, n)
            d = torch.full((nr, 5), float("nan"), device=DEV)
            lib.call("dc_knn_pool_backward", dev(g[:, :5]), 5, nq, 5, drp, b, MR, k, tptr, tedge, int(tedge.numel()), mode, None, 0, n,
                     d, 5)
            assert np.array_equal(bits(o), bits(out[:, :5])) and np.array_equal(bits(d), bits(dx[:, :5]))


# ---- 2. the tensor-level functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", MODES)
def test_knn_pool_differentiable_gives_the_bits_of_pool_rows_and_its_backward(reduce):
    from deltaconv_amd.geometry import knn_pool, pool_rows, pool_rows_backward
    k, c, mode = 8, 67, P.MODES[reduce]
    qry, qptr, ref, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    wptr, wedge, _ = P.ragged_lists(k)
    x, g, out, arg, cnt, dx = P.ragged_case(k, mode)
    leaf = dev(x).requires_grad_(True)
    args = dict(k=k, reduce=reduce, ptr_x=dev(rptr), ptr_y=dev(qptr))
    got = knn_pool(leaf, dev(ref), dev(qry), differentiable=True, **args)
    assert got.requires_grad and got.shape == (int(qptr[-1]), c)
    rows, rarg, rcnt = pool_rows(dev(x), dev(qptr), dev(rptr), dev(idx), MQ, reduce)
    assert torch.equal(got.detach(), rows) and torch.equal(got.detach(), knn_pool(dev(x), dev(ref), dev(qry), **args))
    assert np.array_equal(bits(rows), bits(out)) and np.array_equal(rcnt.cpu().numpy(), cnt)
    assert (rarg is None) == (mode >= 2) and (rarg is None or np.array_equal(rarg.cpu().numpy(), arg))
    grad, = torch.autograd.grad(got, leaf, dev(g))
    back = pool_rows_backward(dev(g), dev(rptr), dev(wptr), dev(wedge), rarg, rcnt, k, MR, reduce)
    assert grad.dtype == torch.float32 and torch.equal(grad, back) and np.array_equal(bits(grad), bits(dx))
    if reduce == "sum":
        assert torch.equal(knn_pool(dev(x), dev(ref), dev(qry), **dict(args, reduce="add")), rows)
    # strided rows and a 1-D x go the same way
    wide = torch.zeros((x.shape[0], 80), device=DEV)
    wide[:, 3:70] = dev(x)
    assert torch.equal(pool_rows(wide[:, 3:70], dev(qptr), dev(rptr), dev(idx), MQ, reduce)[0], rows)
    one = dev(x[:, 0]).requires_grad_(True)
    flat = knn_pool(one, dev(ref), dev(qry), differentiable=True, **args)
    assert torch.equal(flat.detach(), rows[:, :1])
    assert torch.equal(torch.autograd.grad(flat, one, dev(g[:, :1]))[0], back[:, 0])


def test_against_a_torch_composition_in_fp64_on_tie_free_inputs():
    from deltaconv_amd.geometry import knn_pool
    k = 8
    qry, qptr, ref, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    rows, ok = P._gathered(None, qptr, rptr, idx)
    ids, valid = dev(rows), dev(ok)
    n = valid.sum(1)
    for reduce in ("max", "sum", "mean"):
        mode = P.MODES[reduce]
        x, g, _, _, cnt, _ = P.ragged_case(k, mode, "distinct" if mode <= 1 else "gauss")
        leaf = dev(x).requires_grad_(True)
        out = knn_pool(leaf, dev(ref), dev(qry), k=k, reduce=reduce, ptr_x=dev(rptr), ptr_y=dev(qptr), differentiable=True)
        grad, = torch.autograd.grad(out, leaf, dev(g))
        x64 = dev(x).double().requires_grad_(True)
        near = x64[ids]
        if reduce == "max":
            want = torch.where(valid[:, :, None], near, torch.full_like(near, float("-inf"))).amax(1)
        else:
            want = torch.where(valid[:, :, None], near, torch.zeros_like(near)).sum(1)
            want = want / n.clamp(min=1)[:, None] if reduce == "mean" else want
        want = torch.where((n > 0)[:, None], want, torch.zeros_like(want))
        want64, = torch.autograd.grad(want, x64, dev(g).double())
        _, arg64, _, xmag = P.forward64(x, qptr, rptr, idx, mode)
        _, gmag, terms = P.backward64(g, qptr, rptr, idx, mode, arg64, cnt, int(rptr[-1]))
        err = np.abs(out.detach().cpu().numpy().astype(np.float64) - want.detach().cpu().numpy())
        bound = P.forward_bound(mode, cnt, xmag)
        assert (err <= bound).all() and (reduce != "max" or not err.any())
        gerr = np.abs(grad.cpu().numpy().astype(np.float64) - want64.cpu().numpy())
        gbound = P.backward_bound(gmag, terms)
        assert (gerr <= gbound).all(), float((gerr - gbound).max())
        live, glive = bound > 0, gbound > 0
        print(f"{reduce}: worst |out - out64| / bound = {(err[live] / bound[live]).max() if live.any() else 0.0:.3f}, "
              f"worst |dx - dx64| / bound = {(gerr[glive] / gbound[glive]).max():.3f}")


def test_refusals():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import knn_pool
    qry, qptr, ref, rptr = P.ragged_clouds()
    x = dev(P.ragged_features()[:, :4])
    args = dict(ptr_x=dev(rptr), ptr_y=dev(qptr))
    with pytest.raises(RuntimeError, match="inference-only"):
        knn_pool(x.clone().requires_grad_(True), dev(ref), dev(qry), **args)
    with pytest.raises(ValueError, match="k = 17"):
        knn_pool(x, dev(ref), dev(qry), k=17, **args)
    with pytest.raises(ValueError, match="reduce"):
        knn_pool(x, dev(ref), dev(qry), reduce="median", **args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_pool(x.cpu(), dev(ref), dev(qry), **args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_pool(x, dev(ref).cpu(), dev(qry), **args)
    with pytest.raises(RuntimeError, match="pos_x requires grad"):
        knn_pool(x, dev(ref).requires_grad_(True), dev(qry), differentiable=True, **args)
    with pytest.raises(RuntimeError, match="pos_y requires grad"):
        knn_pool(x, dev(ref), dev(qry).requires_grad_(True), **args)
    with torch.no_grad():                                                       # under no_grad nothing is differentiated: no refusal
        assert not knn_pool(x.clone().requires_grad_(True), dev(ref), dev(qry), **args).requires_grad
    # the entry points: DC_ERR_ARG with a message, nothing written
    k, nq, nr, b = 3, int(qptr[-1]), int(rptr[-1]), len(P.PAIRS)
    idx = dev(P.ragged_search(k)[0])
    wptr, wedge, _ = P.ragged_lists(k)
    tptr, tedge, dqp, drp = dev(wptr), dev(wedge), dev(qptr), dev(rptr)
    out, dx = torch.full((nq, 4), -9.0, device=DEV), torch.full((nr, 4), -9.0, device=DEV)
    arg, cnt = torch.full((nq, 4), 77, dtype=torch.uint8, device=DEV), torch.full((nq,), 99, dtype=torch.uint8, device=DEV)
    g = torch.ones((nq, 4), device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    fwd, bwd = lib.raw("dc_knn_pool"), lib.raw("dc_knn_pool_backward")

    def call_fwd(B=b, k=k, xx=x, i=idx, mode=0, o=out, a=arg, n=cnt, C=4, ldx=4, ldo=4, lda=4, mq=MQ):
        return fwd(vp(xx), ldx, C, vp(dqp), vp(drp), B, mq, k, vp(i), mode, vp(o), ldo, vp(a), lda, vp(n), None)

    def call_bwd(B=b, k=k, gg=g, te=tedge, tp=tptr, mode=0, a=arg, n=cnt, o=dx, C=4, ldg=4, ldx=4, lda=4, mr=MR):
        return bwd(vp(gg), ldg, nq, C, vp(drp), B, mr, k, vp(tp), vp(te), nq * k, mode, vp(a), lda, vp(n), vp(o), ldx, None)

    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(mode=4), "mode = 4"),
                    (dict(mode=-1), "mode = -1"), (dict(a=None), "null"), (dict(a=None, mode=1), "null"), (dict(n=None), "null"),
                    (dict(n=None, mode=2), "null"), (dict(lda=3), "ldarg"), (dict(xx=None), "null"), (dict(i=None), "null"),
                    (dict(o=None), "null"), (dict(C=0), "C = 0"), (dict(ldx=3), "ldx"), (dict(ldo=3), "ldo"),
                    (dict(mq=-1), "max_query_cloud")):
        assert call_fwd(**kw) == -1 and msg in lib.last_error() and "dc_knn_pool:" in lib.last_error(), (kw, lib.last_error())
    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(mode=4), "mode = 4"),
                    (dict(a=None), "null"), (dict(n=None), "null"), (dict(n=None, mode=3), "null"), (dict(lda=3), "ldarg"),
                    (dict(gg=None), "null"), (dict(te=None), "null"), (dict(tp=None), "null"), (dict(o=None), "null"),
                    (dict(C=0), "C = 0"), (dict(ldg=3), "ldg"), (dict(ldx=3), "ldx"), (dict(mr=-1), "max_ref_cloud")):
        assert call_bwd(**kw) == -1 and msg in lib.last_error() and "dc_knn_pool_backward:" in lib.last_error(), (kw, lib.last_error())
    assert call_fwd(B=0) == 0 and call_fwd(mq=0) == 0 and call_bwd(B=0) == 0 and call_bwd(mr=0) == 0
    assert call_fwd(a=None, mode=2) == 0 and call_bwd(a=None, mode=3) == 0       # sum / mean may leave arg out
    torch.cuda.synchronize()
    assert bool((arg == 77).all())


# ---- 3. graph capture -------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_are_capturable_in_one_graph():
    from deltaconv_amd.geometry import knn_pool
    k, c = 8, 64
    qry, qptr, ref, rptr = P.ragged_clouds()
    nq, nr = int(qptr[-1]), int(rptr[-1])
    rng = np.random.default_rng(8)
    pos_x, pos_y = dev(ref), dev(qry)
    args = dict(k=k, ptr_x=dev(rptr), ptr_y=dev(qptr), differentiable=True, max_query_cloud=MQ, max_ref_cloud=MR)
    xs = torch.zeros((nr, c), device=DEV, requires_grad=True)
    gs = torch.zeros((nq, c), device=DEV)

    def step():
        outs = [knn_pool(xs, pos_x, pos_y, reduce=r, **args) for r in ("max", "mean")]
        return outs, [torch.autograd.grad(o, xs, gs)[0] for o in outs]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs, grads = step()
    idx = P.ragged_search(k)[0]
    wptr, wedge, _ = P.ragged_lists(k)
    for _ in range(2):
        x = (np.round(rng.standard_normal((nr, c)) * 4) / 4).astype(np.float32)
        g = (rng.standard_normal((nq, c)) * 10).astype(np.float32)
        with torch.no_grad():
            xs.copy_(dev(x))
            gs.copy_(dev(g))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in outs + grads]
        eager_outs, eager_grads = step()
        assert all(torch.equal(a, b.detach()) for a, b in zip(got, eager_outs + eager_grads))
        for i, mode in enumerate((0, 3)):
            out, arg, cnt = P.forward(x, qptr, rptr, idx, mode)
            assert np.array_equal(bits(got[i]), bits(out))
            assert np.array_equal(bits(got[2 + i]), bits(P.backward(g, wptr, wedge, k, mode, arg, cnt)))
