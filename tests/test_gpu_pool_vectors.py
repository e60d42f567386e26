"""The cross-cloud pooling of tangent-vector features on the MI355X (csrc/pool_vectors.hip: ``dc_knn_cross_rotation``,
``dc_knn_pool_vectors``, ``dc_knn_pool_vectors_backward``; ``geometry.knn_cross_rotation`` / ``pool_vectors`` /
``pool_vectors_backward`` / ``knn_pool_vectors``; ``CloudPair.down_vectors(v, reduce=...)``) against the numpy restatement of
csrc/pool_vectors_math.h (tests/pool_vectors_restate.py, itself held to a g++ build of that header and to fp64 by
tests/test_pool_vectors_host.py): table, values, ``arg``, ``cnt`` and the three gradients bit for bit, on the ragged call of
tests/interp_grad_restate.py (a reference cloud smaller than k, an empty pair, query clouds of more than 256 rows, an in-edge
list of about 2 100)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import pool_vectors_restate as P
from tests.test_gpu_pool import GUARD, bits, dev, laid_out, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("max", "sum", "mean")
MQ, MR = max(p[0] for p in P.PAIRS), max(p[1] for p in P.PAIRS)


def frames_dev():
    tf, sf = P.ragged_frames()
    return tuple(dev(a) for a in tf), tuple(dev(a) for a in sf)


# ---- 1. the three entry points against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", P.KS)
def test_device_equals_the_restatement_bitwise(k):
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import interpolate_vectors, interpolate_vectors_backward, knn_cross_rotation
    _, qptr, _, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    wptr, wedge, _ = P.ragged_lists(k)
    nq, nr, b = int(qptr[-1]), int(rptr[-1]), len(P.PAIRS)
    dqp, drp, didx, tptr, tedge = dev(qptr), dev(rptr), dev(idx), dev(wptr), dev(wedge)
    tf, sf = frames_dev()
    for non_oriented in (True, False):
        got = knn_cross_rotation(didx, dqp, drp, tf, sf, non_oriented, max_query_cloud=MQ)
        assert np.array_equal(bits(got), bits(P.ragged_table(k, non_oriented))), (k, non_oriented)
    rmat = knn_cross_rotation(didx, dqp, drp, tf, sf, True, max_query_cloud=MQ)
    assert rmat.data_ptr() % 16 == 0
    for name in MODES:
        mode = P.MODES[name]
        v, g, _, out, arg, cnt, dv = P.ragged_case(k, mode)
        for c in P.CHANNELS:
            for aligned in (True, False):
                vin, ldv, _, _ = laid_out(v[:, :c], aligned)
                gin, ldg, _, _ = laid_out(g[:, :c], aligned)
                assert (vin.data_ptr() % 16 == 0 and ldv % 4 == 0) == (aligned and c % 4 == 0)

                def run():
                    o, ldo, ow, oc = laid_out(np.full((2 * nq, c), -9.0, dtype=np.float32), aligned, fill=-9.0)
                    a, lda, aw, ac = laid_out(np.full((nq, c), 77, dtype=np.uint8), aligned, torch.uint8, 77)
                    n = torch.full((GUARD + nq + GUARD,), 99, dtype=torch.uint8, device=DEV)
                    d, ldd, dw, dc = laid_out(np.full((2 * nr, c), -9.0, dtype=np.float32), aligned, fill=-9.0)
                    o.fill_(float("nan"))
                    d.fill_(float("nan"))
                    lib.call("dc_knn_pool_vectors", vin, ldv, c, dqp, drp, b, MQ, k, didx, rmat, mode, o, ldo, a, lda,
                             n[GUARD:GUARD + nq])
                    lib.call("dc_knn_pool_vectors_backward", gin, ldg, nq, c, drp, b, MR, k, tptr, tedge, int(tedge.numel()), rmat,
                             mode, a, lda, n[GUARD:GUARD + nq], d, ldd)
                    torch.cuda.synchronize()
                    assert untouched(ow, oc, -9.0) and untouched(aw, ac, 77) and untouched(dw, dc, -9.0), \
                        "bytes between the rows or around out / arg / dv were written"
                    assert bool((n[:GUARD] == 99).all()) and bool((n[GUARD + nq:] == 99).all())
                    return o, a, n[GUARD:GUARD + nq], d

                o, a, n, d = run()
                assert not bool(torch.isnan(o).any()) and not bool(torch.isnan(d).any()), "a row of a pair was not written"
                assert np.array_equal(bits(o), bits(out[:, :c])), (k, name, c, aligned)
                assert np.array_equal(n.cpu().numpy(), cnt)
                assert np.array_equal(a.cpu().numpy(), arg[:, :c] if mode == 0 else np.full((nq, c), 77)), (k, name, c, aligned)
                assert np.array_equal(bits(d), bits(dv[:, :c])), (k, name, c, aligned)
                if c == 64:                                                        # a second run gives the same bits
                    again = run()
                    assert all(torch.equal(p, q) for p, q in zip(again, (o, a, n, d)))
        if mode >= 2:                                                             # sum / mean without an arg at all
            o = torch.full((2 * nq, 6), float("nan"), device=DEV)
            n = torch.full((nq,), 99, dtype=torch.uint8, device=DEV)
            lib.call("dc_knn_pool_vectors", dev(v[:, :6]), 6, 6, dqp, drp, b, MQ, k, didx, rmat, mode, o, 6, None, 0, n)
            d = torch.full((2 * nr, 6), float("nan"), device=DEV)
            lib.call("dc_knn_pool_vectors_backward", dev(g[:, :6]), 6, nq, 6, drp, b, MR, k, tptr, tedge, int(tedge.numel()), rmat,
                     mode, None, 0, n, d, 6)
            assert np.array_equal(bits(o), bits(out[:, :6])) and np.array_equal(bits(d), bits(dv[:, :6]))
    # sum IS interpolate_vectors on the rotation table, bit for bit, forward and gradient
    v, g, _, out, _, _, dv = P.ragged_case(k, 2)
    assert np.array_equal(bits(interpolate_vectors(dev(v), dqp, drp, didx, rmat, MQ)), bits(out))
    assert np.array_equal(bits(interpolate_vectors_backward(dev(g), drp, tptr, tedge, rmat, k, MR)), bits(dv))


# ---- 2. the tensor-level functions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", MODES)
def test_knn_pool_vectors_differentiable_gives_the_bits_of_pool_vectors_and_its_backward(reduce):
    from deltaconv_amd.geometry import knn_cross_rotation, knn_pool_vectors, pool_vectors, pool_vectors_backward
    k, mode = 16, P.MODES[reduce]
    qry, qptr, ref, rptr = P.ragged_clouds()
    idx, _ = P.ragged_search(k)
    wptr, wedge, _ = P.ragged_lists(k)
    v, g, _, out, arg, cnt, dv = P.ragged_case(k, mode)
    tf, sf = frames_dev()
    leaf = dev(v).requires_grad_(True)
    args = dict(k=k, reduce=reduce, ptr_x=dev(rptr), ptr_y=dev(qptr))
    got = knn_pool_vectors(leaf, dev(ref), dev(qry), sf, tf, differentiable=True, **args)
    assert got.requires_grad and got.shape == (2 * int(qptr[-1]), P.WIDTH)
    rmat = knn_cross_rotation(dev(idx), dev(qptr), dev(rptr), tf, sf)
    rows, rarg, rcnt = pool_vectors(dev(v), dev(qptr), dev(rptr), dev(idx), rmat, MQ, reduce)
    assert torch.equal(got.detach(), rows) and torch.equal(rows, knn_pool_vectors(dev(v), dev(ref), dev(qry), sf, tf, **args))
    assert np.array_equal(bits(rows), bits(out)) and np.array_equal(rcnt.cpu().numpy(), cnt)
    assert (rarg is None) == (mode >= 2) and (rarg is None or np.array_equal(rarg.cpu().numpy(), arg))
    grad, = torch.autograd.grad(got, leaf, dev(g))
    back = pool_vectors_backward(dev(g), dev(rptr), dev(wptr), dev(wedge), rmat, rarg, rcnt, k, MR, reduce)
    assert grad.dtype == torch.float32 and torch.equal(grad, back) and np.array_equal(bits(grad), bits(dv))
    again, = torch.autograd.grad(knn_pool_vectors(leaf, dev(ref), dev(qry), sf, tf, differentiable=True, **args), leaf, dev(g))
    assert torch.equal(again, grad)                                             # a second run gives the same gradient bits
    if reduce == "sum":
        assert torch.equal(knn_pool_vectors(dev(v), dev(ref), dev(qry), sf, tf, **dict(args, reduce="add")), rows)
    wide = torch.zeros((v.shape[0], 80), device=DEV)                             # strided rows go the same way
    wide[:, 3:67] = dev(v)
    assert torch.equal(pool_vectors(wide[:, 3:67], dev(qptr), dev(rptr), dev(idx), rmat, MQ, reduce)[0], rows)


def test_refusals():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import knn_pool_vectors
    qry, qptr, ref, rptr = P.ragged_clouds()
    tf, sf = frames_dev()
    v = dev(P.ragged_values()[:, :4])
    args = dict(ptr_x=dev(rptr), ptr_y=dev(qptr))
    call = lambda vv=v, px=dev(ref), py=dev(qry), fx=sf, fy=tf, **kw: knn_pool_vectors(vv, px, py, fx, fy, **dict(args, **kw))
    with pytest.raises(RuntimeError, match="inference-only"):
        call(v.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="k = 17"):
        call(k=17)
    with pytest.raises(ValueError, match="reduce"):
        call(reduce="median")
    with pytest.raises(ValueError, match="reduce"):
        call(reduce="min")
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(v.cpu())
    with pytest.raises(RuntimeError, match="no CPU path"):
        call(px=dev(ref).cpu())
    with pytest.raises(RuntimeError, match="pos_x requires grad"):
        call(px=dev(ref).requires_grad_(True), differentiable=True)
    with pytest.raises(RuntimeError, match="pos_y requires grad"):
        call(py=dev(qry).requires_grad_(True))
    with pytest.raises(RuntimeError, match="requires grad"):
        call(fy=(tf[0].clone().requires_grad_(True), tf[1], tf[2]))
    with pytest.raises(RuntimeError, match="requires grad"):
        call(fx=(sf[0], sf[1].clone().requires_grad_(True)))
    with torch.no_grad():                                                       # under no_grad nothing is differentiated: no refusal
        assert not call(v.clone().requires_grad_(True)).requires_grad
    # the entry points: DC_ERR_ARG with a message, nothing written
    k, nq, nr, b = 3, int(qptr[-1]), int(rptr[-1]), len(P.PAIRS)
    idx = dev(P.ragged_search(k)[0])
    wptr, wedge, _ = P.ragged_lists(k)
    tptr, tedge, dqp, drp = dev(wptr), dev(wedge), dev(qptr), dev(rptr)
    rmat = dev(P.ragged_table(k))
    off = torch.zeros(4 * nq * k + 4, device=DEV)[1:]                            # a table one float off alignment
    out, dv = torch.full((2 * nq, 4), -9.0, device=DEV), torch.full((2 * nr, 4), -9.0, device=DEV)
    arg, cnt = torch.full((nq, 4), 77, dtype=torch.uint8, device=DEV), torch.full((nq,), 99, dtype=torch.uint8, device=DEV)
    g = torch.ones((2 * nq, 4), device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    fwd, bwd, rot = lib.raw("dc_knn_pool_vectors"), lib.raw("dc_knn_pool_vectors_backward"), lib.raw("dc_knn_cross_rotation")

    def call_fwd(B=b, k=k, vv=v, i=idx, R=rmat, mode=0, o=out, a=arg, n=cnt, C=4, ldv=4, ldo=4, lda=4, mq=MQ):
        return fwd(vp(vv), ldv, C, vp(dqp), vp(drp), B, mq, k, vp(i), vp(R), mode, vp(o), ldo, vp(a), lda, vp(n), None)

    def call_bwd(B=b, k=k, gg=g, te=tedge, tp=tptr, R=rmat, mode=0, a=arg, n=cnt, o=dv, C=4, ldg=4, ldv=4, lda=4, mr=MR):
        return bwd(vp(gg), ldg, nq, C, vp(drp), B, mr, k, vp(tp), vp(te), nq * k, vp(R), mode, vp(a), lda, vp(n), vp(o), ldv, None)

    def call_rot(B=b, k=k, i=idx, R=rmat, n=nq, mq=MQ, tn=tf[0]):
        return rot(vp(dqp), vp(drp), B, n, mq, k, vp(i), vp(tn), vp(tf[1]), vp(tf[2]), vp(sf[0]), vp(sf[1]), 1, vp(R), None)

    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(mode=4), "mode = 4"),
                    (dict(mode=1), "mode = 1"), (dict(mode=-1), "mode = -1"), (dict(a=None), "null"), (dict(n=None), "null"),
                    (dict(n=None, mode=2), "null"), (dict(lda=3), "ldarg"), (dict(vv=None), "null"), (dict(i=None), "null"),
                    (dict(R=None), "null"), (dict(R=off), "rmat must be 16-byte"), (dict(o=None), "null"), (dict(C=0), "C = 0"),
                    (dict(ldv=3), "ldv"), (dict(ldo=3), "ldo"), (dict(mq=-1), "max_query_cloud")):
        assert call_fwd(**kw) == -1 and msg in lib.last_error() and "dc_knn_pool_vectors:" in lib.last_error(), (kw, lib.last_error())
    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(mode=4), "mode = 4"),
                    (dict(mode=1), "mode = 1"), (dict(a=None), "null"), (dict(n=None), "null"), (dict(n=None, mode=3), "null"),
                    (dict(lda=3), "ldarg"), (dict(gg=None), "null"), (dict(te=None), "null"), (dict(tp=None), "null"),
                    (dict(R=None), "null"), (dict(R=off), "rmat must be 16-byte"), (dict(o=None), "null"), (dict(C=0), "C = 0"),
                    (dict(ldg=3), "ldg"), (dict(ldv=3), "ldv"), (dict(mr=-1), "max_ref_cloud")):
        assert call_bwd(**kw) == -1 and msg in lib.last_error() and "dc_knn_pool_vectors_backward:" in lib.last_error(), \
            (kw, lib.last_error())
    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(i=None), "null"),
                    (dict(tn=None), "null"), (dict(R=None), "null"), (dict(R=off), "rmat must be 16-byte"), (dict(n=-1), "num_query"),
                    (dict(mq=-1), "max_query_cloud")):
        assert call_rot(**kw) == -1 and msg in lib.last_error() and "dc_knn_cross_rotation:" in lib.last_error(), (kw, lib.last_error())
    assert call_fwd(B=0) == 0 and call_fwd(mq=0) == 0 and call_bwd(B=0) == 0 and call_bwd(mr=0) == 0 and call_rot(B=0) == 0
    assert call_fwd(a=None, mode=2) == 0 and call_bwd(a=None, mode=3) == 0       # sum / mean may leave arg out
    torch.cuda.synchronize()
    assert bool((arg == 77).all())


# ---- 3. CloudPair ----------------------------------------------------------------------------------------------------------------------
def test_cloud_pair_down_vectors(monkeypatch):
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import knn_interpolate_vectors, knn_pool_vectors
    from tests.test_gpu_cloud_pair import K_DOWN, inputs, pair, setup, with_grad
    s = setup()
    _, _, vf, _ = inputs(1)
    _, _, _, hc = inputs(2)
    names = []
    call = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    cp = pair()
    down = dict(ptr_x=s["fptr"], ptr_y=s["cptr"], differentiable=True, k=K_DOWN)
    # without reduce: today's bits and today's launches, no rotation table
    out, grad = with_grad(cp.down_vectors, vf, hc)
    assert sorted(names) == ["dc_knn_cross", "dc_knn_cross_transport", "dc_knn_cross_transpose", "dc_knn_interpolate_vectors",
                             "dc_knn_interpolate_vectors_backward"]
    names.clear()
    want, wgrad = with_grad(lambda t: knn_interpolate_vectors(t, s["pos_f"], s["pos_c"], s["frames_f"], s["frames_c"], **down), vf, hc)
    assert torch.equal(out, want) and torch.equal(grad, wgrad)
    assert torch.equal(cp.down_vectors(vf, reduce="interpolate"), out)
    assert not any(key[0] == "rotation" for key in cp._built)
    names.clear()
    # with reduce: the tensor-level call, forward and gradient; the table is built once, on first use
    for i, reduce in enumerate(("max", "mean", "sum", "add")):
        out, grad = with_grad(lambda t: cp.down_vectors(t, reduce=reduce), vf, hc)
        assert names.count("dc_knn_cross_rotation") == 1 and names.count("dc_knn_pool_vectors") == 2 * i + 1
        mark = len(names)
        want, wgrad = with_grad(lambda t: knn_pool_vectors(t, s["pos_f"], s["pos_c"], s["frames_f"], s["frames_c"], reduce=reduce,
                                                           **down), vf, hc)
        del names[mark:]                                                         # (the tensor-level call's own launches)
        assert torch.equal(out, want) and torch.equal(grad, wgrad), reduce
        assert bool(out.abs().sum() > 0) and bool(grad.abs().sum() > 0)
        plain = cp.down_vectors(vf, reduce)
        assert not plain.requires_grad and torch.equal(plain, out)
    assert ("rotation", "down") in cp._built and ("rotation", "up") not in cp._built
    with pytest.raises(ValueError, match="reduce"):
        cp.down_vectors(vf, reduce="min")
    with pytest.raises(ValueError, match="without frames"):
        pair(frames=False).down_vectors(vf, reduce="max")
    names.clear()
    pair().prepare(vector_pool=True)
    assert sorted(names) == ["dc_knn_cross"] * 2 + ["dc_knn_cross_rotation"] + ["dc_knn_cross_transport"] * 2 + \
        ["dc_knn_cross_transpose"] * 2


def test_a_captured_down_vectors_max_replays_to_the_eager_bits():
    from tests.test_gpu_cloud_pair import C, inputs, pair, setup
    s = setup()
    cp = pair().prepare(vector_pool=True)
    vs = torch.zeros((2 * s["nf"], C), device=DEV, requires_grad=True)
    gv = torch.zeros((2 * s["nc"], C), device=DEV)

    def step():
        out = cp.down_vectors(vs, "max")
        return (out,) + torch.autograd.grad(out, vs, gv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for seed in (5, 6):
        _, _, vf, _ = inputs(seed)
        _, _, _, hc = inputs(seed + 10)
        with torch.no_grad():
            vs.copy_(vf)
            gv.copy_(hc)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in held]
        eager = step()
        assert all(torch.equal(a, b.detach()) for a, b in zip(got, eager))
        assert all(bool(t.abs().sum() > 0) for t in got)
