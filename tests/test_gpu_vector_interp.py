"""The transported interpolation of tangent-vector features on the MI355X (csrc/interp_transport.hip: ``dc_knn_cross_transport``,
``dc_knn_interpolate_vectors``, ``dc_knn_interpolate_vectors_backward``; ``geometry.vector_interpolate``;
``Propagator(frames=...).apply_vectors``) against the numpy restatement of csrc/interp_transport_math.h
(tests/vector_interp_restate.py, itself held to a g++ build of that header, to fp64 bounds and to the reference by
tests/test_vector_interp_host.py): table, forward and gradient bit for bit.  The shapes are the smallest at which the kernels can
still go wrong: pair boundaries inside a 256-chunk, a reference cloud with fewer than k points, an empty query cloud between two
others, in-lists longer than the backward keeps in flight and empty ones, whole and partial channel groups, the 16-byte and the
scalar path."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vector_interp_restate as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
CHANNELS = (1, 3, 4, 5, 64, 1021)                                               # 1021: 256 groups, the last of one channel (rpb = 1)
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def case(name):
    return {"three_pairs": lambda: V.batch_set("three_pairs"), "empty_middle": lambda: V.batch_set("empty_middle"),
            "k16": lambda: V.input_set(4, 513, 40, 16), "k1": lambda: V.input_set(3, 700, 700, 1), "hub": V.hub_set}[name]()


CASES = ("three_pairs", "empty_middle", "k16", "k1", "hub")


def restated(name):
    """-> (set, M, (tptr, tedge)) of a case, once."""
    if name not in _cache:
        S = case(name)
        M = V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], S["tframes"], S["sframes"])
        _cache[name] = (S, M, V.lists(S["idx"], S["d2"], S["qptr"], S["rptr"], len(S["pos_s"])))
    return _cache[name]


def laid_out(a, vec):
    """a [n,C] on the device with a leading dimension above C: 16-byte aligned rows (vec) or an odd leading dimension on a base one
    float off alignment (the scalar path).  The gaps hold NaN."""
    n, c = a.shape
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    whole = torch.full((n * ld + 8,), float("nan"), device=DEV)
    off = 0 if vec else 1
    view = whole[off:off + n * ld].view(n, ld)[:, :c]
    view.copy_(dev(a))
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


def in_pairs(ptr, n):
    mask = np.zeros(n, dtype=bool)
    for b in range(len(ptr) - 1):
        mask[int(ptr[b]):int(ptr[b + 1])] = True
    return mask


def device_table(S, flag=True):
    """dc_knn_cross_transport of the restated search into a guarded buffer (16-byte aligned: GUARD rows of 4 floats ahead)."""
    from deltaconv_amd._lib import lib
    nq, k = S["idx"].shape
    whole = torch.full((GUARD + nq * k + GUARD, 4), -9.0, device=DEV)
    tmat = whole[GUARD:GUARD + nq * k]
    fr = [dev(a) for a in S["tframes"] + S["sframes"][:2]]
    mq = int(np.diff(S["qptr"]).max())
    lib.call("dc_knn_cross_transport", dev(S["qptr"]), dev(S["rptr"]), len(S["qptr"]) - 1, nq, mq, k, dev(S["idx"]), dev(S["d2"]),
             *fr, int(flag), tmat)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == -9).all()) and bool((whole[GUARD + nq * k:] == -9).all()), "guard rows around tmat were written"
    return tmat


# ---- 1. device = fp32 restatement, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_table_equals_the_restatement_bitwise(name):
    S, M, _ = restated(name)
    for flag in (True, False):
        want = M if flag else V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], S["tframes"], S["sframes"], False)
        got = device_table(S, flag)
        assert np.array_equal(bits(got), bits(want)), (name, flag, np.argwhere(bits(got) != bits(want))[:5])
        assert torch.equal(device_table(S, flag), got)                          # a second launch: the same bits


def test_the_cases_cover_what_they_are_there_for():
    S, _, _ = restated("three_pairs")
    assert (S["idx"][int(S["qptr"][2]):, 2] == -1).all() and int(S["qptr"][1]) % 256 and int(S["qptr"][2]) % 256
    S, _, _ = restated("empty_middle")
    assert S["qptr"][1] == S["qptr"][2] and S["qptr"][1] > 0 and S["qptr"][3] > S["qptr"][2]
    _, _, (tptr, _) = restated("hub")
    assert sorted(np.diff(tptr)) == [0, 0, 14, 14]                              # no in-edge; more in-edges than the unroll (>= 9)


@pytest.mark.parametrize("name", CASES)
def test_forward_and_gradient_equal_the_restatement_bitwise(name):
    from deltaconv_amd._lib import lib
    S, M, (tptr, tedge) = restated(name)
    nq, k = S["idx"].shape
    nr, b = len(S["pos_s"]), len(S["qptr"]) - 1
    args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
    dqp, drp, didx, dtp, dte = dev(S["qptr"]), dev(S["rptr"]), dev(S["idx"]), dev(tptr), dev(tedge)
    tmat = dev(M)
    assert tmat.data_ptr() % 16 == 0
    mq, mr = int(np.diff(S["qptr"]).max()), int(np.diff(S["rptr"]).max())
    qin, rin = np.repeat(in_pairs(S["qptr"], nq), 2), np.repeat(in_pairs(S["rptr"], nr), 2)
    for c in CHANNELS:
        v, g = V.values(2 * nr, c, 10 + c), V.values(2 * nq, c, 20 + c)
        want_f, want_b = V.forward(v, *args, M), V.backward(g, tptr, tedge, M, k)
        for vec in (True, False):
            vin, ldv = laid_out(v, vec)
            out, whole, ldo, touched = guarded_rows(2 * nq, c, vec)
            run_f = lambda: lib.call("dc_knn_interpolate_vectors", vin, ldv, c, dqp, drp, b, mq, k, didx, tmat, out, ldo)
            run_f()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not np.isnan(got[qin]).any(), "a query row of a pair was not written"
            assert np.array_equal(bits(got[qin]), bits(want_f[qin])), (name, c, vec)
            full = whole.cpu().numpy()
            assert (full[~touched] == -9.0).all(), "floats between the rows or around the output were written"
            out.fill_(float("nan"))
            run_f()                                                             # a second launch: the same bits
            torch.cuda.synchronize()
            assert np.array_equal(bits(whole), bits(full)), (name, c, vec)

            gin, ldg = laid_out(g, vec)
            dv, whole, ldd, touched = guarded_rows(2 * nr, c, vec)
            run_b = lambda: lib.call("dc_knn_interpolate_vectors_backward", gin, ldg, nq, c, drp, b, mr, k, dtp, dte,
                                     int(dte.numel()), 0, tmat, nq * k, dv, ldd)
            run_b()
            torch.cuda.synchronize()
            got = dv.cpu().numpy()
            assert not np.isnan(got[rin]).any(), "a source row of a pair was not written"
            assert np.array_equal(bits(got[rin]), bits(want_b[rin])), (name, c, vec)
            full = whole.cpu().numpy()
            assert (full[~touched] == -9.0).all(), "floats between the rows or around the gradient were written"
            dv.fill_(float("nan"))
            run_b()
            torch.cuda.synchronize()
            assert np.array_equal(bits(whole), bits(full)), (name, c, vec)


def test_one_launch_per_pair_gives_the_same_bits():
    from deltaconv_amd.geometry import interpolate_vectors, interpolate_vectors_backward, knn_cross_transport
    S, M, (tptr, tedge) = restated("three_pairs")
    nq, k = S["idx"].shape
    nr, c = len(S["pos_s"]), 5
    dqp, drp, didx, dd2 = dev(S["qptr"]), dev(S["rptr"]), dev(S["idx"]), dev(S["d2"])
    tf, sf = tuple(dev(a) for a in S["tframes"]), tuple(dev(a) for a in S["sframes"])
    v, g = dev(V.values(2 * nr, c, 1)), dev(V.values(2 * nq, c, 2))
    out, dv = torch.zeros((2 * nq, c), device=DEV), torch.zeros((2 * nr, c), device=DEV)
    whole = knn_cross_transport(didx, dd2, dqp, drp, tf, sf)
    assert np.array_equal(bits(whole), bits(M))
    for b in range(3):
        interpolate_vectors(v, dqp[b:b + 2], drp[b:b + 2], didx, whole, int(np.diff(S["qptr"])[b]), out=out)
        interpolate_vectors_backward(g, drp[b:b + 2], dev(tptr), dev(tedge), whole, k, int(np.diff(S["rptr"])[b]), n_ref=nr, out=dv)
    args = (S["idx"], S["d2"], S["qptr"], S["rptr"])
    assert np.array_equal(bits(out), bits(V.forward(V.values(2 * nr, c, 1), *args, M)))
    assert np.array_equal(bits(dv), bits(V.backward(V.values(2 * nq, c, 2), tptr, tedge, M, k)))


# ---- 2. autograd --------------------------------------------------------------------------------------------------------------------
def test_knn_interpolate_vectors_differentiable_gives_the_restated_gradient():
    from deltaconv_amd.geometry import knn_interpolate_vectors
    S, M, (tptr, tedge) = restated("three_pairs")
    nq, k = S["idx"].shape
    nr, c = len(S["pos_s"]), 5
    v, g = V.values(2 * nr, c, 3), V.values(2 * nq, c, 4)
    tf, sf = tuple(dev(a) for a in S["tframes"]), tuple(dev(a) for a in S["sframes"])
    pos_x, pos_y = dev(S["pos_s"]), dev(S["pos_t"])
    kw = dict(k=k, ptr_x=dev(S["rptr"]), ptr_y=dev(S["qptr"]))
    leaf = dev(v).requires_grad_(True)
    out = knn_interpolate_vectors(leaf, pos_x, pos_y, sf, tf, differentiable=True, **kw)
    assert out.requires_grad and out.shape == (2 * nq, c)
    plain = knn_interpolate_vectors(leaf.detach(), pos_x, pos_y, sf[:2], tf, **kw)
    assert torch.equal(out.detach(), plain)                                     # the forward values: the inference path's bits
    assert np.array_equal(bits(plain), bits(V.forward(v, S["idx"], S["d2"], S["qptr"], S["rptr"], M)))
    out.backward(dev(g))
    want = V.backward(g, tptr, tedge, M, k)
    assert leaf.grad.dtype == torch.float32 and np.array_equal(bits(leaf.grad), bits(want))
    first = leaf.grad.clone()
    leaf.grad = None                                                            # a second forward + backward: the same bits
    knn_interpolate_vectors(leaf, pos_x, pos_y, sf, tf, differentiable=True, **kw).backward(dev(g))
    assert torch.equal(leaf.grad, first)
    with pytest.raises(RuntimeError, match="inference-only"):                   # the default refuses a v that requires grad
        knn_interpolate_vectors(leaf, pos_x, pos_y, sf, tf, **kw)
    with torch.no_grad():
        assert not knn_interpolate_vectors(leaf, pos_x, pos_y, sf, tf, **kw).requires_grad
    for which in range(3):                                                      # none of the geometry is differentiable
        bad = tuple(t.clone().requires_grad_(True) if i == which else t for i, t in enumerate(tf))
        with pytest.raises(RuntimeError, match="requires grad"):
            knn_interpolate_vectors(leaf.detach(), pos_x, pos_y, sf, bad, **kw)
    with pytest.raises(RuntimeError, match="requires grad"):
        knn_interpolate_vectors(leaf, pos_x, pos_y, (sf[0].clone().requires_grad_(True), sf[1]), tf, differentiable=True, **kw)


def test_forward_and_backward_are_capturable_in_one_graph():
    from deltaconv_amd.geometry import knn_interpolate_vectors
    S, M, (tptr, tedge) = restated("three_pairs")
    nq, k = S["idx"].shape
    nr, c = len(S["pos_s"]), 8
    tf, sf = tuple(dev(a) for a in S["tframes"]), tuple(dev(a) for a in S["sframes"])
    pos_x, pos_y = dev(S["pos_s"]), dev(S["pos_t"])
    kw = dict(k=k, ptr_x=dev(S["rptr"]), ptr_y=dev(S["qptr"]), differentiable=True, max_query_cloud=int(np.diff(S["qptr"]).max()),
              max_ref_cloud=int(np.diff(S["rptr"]).max()))
    vs = torch.zeros((2 * nr, c), device=DEV, requires_grad=True)
    gs = torch.zeros((2 * nq, c), device=DEV)

    def step():
        out = knn_interpolate_vectors(vs, pos_x, pos_y, sf, tf, **kw)
        return out, torch.autograd.grad(out, vs, gs)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, dv = step()
    for seed in (1, 2):
        v, g = V.values(2 * nr, c, 30 + seed), V.values(2 * nq, c, 40 + seed)
        with torch.no_grad():
            vs.copy_(dev(v))
            gs.copy_(dev(g))
        graph.replay()
        torch.cuda.synchronize()
        got_out, got_dv = out.detach().clone(), dv.clone()
        eager_out, eager_dv = step()
        assert torch.equal(got_out, eager_out.detach()) and torch.equal(got_dv, eager_dv)
        assert np.array_equal(bits(got_out), bits(V.forward(v, S["idx"], S["d2"], S["qptr"], S["rptr"], M)))
        assert np.array_equal(bits(got_dv), bits(V.backward(g, tptr, tedge, M, k)))


# ---- 3. Propagator --------------------------------------------------------------------------------------------------------------------
def stores(S):
    from deltaconv_amd.loader import DeviceDataset
    source = DeviceDataset(dev(S["pos_s"]), dev(S["rptr"]), np.diff(S["rptr"]), norm=dev(S["sframes"][0]))
    target = DeviceDataset(dev(S["pos_t"]), dev(S["qptr"]), np.diff(S["qptr"]), norm=dev(S["tframes"][0]))
    return source, target


def test_propagator_apply_vectors_and_its_gradient_equal_the_restatement():
    from deltaconv_amd import Propagator
    S, M, (tptr, tedge) = restated("three_pairs")
    nq, k = S["idx"].shape
    nr, c = len(S["pos_s"]), 5
    source, target = stores(S)
    frames = (tuple(dev(a) for a in S["sframes"]), tuple(dev(a) for a in S["tframes"]))
    prop = Propagator(source, target, k=k, differentiable=True, frames=frames)
    assert np.array_equal(bits(prop.tmat), bits(M))
    v, g = V.values(2 * nr, c, 5), V.values(2 * nq, c, 6)
    want_f = V.forward(v, S["idx"], S["d2"], S["qptr"], S["rptr"], M)
    want_b = V.backward(g, tptr, tedge, M, k)
    leaf = dev(v).requires_grad_(True)
    out = prop.apply_vectors(leaf)
    assert out.requires_grad and np.array_equal(bits(out), bits(want_f))
    assert torch.equal(out.detach(), Propagator(source, target, k=k, frames=frames).apply_vectors(dev(v)))
    out.backward(dev(g))
    assert np.array_equal(bits(leaf.grad), bits(want_b))
    # a range of clouds that does not start at cloud 0 against the store-wide lists and table (edge_base != 0)
    lo, hi = 1, 3
    q0, q1, r0, r1 = (int(S["qptr"][lo]), int(S["qptr"][hi]), int(S["rptr"][lo]), int(S["rptr"][hi]))
    part = dev(v[2 * r0:2 * r1]).requires_grad_(True)
    sub = prop.apply_vectors(part, (lo, hi))
    assert np.array_equal(bits(sub), bits(want_f[2 * q0:2 * q1]))
    sub.backward(dev(g[2 * q0:2 * q1]))
    assert np.array_equal(bits(part.grad), bits(want_b[2 * r0:2 * r1]))
    # nothing is recorded without the option, under no_grad, or for values that do not require grad
    assert not Propagator(source, target, k=k, frames=frames).apply_vectors(leaf).requires_grad
    assert not prop.apply_vectors(dev(v)).requires_grad
    with torch.no_grad():
        assert not prop.apply_vectors(leaf).requires_grad
    with pytest.raises(ValueError, match="out="):
        prop.apply_vectors(leaf, out=torch.empty_like(out))
    with pytest.raises(ValueError, match="two rows"):
        prop.apply_vectors(dev(v[:-2]))
    filled = prop.apply_vectors(dev(v), out=torch.full((2 * nq, c), float("nan"), device=DEV))
    assert np.array_equal(bits(filled), bits(want_f))


def test_propagator_frames_from_normals_equal_explicit_frames():
    from deltaconv_amd import Propagator
    from deltaconv_amd.geometry import build_tangent_basis
    from deltaconv_amd.loader import DeviceDataset
    S, _, _ = restated("three_pairs")
    source, target = stores(S)
    auto = Propagator(source, target, k=3, frames="normals")
    sframes = (source.norm,) + tuple(build_tangent_basis(source.norm))
    tframes = (target.norm,) + tuple(build_tangent_basis(target.norm))
    explicit = Propagator(source, target, k=3, frames=(sframes[:2], tframes))
    assert torch.equal(auto.tmat, explicit.tmat)
    want = V.table(S["idx"], S["d2"], S["qptr"], S["rptr"], tuple(t.cpu().numpy() for t in tframes),
                   tuple(t.cpu().numpy() for t in sframes))
    assert np.array_equal(bits(auto.tmat), bits(want))
    bare = DeviceDataset(source.pos, source.ptr, source.sizes)
    with pytest.raises(ValueError, match="normals"):
        Propagator(bare, target, k=3, frames="normals")
    with pytest.raises(ValueError, match="normals"):
        Propagator(source, DeviceDataset(target.pos, target.ptr, target.sizes), k=3, frames="normals")
    with pytest.raises(ValueError, match="frames"):
        Propagator(source, target, k=3, frames="tangent")
    with pytest.raises(RuntimeError, match="requires grad"):                    # frames are never differentiated
        Propagator(source, target, k=3, frames=(sframes, (tframes[0].clone().requires_grad_(True),) + tframes[1:]))
    with pytest.raises(ValueError, match="store's rows"):
        Propagator(source, target, k=3, frames=(sframes, tuple(t[:-1] for t in tframes)))


def test_propagator_with_a_mesh_target_uses_its_vertex_normals():
    from deltaconv_amd import DeviceMeshDataset, Propagator
    from deltaconv_amd.data import synthetic_mesh
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry import build_tangent_basis
    made = [synthetic_mesh(n, 20 + i) for i, n in enumerate((63, 200, 64))]
    items = [Data(pos=m[0], face=m[1]) for m in made]
    meshes = DeviceMeshDataset.from_dataset(items, DEV)
    sampled = meshes.sample_points(48, seed=1)
    assert sampled.norm is not None
    prop = Propagator(sampled, meshes, k=3, frames="normals")
    vn = meshes.vertex_normals()
    tframes = (vn,) + tuple(build_tangent_basis(vn))
    sframes = (sampled.norm,) + tuple(build_tangent_basis(sampled.norm))
    host = lambda fr: tuple(t.cpu().numpy() for t in fr)
    qptr, rptr = meshes.vptr.cpu().numpy(), sampled.ptr.cpu().numpy()
    idx, d2 = prop.idx.cpu().numpy(), prop.d2.cpu().numpy()
    M = V.table(idx, d2, qptr, rptr, host(tframes), host(sframes))
    assert np.array_equal(bits(prop.tmat), bits(M))
    v = V.values(2 * int(rptr[-1]), 4, 9)
    got = prop.apply_vectors(dev(v))
    assert got.shape == (2 * int(qptr[-1]), 4) and np.array_equal(bits(got), bits(V.forward(v, idx, d2, qptr, rptr, M)))


def test_propagator_without_frames_launches_what_it_did_and_refuses_vectors(monkeypatch):
    from deltaconv_amd import Propagator
    from deltaconv_amd._lib import lib
    S, _, _ = restated("three_pairs")
    source, target = stores(S)
    x = dev(V.values(len(S["pos_s"]), 6, 1))
    seen, call = [], lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (seen.append(name), call(name, *a))[1])
    plain = Propagator(source, target, k=3)
    want = plain.apply(x)
    assert seen == ["dc_knn_cross", "dc_knn_interpolate"] and plain.tmat is None
    with pytest.raises(RuntimeError, match="frames"):
        plain.apply_vectors(dev(V.values(2 * len(S["pos_s"]), 6, 1)))
    del seen[:]
    framed = Propagator(source, target, k=3, frames="normals")
    assert seen == ["dc_knn_cross", "dc_tangent_basis", "dc_tangent_basis", "dc_knn_cross_transport"]
    assert torch.equal(framed.apply(x), want)                                   # the scalar stream is unchanged by frames=
    assert torch.equal(framed.idx, plain.idx) and torch.equal(framed.d2, plain.d2)


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_reach_python_as_exceptions():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import (interpolate_vectors, interpolate_vectors_backward, knn_cross_transport,
                                        knn_interpolate_vectors)
    S, M, (tptr, tedge) = restated("three_pairs")
    nq, k = S["idx"].shape
    nr = len(S["pos_s"])
    dqp, drp, didx, dd2 = dev(S["qptr"]), dev(S["rptr"]), dev(S["idx"]), dev(S["d2"])
    tf, sf = tuple(dev(a) for a in S["tframes"]), tuple(dev(a) for a in S["sframes"])
    tmat, v, g = dev(M), dev(V.values(2 * nr, 4, 1)), dev(V.values(2 * nq, 4, 2))
    dtp, dte = dev(tptr), dev(tedge)
    pos_x, pos_y = dev(S["pos_s"]), dev(S["pos_t"])
    # wrong shapes
    with pytest.raises(ValueError, match=r"\[2n, C\]"):
        interpolate_vectors(v[:-1], dqp, drp, didx, tmat, 300)
    with pytest.raises(ValueError, match="tmat"):
        interpolate_vectors(v, dqp, drp, didx, tmat[:-1], 300)
    with pytest.raises(ValueError, match="tmat"):
        interpolate_vectors_backward(g, drp, dtp, dte, tmat.reshape(-1, 2), k, 40)
    with pytest.raises(ValueError, match="query normal"):
        knn_cross_transport(didx, dd2, dqp, drp, (tf[0][:-1], tf[1], tf[2]), sf)
    with pytest.raises(ValueError, match="two rows per point"):
        knn_interpolate_vectors(v[:-2], pos_x, pos_y, sf, tf, k=k, ptr_x=drp, ptr_y=dqp)
    with pytest.raises(ValueError, match="out must be"):
        interpolate_vectors(v, dqp, drp, didx, tmat, 300, out=torch.zeros((2 * nq, 5), device=DEV))
    # k outside [1, 16]
    with pytest.raises(ValueError, match="outside"):
        knn_interpolate_vectors(v, pos_x, pos_y, sf, tf, k=17, ptr_x=drp, ptr_y=dqp)
    with pytest.raises(ValueError, match="outside"):
        interpolate_vectors_backward(g, drp, dtp, dte, tmat, 0, 40)
    with pytest.raises(RuntimeError, match="k = 17"):
        lib.call("dc_knn_interpolate_vectors", v, 4, 4, dqp, drp, 3, 300, 17, didx, tmat, torch.zeros((2 * nq, 4), device=DEV), 4)
    with pytest.raises(RuntimeError, match="k = 0"):
        lib.call("dc_knn_cross_transport", dqp, drp, 3, nq, 300, 0, didx, dd2, *tf, *sf[:2], 1, torch.zeros((nq * k, 4), device=DEV))
    # an unaligned table
    off = torch.zeros(nq * k * 4 + 4, device=DEV)[1:1 + nq * k * 4].view(nq * k, 4)
    assert off.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="16-byte aligned"):
        interpolate_vectors(v, dqp, drp, didx, off, 300)
    with pytest.raises(ValueError, match="16-byte aligned"):
        interpolate_vectors_backward(g, drp, dtp, dte, off, k, 40)
    out, dv = torch.full((2 * nq, 4), -9.0, device=DEV), torch.full((2 * nr, 4), -9.0, device=DEV)
    for name, a in (("dc_knn_cross_transport", (dqp, drp, 3, nq, 300, k, didx, dd2, *tf, *sf[:2], 1, off)),
                    ("dc_knn_interpolate_vectors", (v, 4, 4, dqp, drp, 3, 300, k, didx, off, out, 4)),
                    ("dc_knn_interpolate_vectors_backward", (g, 4, nq, 4, drp, 3, 40, k, dtp, dte, int(dte.numel()), 0, off, nq * k,
                                                             dv, 4))):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            lib.call(name, *a)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    assert lib.raw("dc_knn_interpolate_vectors")(None, 4, 4, vp(dqp), vp(drp), 3, 300, k, vp(didx), vp(tmat), vp(out), 4, None) == -1
    assert "null" in lib.last_error()
    assert lib.raw("dc_knn_interpolate_vectors")(vp(v), 3, 4, vp(dqp), vp(drp), 3, 300, k, vp(didx), vp(tmat), vp(out), 4, None) == -1
    assert "ldv" in lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == -9).all()) and bool((dv == -9).all()) and not bool(off.any())      # nothing was launched
    # CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        interpolate_vectors(v.cpu(), dqp, drp, didx, tmat, 300)
    with pytest.raises(RuntimeError, match="no CPU path"):
        interpolate_vectors(v, dqp, drp, didx, tmat.cpu(), 300)
    with pytest.raises(RuntimeError, match="no CPU path"):
        interpolate_vectors_backward(g.cpu(), drp, dtp, dte, tmat, k, 40)
    with pytest.raises(RuntimeError, match="out must be a tensor on a HIP device"):
        interpolate_vectors(v, dqp, drp, didx, tmat, 300, out=torch.zeros((2 * nq, 4)))
    with pytest.raises(RuntimeError, match="out must be a tensor on a HIP device"):
        interpolate_vectors_backward(g, drp, dtp, dte, tmat, k, 40, out=torch.zeros((2 * nr, 4)))
    with pytest.raises(RuntimeError, match="tptr must be a tensor on a HIP device"):
        interpolate_vectors_backward(g, drp, dtp.cpu(), dte, tmat, k, 40)
    with pytest.raises(ValueError, match="tedge must be contiguous int64"):
        interpolate_vectors_backward(g, drp, dtp, dte.int(), tmat, k, 40)
    # offsets: a list or a host tensor is brought over (the same result), anything that is no [B+1] vector is refused
    want = interpolate_vectors(v, dqp, drp, didx, tmat, 300)
    assert torch.equal(interpolate_vectors(v, S["qptr"].tolist(), drp.cpu(), didx, tmat, 300), want)
    assert torch.equal(interpolate_vectors_backward(g, S["rptr"].tolist(), dtp, dte, tmat, k, 40),
                       interpolate_vectors_backward(g, drp, dtp, dte, tmat, k, 40))
    with pytest.raises(ValueError, match="B\\+1 offsets"):
        interpolate_vectors(v, dqp, drp[:-1], didx, tmat, 300)
    with pytest.raises(ValueError, match="B\\+1 offsets"):
        interpolate_vectors_backward(g, drp.view(2, 2), dtp, dte, tmat, k, 40)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_cross_transport(didx.cpu(), dd2, dqp, drp, tf, sf)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_cross_transport(didx, dd2, dqp, drp, (tf[0].cpu(), tf[1], tf[2]), sf)
    with pytest.raises(RuntimeError, match="no CPU path"):
        knn_interpolate_vectors(v.cpu(), pos_x, pos_y, sf, tf, k=k, ptr_x=drp, ptr_y=dqp)
