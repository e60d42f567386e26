"""The parallel-transport module on the MI355X (csrc/connection.hip: ``dc_build_transport``, ``dc_angle_in_plane``,
``dc_rotate_around``, ``dc_transport_sum``, ``dc_transport_sum_backward``; ``deltaconv_amd.geometry.connection``) against the
numpy restatement of csrc/connection_math.h (tests/connection_restate.py, itself held to a g++ build of that header and to the
reference's fp64 output by tests/test_connection_host.py): connections, sums and gradients bit for bit; the two libm helpers
within twice the reference's own fp32 error on set (d) of tests/golden/connection.npz.  Measured on an MI355X, largest
|. - fp64|, reference fp32 / device: rotate_around 9.20e-08 / 1.21e-07, angle_in_plane 1.77e-07 / 2.65e-07.

The three property tests of the reference's test/geometry/test_connection.py run on the product API at that file's tolerances.
Its inputs are random; they are drawn on the host with ``torch.manual_seed(42)`` (the seed that file uses where it sets one), at
which the reference's own fp32 functions pass their assertions (rtol 1e-5 on an angle holds only while no drawn angle is near 0)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import connection_restate as R
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
F32, F64 = np.float32, np.float64
NAMES = ("tn", "tx", "ty", "sn", "sx")
_cache = {}


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gold():
    if "gold" not in _cache:
        _cache["gold"] = np.load(os.path.join(ROOT, "tests", "golden", "connection.npz"))
    return _cache["gold"]


def scene():
    if "scene" not in _cache:
        s = np.load(os.path.join(ROOT, "tests", "golden", "geom_normals_B2_N128_k20.npz"))
        _cache["scene"] = (s["normal_f32"], s["x_basis_f32"], s["y_basis_f32"], s["edge_index"])
    return _cache["scene"]


def knn_case(n, k):
    """a cloud of n points with frames and its kNN graph (built on the device) -> (nrm, xb, yb, Graph, nbr as numpy)"""
    if (n, k) not in _cache:
        from deltaconv_amd.geometry import Graph
        pos, nrm, xb, yb = R.cloud(n, 20 + n)
        g = Graph.knn(dev(pos), k)
        _cache[n, k] = (nrm, xb, yb, g, g.nbr.cpu().numpy())
    return _cache[n, k]


def hand_case():
    if "hand" not in _cache:
        from deltaconv_amd.geometry import Graph
        _, nrm, xb, yb = R.cloud(300, 23)
        nbr = R.hand_table()
        ei = torch.stack([torch.arange(300).repeat_interleave(nbr.shape[1]), torch.from_numpy(nbr.reshape(-1)).long()]).to(DEV)
        _cache["hand"] = (nrm, xb, yb, Graph.from_edge_index(ei, 300), nbr)
    return _cache["hand"]


def abi_transport(ins, flag, nbr=None):
    """dc_build_transport through the C ABI into a guarded buffer -> [M,4] numpy"""
    from deltaconv_amd._lib import lib
    m = ins[0].shape[0] if nbr is None else nbr.size
    whole = torch.full((GUARD + 4 * m + GUARD,), -9.0, device=DEV)
    out = whole[GUARD:GUARD + 4 * m]
    lib.call("dc_build_transport", *[dev(a) for a in ins], None if nbr is None else dev(nbr), 1 if nbr is None else nbr.shape[1],
             m, int(flag), out)
    torch.cuda.synchronize()
    assert bool((whole[:GUARD] == -9).all()) and bool((whole[GUARD + 4 * m:] == -9).all()), "guard words around out were written"
    return out.view(m, 4).cpu().numpy()


# ---- 1. the connection, pair form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1025])
def test_pair_form_equals_the_restatement_bitwise(m):
    ins = R.random_pairs(m, 100 + m)
    for flag in (True, False):
        assert np.array_equal(bits(abi_transport(ins, flag)), bits(R.transport(*ins, flag))), (m, flag)
    tn, tx, ty, sn, sx = ins                                                    # normals apart: the flip and the reflection
    for flag in (True, False):
        assert np.array_equal(bits(abi_transport((tn, tx, ty, -sn, sx), flag)), bits(R.transport(tn, tx, ty, -sn, sx, flag)))


def test_pair_form_on_the_golden_sets():
    from deltaconv_amd.geometry import build_transport
    g = gold()
    for tag, flags in (("a", "TF"), ("b", "T")):
        ins = [g[f"{tag}_{n}"] for n in NAMES]
        for f in flags:
            want = R.transport(*ins, f == "T")
            assert np.array_equal(bits(abi_transport(ins, f == "T")), bits(want)), (tag, f)
            got = build_transport(*[dev(a) for a in ins], non_oriented=f == "T")
            assert got.shape == (2048, 4) and np.array_equal(bits(got), bits(want))
            e_ref = np.abs(g[f"{tag}_out32_{f}"].astype(F64) - g[f"{tag}_out64_{f}"]).max()
            assert np.abs(got.cpu().numpy().astype(F64) - g[f"{tag}_out64_{f}"]).max() <= 2 * e_ref


def test_no_pairs_give_an_empty_result():
    from deltaconv_amd.geometry import build_transport
    from deltaconv_amd._lib import lib
    z = torch.empty((0, 3), device=DEV)
    out = build_transport(z, z, z, z, z)
    assert out.shape == (0, 4) and out.dtype == torch.float32
    assert lib.raw("dc_build_transport")(None, None, None, None, None, None, 1, 0, 1, None, None) == 0
    assert lib.raw("dc_build_transport")(None, None, None, None, None, None, 1, 5, 1, None, None) == -1 and "null" in lib.last_error()
    one = torch.zeros((1, 3), device=DEV)
    nb = torch.zeros((1, 1), dtype=torch.int32, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for k in (0, 256):
        assert lib.raw("dc_build_transport")(vp(one), vp(one), vp(one), vp(one), vp(one), vp(nb), k, 1, 1, vp(one), None) == -1


# ---- 2. the graph form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(37, 5), (37, 20), (300, 5), (300, 20)])
def test_graph_form_equals_the_pair_form_and_the_restatement(n, k):
    from deltaconv_amd.geometry import build_graph_transport, build_transport
    nrm, xb, yb, graph, nbr = knn_case(n, k)
    assert (nbr[:, 0] == np.arange(n)).all()
    dn, dx, dy = dev(nrm), dev(xb), dev(yb)
    row, col = graph.edge_index
    for flag in (True, False):
        want = R.graph_transport(nrm, xb, yb, nbr, flag)
        got = build_graph_transport(dn, dx, dy, graph, non_oriented=flag)
        assert got.shape == (n * k, 4) and np.array_equal(bits(got), bits(want))
        assert torch.equal(got, build_transport(dn[row], dx[row], dy[row], dn[col], dx[col], flag))
        assert torch.equal(got, build_graph_transport(dn, dx, dy, graph.edge_index, flag))
        assert np.array_equal(bits(abi_transport((nrm, xb, yb, nrm, xb), flag, nbr=nbr)), bits(want))
    assert bool((got.view(n, k, 4)[:, 0] == torch.tensor([1.0, 0, 0, 1], device=DEV)).all())        # self edges: the identity


def test_graph_form_on_the_golden_scene():
    from deltaconv_amd.geometry import build_graph_transport
    nrm, xb, yb, ei = scene()
    n = nrm.shape[0]
    k = ei.shape[1] // n
    got = build_graph_transport(dev(nrm), dev(xb), dev(yb), dev(ei))             # a plain centre-major edge_index
    want = R.graph_transport(nrm, xb, yb, ei[1].reshape(n, k))
    assert np.array_equal(bits(got), bits(want))
    g = gold()
    e_ref = np.abs(g["c_out32"].astype(F64) - g["c_out64"]).max()
    assert np.abs(got.cpu().numpy().astype(F64) - g["c_out64"]).max() <= 2 * e_ref
    own = ei[0] == ei[1]
    assert own.sum() == n and (got.cpu().numpy()[own] == np.array([1, 0, 0, 1], dtype=F32)).all()


# ---- 3. the reference's property tests on the product API ---------------------------------------------------------------------
def test_reference_rotate_around_properties():
    from deltaconv_amd.geometry import build_tangent_basis, rotate_around
    n = 1000
    torch.manual_seed(42)
    v = torch.rand(n, 3)
    v = v / torch.linalg.norm(v, dim=1, keepdim=True).clamp(1e-8)
    any_axis = torch.rand(n, 3).to(DEV)
    v = v.to(DEV)
    axis, _ = build_tangent_basis(v)
    ones = torch.ones(n, 1, device=DEV)
    assert torch.allclose(rotate_around(v, axis, torch.pi / 2 * ones), torch.linalg.cross(axis, v), 1e-4)
    assert torch.allclose(rotate_around(v, axis, torch.pi * ones), -v, atol=1e-4)
    assert torch.allclose(rotate_around(v, axis, 2 * torch.pi * ones), v, atol=1e-4)
    assert torch.allclose(rotate_around(v, any_axis, 2 * torch.pi * ones), v, atol=1e-4)
    assert rotate_around(v, axis, ones[:, 0]).shape == (n, 3)                   # angle [M] as well as [M,1]


def test_reference_angle_in_plane_properties():
    from deltaconv_amd.geometry import angle_in_plane, build_tangent_basis
    n = 1000
    torch.manual_seed(42)
    u = torch.zeros(n, 3)
    u[:, 0] = 1
    angle = torch.rand(n, 1) * torch.pi
    v = torch.concat([torch.cos(angle), torch.sin(angle), torch.zeros_like(angle)], dim=1)
    normal = torch.rand(n, 3)
    normal = (normal / torch.linalg.norm(normal, dim=1, keepdim=True).clamp(1e-8)).to(DEV)
    x_basis, y_basis = build_tangent_basis(normal)
    T = torch.stack([x_basis, y_basis, normal], dim=2)
    u = torch.bmm(T, u.to(DEV).unsqueeze(-1)).squeeze(-1)
    v = torch.bmm(T, v.to(DEV).unsqueeze(-1)).squeeze(-1)
    out_angle = angle_in_plane(u, v, normal)
    assert out_angle.isnan().sum() == 0
    assert out_angle.size() == (n, 1)
    assert torch.allclose(out_angle, angle.to(DEV))


def test_reference_build_transport_properties():
    from deltaconv_amd.geometry import build_tangent_basis, build_transport, rotate_around
    n = 1
    torch.manual_seed(42)
    target_n = torch.rand(n, 3)
    target_n = (target_n / torch.linalg.norm(target_n, dim=1, keepdim=True).clamp(1e-8)).to(DEV)
    target_x, target_y = build_tangent_basis(target_n)
    rotation_angle = (torch.rand(n) * 2 * torch.pi).to(DEV)
    source_x = rotate_around(target_x, target_n, rotation_angle)
    axis = rotate_around(target_x, target_n, torch.rand(n).to(DEV))
    axis = axis / torch.linalg.norm(axis, dim=1, keepdim=True).clamp(1e-8)
    basis_angle = (torch.rand(n) * 0.5 * torch.pi).to(DEV)
    source_n = rotate_around(target_n, axis, basis_angle)
    source_x = rotate_around(source_x, axis, basis_angle)
    out = build_transport(target_n, target_x, target_y, source_n, source_x, non_oriented=False)
    assert out.size() == (n, 4)
    assert out.isnan().sum() == 0
    out = out.view(-1, 2, 2)
    v = torch.rand(n, 2, 1).to(DEV)
    assert torch.allclose(torch.linalg.norm(v, dim=1), torch.linalg.norm(torch.bmm(out, v), dim=1))
    assert torch.allclose(out[:, 0, 0], torch.cos(rotation_angle))
    assert torch.allclose(out[:, 1, 0], torch.sin(rotation_angle))


# ---- 4. the two libm helpers against fp64 ---------------------------------------------------------------------------------------
def test_helpers_are_within_twice_the_reference_fp32_error():
    from deltaconv_amd.geometry import angle_in_plane, rotate_around
    g = gold()
    v, axis, angle = g["d_rot_v"], g["d_rot_axis"], g["d_rot_angle"]
    want = R.rotate_around(v, axis, angle)
    e_ref = np.abs(g["d_rot_out32"].astype(F64) - want).max()
    got = rotate_around(dev(v), dev(axis), dev(angle))
    e_own = np.abs(got.cpu().numpy().astype(F64) - want).max()
    print(f"rotate_around: |ref32 - fp64| {e_ref:.3e}, |device - fp64| {e_own:.3e}")
    assert got.shape == (1024, 3) and e_own <= 2 * e_ref
    assert torch.equal(got, rotate_around(dev(v), dev(axis), dev(angle)[:, None]))
    u, w, normal = g["d_ang_u"], g["d_ang_v"], g["d_ang_normal"]
    want = R.angle_in_plane(u, w, normal)
    e_ref = np.abs(g["d_ang_out32"].reshape(-1).astype(F64) - want).max()
    got = angle_in_plane(dev(u), dev(w), dev(normal))
    e_own = np.abs(got.cpu().numpy().reshape(-1).astype(F64) - want).max()
    print(f"angle_in_plane: |ref32 - fp64| {e_ref:.3e}, |device - fp64| {e_own:.3e}")
    assert got.shape == (1024, 1) and e_own <= 2 * e_ref


# ---- 5. the sums ------------------------------------------------------------------------------------------------------------------
def sum_cases():
    return [("knn37k5", knn_case(37, 5)), ("knn37k20", knn_case(37, 20)), ("knn300k5", knn_case(300, 5)),
            ("knn300k20", knn_case(300, 20)), ("hand", hand_case())]


@pytest.mark.parametrize("c", [1, 3, 64, 65, 130])
def test_transport_sum_and_its_gradient_equal_the_restatement_bitwise(c):
    from deltaconv_amd.geometry import build_graph_transport, transport_sum
    rng = np.random.default_rng(50 + c)
    for label, (nrm, xb, yb, graph, nbr) in sum_cases():
        n, k = nbr.shape
        conn = build_graph_transport(dev(nrm), dev(xb), dev(yb), graph)
        conn_np = conn.cpu().numpy()
        w = rng.random(n * k, dtype=F32)
        v, g = rng.standard_normal((2 * n, c)).astype(F32), rng.standard_normal((2 * n, c)).astype(F32)
        for reduce in ("sum", "mean"):
            scale = F32(1.0 / k) if reduce == "mean" else 1.0
            for weights in (None, w):
                coef = R.fold_weights(conn_np, weights)
                leaf = dev(v).requires_grad_(True)
                out = transport_sum(leaf, conn, graph, None if weights is None else dev(weights), reduce)
                assert out.shape == (2 * n, c) and out.requires_grad
                assert np.array_equal(bits(out), bits(R.transport_sum(v, coef, nbr, scale))), (label, c, reduce)
                out.backward(dev(g))
                assert np.array_equal(bits(leaf.grad), bits(R.transport_sum_backward(g, coef, nbr, scale))), (label, c, reduce)
        assert torch.equal(transport_sum(dev(v), conn, graph, reduce="add"), transport_sum(dev(v), conn, graph))


def laid_out(a, vec, fill=float("nan")):
    """a [rows,C] on the device inside a buffer with a leading dimension above C: 16-byte aligned rows (vec) or an odd leading
    dimension on a base one float off alignment (the scalar path).  -> (view, ld, whole buffer, mask of the view's floats)"""
    rows, c = a.shape
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    whole = torch.full((GUARD + rows * ld + GUARD,), fill, device=DEV)
    start = GUARD if vec else GUARD + 1
    view = whole[start:start + (rows - 1) * ld + c].as_strided((rows, c), (ld, 1))
    view.copy_(dev(a))
    touched = np.zeros(whole.numel(), dtype=bool)
    for r in range(rows):
        touched[start + r * ld:start + r * ld + c] = True
    assert (view.data_ptr() % 16 == 0) == vec
    return view, ld, whole, touched


@pytest.mark.parametrize("c", [3, 64])
def test_sums_through_the_c_abi_with_strided_rows(c):
    from deltaconv_amd._lib import lib
    nrm, xb, yb, graph, nbr = hand_case()
    n, k = nbr.shape
    coef = R.fold_weights(R.graph_transport(nrm, xb, yb, nbr), np.random.default_rng(3).random(n * k, dtype=F32))
    dcoef = dev(coef)
    tptr, tedge = graph.csc()
    wptr, wedge = R.csc(nbr)
    assert np.array_equal(tptr.cpu().numpy(), wptr) and np.array_equal(tedge.cpu().numpy(), wedge)
    rng = np.random.default_rng(60 + c)
    v, g, prior = (rng.standard_normal((2 * n, c)).astype(F32) for _ in range(3))
    scale = 0.25
    for vec in ((True, False) if c % 4 == 0 else (False,)):
        vin, ldv, _, _ = laid_out(v, vec)
        out, ldo, whole, touched = laid_out(np.zeros((2 * n, c), dtype=F32), vec, fill=-9.0)
        lib.call("dc_transport_sum", graph.nbr, n, k, dcoef, vin, c, ldv, scale, out, ldo)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(R.transport_sum(v, coef, nbr, scale))), (c, vec)
        assert (whole.cpu().numpy()[~touched] == -9.0).all(), "floats between the rows or around out were written"
        gin, ldg, _, _ = laid_out(g, vec)
        for accumulate in (0, 1):
            dv, ldd, whole, touched = laid_out(prior, vec, fill=-9.0)
            lib.call("dc_transport_sum_backward", tptr, tedge, n, k, dcoef, gin, c, ldg, scale, dv, ldd, accumulate)
            torch.cuda.synchronize()
            want = R.transport_sum_backward(g, coef, nbr, scale, into=prior if accumulate else None)
            assert np.array_equal(bits(dv), bits(want)), (c, vec, accumulate)
            assert (whole.cpu().numpy()[~touched] == -9.0).all(), "floats between the rows or around dv were written"


def test_sum_argument_errors_return_dc_err_arg():
    from deltaconv_amd._lib import lib
    nrm, xb, yb, graph, nbr = hand_case()
    n, k = nbr.shape
    coef = torch.zeros((n * k, 4), device=DEV)
    v, out = torch.ones((2 * n, 4), device=DEV), torch.full((2 * n, 4), -9.0, device=DEV)
    tptr, tedge = graph.csc()
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    fwd, bwd = lib.raw("dc_transport_sum"), lib.raw("dc_transport_sum_backward")

    def call_fwd(nb=graph.nbr, k=k, cf=coef, vv=v, C=4, ldv=4, o=out, ldo=4, n=n):
        return fwd(vp(nb), n, k, vp(cf), vp(vv), C, ldv, 1.0, vp(o), ldo, None)

    def call_bwd(tp=tptr, te=tedge, k=k, cf=coef, gg=v, C=4, ldg=4, o=out, ldo=4, n=n):
        return bwd(vp(tp), vp(te), n, k, vp(cf), vp(gg), C, ldg, 1.0, vp(o), ldo, 0, None)

    for kw, msg in ((dict(nb=None), "null"), (dict(cf=None), "null"), (dict(vv=None), "null"), (dict(o=None), "null"), (dict(k=0), "k"),
                    (dict(k=256), "k"), (dict(ldv=3), "leading"), (dict(ldo=3), "leading"), (dict(n=-1), "size"),
                    (dict(cf=coef.view(-1)[1:]), "aligned")):
        assert call_fwd(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    for kw, msg in ((dict(tp=None), "null"), (dict(te=None), "null"), (dict(cf=None), "null"), (dict(gg=None), "null"),
                    (dict(o=None), "null"), (dict(k=0), "k"), (dict(k=256), "k"), (dict(ldg=3), "leading"), (dict(ldo=3), "leading")):
        assert call_bwd(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    assert call_fwd(n=0) == 0 and call_fwd(C=0) == 0 and call_bwd(n=0) == 0 and call_bwd(C=0) == 0
    torch.cuda.synchronize()
    assert bool((out == -9).all())


# ---- 6. autograd: determinism, capture, refusals ----------------------------------------------------------------------------------
def test_backward_gives_the_same_bits_on_two_runs():
    from deltaconv_amd.geometry import build_graph_transport, transport_sum
    nrm, xb, yb, graph, nbr = hand_case()
    conn = build_graph_transport(dev(nrm), dev(xb), dev(yb), graph)
    rng = np.random.default_rng(70)
    v, g = dev(rng.standard_normal((600, 65)).astype(F32)), dev(rng.standard_normal((600, 65)).astype(F32))
    grads = []
    for _ in range(2):
        leaf = v.clone().requires_grad_(True)
        transport_sum(leaf, conn, graph, reduce="mean").backward(g)
        grads.append(leaf.grad)
    assert torch.equal(grads[0], grads[1])
    assert not transport_sum(v, conn, graph).requires_grad
    with torch.no_grad():
        assert not transport_sum(v.clone().requires_grad_(True), conn, graph).requires_grad


def test_forward_and_backward_are_capturable_in_one_graph():
    from deltaconv_amd.geometry import build_graph_transport, transport_sum
    nrm, xb, yb, graph, nbr = knn_case(300, 20)
    n, k, c = 300, 20, 64
    conn = build_graph_transport(dev(nrm), dev(xb), dev(yb), graph)
    coef = conn.cpu().numpy()
    vs = torch.zeros((2 * n, c), device=DEV, requires_grad=True)
    gs = torch.zeros((2 * n, c), device=DEV)

    def step():
        out = transport_sum(vs, conn, graph, reduce="mean")
        return out, torch.autograd.grad(out, vs, gs)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                  # loads the code objects and builds the CSC outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    cuda_graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cuda_graph):
        out, dv = step()
    rng = np.random.default_rng(80)
    for _ in range(2):
        v, g = rng.standard_normal((2 * n, c)).astype(F32), rng.standard_normal((2 * n, c)).astype(F32)
        with torch.no_grad():
            vs.copy_(dev(v))
            gs.copy_(dev(g))
        cuda_graph.replay()
        torch.cuda.synchronize()
        got_out, got_dv = out.detach().clone(), dv.clone()
        eager_out, eager_dv = step()
        assert torch.equal(got_out, eager_out.detach()) and torch.equal(got_dv, eager_dv)
        assert np.array_equal(bits(got_out), bits(R.transport_sum(v, coef, nbr, F32(1.0 / k))))
        assert np.array_equal(bits(got_dv), bits(R.transport_sum_backward(g, coef, nbr, F32(1.0 / k))))


def test_error_paths_raise():
    from deltaconv_amd.geometry import angle_in_plane, build_graph_transport, build_transport, rotate_around, transport_sum
    nrm, xb, yb, graph, nbr = knn_case(37, 5)
    dn, dx, dy = dev(nrm), dev(xb), dev(yb)
    conn = build_graph_transport(dn, dx, dy, graph)
    v = torch.ones((74, 4), device=DEV)
    hot = dn.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        build_transport(hot, dx, dy, dn, dx)
    with pytest.raises(RuntimeError, match="requires grad"):
        build_graph_transport(dn, hot, dy, graph)
    with pytest.raises(RuntimeError, match="requires grad"):
        angle_in_plane(dn, hot, dx)
    with pytest.raises(RuntimeError, match="requires grad"):
        rotate_around(dn, dx, torch.ones(37, device=DEV, requires_grad=True))
    with torch.no_grad():
        assert build_transport(hot, dx, dy, dn, dx).shape == (37, 4)            # no graph to cut: allowed
    with pytest.raises(RuntimeError, match="connection requires grad"):
        transport_sum(v, conn.clone().requires_grad_(True), graph)
    with pytest.raises(RuntimeError, match="weights requires grad"):
        transport_sum(v, conn, graph, weights=torch.ones(37 * 5, device=DEV, requires_grad=True))
    with pytest.raises(ValueError, match="connection"):
        transport_sum(v, conn[:-1], graph)
    with pytest.raises(ValueError, match="weights"):
        transport_sum(v, conn, graph, weights=torch.ones(7, device=DEV))
    with pytest.raises(ValueError, match="reduce"):
        transport_sum(v, conn, graph, reduce="max")
    with pytest.raises(ValueError, match="v must be"):
        transport_sum(v[:-1], conn, graph)
    with pytest.raises(ValueError, match="graph of 37 points"):
        transport_sum(torch.ones((80, 4), device=DEV), conn, graph)
    with pytest.raises(ValueError, match="target_x"):
        build_transport(dn, dx[:-1], dy, dn, dx)
    with pytest.raises(ValueError, match="angle"):
        rotate_around(dn, dx, torch.ones(36, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        build_transport(dn.cpu(), dx, dy, dn, dx)
