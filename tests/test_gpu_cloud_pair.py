"""``geometry.CloudPair`` on the MI355X: one object for a pair of resolutions.  Its four methods equal the tensor-level calls they
stand for -- ``knn_pool``, ``knn_interpolate`` and ``knn_interpolate_vectors`` with the roles as documented -- bit for bit, forward
and gradient; every search, list and table is built once; a composition of all four, forward + backward, replays from a
``torch.cuda.graph`` to the eager bits.  3 clouds of 300, 257 and 40 points, the coarse clouds every 4th point, k_down = 8,
k_up = 3, frames from ``build_tangent_basis`` of random unit normals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (300, 257, 40)
K_DOWN, K_UP, C = 8, 3, 20
_cache = {}


def setup():
    if not _cache:
        from deltaconv_amd.geometry import build_tangent_basis
        rng = np.random.default_rng(21)
        fptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
        keep = np.concatenate([np.arange(fptr[b], fptr[b + 1], 4) for b in range(len(SIZES))])
        cptr = np.concatenate([[0], np.cumsum([len(range(0, n, 4)) for n in SIZES])]).astype(np.int64)
        pos = torch.from_numpy(rng.random((int(fptr[-1]), 3), dtype=np.float32)).to(DEV)
        normal = rng.standard_normal((int(fptr[-1]), 3))
        normal = torch.from_numpy((normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)).to(DEV)
        frames = (normal,) + tuple(build_tangent_basis(normal))
        pick = torch.from_numpy(keep).to(DEV)
        _cache.update(pos_f=pos, pos_c=pos[pick].contiguous(), fptr=torch.from_numpy(fptr).to(DEV), cptr=torch.from_numpy(cptr).to(DEV),
                      frames_f=frames, frames_c=tuple(t[pick].contiguous() for t in frames), nf=int(fptr[-1]), nc=int(cptr[-1]),
                      maxima=dict(max_fine_cloud=max(SIZES), max_coarse_cloud=int(np.diff(cptr).max())))
    return _cache


def pair(frames=True, **kw):
    from deltaconv_amd.geometry import CloudPair
    s = setup()
    fr = dict(frames_fine=s["frames_f"], frames_coarse=s["frames_c"]) if frames else {}
    return CloudPair(s["pos_f"], s["pos_c"], s["fptr"], s["cptr"], k_down=K_DOWN, k_up=K_UP, **fr, **s["maxima"], **kw)


def inputs(seed):
    s = setup()
    gen = torch.Generator().manual_seed(seed)
    mk = lambda n: (torch.randn(n, C, generator=gen) * 4).round().div(4).to(DEV)     # multiples of 0.25: ties among the maxima
    return mk(s["nf"]), mk(s["nc"]), mk(2 * s["nf"]), mk(2 * s["nc"])


def with_grad(fn, t, g):
    leaf = t.clone().requires_grad_(True)
    out = fn(leaf)
    assert out.requires_grad
    return out.detach(), torch.autograd.grad(out, leaf, g)[0]


def test_the_four_methods_equal_the_tensor_level_calls_bitwise():
    from deltaconv_amd.geometry import knn_interpolate, knn_interpolate_vectors, knn_pool
    s = setup()
    cp = pair()
    xf, xc, vf, vc = inputs(1)
    gf, gc, hf, hc = inputs(2)
    down = dict(ptr_x=s["fptr"], ptr_y=s["cptr"], differentiable=True)           # fine sources, coarse targets
    up = dict(ptr_x=s["cptr"], ptr_y=s["fptr"], differentiable=True)
    cases = []
    for reduce in ("max", "min", "sum", "mean"):
        cases.append((f"down {reduce}", lambda t, r=reduce: cp.down(t, r),
                      lambda t, r=reduce: knn_pool(t, s["pos_f"], s["pos_c"], k=K_DOWN, reduce=r, **down), xf, gc))
    cases.append(("up", cp.up, lambda t: knn_interpolate(t, s["pos_c"], s["pos_f"], k=K_UP, **up), xc, gf))
    cases.append(("down_vectors", cp.down_vectors,
                  lambda t: knn_interpolate_vectors(t, s["pos_f"], s["pos_c"], s["frames_f"], s["frames_c"], k=K_DOWN, **down), vf, hc))
    cases.append(("up_vectors", cp.up_vectors,
                  lambda t: knn_interpolate_vectors(t, s["pos_c"], s["pos_f"], s["frames_c"], s["frames_f"], k=K_UP, **up), vc, hf))
    for name, mine, theirs, t, g in cases:
        (out, grad), (want, wgrad) = with_grad(mine, t, g), with_grad(theirs, t, g)
        assert out.shape == g.shape and torch.equal(out, want), name
        assert grad.shape == t.shape and torch.equal(grad, wgrad), name
        assert bool(out.abs().sum() > 0) and bool(grad.abs().sum() > 0), name
        plain = mine(t)                                                          # an input without grad: the inference bits, unrecorded
        assert not plain.requires_grad and torch.equal(plain, out), name
        with torch.no_grad():
            assert not mine(t.clone().requires_grad_(True)).requires_grad
    # differentiable=False records nothing
    frozen = pair(differentiable=False)
    out = frozen.down(xf.clone().requires_grad_(True))
    assert not out.requires_grad and torch.equal(out, cp.down(xf))
    assert not frozen.up_vectors(vc.clone().requires_grad_(True)).requires_grad
    assert not any(key[0] == "lists" for key in frozen._built)


def test_every_piece_is_built_once(monkeypatch):
    from deltaconv_amd._lib import lib
    setup()                                                                     # (its own launches stay out of the count)
    names = []
    call = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    cp = pair()
    assert not names                                                            # nothing is built before its first use
    xf, xc, vf, vc = inputs(3)
    for _ in range(2):
        for fn, t in ((cp.down, xf), (cp.up, xc), (cp.down_vectors, vf), (cp.up_vectors, vc)):
            leaf = t.clone().requires_grad_(True)
            fn(leaf).sum().backward()
    count = {n: names.count(n) for n in set(names)}
    assert count == {"dc_knn_cross": 2, "dc_knn_cross_transpose": 2, "dc_knn_cross_transport": 2, "dc_knn_pool": 2,
                     "dc_knn_pool_backward": 2, "dc_knn_interpolate": 2, "dc_knn_interpolate_backward": 2,
                     "dc_knn_interpolate_vectors": 4, "dc_knn_interpolate_vectors_backward": 4}, count
    names.clear()
    ready = pair().prepare()
    assert sorted(names) == ["dc_knn_cross"] * 2 + ["dc_knn_cross_transport"] * 2 + ["dc_knn_cross_transpose"] * 2
    names.clear()
    ready.prepare()
    ready.up(ready.down(xf))
    assert sorted(names) == ["dc_knn_interpolate", "dc_knn_pool"]
    names.clear()
    pair(frames=False, differentiable=False).prepare()
    assert sorted(names) == ["dc_knn_cross"] * 2


def test_a_composition_of_all_four_is_capturable():
    s = setup()
    cp = pair().prepare()
    xs = torch.zeros((s["nf"], C), device=DEV, requires_grad=True)
    vs = torch.zeros((2 * s["nf"], C), device=DEV, requires_grad=True)
    gx, gv = torch.zeros((s["nf"], C), device=DEV), torch.zeros((2 * s["nf"], C), device=DEV)

    def step():
        a, b = cp.up(cp.down(xs)), cp.up_vectors(cp.down_vectors(vs))
        return (a, b) + torch.autograd.grad([a, b], [xs, vs], [gx, gv])

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
        xf, _, vf, _ = inputs(seed)
        gf, _, hf, _ = inputs(seed + 10)
        with torch.no_grad():
            for dst, src in ((xs, xf), (vs, vf), (gx, gf), (gv, hf)):
                dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach().clone() for t in held]
        eager = step()
        assert all(torch.equal(a, b.detach()) for a, b in zip(got, eager))
        assert all(bool(t.abs().sum() > 0) for t in got)


def test_refusals():
    s = setup()
    bare = pair(frames=False)
    _, _, vf, vc = inputs(7)
    with pytest.raises(ValueError, match="without frames"):
        bare.down_vectors(vf)
    with pytest.raises(ValueError, match="without frames"):
        bare.up_vectors(vc)
    from deltaconv_amd.geometry import CloudPair
    with pytest.raises(RuntimeError, match="pos_fine requires grad"):
        CloudPair(s["pos_f"].clone().requires_grad_(True), s["pos_c"], s["fptr"], s["cptr"])
    moving = (s["frames_c"][0].clone().requires_grad_(True),) + s["frames_c"][1:]
    with pytest.raises(RuntimeError, match="requires grad"):
        CloudPair(s["pos_f"], s["pos_c"], s["fptr"], s["cptr"], frames_fine=s["frames_f"], frames_coarse=moving)
    with pytest.raises(ValueError, match="k_down = 17"):
        CloudPair(s["pos_f"], s["pos_c"], s["fptr"], s["cptr"], k_down=17)
    with pytest.raises(ValueError, match="reduce"):
        bare.down(inputs(7)[0], reduce="median")
    with pytest.raises(ValueError, match="one row per fine point"):
        bare.down(inputs(7)[1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        bare.down(inputs(7)[0].cpu())
