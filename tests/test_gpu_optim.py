"""deltaconv_amd.optim.SGD (csrc/optim.hip: dc_sgd_step) against torch.optim.SGD -- the optimizer of the reference's
training scripts (experiments/train_modelnet.py:67: lr 0.1, momentum 0.9, weight decay 1e-4, cosine schedule).
Tolerance: 1e-6 of the parameter scale per step (fused multiply-adds here, separate roundings in ATen)."""
import pytest
import torch

from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1,), (3,), (5, 7), (4097,), (64, 64), (1024, 512), (40, 256), (256,)]


def _pair(shapes, seed=0, **kw):
    import deltaconv_amd as dc
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    return pa, pb, dc.optim.SGD(pa, **kw), torch.optim.SGD(pb, **kw), g


@pytest.mark.parametrize("kw", [dict(lr=0.1, momentum=0.9, weight_decay=1e-4), dict(lr=0.01, momentum=0.0, weight_decay=0.0),
                                dict(lr=0.5, momentum=0.5, weight_decay=1e-2)])
def test_sgd_matches_torch_over_steps(kw):
    pa, pb, oa, ob, g = _pair(SHAPES, **kw)
    sched_a = torch.optim.lr_scheduler.CosineAnnealingLR(oa, 6, eta_min=0.001)
    sched_b = torch.optim.lr_scheduler.CosineAnnealingLR(ob, 6, eta_min=0.001)
    for step in range(6):
        for a, b in zip(pa, pb):
            gr = torch.randn(*a.shape, generator=g).to(DEV)
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
        sched_a.step(); sched_b.step()                      # the learning rate moves between the steps
        for a, b in zip(pa, pb):
            assert rel_err(a, b) < 2e-6, (step, tuple(a.shape))
    if kw["momentum"] != 0.0:                               # (torch keeps no buffer without momentum)
        for a, b in zip(pa, pb):
            assert rel_err(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"]) < 2e-6


def test_sgd_many_tensors_unaligned_views_and_missing_grads():
    """> 96 tensors (two launches), parameters that are unaligned views of a larger buffer (scalar path), parameters without a
    gradient (skipped, like torch)."""
    import deltaconv_amd as dc
    g = torch.Generator().manual_seed(1)
    base_a = torch.randn(200 * 37 + 3, generator=g).to(DEV)
    base_b = base_a.clone()
    pa = [torch.nn.Parameter(base_a[1 + i * 37:1 + i * 37 + 35]) for i in range(200)]
    pb = [torch.nn.Parameter(base_b[1 + i * 37:1 + i * 37 + 35]) for i in range(200)]
    oa = dc.optim.SGD(pa, lr=0.1, momentum=0.9, weight_decay=1e-4)
    ob = torch.optim.SGD(pb, lr=0.1, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i % 7 == 3:
                a.grad = b.grad = None
                continue
            gr = torch.randn(35, generator=g).to(DEV)
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
    assert rel_err(base_a, base_b) < 2e-6
    assert torch.equal(base_a[:1], base_b[:1]) and torch.equal(base_a[-2:], base_b[-2:])       # nothing outside the views moved


def test_sgd_state_dict_and_fallback_groups():
    """state_dict round trip with torch.optim.SGD in both directions; a Nesterov group runs torch's own step."""
    import deltaconv_amd as dc
    pa, pb, oa, ob, g = _pair([(33,), (8, 8)], lr=0.1, momentum=0.9, weight_decay=1e-4)
    for a, b in zip(pa, pb):
        gr = torch.randn(*a.shape, generator=g).to(DEV)
        a.grad, b.grad = gr.clone(), gr.clone()
    oa.step(); ob.step()
    import copy
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))      # ours -> torch (deep copy: load_state_dict adopts same-dtype tensors)
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))      # and back
    for a, b in zip(pa, pb):
        gr = torch.randn(*a.shape, generator=g).to(DEV)
        a.grad, b.grad = gr.clone(), gr.clone()
    oa.step(); ob.step()
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 2e-6
    qa, qb = torch.nn.Parameter(torch.ones(5, device=DEV)), torch.nn.Parameter(torch.ones(5, device=DEV))
    na = dc.optim.SGD([qa], lr=0.1, momentum=0.9, nesterov=True)
    nb = torch.optim.SGD([qb], lr=0.1, momentum=0.9, nesterov=True)
    qa.grad, qb.grad = torch.full((5,), 2.0, device=DEV), torch.full((5,), 2.0, device=DEV)
    na.step(); nb.step()
    assert torch.equal(qa, qb)


def test_sgd_learning_rate_moves_between_graph_replays(monkeypatch):
    """The captured step reads the learning rate from a device scalar: a scheduler step between replays takes effect
    without a re-capture."""
    import deltaconv_amd as dc
    p = torch.nn.Parameter(torch.zeros(1000, device=DEV))
    p.grad = torch.ones(1000, device=DEV)
    opt = dc.optim.SGD([p], lr=0.5, momentum=0.0)
    opt.step()                                              # eager first step: state + device scalar exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    before = p.detach().clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.allclose(p, before - 0.5)
    opt.param_groups[0]["lr"] = 0.125
    opt.sync_lr()
    before = p.detach().clone()
    g.replay()
    torch.cuda.synchronize()
    assert torch.allclose(p, before - 0.125)
    q = torch.nn.Parameter(torch.zeros(4, device=DEV))
    q.grad = torch.ones(4, device=DEV)
    fresh = dc.optim.SGD([q], lr=0.1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)      # (no real capture: nothing to poison)
    with pytest.raises(RuntimeError, match="before capturing"):
        fresh.step()


def test_copy_many_one_launch_for_the_batch_load_and_the_first_layer_blocks():
    """dc_copy_many (csrc/optim.hip): several small, possibly row-strided copies of 4- / 8-byte elements in one launch == torch's
    copies; pairs it does not take (1-byte elements, host tensors) fall through to torch, empty ones are skipped."""
    from deltaconv_amd import _ops
    g = torch.Generator().manual_seed(0)
    n = 5000
    pos, wide = torch.rand(n, 3, generator=g).to(DEV), torch.zeros(n, 12, device=DEV)
    v, vpad = torch.rand(2 * n, 3, generator=g).to(DEV), torch.zeros(2 * n, 72, device=DEV)[:, 2:]
    y, ydst = torch.randint(0, 40, (32,), generator=g).to(DEV), torch.zeros(32, dtype=torch.int64, device=DEV)
    big, bigdst = torch.rand(3000, 130, generator=g).to(DEV)[:, 1:129], torch.zeros(3000, 128, device=DEV)
    i32, i32dst = torch.randint(0, 9, (777,), generator=g, dtype=torch.int32).to(DEV), torch.zeros(777, dtype=torch.int32, device=DEV)
    u8, u8dst = torch.randint(0, 255, (100, 7), generator=g, dtype=torch.uint8).to(DEV), torch.zeros(100, 7, dtype=torch.uint8, device=DEV)
    host, hostdst = torch.rand(10, 3, generator=g), torch.zeros(10, 3, device=DEV)
    empty, emptydst = torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV)
    pairs = [(pos, wide[:, :3]), (v, vpad[:, :3]), (y, ydst), (big, bigdst), (i32, i32dst), (u8, u8dst), (host, hostdst),
             (empty, emptydst)]
    _ops.copy_many(pairs)
    torch.cuda.synchronize()
    for src, dst in pairs:
        assert torch.equal(dst.cpu(), src.cpu())
    assert float(wide[:, 3:].abs().max()) == 0 and float(vpad[:, 3:].abs().max()) == 0      # nothing beyond the blocks
    # more pairs than one table holds (16 per launch)
    many = [(torch.full((50, 5), float(i), device=DEV), torch.zeros(50, 8, device=DEV)[:, :5]) for i in range(40)]
    _ops.copy_many(many)
    assert all(torch.equal(d, s) for s, d in many)
    # capturable: the copies of a captured graph replay with new source contents
    src, dst = torch.zeros(1000, 3, device=DEV), torch.zeros(1000, 4, device=DEV)
    _ops.copy_many([(src, dst[:, :3])])
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        _ops.copy_many([(src, dst[:, :3])])
    src.fill_(3.0)
    gr.replay()
    torch.cuda.synchronize()
    assert float(dst[:, :3].min()) == 3.0 and float(dst[:, 3].max()) == 0.0


# ---- Adam (experiments/train_shapeseg.py:82) -----------------------------------------------------------------------------------
def _adam_pair(shapes, seed=0, **kw):
    import deltaconv_amd as dc
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(*s, generator=g) for s in shapes]
    pa = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    pb = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    return pa, pb, dc.optim.Adam(pa, **kw), torch.optim.Adam(pb, foreach=False, **kw), g      # torch's single-tensor form


def _grads(pa, pb, g, scale=1.0):
    for a, b in zip(pa, pb):
        gr = (torch.randn(*a.shape, generator=g) * scale).to(DEV)
        a.grad, b.grad = gr.clone(), gr.clone()


@pytest.mark.parametrize("kw", [dict(lr=5e-3), dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)])
def test_adam_matches_torch_over_steps(kw):
    """dc_adam_step vs torch.optim.Adam (the reference's default, single-tensor form) over 8 steps with a StepLR schedule
    (train_shapeseg.py:83).  Tolerance: 2e-6 of the parameter scale per step for the parameters, 1e-6 for the moments."""
    pa, pb, oa, ob, g = _adam_pair(SHAPES, **kw)
    sa, sb = torch.optim.lr_scheduler.StepLR(oa, 3, gamma=0.1), torch.optim.lr_scheduler.StepLR(ob, 3, gamma=0.1)
    for step in range(8):
        _grads(pa, pb, g, scale=10.0 ** (step % 3 - 1))
        oa.step(); ob.step()
        sa.step(); sb.step()
        for a, b in zip(pa, pb):
            assert rel_err(a, b) < 2e-6 * (step + 1), (step, tuple(a.shape))
    for a, b in zip(pa, pb):
        assert rel_err(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) < 1e-6
        assert rel_err(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) < 1e-6
        assert float(oa.state[a]["step"]) == 8.0 == float(ob.state[b]["step"])
    assert len({id(oa.state[a]["step"]) for a in pa}) == 1                   # ONE device counter for the group


def test_adam_many_tensors_missing_grads_state_dict_and_fallback():
    """> 80 tensors (two launches, the step counter moves once), unaligned views (scalar path), parameters without a gradient;
    state_dict round trip with torch.optim.Adam in both directions (the loaded per-parameter counters are re-shared); an
    amsgrad group runs torch's own step."""
    import copy
    import deltaconv_amd as dc
    g = torch.Generator().manual_seed(1)
    base_a = torch.randn(170 * 37 + 3, generator=g).to(DEV)
    base_b = base_a.clone()
    pa = [torch.nn.Parameter(base_a[1 + i * 37:1 + i * 37 + 35]) for i in range(170)]
    pb = [torch.nn.Parameter(base_b[1 + i * 37:1 + i * 37 + 35]) for i in range(170)]
    oa, ob = dc.optim.Adam(pa, lr=5e-3), torch.optim.Adam(pb, lr=5e-3, foreach=False)
    skip = lambda i: i % 7 == 3
    for step in range(3):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if skip(i):
                a.grad = b.grad = None
                continue
            gr = torch.randn(35, generator=g).to(DEV)
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
    assert rel_err(base_a, base_b) < 5e-6
    assert torch.equal(base_a[:1], base_b[:1]) and torch.equal(base_a[-2:], base_b[-2:])
    assert float(oa.state[pa[0]]["step"]) == 3.0
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))       # ours -> torch
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))       # torch -> ours: every parameter comes back with its own counter
    for i, (a, b) in enumerate(zip(pa, pb)):
        if not skip(i):
            gr = torch.randn(35, generator=g).to(DEV)
            a.grad, b.grad = gr.clone(), gr.clone()
    oa.step(); ob.step()
    assert rel_err(base_a, base_b) < 5e-6
    assert float(oa.state[pa[0]]["step"]) == 4.0 and len({id(oa.state[a]["step"]) for i, a in enumerate(pa) if not skip(i)}) == 1
    qa, qb = torch.nn.Parameter(torch.ones(5, device=DEV)), torch.nn.Parameter(torch.ones(5, device=DEV))
    na, nb = dc.optim.Adam([qa], lr=0.1, amsgrad=True), torch.optim.Adam([qb], lr=0.1, amsgrad=True)
    qa.grad, qb.grad = torch.full((5,), 2.0, device=DEV), torch.full((5,), 2.0, device=DEV)
    na.step(); nb.step()
    assert rel_err(qa, qb) < 1e-6


def test_adam_in_a_captured_step():
    """Replays of a captured step advance the shared device counter (bias corrections move) and read the learning rate from
    its device scalar; the first step must be eager."""
    import deltaconv_amd as dc
    pa, pb, oa, ob, g = _adam_pair([(1000,), (64, 33)], lr=5e-3)
    _grads(pa, pb, g)
    oa.step(); ob.step()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        oa.step()
    ob.step()                                               # (the capture itself runs nothing)
    for rep in range(3):
        if rep == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 1e-3
            oa.sync_lr()
        gr.replay()
        if rep:
            ob.step()
        torch.cuda.synchronize()
    # both sides: one eager step, then three more with the same gradients, the last one at the lower learning rate
    assert float(oa.state[pa[0]]["step"]) == 4.0 and float(ob.state[pb[0]]["step"]) == 4.0
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 1e-5


# ---- launch tables at capacity (dc_sgd_step: 96 tensors per launch, dc_adam_step: 80) ------------------------------------------
# Empty parameters are skipped while a table fills: every window must start behind the last entry the previous one looked at.
# The reference is a float64 restatement of the kernels' formulas (csrc/optim.hip) with lr / momentum / weight decay / betas as
# the kernels receive them (fp32 scalars; Adam's betas as doubles).
NUMELS = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8193, 37, 64, 300]
BIG = (1 << 20) + 5                 # one tensor above 2^20 elements (257 chunks of 4096)


def _table_params(count, window, seed):
    """count parameters: empty ones at 0, at the window edge (window - 1, window), inside one window and at the end; numel
    tails around the float4 path and the 4096-element chunk; every fifth one a view at 1, 2 or 3 floats into its base (scalar
    path), next to aligned ones.  -> [(base, offset, numel)] (base: device tensor with guard elements on both sides)."""
    g = torch.Generator().manual_seed(seed)
    empty = {0, window - 1, window, count - 1, 10, 11, 12, 40}
    out = []
    for i in range(count):
        n = 0 if i in empty else (BIG if i == 7 else NUMELS[i % len(NUMELS)])
        off = (i % 3) + 1 if i % 5 == 2 else 0
        out.append((torch.randn(n + off + 5, generator=g).to(DEV), off, n))
    return out


def _f32(x):
    return x.astype("float32").astype("float64")


def _update_close(got, ref, lr):
    """got (fp32 parameter) within 2 fp32 spacings of the float64 reference plus 1e-5 of the learning rate."""
    import numpy as np
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    bound = 2 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + 1e-5 * lr
    return float((np.abs(got - ref) / bound).max(initial=0.0))


def _ulps(got, ref):
    """|got - ref| in units of the fp32 spacing at ref (both fp32 values)."""
    import numpy as np
    got, ref = got.detach().cpu().double().numpy(), ref.detach().cpu().double().numpy()
    return float((np.abs(got - ref) / np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64)).max(initial=0.0))


@pytest.mark.parametrize("count", [95, 96, 97, 192, 193, 300])
def test_sgd_table_windows_with_empty_parameters(count):
    """dc_sgd_step over 95 .. 300 tensors with empty ones at the window edges: after 3 steps every parameter and momentum buffer
    is within 1 ulp of the float64 restatement (rounded to fp32 at the kernel's two fmaf points: g' + momentum * buf and
    p - lr * buf), bit-identical to each tensor through dc_sgd_step on its own, and no guard element moved.  A tensor that two
    windows both hold is updated twice per step (hundreds of ulps off, and off the single-tensor bits)."""
    import numpy as np
    import deltaconv_amd as dc
    lr, mom, wd = 0.1, 0.9, 1e-4
    spec = _table_params(count, 96, seed=count)
    bases = [b.clone() for b, _, _ in spec]
    singles = [b.clone() for b, _, _ in spec]
    pa = [torch.nn.Parameter(b[o:o + n]) for b, (_, o, n) in zip(bases, spec)]
    ps = [torch.nn.Parameter(b[o:o + n]) for b, (_, o, n) in zip(singles, spec)]
    opt = dc.optim.SGD(pa, lr=lr, momentum=mom, weight_decay=wd)
    one = [dc.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd) for p in ps]
    ref_p = [b[o:o + n].double().cpu().numpy() for b, o, n in spec]
    ref_b = [np.zeros(n) for _, _, n in spec]
    lr32, mom32, wd32 = (float(np.float32(v)) for v in (lr, mom, wd))
    g = torch.Generator().manual_seed(1000 + count)
    for step in range(3):
        for i, (a, s) in enumerate(zip(pa, ps)):
            gr = torch.randn(a.numel(), generator=g)
            a.grad, s.grad = gr.to(DEV), gr.to(DEV)
            gd = gr.double().numpy()
            ref_b[i] = _f32(mom32 * ref_b[i] + _f32(wd32 * ref_p[i] + gd))
            ref_p[i] = _f32(ref_p[i] - lr32 * ref_b[i])
        opt.step()
        for o in one:
            o.step()
    torch.cuda.synchronize()
    for i, ((b0, o, n), a, s) in enumerate(zip(spec, pa, ps)):
        u = _ulps(a, torch.from_numpy(ref_p[i]))
        assert u <= 1.0, (i, n, "parameter ulps", u)
        u = _ulps(opt.state[a]["momentum_buffer"], torch.from_numpy(ref_b[i]))
        assert u <= 1.0, (i, n, "momentum buffer ulps", u)
        assert torch.equal(a, s) and torch.equal(opt.state[a]["momentum_buffer"], one[i].state[s]["momentum_buffer"]), (i, n)
        assert torch.equal(bases[i][:o], b0[:o]) and torch.equal(bases[i][o + n:], b0[o + n:]), (i, "guard elements moved")


@pytest.mark.parametrize("count", [79, 80, 81, 161])
def test_adam_table_windows_with_empty_parameters(count):
    """dc_adam_step over 79 .. 161 tensors with empty ones at the window edges (80 per launch): 3 steps against the float64
    restatement of torch's single-tensor Adam (parameters within 2 fp32 spacings + 1e-5 lr, moments within 1e-6 of their
    scale), against
    torch.optim.Adam(foreach=False), and bit-identical to each tensor on its own; the shared counter moved once per step and the
    last-workgroup ticket is back at zero."""
    import numpy as np
    import deltaconv_amd as dc
    lr, b1, b2, eps = 5e-3, 0.9, 0.999, 1e-8
    spec = _table_params(count, 80, seed=count)
    bases, singles, tb = ([b.clone() for b, _, _ in spec] for _ in range(3))
    view = lambda bs: [torch.nn.Parameter(b[o:o + n]) for b, (_, o, n) in zip(bs, spec)]
    pa, ps, pt = view(bases), view(singles), view(tb)
    opt = dc.optim.Adam(pa, lr=lr)
    one = [dc.optim.Adam([p], lr=lr) for p in ps]
    ot = torch.optim.Adam(pt, lr=lr, foreach=False)
    rp = [b[o:o + n].double().cpu().numpy() for b, o, n in spec]
    rm, rv = [np.zeros(n) for _, _, n in spec], [np.zeros(n) for _, _, n in spec]
    lr32 = float(np.float32(lr))
    g = torch.Generator().manual_seed(2000 + count)
    for step in range(3):
        t = step + 1
        for i, (a, s, q) in enumerate(zip(pa, ps, pt)):
            gr = torch.randn(a.numel(), generator=g)
            a.grad, s.grad, q.grad = gr.to(DEV), gr.to(DEV), gr.to(DEV)
            gd = gr.double().numpy()
            rm[i] = rm[i] + (1 - b1) * (gd - rm[i])
            rv[i] = b2 * rv[i] + (1 - b2) * gd * gd
            rp[i] = rp[i] - lr32 / (1 - b1 ** t) * (rm[i] / (np.sqrt(rv[i]) / np.sqrt(1 - b2 ** t) + eps))
        opt.step(); ot.step()
        for o in one:
            o.step()
    torch.cuda.synchronize()
    live = [a for a in pa if a.numel()]
    assert float(opt.state[live[0]]["step"]) == 3.0 and len({id(opt.state[a]["step"]) for a in pa}) == 1
    assert int(opt._ticket[live[0].device]) == 0
    for i, ((b0, o, n), a, s, q) in enumerate(zip(spec, pa, ps, pt)):
        st = opt.state[a]
        if n:
            assert _update_close(a, torch.from_numpy(rp[i]), lr) <= 1.0, (i, n)
            assert rel_err(st["exp_avg"], torch.from_numpy(rm[i])) < 1e-6 and rel_err(st["exp_avg_sq"], torch.from_numpy(rv[i])) < 1e-6
            assert rel_err(a, q) < 5e-6, (i, n)
        assert torch.equal(a, s) and torch.equal(st["exp_avg"], one[i].state[s]["exp_avg"]), (i, n)
        assert torch.equal(st["exp_avg_sq"], one[i].state[s]["exp_avg_sq"]), (i, n)
        assert torch.equal(bases[i][:o], b0[:o]) and torch.equal(bases[i][o + n:], b0[o + n:]), (i, "guard elements moved")


@pytest.mark.parametrize("step0", [1000, 100000])
def test_adam_bias_correction_at_large_step_counts(step0):
    """A state loaded at step 1000 / 10^5 (1 - b2^t far from 0 and below fp32's resolution of 1): the next update against the
    float64 formula and against torch.optim.Adam(foreach=False) loaded with the same state."""
    import copy
    import numpy as np
    import deltaconv_amd as dc
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    pa, pb, oa, ob, g = _adam_pair([(4099,), (64, 33), (1,)], seed=3, lr=lr)
    _grads(pa, pb, g)
    oa.step(); ob.step()
    sd = copy.deepcopy(ob.state_dict())
    for k, st in sd["state"].items():
        st["step"] = torch.tensor(float(step0))
        st["exp_avg"] = torch.randn(st["exp_avg"].shape, generator=g).to(DEV) * 0.1
        st["exp_avg_sq"] = torch.rand(st["exp_avg_sq"].shape, generator=g).to(DEV) * 0.01 + 1e-4
    oa.load_state_dict(copy.deepcopy(sd)); ob.load_state_dict(copy.deepcopy(sd))
    p0 = [p.detach().double().cpu() for p in pa]
    _grads(pa, pb, g)
    oa.step(); ob.step()
    torch.cuda.synchronize()
    t = step0 + 1
    for i, (a, b) in enumerate(zip(pa, pb)):
        st = sd["state"][i]
        gd = a.grad.double().cpu()
        m = st["exp_avg"].double().cpu() * b1 + (1 - b1) * gd
        v = st["exp_avg_sq"].double().cpu() * b2 + (1 - b2) * gd * gd
        ref = p0[i] - float(np.float32(lr)) / (1 - b1 ** t) * (m / (v.sqrt() / np.sqrt(1 - b2 ** t) + eps))
        assert _update_close(a, ref, lr) <= 1.0, i
        assert rel_err(a, b) < 1e-6
        assert float(oa.state[a]["step"]) == t == float(ob.state[b]["step"])


def test_adam_all_empty_group_counts_its_steps_like_torch():
    """A group whose parameters are all empty: nothing to launch, but torch counts the step (state created, step 1, 2)."""
    import deltaconv_amd as dc
    pa = [torch.nn.Parameter(torch.zeros(0, device=DEV)) for _ in range(3)]
    pb = [torch.nn.Parameter(torch.zeros(0, device=DEV)) for _ in range(3)]
    oa, ob = dc.optim.Adam(pa, lr=1e-3), torch.optim.Adam(pb, lr=1e-3, foreach=False)
    for _ in range(2):
        for a, b in zip(pa, pb):
            a.grad, b.grad = torch.zeros(0, device=DEV), torch.zeros(0, device=DEV)
        oa.step(); ob.step()
    assert len(oa.state) == len(ob.state) == 3
    assert [float(oa.state[a]["step"]) for a in pa] == [float(ob.state[b]["step"]) for b in pb] == [2.0] * 3


def test_adam_parameter_that_joins_late_or_sits_a_step_out_matches_torch():
    """Parameter 1 gets its first gradient at step 3, parameter 2 has none at step 2: torch counts steps per parameter, so their
    bias corrections differ from the group's -- 6 steps against torch.optim.Adam(foreach=False).  No state for a parameter
    before its first gradient (checked after the run)."""
    import deltaconv_amd as dc
    pa, pb, oa, ob, g = _adam_pair([(1000,), (257,), (64, 8), (3,)], seed=4, lr=5e-3)
    has_grad = lambda i, step: not ((i == 1 and step < 3) or (i == 2 and step == 2))
    for step in range(6):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if has_grad(i, step):
                gr = torch.randn(*a.shape, generator=g).to(DEV)
                a.grad, b.grad = gr.clone(), gr.clone()
            else:
                a.grad = b.grad = None
        oa.step(); ob.step()
        if step == 2:
            early = pa[1] in oa.state
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert rel_err(a, b) < 2e-6 * (step + 1), (step, i, rel_err(a, b))
    assert [float(oa.state[a]["step"]) for a in pa] == [float(ob.state[b]["step"]) for b in pb] == [6.0, 3.0, 5.0, 6.0]
    assert not early


def test_optimizer_host_bookkeeping_on_device_parameters():
    """The learning-rate cache holds one device scalar per group and keeps its address across load_state_dict (the loaded lr
    is written into it); `state` gains no entries for parameters that never had a gradient (SGD and Adam)."""
    import copy
    import deltaconv_amd as dc
    for cls in (dc.optim.SGD, dc.optim.Adam):
        ps = [torch.nn.Parameter(torch.randn(33, device=DEV)) for _ in range(4)]
        opt = cls([{"params": ps[:2]}, {"params": ps[2:]}], lr=0.01)
        for step in range(2):
            for i, p in enumerate(ps):
                p.grad = torch.randn(33, device=DEV) if i != 3 else None
            opt.step()
        assert len(opt.state) == 3 and ps[3] not in opt.state, cls
        assert sorted(opt._lr_dev) == [0, 1]
        addr = [opt._lr_dev[i][0].data_ptr() for i in (0, 1)]
        sd = copy.deepcopy(opt.state_dict())
        sd["param_groups"][1]["lr"] = 0.25
        opt.load_state_dict(sd)
        opt.sync_lr()
        for i, p in enumerate(ps):
            p.grad = torch.randn(33, device=DEV) if i != 3 else None
        opt.step()
        torch.cuda.synchronize()
        assert sorted(opt._lr_dev) == [0, 1] and [opt._lr_dev[i][0].data_ptr() for i in (0, 1)] == addr, cls
        assert float(opt._lr_dev[1][0]) == 0.25
        assert len(opt.state) == 3 and ps[3] not in opt.state, cls


# ---- the learning rate and the optimizer state under graph replay (deltaconv_amd/graph_step.py) -----------------------------------
class _TinyBatch:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(16, 256, generator=g).to(DEV)
        self.y = torch.randn(16, generator=g).to(DEV)


class _Tiny(torch.nn.Module):
    """Elementwise model (no library GEMM in the captured step)."""
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(7)
        self.a = torch.nn.Parameter(torch.randn(256, generator=g) * 0.5)
        self.c = torch.nn.Parameter(torch.randn(256, generator=g) * 0.1)
        self.w = torch.nn.Parameter(torch.randn(4, 64, generator=g) * 0.3)

    def forward(self, b):
        return (torch.tanh(b.x * self.a + self.c) * self.w.reshape(-1)).sum(1)


def _mse(out, y):
    return ((out - y) ** 2).mean()


def _copy_model(model):
    import copy
    twin = copy.deepcopy(model)
    for p in twin.parameters():
        p.grad = None
    return twin


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_graphed_step_after_load_state_dict_never_replays_old_state(which):
    """A GraphedTrainStep captured with dc.optim.SGD / Adam, then load_state_dict of a state whose lr and buffers / moments
    differ: the next call either raises the documented RuntimeError (parameters untouched) or updates exactly like an eager
    torch.optim step from the loaded state.  Replaying on the old lr or the old buffers fails."""
    import copy
    import deltaconv_amd as dc
    from deltaconv_amd.graph_step import GraphedTrainStep
    model = _Tiny().to(DEV)
    make = (lambda ps, cls: cls(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)) if which == "sgd" else \
        (lambda ps, cls: cls(ps, lr=5e-3))
    opt = make(model.parameters(), dc.optim.SGD if which == "sgd" else dc.optim.Adam)
    static = _TinyBatch(1)
    step = GraphedTrainStep(model, _mse, static, optimizer=opt, warmup=2)
    step()
    torch.cuda.synchronize()
    sd = copy.deepcopy(opt.state_dict())
    sd["param_groups"][0]["lr"] = 0.03 if which == "sgd" else 1e-3
    for st in sd["state"].values():
        for k in ("momentum_buffer", "exp_avg"):
            if k in st:
                st[k].mul_(-0.5)
    opt.load_state_dict(copy.deepcopy(sd))
    before = [p.detach().clone() for p in model.parameters()]
    batch = _TinyBatch(2)
    try:
        step(batch)
    except RuntimeError as e:
        assert "recapture()" in str(e)
        assert all(torch.equal(p, b) for p, b in zip(model.parameters(), before))
        return
    torch.cuda.synchronize()
    twin = _copy_model(model)
    with torch.no_grad():
        for p, b in zip(twin.parameters(), before):
            p.copy_(b)
    ref = torch.optim.SGD(twin.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4) if which == "sgd" else \
        torch.optim.Adam(twin.parameters(), lr=5e-3, foreach=False)
    _mse(twin(batch), batch.y).backward()
    ref.load_state_dict(copy.deepcopy(sd))
    ref.step()
    for p, q, b in zip(model.parameters(), twin.parameters(), before):
        assert rel_err(p - b, q.detach() - b) < 1e-3, ("the replay updated from the state of the capture",
                                                        rel_err(p - b, q.detach() - b))


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_graphed_step_follows_the_scheduler_without_sync_lr(which):
    """A scheduler steps between calls of a GraphedTrainStep (CosineAnnealingLR for SGD, StepLR for Adam) and nobody calls
    sync_lr(): every replay still applies the scheduler's current learning rate (read back from the update itself: SGD
    p' = p - lr buf, Adam p' = p - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps))."""
    import deltaconv_amd as dc
    from deltaconv_amd.graph_step import GraphedTrainStep
    model = _Tiny().to(DEV)
    if which == "sgd":
        opt = dc.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 4, eta_min=0.005)
    else:
        opt = dc.optim.Adam(model.parameters(), lr=5e-3)
        sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5)
    step = GraphedTrainStep(model, _mse, _TinyBatch(3), optimizer=opt, warmup=2)
    seen = []
    for k in range(4):
        lr = opt.param_groups[0]["lr"]
        before = [p.detach().double().clone() for p in model.parameters()]
        step(_TinyBatch(10 + k))
        torch.cuda.synchronize()
        for p, b in zip(model.parameters(), before):
            st = opt.state[p]
            if which == "sgd":
                upd = lr * st["momentum_buffer"].double()
            else:
                t = float(st["step"])
                upd = lr / (1 - 0.9 ** t) * (st["exp_avg"].double() / (st["exp_avg_sq"].double().sqrt() / (1 - 0.999 ** t) ** 0.5 + 1e-8))
            assert rel_err(b - p.detach().double(), upd) < 1e-3, (k, lr, rel_err(b - p.detach().double(), upd))
        seen.append(lr)
        sched.step()
    assert len(set(seen)) == 4, seen
