"""``models.DeltaNetMultiscaleSegmentation`` on the MI355X at the smallest shapes that still take every path: 2 clouds of 256
points, ``ratios=(4, 2)`` (64, then 32 points a cloud), ``num_neighbors=16``, ``k_down=8``, ``k_up=3``,
``enc_channels=((16, 16), (32,), (32,))``, ``dec_channels=(32, 16)``, per-point labels.

1. the backbone equals, bit for bit, a composition written out here from the model's own layers (``Graph.knn``,
   ``build_grad_div``, ``CloudPair``): a wiring check
2. logits and every parameter gradient against an fp64 CPU composition (``oracle.nn.DeltaConv``, ``oracle.geometry`` and torch
   forms of the four transitions) on the same ``state_dict``, dropout off; the yardstick of ``test_model_step_vs_oracle``: the
   same composition in fp32 gives the reference error, the HIP path must be within 3 x that + 1e-3
3. two ``GraphedTrainStep`` replays equal two eager steps bit for bit, loss and parameters (the default three warm-up steps; after a
   single one the capture finds no weight planes and 64-column products run the exact chain where eager ones split: last-bit
   differences, for this model as for ``DeltaNetSegmentation``)
4. a ragged batch (256 and 200 points) runs eagerly and equals the per-cloud results: on the exact product chain the backbone
   features and the general-form logits to the bit, the uniform-batch form of the head within its forward error bound
5. ``num_neighbors=20`` with ``ratios=(4, 4)`` raises the ``ValueError`` that names level 2 before anything is launched
6. ``vector_pool="interpolate"`` and ``"max"`` give different logits"""
import numpy as np
import pytest
import torch

import oracle
from oracle import geometry as geo
from tests import connection_restate as CR
from tests.helpers import rel_err
from deltaconv_amd.data import Batch, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, N, CLASSES = 2, 256, 6
CFG = dict(enc_channels=((16, 16), (32,), (32,)), dec_channels=(32, 16), ratios=(4, 2), num_neighbors=16, k_down=8, k_up=3)
SIZES = (256, 64, 32)


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return model


def make(seed=1, **kw):
    import deltaconv_amd as dc
    torch.manual_seed(seed)
    return no_dropout(dc.models.DeltaNetMultiscaleSegmentation(3, CLASSES, **{**CFG, **kw}).to(DEV).train())


def batch(seed=70, **kw):
    return synthetic_batch(B, N, seed=seed, num_classes=CLASSES, per_point_labels=True, **kw)


# ---- 1. wiring -------------------------------------------------------------------------------------------------------------------------
def test_the_backbone_equals_a_composition_of_its_own_layers_bitwise():
    from deltaconv_amd.geometry import CloudPair, Graph, build_grad_div, build_tangent_basis
    from deltaconv_amd.geometry.graph import PtrInfo
    model, data = make(), batch().to(DEV)
    base = model.deltanet_base
    with torch.no_grad():
        got = [t.clone() for t in base(data)]
        logits = model(data)
        frames = (data.norm,) + tuple(build_tangent_basis(data.norm))
        levels = []
        for n in SIZES:
            rows = (torch.arange(B)[:, None] * N + torch.arange(n)[None, :]).reshape(-1).to(DEV)
            pos, fr = data.pos[rows], tuple(t[rows] for t in frames)
            ptr = (torch.arange(B + 1) * n).to(DEV)
            graph = Graph.knn(pos, 16, ptr_info=PtrInfo(ptr.to(torch.int32), B, n, n))
            levels.append((pos, fr, ptr, n, graph) + tuple(build_grad_div(pos, fr[0], fr[1], fr[2], graph, kernel_width=1,
                                                                          regularizer=0.001)))
        pairs = [CloudPair(f[0], c[0], f[2], c[2], 8, 3, f[1], c[1], max_fine_cloud=f[3], max_coarse_cloud=c[3])
                 for f, c in zip(levels[:-1], levels[1:])]
        ops = lambda l: (levels[l][5], levels[l][6], levels[l][4])
        x = data.pos
        v = levels[0][5] @ x
        x, v = base.enc[0][0](x, v, *ops(0))
        want = [x]
        x, v = base.enc[0][1](x, v, *ops(0))
        want.append(x)
        x0, v0 = x, v
        x, v = pairs[0].down(x, "max"), pairs[0].down_vectors(v, reduce="max")
        x, v = base.enc[1][0](x, v, *ops(1))
        x1, v1 = x, v
        x, v = pairs[1].down(x, "max"), pairs[1].down_vectors(v, reduce="max")
        x, v = base.enc[2][0](x, v, *ops(2))
        x, v = base.dec[1](torch.cat([x1, pairs[1].up(x)], 1), torch.cat([v1, pairs[1].up_vectors(v)], 1), *ops(1))
        assert x.shape == (B * 64, 16) and v.shape == (2 * B * 64, 16)
        x, v = base.dec[0](torch.cat([x0, pairs[0].up(x)], 1), torch.cat([v0, pairs[0].up_vectors(v)], 1), *ops(0))
        want.append(x)
    assert len(got) == 3 and [tuple(t.shape) for t in got] == [(B * N, 16), (B * N, 16), (B * N, 32)] and logits.shape == (B * N, CLASSES)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    assert all(bool(torch.isfinite(t).all()) and bool(t.abs().sum() > 0) for t in got + [logits])


# ---- 2. against an fp64 composition on the CPU ------------------------------------------------------------------------------------
class OracleMultiscale(torch.nn.Module):
    """The same network from oracle.nn.DeltaConv / oracle.geometry and dense torch forms of the four transitions, in the dtype
    of its parameters; the parameter names are the model's."""

    def __init__(self):
        super().__init__()
        tnn, DC = torch.nn, oracle.nn.DeltaConv
        base = tnn.Module()
        base.enc = tnn.ModuleList([tnn.ModuleList([DC(3, 16, centralized=True), DC(16, 16)]), tnn.ModuleList([DC(16, 32)]),
                                   tnn.ModuleList([DC(32, 32)])])
        base.dec = tnn.ModuleList([DC(16 + 16, 32, vector=False), DC(32 + 32, 16)])
        self.deltanet_base = base
        self.lin_global = oracle.nn.MLP([64, 1024])
        self.segmentation_head = tnn.Sequential(
            oracle.nn.MLP([1024 + 64, 256]), tnn.Dropout(0.5), oracle.nn.MLP([256, 256]), tnn.Dropout(0.5), tnn.Linear(256, 128),
            tnn.LeakyReLU(negative_slope=0.2), tnn.Linear(128, CLASSES))

    @staticmethod
    def search(q, r, nq, nr, k):
        """Per cloud the k nearest rows of r for every row of q: chosen in fp32 as the device chooses (ascending
        ((dx*dx + dy*dy) + dz*dz), ties by the lower index), the squared distances in the dtype of q.  -> (idx absolute, d2)."""
        idx, d2 = [], []
        for b in range(B):
            Q, R = q[b * nq:(b + 1) * nq], r[b * nr:(b + 1) * nr]
            d = lambda Q, R: ((Q[:, None, 0] - R[None, :, 0]) ** 2 + (Q[:, None, 1] - R[None, :, 1]) ** 2) + (Q[:, None, 2] - R[None, :, 2]) ** 2
            order = torch.sort(d(Q.float(), R.float()), dim=1, stable=True).indices[:, :k]
            idx.append(order + b * nr)
            d2.append(d(Q, R).gather(1, order))
        return torch.cat(idx), torch.cat(d2)

    @staticmethod
    def rotations(idx, tframes, sframes):
        dt = np.float64 if tframes[0].dtype == torch.float64 else np.float32
        q = torch.arange(idx.shape[0])[:, None].expand_as(idx).reshape(-1)
        j = idx.reshape(-1)
        R = CR.transport(*(t[q].numpy() for t in tframes), sframes[0][j].numpy(), sframes[1][j].numpy(), True, dt)
        return torch.from_numpy(np.ascontiguousarray(R)).view(idx.shape[0], idx.shape[1], 4, 1)

    @staticmethod
    def carried(v, idx, R):
        a, b = v[0::2][idx], v[1::2][idx]                                        # [Nq, k, C]
        return a, b, R[:, :, 0] * a + R[:, :, 1] * b, R[:, :, 2] * a + R[:, :, 3] * b

    @staticmethod
    def rows2(u, w):
        return torch.stack([u, w], 1).reshape(2 * u.shape[0], u.shape[1])

    def forward(self, data):
        base = self.deltanet_base
        with torch.no_grad():
            frames = (data.norm,) + tuple(geo.build_tangent_basis(data.norm))
            levels = []
            for n in SIZES:
                rows = (torch.arange(B)[:, None] * N + torch.arange(n)[None, :]).reshape(-1)
                pos, fr = data.pos[rows], tuple(t[rows] for t in frames)
                ptr = [b * n for b in range(B + 1)]
                nbr = geo.knn(pos, 16, ptr)
                levels.append((pos, fr, n, nbr) + tuple(geo.build_grad_div(pos, fr[0], fr[1], fr[2], nbr, ptr, 1, 0.001)))
            trans = []
            for f, c in zip(levels[:-1], levels[1:]):
                down, _ = self.search(c[0], f[0], c[2], f[2], 8)
                up, d2 = self.search(f[0], c[0], f[2], c[2], 3)
                w = 1.0 / d2.clamp(min=1e-16)
                trans.append((down, self.rotations(down, c[1], f[1]), up, (w / w.sum(1, keepdim=True))[:, :, None],
                              self.rotations(up, f[1], c[1])))

        def go_down(l, x, v):
            down, R = trans[l][:2]
            a, b, tu, tv = self.carried(v, down, R)
            at = (a * a + b * b).argmax(1, keepdim=True)
            return x[down].max(1).values, self.rows2(tu.gather(1, at)[:, 0], tv.gather(1, at)[:, 0])

        def go_up(l, x, v):
            up, c, R = trans[l][2:]
            _, _, tu, tv = self.carried(v, up, R)
            return (c * x[up]).sum(1), self.rows2((c * tu).sum(1), (c * tv).sum(1))

        ops = lambda l: (levels[l][4], levels[l][5], levels[l][3])
        x = data.pos
        v = levels[0][4] @ x
        out, skips = [], []
        for l in range(3):
            for conv in base.enc[l]:
                x, v = conv(x, v, *ops(l))
                if l == 0:
                    out.append(x)
            if l < 2:
                skips.append((x, v))
                x, v = go_down(l, x, v)
        for l in (1, 0):
            ux, uv = go_up(l, x, v)
            x, v = base.dec[l](torch.cat([skips[l][0], ux], 1), torch.cat([skips[l][1], uv], 1), *ops(l))
        out.append(x)
        glob = self.lin_global(torch.cat(out, 1)).view(B, N, -1).max(1).values[data.batch]
        return self.segmentation_head(torch.cat([glob] + out, 1))


def test_model_step_vs_an_fp64_composition():
    b = batch(seed=71)
    model = make()
    ref32 = no_dropout(OracleMultiscale().train())
    ref64 = no_dropout(OracleMultiscale().double().train())
    sd = {k: t.detach().cpu() for k, t in model.state_dict().items()}
    ref32.load_state_dict(sd)
    ref64.load_state_dict(sd)
    l32 = ref32(b)
    oracle.loss.calc_loss(l32, b.y, smoothing=False).backward()
    l64 = ref64(Batch(b.pos.double(), b.batch, b.norm.double(), None, b.y, None, B))
    oracle.loss.calc_loss(l64, b.y, smoothing=False).backward()
    bd = b.to(DEV)
    ld = model(bd)
    oracle.loss.calc_loss(ld, bd.y, smoothing=False).backward()
    e_hip, e_ref = rel_err(ld, l64), rel_err(l32, l64)
    print(f"logits: hip-vs-f64 {e_hip:.2e}  composition32-vs-f64 {e_ref:.2e}")
    gmax = max(float(p.grad.abs().max()) for p in ref64.parameters() if p.grad is not None)
    worst_hip = worst_ref = 0.0
    for (n1, p1), (n2, p2), (n3, p3) in zip(model.named_parameters(), ref32.named_parameters(), ref64.named_parameters()):
        assert n1 == n2 == n3
        if p3.grad is None:
            assert p1.grad is None, n1
            continue
        scale = max(float(p3.grad.abs().max()), 1e-3 * gmax)
        worst_hip = max(worst_hip, float((p1.grad.cpu().double() - p3.grad).abs().max()) / scale)
        worst_ref = max(worst_ref, float((p2.grad.double() - p3.grad).abs().max()) / scale)
    print(f"worst per-parameter grad error: hip-vs-f64 {worst_hip:.2e}  composition32-vs-f64 {worst_ref:.2e}")
    assert e_hip < 3 * e_ref + 1e-3
    assert worst_hip < 3 * worst_ref + 1e-3


# ---- 3. the captured training step ---------------------------------------------------------------------------------------------------
def test_graphed_training_matches_eager():
    from deltaconv_amd.graph_step import GraphedTrainStep
    from deltaconv_amd.utils import calc_loss
    loss_fn = lambda out, y: calc_loss(out, y, smoothing=False)
    batches = [batch(seed=80 + i).to(DEV) for i in range(3)]

    def build():
        m = make(seed=5)
        return m, torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)

    def eager_step(m, opt, b):
        for p in m.parameters():
            p.grad = None
        loss = loss_fn(m(b), b.y)
        loss.backward()
        opt.step()
        return float(loss)

    m1, o1 = build()
    for _ in range(3):
        eager_step(m1, o1, batches[0])                                          # = the warm-up steps of the capture (its default)
    ref_losses = [eager_step(m1, o1, b) for b in (batches[1], batches[2])]
    m2, o2 = build()
    step = GraphedTrainStep(m2, loss_fn, batch(seed=80).to(DEV), optimizer=o2)
    losses = [float(step(b)) for b in (batches[1], batches[2])]
    assert losses == ref_losses
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for key in sd1:
        assert torch.equal(sd1[key], sd2[key]), key


# ---- 4. ragged batches -----------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24 * 1.001                                                        # unit roundoff of fp32, second order included


def general_head(model, feats, data):
    """The head of DeltaNetSegmentation in its general form (the one a ragged batch takes), from the model's own layers
    -> (logits, the head's input [x_max[batch] | features])."""
    from deltaconv_amd.models.deltanet_base import _ptr_info
    from deltaconv_amd.models.pool import broadcast_to_points, embed_and_pool
    from deltaconv_amd.nn.layer import cat_outputs
    from deltaconv_amd.nn.mlp import run_head
    info, n = _ptr_info(data), data.pos.shape[0]
    conv_cat = cat_outputs(feats)
    pooled = embed_and_pool(model.lin_global, conv_cat, info, with_mean=False)
    z = torch.cat([broadcast_to_points(pooled, data.batch, info, n), conv_cat], dim=1)
    return run_head(model.segmentation_head, z), z


def head_error_bound(model, z):
    """First-order forward error of the eval-mode head on input z, in fp64: every product sums K terms in SOME order, so it is
    within (K + 2) u sum |w| |z| of the exact value whatever the association (K - 1 additions, one rounding a product, the bias);
    the folded BatchNorm map within 5 u (|s h| + |t|) (its fp32 coefficients and two operations); an activation of slope <= 1
    passes an error on unamplified and rounds once.  Two fp32 evaluations that differ ONLY in how they associate -- the head's
    joined first product on a uniform batch against the plain one -- are each within this bound of the exact value."""
    from deltaconv_amd.nn import fused
    val, err = z.double(), torch.zeros_like(z, dtype=torch.float64)

    def linear(lin):
        nonlocal val, err
        w = lin.weight.double()
        b = lin.bias.double() if lin.bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
        err = err @ w.abs().T + (w.shape[1] + 2) * U * (val.abs() @ w.abs().T + b.abs())
        val = val @ w.T + b

    def act(slope):
        nonlocal val, err
        assert abs(slope) <= 1
        val = torch.where(val > 0, val, slope * val)
        err = err + U * val.abs()

    for mod in model.segmentation_head:
        if isinstance(mod, torch.nn.Dropout):
            continue
        if isinstance(mod, torch.nn.LeakyReLU):
            act(mod.negative_slope)
        elif isinstance(mod, torch.nn.Sequential):
            for blk in mod:
                linear(blk[0])
                bn = blk[1].bn
                scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
                shift = bn.bias.double() - bn.running_mean.double() * scale
                err = err * scale.abs() + 5 * U * ((val * scale).abs() + shift.abs())
                val = val * scale + shift
                act(fused.slope_of(blk[2]))
        else:
            linear(mod)
    return val, err


def test_a_ragged_batch_equals_the_per_cloud_results():
    """A cloud's result does not depend on what else is in the batch: every kernel this model adds works per cloud pair and per
    row.  The dense product the layers share (csrc/gemm.hip, launch_fast) does depend on the batch's ROW COUNT: a product whose
    rows, columns and depth fill whole tiles multiplies through the bf16 split products, a ragged one runs the exact fp32 chain.
    Cloud 0 alone gives the vector block of enc[1] 2 x 64 = 128 rows (whole tiles), inside the batch 2 x 114 = 228 (ragged): its
    v differs in the last bit, and everything behind it with it (measured: 2.8e-09 of 7.3e-03 there, 1.5e-08 of 0.18 in the decoder
    feature; cloud 1, 50 rows, is ragged either way and equal to the bit; the single-resolution DeltaNetBase does the same on a
    batch of 64 + 50 points).  So the comparison is made with every product on the exact chain (dc_set_option(3, 1), the switch of
    test_model_step_golden_exact_chain_fixed_bound), where that choice does not exist:

      * the three backbone features equal the per-cloud ones bit for bit
      * the logits equal, bit for bit, the head in its general form on each cloud's own features
      * the logits of model(cloud) -- the head joins the pooled half of its first product per cloud where the batch is uniform, as
        one cloud is: "same sum, different association" (deltanet_segmentation.py) -- lie within twice the head's forward error
        bound (head_error_bound: both associations are within it of the exact value)

    With the default products the level-0 encoder features (256 and 200 rows: ragged both ways) are held to the bit and the rest
    is printed."""
    from deltaconv_amd._lib import lib
    model = make().eval()                                                       # running statistics: a cloud does not see its neighbour
    data = synthetic_batch(2, 0, seed=72, num_classes=CLASSES, per_point_labels=True, sizes=(256, 200)).to(DEV)
    clouds = [Batch(data.pos[a:b].contiguous(), torch.zeros(b - a, dtype=torch.long, device=DEV), data.norm[a:b].contiguous(), None,
                    data.y[a:b], None, 1) for a, b in ((0, 256), (256, 456))]

    def run():
        with torch.no_grad():
            whole, feats = model(data), model.deltanet_base(data)
            alone = [(model(one), model.deltanet_base(one)) for one in clouds]
            general = [general_head(model, f, one) for (_, f), one in zip(alone, clouds)]
        return whole, feats, alone, general

    whole, feats, alone, _ = run()
    joined = [torch.cat([f[i] for _, f in alone]) for i in range(3)]
    print("default products: features, largest difference / largest entry:",
          [f"{float((f - j).abs().max()):.3e} / {float(f.abs().max()):.3e}" for f, j in zip(feats, joined)],
          f"logits {float((whole - torch.cat([l for l, _ in alone])).abs().max()):.3e} / {float(whole.abs().max()):.3e}")
    assert whole.shape == (456, CLASSES) and bool(torch.isfinite(whole).all())
    assert torch.equal(feats[0], joined[0]) and torch.equal(feats[1], joined[1])
    lib.raw("dc_set_option")(3, 1)
    try:
        whole, feats, alone, general = run()
        torch.cuda.synchronize()
    finally:
        lib.raw("dc_set_option")(3, 0)
    for i in range(3):
        assert torch.equal(feats[i], torch.cat([f[i] for _, f in alone])), i
    assert torch.equal(whole, torch.cat([l for l, _ in general]))
    worst = 0.0
    for (logits, _), (plain, z) in zip(alone, general):
        _, err = head_error_bound(model, z)
        diff = (logits.double() - plain.double()).abs()
        worst = max(worst, float((diff / (2 * err)).max()))
        assert bool((diff <= 2 * err).all())
    print(f"exact chain: features and general-form logits equal; model(cloud) against the general form: worst |difference| / bound = {worst:.3e}")


# ---- 5. / 6. -----------------------------------------------------------------------------------------------------------------------------
def test_a_level_smaller_than_num_neighbors_raises_before_any_launch(monkeypatch):
    from deltaconv_amd._lib import lib
    data = batch().to(DEV)
    model = make(num_neighbors=20, ratios=(4, 4))
    assert make(num_neighbors=20)(data).shape == (B * N, CLASSES)                 # ratios (4, 2): level 2 has 32 points >= 20
    names = []
    call = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    with pytest.raises(ValueError, match="level 2 has a cloud of 16 points"):
        model(data)
    assert not names


def test_interpolate_and_max_give_different_logits():
    data = batch().to(DEV)
    with torch.no_grad():
        a, b = make(vector_pool="max")(data), make(vector_pool="interpolate")(data)
    assert a.shape == b.shape and not torch.equal(a, b)
    assert float((a - b).abs().max()) > 1e-4
