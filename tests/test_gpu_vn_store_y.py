"""First block of a VectorMLP with the combined output stored by the GEMM epilogue: `interleaved = 2` of
dc_linear_vn_stats_forward / dc_linear_vn_sums_forward writes y[2n, co] (y_u = P_u - Q_v, y_v = P_v + Q_u) instead of the
interleaved (P, Q) pair, `combine = 3` of the backward kernels reads that y and still writes the interleaved d(P, Q).
Both are the same single fp32 subtract / add of the same two floats wherever they run, so everything here is bitwise."""
import math

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 12345.0


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(DEV)


def _tol(k):            # the bound of tests/test_gpu_gemm.py for a product against fp64
    return 2e-6 * math.sqrt(k) + 1e-6


def _combine(pq):
    """Host-side vn_combine of an interleaved [2n, 2co] (P_c, Q_c) matrix -> y [2n, co] (one rounding per element)."""
    pu, qu, pv, qv = pq[0::2, 0::2], pq[0::2, 1::2], pq[1::2, 0::2], pq[1::2, 1::2]
    y = torch.empty(pq.shape[0], pq.shape[1] // 2, dtype=pq.dtype, device=pq.device)
    y[0::2] = pu - qv
    y[1::2] = pv + qu
    return y


class _Case:
    """Operands of one (n, co, K) product, shared by the runs that are compared."""

    def __init__(self, n, co, K):
        self.n, self.co, self.K = n, co, K
        self.v, self.w = _rand(2 * n, K, seed=20), _rand(2 * co, K, seed=21)
        self.gamma, self.beta = _rand(co, seed=22) + 1.5, _rand(co, seed=23)
        self.rm, self.rv = _rand(co, seed=24), _rand(co, seed=25) + 2

    def run(self, out, ld, interleaved, tile, sums=False):
        """-> (coef [4, co], running mean, running var), or the fp64 sums record with sums=True; `out` receives the product."""
        n, co, K = self.n, self.co, self.K
        nb = lib.raw("dc_linear_stats_workspace_bytes")(2 * n, 2 * co, K, tile)
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
        if sums:
            rec = torch.zeros(2, 2 * co + 1, dtype=torch.float64, device=DEV)      # the kernels write two records (SumsFin)
            lib.call("dc_linear_vn_sums_forward", self.v, K, self.w, K, n, co, K, out, ld, interleaved, rec, tile, ws, nb)
            return rec
        coef = torch.empty(4, co, device=DEV)
        rm, rv = self.rm.clone(), self.rv.clone()
        lib.call("dc_linear_vn_stats_forward", self.v, K, self.w, K, n, co, K, out, ld, interleaved, self.gamma, self.beta,
                 1e-5, 0.1, rm, rv, coef[0], coef[1], coef[2], coef[3], tile, ws, nb)
        return coef, rm, rv

    def reference(self, tile, misaligned=False):
        """(y, coef, rm, rv) through the (P, Q) pair: interleaved = 1, combined on the host.  misaligned: PQ starts 8 bytes
        behind a 16-byte boundary as well -- an output that is not 16-byte aligned sends the product down the guarded path,
        whose exact chain differs from the split products of whole tiles in the last bits, whatever is stored."""
        flat = torch.empty(4 * self.n * self.co + 2, device=DEV)
        pq = flat[2:].view(2 * self.n, 2 * self.co) if misaligned else flat[:-2].view(2 * self.n, 2 * self.co)
        assert pq.data_ptr() % 16 == (8 if misaligned else 0)
        coef, rm, rv = self.run(pq, 2 * self.co, 1, tile)
        return _combine(pq), coef, rm, rv

    def fp64(self):
        return _combine(self.v.double() @ self.w.double().t())


def _check(case, y, got, tile, misaligned=False):
    y_ref, coef_ref, rm_ref, rv_ref = case.reference(tile, misaligned)
    coef, rm, rv = got
    assert torch.equal(y, y_ref)
    for q in range(4):
        assert torch.equal(coef[q], coef_ref[q]), q
    assert torch.equal(rm, rm_ref) and torch.equal(rv, rv_ref)
    assert rel_err(y, case.fp64()) < _tol(case.K)


SHAPES = [(1, 16, 32), (65, 20, 35), (500, 32, 70), (2048, 128, 256)]


@pytest.fixture
def exact_chain(request):
    opt = lib.raw("dc_set_option")
    if request.param:
        opt(3, 1)
    try:
        yield request.param
    finally:
        opt(3, 0)


@pytest.mark.parametrize("n,co,K", SHAPES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("exact_chain", [0, 1], indirect=True)
def test_store_y_bits(n, co, K, tile, exact_chain):
    case = _Case(n, co, K)
    buf = torch.full((2 * n + 2, co), CANARY, device=DEV)        # rows >= 2n: canary
    got = case.run(buf, co, 2, tile)
    _check(case, buf[:2 * n], got, tile)
    assert bool((buf[2 * n:] == CANARY).all())


@pytest.mark.parametrize("n,co,K,off,width", [(2048, 128, 256, 4, 136), (65, 20, 35, 3, 29), (500, 32, 70, 8, 44)])
@pytest.mark.parametrize("tile", [0, 3])
def test_store_y_column_block(n, co, K, off, width, tile):
    """ldpq > co: the output is a column block of a wider buffer; every other column and the rows behind stay untouched."""
    case = _Case(n, co, K)
    buf = torch.full((2 * n + 1, width), CANARY, device=DEV)
    got = case.run(buf[:, off:off + co], width, 2, tile)
    _check(case, buf[:2 * n, off:off + co], got, tile)
    assert bool((buf[:, :off] == CANARY).all()) and bool((buf[:, off + co:] == CANARY).all())
    assert bool((buf[2 * n:] == CANARY).all())


@pytest.mark.parametrize("n,co,K", [(2048, 128, 256), (65, 20, 35)])
@pytest.mark.parametrize("tile", [0, 1])
def test_store_y_eight_byte_aligned(n, co, K, tile):
    """An output that starts 8 bytes behind a 16-byte boundary takes the guarded store."""
    case = _Case(n, co, K)
    flat = torch.full((2 * n * co + 2 + 64,), CANARY, device=DEV)
    assert flat.data_ptr() % 16 == 0
    y = flat[2:2 + 2 * n * co].view(2 * n, co)
    assert y.data_ptr() % 16 == 8
    got = case.run(y, co, 2, tile)
    _check(case, y, got, tile, misaligned=True)
    assert bool((flat[:2] == CANARY).all()) and bool((flat[2 + 2 * n * co:] == CANARY).all())


@pytest.mark.parametrize("n,co,K", [(65, 20, 35), (2048, 128, 256)])
def test_store_y_sums(n, co, K):
    """The synchronised-BatchNorm form (statistics cut at the reduction) takes the same store."""
    case = _Case(n, co, K)
    pq = torch.empty(2 * n, 2 * co, device=DEV)
    ref = case.run(pq, 2 * co, 1, 0, sums=True)
    buf = torch.full((2 * n + 2, co), CANARY, device=DEV)
    rec = case.run(buf, co, 2, 0, sums=True)
    assert torch.equal(buf[:2 * n], _combine(pq)) and torch.equal(rec, ref)
    assert bool((buf[2 * n:] == CANARY).all())


def test_store_y_rejects_short_rows():
    case = _Case(4, 16, 32)
    with pytest.raises(RuntimeError, match="bad size"):
        case.run(torch.empty(8, 16, device=DEV), 15, 2, 0)


@pytest.mark.parametrize("n,co", [(1, 4), (65, 20), (2048, 128)])
@pytest.mark.parametrize("training", [1, 0])
def test_vn_backward_from_y(n, co, training):
    """combine = 3 on y against combine = 2 on the (P, Q) pair y was combined from."""
    pq = _rand(2 * n, 2 * co, seed=40)
    y = _combine(pq)
    dout = _rand(2 * n, co, seed=41)
    gamma, beta = _rand(co, seed=42) + 1.5, _rand(co, seed=43)
    coef = torch.empty(4, co, device=DEV)
    nb = lib.raw("dc_bn_workspace_bytes")(n, co)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    if training:
        lib.call("dc_vn_stats", y, n, co, co, 0, gamma, beta, 1e-5, 0.1, None, None, coef[0], coef[1], coef[2], coef[3], ws, nb)
    else:       # running statistics: scale / shift from stored moments
        mean, var = _rand(co, seed=44) * 0.2 + 0.6, _rand(co, seed=45) * 0.1 + 0.3
        coef[0], coef[1] = mean, (var + 1e-5).rsqrt()
        coef[2] = gamma * coef[1]
        coef[3] = beta - mean * coef[2]
    res = []
    for h, combine in ((pq, 2), (y, 3)):
        dh = torch.full((2 * n + 1, 2 * co), CANARY, device=DEV)
        dg, db = torch.empty(co, device=DEV), torch.empty(co, device=DEV)
        lib.call("dc_vn_backward", dout, co, h, h.shape[1], combine, n, co, coef[2], coef[3], coef[0], coef[1], gamma, training,
                 dh, 2 * co, dg, db, ws, nb)
        assert bool((dh[2 * n:] == CANARY).all())
        # the two halves of the synchronised form: this rank's sums, then the apply from given means
        sums = torch.zeros(2, 2 * co + 1, dtype=torch.float64, device=DEV)         # two records (SumsFin)
        lib.call("dc_vn_backward_sums", dout, co, h, h.shape[1], combine, n, co, coef[2], coef[3], coef[0], coef[1], sums, ws, nb)
        m1, m2 = _rand(co, seed=46) * 0.01, _rand(co, seed=47) * 0.01
        dh2 = torch.empty(2 * n, 2 * co, device=DEV)
        lib.call("dc_vn_backward_apply", dout, co, h, h.shape[1], combine, n, co, coef[2], coef[3], coef[0], coef[1], gamma,
                 training, m1, m2, dh2, 2 * co)
        res.append((dh[:2 * n], dg, db, sums, dh2))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(res[0][0]).all()) and float(res[0][0].abs().max()) > 0


def test_vn_backward_rejects_unknown_code():
    n, co = 4, 8
    y, dout, c = _rand(2 * n, co, seed=50), _rand(2 * n, co, seed=51), _rand(co, seed=52) + 1.5
    dh, dg, db = torch.empty(2 * n, 2 * co, device=DEV), torch.empty(co, device=DEV), torch.empty(co, device=DEV)
    nb = lib.raw("dc_bn_workspace_bytes")(n, co)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="bad size"):
        lib.call("dc_vn_backward", dout, co, y, co, 4, n, co, c, c, c, c, c, 1, dh, 2 * co, dg, db, ws, nb)
    with pytest.raises(RuntimeError, match="bad size"):       # code 3 writes [2n, 2co]: lddi = co is too short
        lib.call("dc_vn_backward", dout, co, y, co, 3, n, co, c, c, c, c, c, 1, dh, co, dg, db, ws, nb)


def _layer_run(conv, graph, G, D, x0, v0, sd0, store_y, train):
    from deltaconv_amd.nn import fused
    old = fused.VN_STORE_Y[0]
    fused.VN_STORE_Y[0] = store_y
    widths = []
    real = fused.linear_stats

    def tap(*a, **kw):
        out = real(*a, **kw)
        if kw.get("vn") == 2:
            widths.append(out[0].shape[1])
        return out
    fused.linear_stats = tap
    try:
        conv.load_state_dict(sd0)
        conv.zero_grad()
        conv.train(train)
        if not train:
            with torch.no_grad():
                xo, vo = conv(x0, v0, G, D, graph)
            grads = ()
        else:
            x = x0.clone().requires_grad_(True)
            v = v0.clone().requires_grad_(True)
            xo, vo = conv(x, v, G, D, graph)
            gen = torch.Generator(device=DEV).manual_seed(1)
            loss = (xo * torch.randn(xo.shape, device=DEV, generator=gen)).sum() + \
                   (vo * torch.randn(vo.shape, device=DEV, generator=gen)).sum()
            loss.backward()
            grads = (x.grad, v.grad) + tuple(None if p.grad is None else p.grad.clone() for p in conv.parameters())
        bufs = tuple(b.clone() for b in conv.buffers())
        return (xo.detach(), vo.detach()) + grads + bufs, widths
    finally:
        fused.linear_stats = real
        fused.VN_STORE_Y[0] = old


@pytest.mark.parametrize("ci,co", [(3, 16), (16, 32)])
def test_layer_switch_is_bitwise(ci, co):
    """One fused layer node with the switch on against off: outputs, every gradient and the BatchNorm buffers; in eval mode
    under no_grad both forms run the inference branch on the (P, Q) pair."""
    import deltaconv_amd as dc
    from deltaconv_amd.data import synthetic_batch
    b = synthetic_batch(2, 256, seed=60).to(DEV)
    graph = dc.geometry.Graph.knn(b.pos, 8, b.batch)
    xb, yb = dc.geometry.build_tangent_basis(b.norm)
    G, D = dc.geometry.build_grad_div(b.pos, b.norm, xb, yb, graph, b.batch)
    torch.manual_seed(7)
    conv = dc.nn.DeltaConv(ci, co, depth=1, centralized=False, vector=True).to(DEV)
    with torch.no_grad():
        for name, p in conv.named_parameters():
            if name.endswith("bn.weight"):
                g = torch.linspace(0.4, 1.6, p.numel(), device=DEV); g[::5] *= -1
                p.copy_(g)
            if name.endswith("bn.bias"):
                p.copy_(torch.linspace(-0.3, 0.3, p.numel(), device=DEV))
    assert conv._fusable() is not None
    x0 = torch.randn(graph.n, ci, device=DEV)
    v0 = torch.randn(2 * graph.n, ci, device=DEV)
    sd0 = {k: t.clone() for k, t in conv.state_dict().items()}
    for train in (True, False):
        on, w_on = _layer_run(conv, graph, G, D, x0, v0, sd0, True, train)
        off, w_off = _layer_run(conv, graph, G, D, x0, v0, sd0, False, train)
        assert w_on == [co if train else 2 * co] and w_off == [2 * co]      # the form that actually ran
        assert len(on) == len(off) and sum(a is not None for a in on) > (2 if not train else 6)
        for a, c in zip(on, off):
            assert (a is None) == (c is None)
            if a is not None:
                assert torch.equal(a, c)
