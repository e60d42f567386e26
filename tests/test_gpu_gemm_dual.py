"""A block's weight- and input-gradient products through one entry point (dc_linear_backward_both, dc_linear_bn_backward_both and
their _slabs forms): where csrc/gemm.hip holds the pair of kernel instantiations the two run as ONE launch (gemm_dual_kernel), else
as the launches of the separate calls.  Every workgroup of the paired launch runs the body of the single kernel on the same data
in the same order, so every comparison here is torch.equal against dc_gemm_tn / dc_linear_bn_backward_weight (+ the ordered slab
reduction, alone and through dc_gemm_tn_reduce_many) and dc_linear_backward_input / dc_linear_bn_backward_input.

Shapes: the smallest that reach each entry of the table -- a few hundred rows, (N, K) from {64, 128, 192, 256}^2, the
input-gradient tile forced through `tile`; the 128 x 128 weight-gradient tiles that stay on gemm_kernel are reached at few rows with
the wide-tiles option (11).  Which kernels ran is read from the profiler's kernel names (as tests/test_gpu_gemm_abi.py does)."""
import contextlib
import ctypes
import re

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.test_gpu_gemm_dma import Planes, _binades
from tests.test_gpu_gemm_tn_planes import _bn_coefficients, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7.5
SLOPE = 0.2

# instantiation tuples (BM, BN, AL, BL, MODE, EPI, PRO, X3, BP, DMA) of the table in csrc/gemm.hip
TN_PRO_128 = (128, 128, 1, 1, 0, 0, 1, 1, 0, 0)
TN_PRO_64 = (64, 64, 1, 1, 0, 0, 1, 0, 0, 0)
TN_PLAIN_64 = (64, 64, 1, 1, 0, 0, 0, 0, 0, 0)
DX_PRO_128 = (128, 128, 0, 0, 0, 0, 1, 2, 1, 0)
DX_PRO_64x128 = (64, 128, 0, 0, 0, 0, 1, 2, 1, 0)
DX_PRO_64 = (64, 64, 0, 0, 0, 0, 1, 2, 1, 0)
DX_PLAIN_128x64 = (128, 64, 0, 0, 0, 0, 0, 2, 1, 1)
# (pro, R, N, K, tile of the input gradient, wide-tiles option, IA, IB): dW [N, K], dX [R, K], dh [R, N]
PAIRED = [
    (True, 512, 256, 128, 4, 1, TN_PRO_128, DX_PRO_64x128),
    (True, 384, 128, 192, 3, 0, TN_PRO_64, DX_PRO_64),
    (True, 512, 192, 256, 1, 0, TN_PRO_64, DX_PRO_128),
    (False, 256, 256, 64, 2, 0, TN_PLAIN_64, DX_PLAIN_128x64),
]
IDS = ["pro128+64x128", "pro64+64", "pro64+128", "plain64+128x64"]


def _kernels(fn):
    """Names of the dense-product kernels that fn() launches, in order."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = sorted((e for e in prof.events() if re.search(r"gemm_(dual_|tn_planes_)?kernel<", e.name)), key=lambda e: e.time_range.start)
    return [e.name for e in ev]


def _ints(name):
    return tuple(int(v) for v in re.findall(r"-?\d+", name[name.index("<"):]))


@contextlib.contextmanager
def never_paired():
    with options(o14=1):
        yield


class Block:
    """Operands of one block's backward: dy [R, N] as a column block of a wider buffer, x [R, K], w [N, K] with its planes, and in the
    prologue form h [R, N] with the coefficients of dc_bn_act_backward_reduce."""

    def __init__(self, pro, R, N, K, seed=0):
        self.pro, self.R, self.N, self.K = pro, R, N, K
        self.dy_buf = _binades(R, N + 8, seed=seed + 1)
        self.dy = self.dy_buf[:, 4:4 + N]
        self.x = _binades(R, K, seed=seed + 2)
        self.w = _binades(N, K, seed=seed + 3)
        self.planes = Planes(self.w) if N % 32 == 0 and K % 32 == 0 else None
        self.h = self.coefs = None
        if pro:
            g = torch.Generator().manual_seed(seed + 4)
            self.h = torch.randn(R, N, generator=g).to(DEV)
            gamma = (torch.rand(N, generator=g) + 0.5).to(DEV)
            gamma[::3] *= -1
            beta = (torch.rand(N, generator=g) * 2 - 1).to(DEV)
            coef = _bn_coefficients(self.h, gamma, beta)
            nb = lib.raw("dc_bn_workspace_bytes")(R, N)
            ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
            self.coefs = torch.empty(5 * N, device=DEV)
            dg, db = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
            lib.call("dc_bn_act_backward_reduce", self.dy, self.dy.stride(0), self.h, N, R, N, coef[2], coef[3], coef[0], coef[1],
                     gamma, SLOPE, 1, dg, db, self.coefs, ws, nb)
        self.base = _binades(R, K, seed=seed + 5)
        torch.cuda.synchronize()
        self.inputs = [t.clone() for t in self._inputs()]

    def _inputs(self):
        return [t for t in (self.dy_buf, self.x, self.w, self.h, self.coefs) if t is not None]

    def inputs_intact(self):
        return all(torch.equal(a, b) for a, b in zip(self._inputs(), self.inputs))

    def workspace(self):
        nb = lib.raw("dc_gemm_tn_workspace_bytes")(self.R, self.N, self.K)
        return torch.empty((nb + 3) // 4, device=DEV)

    def dx_buffer(self, accumulate):
        """dX as a column block, 4 columns in, of a sentinel-filled buffer with a spare row."""
        buf = torch.full((self.R + 1, self.K + 8), SENT, device=DEV)
        view = buf[:self.R, 4:4 + self.K]
        view.copy_(self.base) if accumulate else view.fill_(float("nan"))
        return buf, view

    def dw_buffer(self):
        buf = torch.full((self.N + 1, self.K + 8), SENT, device=DEV)
        view = buf[:self.N, 4:4 + self.K]
        view.fill_(float("nan"))
        return buf, view

    def hint(self):
        if self.planes is not None:
            self.planes.hint(True)

    def _reduce_many(self, ws, slabs, dw):
        i64, i32 = ctypes.c_int64 * 1, ctypes.c_int32 * 1
        lib.call("dc_gemm_tn_reduce_many", i64(ws.data_ptr()), i64(dw.data_ptr()), i64(dw.stride(0)), i32(self.N), i32(self.K),
                 i32(slabs), None, 1)

    def _head(self):
        dy, ld = self.dy, self.dy.stride(0)
        return (dy, ld, self.h, self.N, self.coefs, SLOPE) if self.pro else (dy, ld)

    def separate(self, accumulate, tile, deferred):
        """The calls the new entry stands in for -> (dW buffer, dW, dX buffer, dX)."""
        R, N, K = self.R, self.N, self.K
        (wbuf, dw), (xbuf, dx), ws = self.dw_buffer(), self.dx_buffer(accumulate), self.workspace()
        slabs = ctypes.c_int32(0)
        tail = (ws, ws.numel() * 4, ctypes.byref(slabs)) if deferred else (dw, dw.stride(0), 0, ws, ws.numel() * 4)
        if self.pro:
            lib.call("dc_linear_bn_backward_weight" + ("_slabs" if deferred else ""), *self._head(), self.x, K, R, N, K, *tail)
        else:
            lib.call("dc_gemm_tn" + ("_slabs" if deferred else ""), self.dy, self.dy.stride(0), self.x, K, R, N, K, *tail)
        if deferred:
            self._reduce_many(ws, slabs.value, dw)
        self.hint()
        if self.pro:
            lib.call("dc_linear_bn_backward_input", *self._head(), self.w, K, R, N, K, dx, dx.stride(0), accumulate, tile)
        else:
            lib.call("dc_linear_backward_input", self.dy, self.dy.stride(0), self.w, K, R, N, K, dx, dx.stride(0), accumulate, tile)
        return wbuf, dw, xbuf, dx

    def both(self, accumulate, tile, deferred, bufs=None):
        R, N, K = self.R, self.N, self.K
        (wbuf, dw), (xbuf, dx), ws = bufs or (self.dw_buffer(), self.dx_buffer(accumulate), self.workspace())
        slabs = ctypes.c_int32(0)
        name = ("dc_linear_bn_backward_both" if self.pro else "dc_linear_backward_both") + ("_slabs" if deferred else "")
        self.hint()
        if deferred:
            lib.call(name, *self._head(), self.x, K, self.w, K, R, N, K, dx, dx.stride(0), accumulate, tile, ws, ws.numel() * 4,
                     ctypes.byref(slabs))
            self._reduce_many(ws, slabs.value, dw)
        else:
            lib.call(name, *self._head(), self.x, K, self.w, K, R, N, K, dw, dw.stride(0), 0, dx, dx.stride(0), accumulate, tile, ws,
                     ws.numel() * 4)
        return wbuf, dw, xbuf, dx


def _bits(t):
    return t.contiguous().view(torch.int32)


def _equal_buffers(got, want):
    """Whole buffers, sentinels included, bit for bit."""
    return torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[2]), _bits(want[2]))


def _sentinels_ok(res):
    wbuf, dw, xbuf, dx = res
    ok = True
    for buf, view in ((wbuf, dw), (xbuf, dx)):
        w = view.shape[1]
        ok = ok and bool((buf[:, :4] == SENT).all()) and bool((buf[:, 4 + w:] == SENT).all()) and bool((buf[-1] == SENT).all())
        ok = ok and bool(torch.isfinite(view).all())
    return ok


@pytest.fixture(scope="module")
def blocks():
    return {i: Block(c[0], c[1], c[2], c[3], seed=10 * n) for n, (i, c) in enumerate(zip(IDS, PAIRED))}


@pytest.mark.parametrize("case", PAIRED, ids=IDS)
def test_paired_call_gives_the_bits_of_the_separate_calls(case, blocks):
    pro, R, N, K, tile, wide, ia, ib = case
    blk = blocks[IDS[PAIRED.index(case)]]
    with options(o11=wide):
        for accumulate in (0, 1):
            for deferred in (False, True):
                want = blk.separate(accumulate, tile, deferred)
                got, again = blk.both(accumulate, tile, deferred), blk.both(accumulate, tile, deferred)
                with never_paired():
                    off = blk.both(accumulate, tile, deferred)
                torch.cuda.synchronize()
                assert _sentinels_ok(want) and _sentinels_ok(got)
                assert _equal_buffers(got, want), (accumulate, deferred)
                assert _equal_buffers(again, got) and _equal_buffers(off, want)
        assert torch.equal(got[3], blk.base + blk.both(0, tile, False)[3])          # the accumulate form adds the same product
        # one launch with the table's template arguments; with the switch at 1 the two single kernels
        names = _kernels(lambda: blk.both(0, tile, False))
        assert len(names) == 1 and "gemm_dual_kernel<" in names[0], names
        assert _ints(names[0]) == ia + ib, names[0]
        with never_paired():
            names = _kernels(lambda: blk.both(0, tile, False))
        assert [n.count("gemm_kernel<") for n in names] == [1, 1] and [_ints(n) for n in names] == [ia, ib], names
    assert blk.inputs_intact()


def _fallback_case(which):
    if which == "ragged":          # R not a multiple of 32: both products leave the unguarded mode
        return Block(True, 500, 128, 192, seed=100), 3, {}
    if which == "exact":           # the exact chain: the input gradient ignores the planes
        return Block(False, 256, 256, 64, seed=110), 2, dict(o3=1)
    if which == "unlisted":        # whole tiles, split products, but a pair the table leaves out (measured no faster)
        return Block(True, 512, 256, 128, seed=140), 1, dict(o11=1)
    return Block(True, 8320, 256, 256, seed=120), 1, {}      # 4 tiles x 65 slabs of 128 x 128: the plane-image kernel


@pytest.mark.parametrize("which", ["ragged", "exact", "planes", "unlisted"])
def test_fallbacks_run_two_kernels_with_the_same_bits(which):
    blk, tile, opts = _fallback_case(which)
    with options(**opts):
        for deferred in (False, True):
            want, got = blk.separate(1, tile, deferred), blk.both(1, tile, deferred)
            torch.cuda.synchronize()
            assert _sentinels_ok(got) and _equal_buffers(got, want), deferred
        names = _kernels(lambda: blk.both(0, tile, False))
    assert len(names) == 2 and not any("gemm_dual_kernel<" in n for n in names), names
    assert ("gemm_tn_planes_kernel<" in names[0]) == (which == "planes") and "gemm_kernel<" in names[1], names
    if which == "unlisted":
        assert [_ints(n) for n in names] == [TN_PRO_128, DX_PRO_128], names
    if which == "exact":
        assert _ints(names[0]) == TN_PLAIN_64 and _ints(names[1])[7:] == (0, 0, 0), names
    assert blk.inputs_intact()


def test_paired_call_in_a_captured_graph(blocks):
    case = PAIRED[1]
    blk, tile = blocks[IDS[1]], case[4]
    eager = blk.both(1, tile, False)
    torch.cuda.synchronize()
    bufs = (blk.dw_buffer(), blk.dx_buffer(1), blk.workspace())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        blk.both(1, tile, False, bufs)                    # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = blk.both(1, tile, False, bufs)
    for _ in range(2):
        bufs[0][1].fill_(float("nan"))
        bufs[1][1].copy_(blk.base)
        g.replay()
        torch.cuda.synchronize()
        assert _sentinels_ok(res) and _equal_buffers(res, eager)


def test_refusals():
    blk = Block(False, 64, 64, 64, seed=130)
    (_, dw), (_, dx), ws = blk.dw_buffer(), blk.dx_buffer(0), blk.workspace()
    s = torch.cuda.current_stream().cuda_stream
    fn = lib.raw("dc_linear_backward_both")
    p = lambda t: t.data_ptr()
    assert fn(None, 72, p(blk.x), 64, p(blk.w), 64, 64, 64, 64, p(dw), 72, 0, p(dx), 72, 0, 0, p(ws), ws.numel() * 4, s) == -1
    assert "null pointer" in lib.last_error()
    assert fn(p(blk.dy), 72, p(blk.x), 63, p(blk.w), 64, 64, 64, 64, p(dw), 72, 0, p(dx), 72, 0, 0, p(ws), ws.numel() * 4, s) == -1
    assert "bad size" in lib.last_error()
    assert fn(p(blk.dy), 72, p(blk.x), 64, p(blk.w), 64, 64, 64, 64, p(dw), 72, 0, p(dx), 72, 0, 0, p(ws), ws.numel() * 4 - 1, s) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(dx).all())


def test_model_gradients_do_not_depend_on_the_switch():
    """One reduced C2 step (2 clouds): every parameter gradient with the switch at 0 and at 1; paired launches ran only at 0."""
    from deltaconv_amd import configs
    from deltaconv_amd.utils import calc_loss
    torch.manual_seed(3)
    model = configs.build_model("C2").to(DEV).train()
    b = configs.make_batch("C2", 2, seed=5).to(DEV)
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def grads():
        model.load_state_dict(sd)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)                              # dropout
        calc_loss(model(b), b.y).backward()
        return [None if q.grad is None else q.grad.clone() for q in model.parameters()]
    on = grads()
    with never_paired():
        off = grads()
    assert sum(g is not None for g in on) > 10
    for a, c in zip(on, off):
        assert (a is None) == (c is None) and (a is None or torch.equal(_bits(a), _bits(c)))
    assert any("gemm_dual_kernel<" in n for n in _kernels(grads))
    with never_paired():
        assert not any("gemm_dual_kernel<" in n for n in _kernels(grads))
