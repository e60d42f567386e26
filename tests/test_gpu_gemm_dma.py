"""Plain dense products over pre-split weight planes (csrc/gemm.hip): the loop that brings the fp32 activation tiles into a ring of
three LDS buffers by LDS-DMA (switch 13 = 0, the default) against the loop that stages them through registers (13 = 1), in one
process.  The same floats reach the same MFMA operands in the same order, so every output is compared with torch.equal: forward,
input gradient (with and without accumulate), the BatchNorm-statistics and vector-statistics epilogues, and two deferred products
in one launch.  Shapes are the smallest at which the ring can go wrong: one K tile (32), a ring that has not wrapped (64, 96), one
that has (128, 160); every tile shape (forced through `tile`), one and several workgroups.  The weight planes are cut here by
dc_presplit_weights."""
import contextlib

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.helpers import rel_err
from tests.test_gpu_gemm import _tol

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = [32, 64, 96, 128, 160]
# (tile, M, N): tile 1..4 = 128 x 128, 128 x 64, 64 x 64, 64 x 128; whole tiles only (anything else leaves the plane kernels)
CASES = [(1, 128, 128), (1, 640, 256), (2, 256, 64), (2, 128, 128), (3, 64, 64), (3, 640, 256), (4, 64, 128), (4, 256, 256)]


@contextlib.contextmanager
def staging(value):
    opt = lib.raw("dc_set_option")
    assert opt(13, value) == 0
    try:
        yield
    finally:
        opt(13, 0)


def _binades(*shape, seed):
    """Normal values scaled by 2^-6 .. 2^6 per element: every plane of the split carries bits."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-6, 7, shape, generator=g).float())).to(DEV)


class Planes:
    """The bf16 planes of w [n, k] and of its transpose, cut by dc_presplit_weights (one record)."""

    def __init__(self, w):
        n, k = w.shape
        assert n % 32 == 0 and k % 32 == 0 and w.is_contiguous()
        self.w, self.n, self.k = w, n, k
        self.fwd = torch.zeros(3 * n * k, dtype=torch.int16, device=DEV)
        self.bwd = torch.zeros(3 * n * k, dtype=torch.int16, device=DEV)
        chunks = n * k // 1024
        table = torch.tensor([[w.data_ptr(), self.fwd.data_ptr(), self.bwd.data_ptr(), n, k, k]], dtype=torch.int64).to(DEV)
        lib.call("dc_presplit_weights", table, torch.tensor([0, chunks], dtype=torch.int32).to(DEV), 1, chunks)

    def hint(self, transposed):
        pl = self.bwd if transposed else self.fwd
        lib.raw("dc_gemm_next_b_planes")(self.w.data_ptr(), pl.data_ptr(), self.n * self.k, self.n if transposed else self.k,
                                         1 if transposed else 0)


def _both(run):
    """run() under the DMA loop and under the register loop."""
    with staging(0):
        a = run()
    with staging(1):
        b = run()
    return a, b


def _forward(x, ldx, pl, M, tile):
    y = torch.full((M, pl.n), float("nan"), device=DEV)
    pl.hint(False)
    lib.call("dc_linear_forward", x, ldx, pl.w, pl.k, M, pl.n, pl.k, y, pl.n, tile)
    return y


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tile,M,N", CASES)
def test_forward_same_bits(tile, M, N, K):
    x, pl = _binades(M, K, seed=1), Planes(_binades(N, K, seed=2))
    a, b = _both(lambda: _forward(x, K, pl, M, tile))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("tile,M,N", CASES)
def test_backward_input_same_bits(tile, M, N, K):
    """dX[M, N] (+)= dY[M, K] W[K, N]: the reduction runs over W's rows (K of them), the planes are those of W^T."""
    dy, pl = _binades(M, K, seed=3), Planes(_binades(K, N, seed=4))
    base = _binades(M, N, seed=5)

    def run():
        out = []
        for acc in (0, 1):
            dx = base.clone() if acc else torch.full((M, N), float("nan"), device=DEV)
            pl.hint(True)
            lib.call("dc_linear_backward_input", dy, K, pl.w, N, M, K, N, dx, N, acc, tile)
            out.append(dx)
        return out
    (a0, a1), (b0, b1) = _both(run)
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    assert torch.equal(a1, base + a0)                     # the accumulate form adds the same product


@pytest.mark.parametrize("K", [32, 96, 160])
@pytest.mark.parametrize("tile,M,N", [(1, 640, 256), (2, 128, 128), (3, 640, 256), (4, 64, 128)])
def test_bn_stats_same_bits(tile, M, N, K):
    x, pl = _binades(M, K, seed=6), Planes(_binades(N, K, seed=7))
    g = torch.Generator().manual_seed(8)
    gamma, beta = (torch.rand(N, generator=g) + 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    rm0, rv0 = torch.randn(N, generator=g).to(DEV), (torch.rand(N, generator=g) + 1).to(DEV)
    nb = lib.raw("dc_linear_stats_workspace_bytes")(M, N, K, tile)

    def run():
        y, coef = torch.full((M, N), float("nan"), device=DEV), torch.full((4, N), float("nan"), device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
        pl.hint(False)
        lib.call("dc_linear_bn_stats_forward", x, K, pl.w, K, M, N, K, y, N, gamma, beta, 1e-5, 0.1, rm, rv, coef[0], coef[1],
                 coef[2], coef[3], tile, ws, nb)
        return y, coef, rm, rv
    a, b = _both(run)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bool(torch.isfinite(a[1]).all())


@pytest.mark.parametrize("K", [32, 96, 160])
@pytest.mark.parametrize("tile,n,co", [(1, 320, 128), (2, 64, 64), (3, 320, 64), (4, 32, 64)])
def test_vn_stats_stored_y_same_bits(tile, n, co, K):
    """interleaved = 2: the product over the stacked [2 co, K] weight, statistics of |y|, and the combined y[2n, co] stored."""
    v, pl = _binades(2 * n, K, seed=9), Planes(_binades(2 * co, K, seed=10))
    g = torch.Generator().manual_seed(11)
    gamma, beta = (torch.rand(co, generator=g) + 0.5).to(DEV), torch.randn(co, generator=g).to(DEV)
    rm0, rv0 = torch.randn(co, generator=g).to(DEV), (torch.rand(co, generator=g) + 1).to(DEV)
    nb = lib.raw("dc_linear_stats_workspace_bytes")(2 * n, 2 * co, K, tile)

    def run():
        y, coef = torch.full((2 * n, co), float("nan"), device=DEV), torch.full((4, co), float("nan"), device=DEV)
        rm, rv = rm0.clone(), rv0.clone()
        ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
        pl.hint(False)
        lib.call("dc_linear_vn_stats_forward", v, K, pl.w, K, n, co, K, y, co, 2, gamma, beta, 1e-5, 0.1, rm, rv, coef[0],
                 coef[1], coef[2], coef[3], tile, ws, nb)
        return y, coef, rm, rv
    a, b = _both(run)
    for u, w in zip(a, b):
        assert torch.equal(u, w)
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


@pytest.mark.parametrize("K", [32, 128, 160])
@pytest.mark.parametrize("tile,M,N", [(1, 256, 128), (3, 128, 64)])
def test_deferred_pair_same_bits(tile, M, N, K):
    """Two announced products of one instantiation between dc_finalisers_begin and dc_finalisers_end run as ONE launch
    (gemm_pair_kernel); the second has other rows, so the pair's two halves differ in size."""
    M2 = 2 * M
    x1, x2 = _binades(M, K, seed=12), _binades(M2, K, seed=13)
    p1, p2 = Planes(_binades(N, K, seed=14)), Planes(_binades(N, K, seed=15))
    g = torch.Generator().manual_seed(16)
    gamma, beta = (torch.rand(N, generator=g) + 0.5).to(DEV), torch.randn(N, generator=g).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def run():
        outs, keep = [], []
        assert lib.raw("dc_finalisers_begin")() == 0
        ok = False
        try:
            for x, pl, m in ((x1, p1, M), (x2, p2, M2)):
                nb = lib.raw("dc_linear_stats_workspace_bytes")(m, N, K, tile)
                ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
                y, coef = torch.full((m, N), float("nan"), device=DEV), torch.full((4, N), float("nan"), device=DEV)
                rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
                keep.append(ws)
                lib.raw("dc_finaliser_defer_next")()
                lib.raw("dc_gemm_defer_next")()
                pl.hint(False)
                lib.call("dc_linear_bn_stats_forward", x, K, pl.w, K, m, N, K, y, N, gamma, beta, 1e-5, 0.1, rm, rv, coef[0],
                         coef[1], coef[2], coef[3], tile, ws, nb)
                outs += [y, coef, rm, rv]
            ok = True
        finally:
            rc = lib.raw("dc_finalisers_end")(0 if ok else 1, stream)
        assert rc == 0, lib.last_error()
        torch.cuda.synchronize()
        return outs
    a, b = _both(run)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # the pair computes what the single launches compute
    single = _forward(x2, K, p2, M2, tile)
    assert torch.equal(a[4], single)


@pytest.mark.parametrize("K", [64, 160])
def test_operand_as_a_column_block_of_a_wider_buffer(K):
    """The embedding reads its operand as a column block of the layer buffer: lda > K, base offset a multiple of 16 bytes."""
    M, N = 256, 128
    buf = _binades(M, 3 * K + 8, seed=17)
    x = buf[:, K + 4:2 * K + 4]
    assert x.data_ptr() % 16 == 0 and x.stride(0) == 3 * K + 8
    pl = Planes(_binades(N, K, seed=18))
    for tile in (1, 3):
        a, b = _both(lambda: _forward(x, 3 * K + 8, pl, M, tile))
        assert torch.equal(a, b)
        assert torch.equal(a, _forward(x.contiguous(), K, pl, M, tile))       # the same rows from a dense copy


@pytest.mark.parametrize("tile,M,N,K", [(1, 640, 256, 160), (3, 640, 64, 96)])
def test_against_fp64(tile, M, N, K):
    """The DMA loop against a float64 product, under the bound of tests/test_gpu_gemm.py; on 64-column tiles the product
    without planes is the exact chain, so differing bits show that the plane kernels (the ones switch 13 selects between) ran."""
    g = torch.Generator().manual_seed(19)
    x = (torch.rand(M, K, generator=g) * 2 - 1).to(DEV)
    pl = Planes((torch.rand(N, K, generator=g) * 2 - 1).to(DEV))
    y = _forward(x, K, pl, M, tile)
    assert rel_err(y, x.double() @ pl.w.double().t()) < _tol(K)
    if tile == 3:
        plain = torch.empty(M, N, device=DEV)
        lib.call("dc_linear_forward", x, K, pl.w, K, M, N, K, plain, N, tile)
        assert not torch.equal(plain, y)
