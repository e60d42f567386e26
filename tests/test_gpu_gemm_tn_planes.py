"""Weight gradients dW = A^T B on bf16 plane images in LDS (csrc/gemm_tn_planes.hip) through the C ABI: every weight-gradient
shape of the C2 step and of the per-rank steps against a float64 product, under the three settings that select the kernel
(switch 12 = 0: the plan's choice, 12 = 1: the gemm_kernel path, switch 3 = 1: the exact fp32 chain).
Bound: the project's rule for split products -- error vs fp64 <= 1.5 x the exact chain's + 1e-7 -- and bit-identity between
repeats and between launch forms of one build.  The plane kernel keeps gemm_kernel's reduction order (same k per MFMA, same order
of the six partial products), so on 128 x 128 tiles -- where gemm_kernel runs the split products too -- the two return the SAME
bits: which kernel ran is read from the profiler's kernel names, not from the bits.  The prologue variant against dc_bn_act_backward + plain dc_gemm_tn at 2e-5
(the bound of test_gpu_gemm.py::test_bn_block_backward_fused_matches_unfused)."""
import ctypes
import math

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (R, M, N): dW[M, N] = A[R, M]^T B[R, N]
SHAPES = [(32768, 1024, 448), (32768, 1024, 512), (32768, 256, 512), (65536, 256, 256), (32768, 128, 128), (32768, 64, 256),
          (32768, 64, 64), (8192, 128, 64)]
# shapes whose plan (dc_tn_lds_plan + tn_planes_faster, csrc/gemm.hip) is the plane-image kernel on 128 x 128 tiles ...
ON_PLANES = [(32768, 1024, 512), (32768, 256, 512), (65536, 256, 256)]
# ... on 128 x 64 tiles (gemm_kernel: exact chain), and shapes whose plan stays on gemm_kernel (64 x 64 tiles)
ON_PLANES_NARROW = [(32768, 1024, 448)]
ON_GEMM_KERNEL = [(32768, 128, 128), (32768, 64, 256), (32768, 64, 64), (8192, 128, 64)]


def _gemm_kernels(fn):
    """Names of the dense-product kernels that fn() launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "gemm_kernel<" in e.name or "gemm_tn_planes_kernel<" in e.name]


def _on_planes(names):
    assert names, "no dense-product kernel in the trace"
    return all("gemm_tn_planes_kernel<" in n for n in names)


class options:
    """dc_set_option(key, value) for the duration of a block."""

    def __init__(self, **kv):
        self.kv = {int(k[1:]): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            lib.raw("dc_set_option")(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            lib.raw("dc_set_option")(k, 0)


def _operands(r, m, n, binades, seed):
    """The generator of test_split_products_no_worse_than_exact_chain: normal operands, optionally spread over many binades
    with exact zeros (post-ReLU-like)."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(r, m, generator=g), torch.randn(r, n, generator=g)
    if binades:
        b = b * torch.exp(binades * torch.randn(r, n, generator=g))
        b[b.abs() < 0.5] = 0
        a = a * torch.exp(0.5 * binades * torch.randn(r, m, generator=g))
    return a.to(DEV), b.to(DEV)


def _tn(a, b, m=None, n=None):
    r = a.shape[0]
    m, n = m or a.shape[1], n or b.shape[1]
    nb = lib.raw("dc_gemm_tn_workspace_bytes")(r, m, n)
    ws = torch.empty((nb + 3) // 4, device=DEV)
    c = torch.full((m, n), float("nan"), device=DEV)
    lib.call("dc_gemm_tn", a, a.stride(0), b, b.stride(0), r, m, n, c, n, 0, ws, ws.numel() * 4)
    return c


def _three_ways(a, b):
    """-> (plan's kernel, the same again, gemm_kernel path, exact chain)"""
    new, again = _tn(a, b), _tn(a, b)
    with options(o12=1):
        old = _tn(a, b)
    with options(o3=1):
        exact = _tn(a, b)
    return new, again, old, exact


@pytest.mark.parametrize("R,M,N", SHAPES)
@pytest.mark.parametrize("binades", [0.0, 3.0])
def test_weight_gradient_shapes(R, M, N, binades):
    a, b = _operands(R, M, N, binades, seed=M + N + int(binades))
    ref = a.double().t() @ b.double()
    new, again, old, exact = _three_ways(a, b)
    e_new, e_old, e_exact = rel_err(new, ref), rel_err(old, ref), rel_err(exact, ref)
    print(f"dW {R} x {M} x {N} binades {binades}: planes {e_new:.3e}  gemm_kernel {e_old:.3e}  exact chain {e_exact:.3e}")
    assert e_new <= 1.5 * e_exact + 1e-7, (e_new, e_exact)
    assert e_old <= 1.5 * e_exact + 1e-7, (e_old, e_exact)
    assert torch.equal(new, again)
    if (R, M, N) in ON_PLANES:
        assert torch.equal(new, old)                     # same reduction order as gemm_kernel's split products
        assert not torch.equal(new, exact)
    if (R, M, N) in ON_PLANES_NARROW:
        assert not torch.equal(new, old)                 # gemm_kernel runs these tiles on the exact chain
        assert torch.equal(old, exact)


@pytest.mark.parametrize("R,M,N", SHAPES)
def test_the_switch_selects_the_kernel(R, M, N):
    a, b = _operands(R, M, N, 0.0, seed=1)
    planned = (R, M, N) in ON_PLANES + ON_PLANES_NARROW
    assert planned != ((R, M, N) in ON_GEMM_KERNEL)
    assert _on_planes(_gemm_kernels(lambda: _tn(a, b))) == planned
    with options(o12=1):
        assert not _on_planes(_gemm_kernels(lambda: _tn(a, b)))
    with options(o12=2):
        assert _on_planes(_gemm_kernels(lambda: _tn(a, b)))            # lab: every whole tile
    with options(o3=1):
        assert not _on_planes(_gemm_kernels(lambda: _tn(a, b)))        # the exact chain never goes through the plane kernel
    with options(o3=1, o12=2):
        assert not _on_planes(_gemm_kernels(lambda: _tn(a, b)))


@pytest.mark.parametrize("R", [8192 - 32, 8192, 8192 + 32, 32768 + 96, 65536 - 2048 + 32])
def test_row_counts_around_the_plan_bounds(R):
    """Rows just below / at / above the small-plan bound (8192) and row counts that are no multiple of the slab length (the last
    slab is shorter)."""
    M, N = 256, 256
    a, b = _operands(R, M, N, 3.0, seed=R)
    ref = a.double().t() @ b.double()
    new, again, old, exact = _three_ways(a, b)
    e_new, e_exact = rel_err(new, ref), rel_err(exact, ref)
    print(f"dW {R} x {M} x {N}: planes {e_new:.3e}  exact chain {e_exact:.3e}")
    assert e_new <= 1.5 * e_exact + 1e-7, (e_new, e_exact)
    assert torch.equal(new, again)
    assert _on_planes(_gemm_kernels(lambda: _tn(a, b))) == (R > 8192)        # at most 8192 rows: the small plan, 64 x 64 tiles
    assert torch.equal(new, old)


def test_strided_operands():
    """Column slices of wider buffers, as gemm_tn passes b[:, j0:j0 + nj]."""
    R, M, N = 32768, 256, 256
    abuf, bbuf = _operands(R, M + 64, 3 * N, 3.0, seed=5)
    a, b = abuf[:, 32:32 + M], bbuf[:, N:2 * N]
    ref = a.double().t() @ b.double()
    new, again, old, exact = _three_ways(a, b)
    assert rel_err(new, ref) <= 1.5 * rel_err(exact, ref) + 1e-7
    assert torch.equal(new, again) and torch.equal(new, old)
    assert _on_planes(_gemm_kernels(lambda: _tn(a, b)))
    assert torch.equal(new, _tn(a.contiguous(), b.contiguous()))         # the leading dimension changes nothing


@pytest.mark.parametrize("R,M,N", [(3000, 40, 70), (1030, 64, 12), (32768 + 8, 256, 256)])
def test_ragged_shapes_stay_on_the_guarded_kernels(R, M, N):
    a, b = _operands(R, M, N, 0.0, seed=R + M)
    new = _tn(a, b)
    with options(o12=1):
        old = _tn(a, b)
    assert torch.equal(new, old)
    with options(o12=2):
        assert not _on_planes(_gemm_kernels(lambda: _tn(a, b)))
    assert rel_err(new, a.double().t() @ b.double()) < 2e-6 * math.sqrt(R) + 1e-6


@pytest.mark.parametrize("R,M,N", SHAPES[2:])
def test_deferred_slab_reduction_gives_the_same_bits(R, M, N):
    """dc_gemm_tn_slabs + dc_gemm_tn_reduce_many == dc_gemm_tn on the plan's kernel."""
    a, b = _operands(R, M, N, 3.0, seed=R + N)
    nb = lib.raw("dc_gemm_tn_workspace_bytes")(R, M, N)
    ws = torch.empty((nb + 3) // 4, device=DEV)
    slabs = ctypes.c_int32(0)
    lib.call("dc_gemm_tn_slabs", a, M, b, N, R, M, N, ws, ws.numel() * 4, ctypes.byref(slabs))
    out = torch.full((M, N), float("nan"), device=DEV)
    i64, i32 = ctypes.c_int64 * 1, ctypes.c_int32 * 1
    lib.call("dc_gemm_tn_reduce_many", i64(ws.data_ptr()), i64(out.data_ptr()), i64(N), i32(M), i32(N), i32(slabs.value), None, 1)
    assert torch.equal(out, _tn(a, b))


def _bn_coefficients(h, gamma, beta):
    r, c = h.shape
    coef = torch.empty(4, c, device=DEV)
    nb = lib.raw("dc_bn_workspace_bytes")(r, c)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    lib.call("dc_bn_stats", h, r, c, c, gamma, beta, 1e-5, 0.1, None, None, coef[0], coef[1], coef[2], coef[3], ws, nb)
    return coef


@pytest.mark.parametrize("R,C,K", [(32768, 256, 512), (32768, 128, 128), (32768, 64, 256), (8192, 128, 64), (16384, 512, 256)])
@pytest.mark.parametrize("training", [True, False])
def test_prologue_variant_matches_unfused(R, C, K, training):
    """dW of a Linear + BatchNorm + LeakyReLU block with dh = bn_act_backward(dy, h) formed in the operand loader
    (dc_linear_bn_backward_weight) against dc_bn_act_backward + plain dc_gemm_tn: training and eval coefficients, negative
    gamma, strided dy; also the deferred form, and both against the gemm_kernel path."""
    from deltaconv_amd.nn import fused
    g = torch.Generator().manual_seed(R + C + K)
    x = (torch.rand(R, K, generator=g) * 2 - 1).to(DEV)
    w = (torch.rand(C, K, generator=g) * 2 - 1).to(DEV)
    h = x @ w.t()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) * 2 - 1).to(DEV)
    gamma[::3] *= -1
    coef = _bn_coefficients(h, gamma, beta)
    dy = (torch.rand(R, C + 8, generator=g) * 2 - 1).to(DEV)[:, 4:4 + C]

    def d_w(fuse):
        fused.FUSE_BN_BWD = fuse
        try:
            return fused.bn_block_backward(dy, dy.stride(0), x, h, coef, training, gamma, 0.2, w, False)[0]
        finally:
            fused.FUSE_BN_BWD = True
    new, again, unfused = d_w(True), d_w(True), d_w(False)
    with options(o12=1):
        old = d_w(True)
    with fused.tn_batch():
        deferred = d_w(True)
    torch.cuda.synchronize()
    print(f"prologue dW {R} x {C} x {K}: planes vs unfused {rel_err(new, unfused):.3e}  gemm_kernel vs unfused {rel_err(old, unfused):.3e}")
    assert rel_err(new, unfused) < 2e-5
    assert torch.equal(new, again) and torch.equal(new, deferred)
    planned = C % 128 == 0 and K % 64 == 0 and C * K >= 32768 and R > 8192       # 128-row tiles of the large plan
    assert _on_planes(_gemm_kernels(lambda: d_w(True))) == planned
    with options(o12=1):
        assert not _on_planes(_gemm_kernels(lambda: d_w(True)))
    if planned and K % 128 == 0:
        assert torch.equal(new, old)
