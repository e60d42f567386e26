"""Entry points that pack many tensors into one table passed by value, or into one deferred queue, at and beyond their capacity:
dc_copy_many (16 entries per launch, csrc/optim.hip), dc_gemm_tn_reduce_many (16, csrc/gemm_tn.hip) and the deferred finaliser /
product queues of dc_finalisers_begin .. dc_finalisers_end (4 each, csrc/error.hip, nn.hip, gemm.hip).  Empty entries sit exactly
at the window edges; every result is compared with torch's copy / a float64 product / the unbatched call's bits."""
import copy
import ctypes

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _copy_entry(i, g):
    """(src, dst block, dst base, sentinel) for entry i: fp32 / int32 / int64 rows, contiguous or row-strided on both sides."""
    kind = i % 3
    rows, cols = 1 + (i * 37) % 300, 1 + (i * 5) % 9
    if kind == 0:
        src = torch.randn(rows, cols + 2, generator=g).to(DEV)[:, 1:1 + cols]
        base = torch.full((rows, cols + 5), -7.0, device=DEV)
    elif kind == 1:
        src = torch.randint(-1 << 30, 1 << 30, (rows, cols), generator=g, dtype=torch.int32).to(DEV)
        base = torch.full((rows, cols + 3), -7, dtype=torch.int32, device=DEV)
    else:
        src = torch.randint(-1 << 62, 1 << 62, (rows, cols), generator=g, dtype=torch.int64).to(DEV)
        base = torch.full((rows, cols + 4), -7, dtype=torch.int64, device=DEV)
    off = i % 2
    return src, base[:, off:off + cols], base, off


@pytest.mark.parametrize("count", [15, 16, 17, 33])
def test_copy_many_beyond_one_table(count):
    """dc_copy_many with 15 .. 33 entries (16 per launch), empty entries (0 rows / 0 columns) at 0, 15, 16 and the end, fp32 /
    int32 / int64 rows in 4-byte words, row-strided sources and destinations: each block == torch's copy, every destination column
    outside the block keeps its sentinel."""
    g = torch.Generator().manual_seed(count)
    empty = {0, 15, 16, count - 1}
    entries = [None if i in empty else _copy_entry(i, g) for i in range(count)]
    srcs, dsts, lds, ldd, rows, cols = [], [], [], [], [], []
    keep = []
    for i, e in enumerate(entries):
        if e is None:                   # an empty entry: valid addresses, no rows (or no columns)
            t = torch.zeros(4, 4, device=DEV)
            keep.append(t)
            srcs.append(t.data_ptr()); dsts.append(t.data_ptr()); lds.append(4); ldd.append(4)
            rows.append(0 if i % 2 == 0 else 3); cols.append(3 if i % 2 == 0 else 0)
            continue
        src, dst, _, _ = e
        w = src.element_size() // 4
        srcs.append(src.data_ptr()); dsts.append(dst.data_ptr())
        lds.append(src.stride(0) * w); ldd.append(dst.stride(0) * w)
        rows.append(src.shape[0]); cols.append(src.shape[1] * w)
    n = count
    i64, i32 = ctypes.c_int64 * n, ctypes.c_int32 * n
    lib.call("dc_copy_many", i64(*srcs), i64(*dsts), i64(*lds), i64(*ldd), i32(*rows), i32(*cols), n)
    torch.cuda.synchronize()
    for i, e in enumerate(entries):
        if e is None:
            continue
        src, dst, base, off = e
        assert torch.equal(dst, src), i
        outside = torch.cat([base[:, :off], base[:, off + src.shape[1]:]], 1)
        assert bool((outside == -7).all()), (i, "column outside the block written")
    assert all(float(t.abs().max()) == 0 for t in keep)
    # the same pairs through the wrapper (which drops empty pairs itself) into fresh destinations
    pairs = []
    for e in entries:
        if e is not None:
            src, _, base, off = e
            fresh = torch.zeros_like(base)
            pairs.append((src, fresh[:, off:off + src.shape[1]]))
    from deltaconv_amd import _ops
    _ops.copy_many(pairs)
    assert all(torch.equal(d, s) for s, d in pairs)


TN_SHAPES = [(16, 8, 8), (777, 50, 128), (1030, 13, 7), (4096, 64, 3), (300, 5, 3), (3000, 40, 70), (2048, 96, 64),
             (20000, 32, 32), (64, 3, 5)]


@pytest.mark.parametrize("count", [17, 40])
def test_slab_reductions_beyond_one_table(count):
    """dc_gemm_tn_reduce_many with 17 / 40 entries (16 per launch): streamed (<= 16 slabs, 16-byte geometry) and chained (> 16
    slabs, or outputs whose size is no multiple of 4) entries mixed, some written as column blocks of a wider output.  Each output
    == the unbatched dc_gemm_tn bits and within 1e-5 of float64 a^T b (the bound of
    test_gpu_gemm.py::test_batched_slab_reductions_write_the_same_bits); columns outside the blocks untouched."""
    from deltaconv_amd.nn import fused
    g = torch.Generator().manual_seed(count)
    ents = []
    for i in range(count):
        r, m, nn = TN_SHAPES[i % len(TN_SHAPES)]
        a, b = torch.randn(r, m, generator=g).to(DEV), torch.randn(r, nn, generator=g).to(DEV)
        nb = lib.raw("dc_gemm_tn_workspace_bytes")(r, m, nn)
        ws = torch.empty((nb + 3) // 4 + 4, dtype=torch.float32, device=DEV)
        slabs = ctypes.c_int32(0)
        lib.call("dc_gemm_tn_slabs", a, m, b, nn, r, m, nn, ws, ws.numel() * 4, ctypes.byref(slabs))
        pad = 4 if i % 4 == 1 else 0             # column block of a wider output (ldc = nn + 4)
        wide = torch.full((m, nn + pad), 5.0, device=DEV)
        ents.append((a, b, ws, slabs.value, wide, pad))
    assert any(e[3] <= 16 for e in ents) and any(e[3] > 16 for e in ents), [e[3] for e in ents]
    n = count
    i64, i32 = ctypes.c_int64 * n, ctypes.c_int32 * n
    outs = [e[4][:, e[5]:] for e in ents]
    lib.call("dc_gemm_tn_reduce_many", i64(*[e[2].data_ptr() for e in ents]), i64(*[o.data_ptr() for o in outs]),
             i64(*[e[4].stride(0) for e in ents]), i32(*[o.shape[0] for o in outs]), i32(*[o.shape[1] for o in outs]),
             i32(*[e[3] for e in ents]), None, n)
    torch.cuda.synchronize()
    for i, ((a, b, _, slabs, wide, pad), out) in enumerate(zip(ents, outs)):
        assert torch.equal(out, fused.gemm_tn(a, b)), (i, slabs)
        assert rel_err(out, a.double().t() @ b.double()) < 1e-5, (i, slabs)
        assert bool((wide[:, :pad] == 5.0).all()), i
    # the same through fused.tn_batch(): the queue of one node, flushed as tables of 16
    with fused.tn_batch():
        got = [fused.gemm_tn(e[0], e[1]) for e in ents]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, outs))


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bn_block(seed, R=4096, C=64, K=128):
    """Operands of one BatchNorm-backward reduction (bn_block_reduce): dy strided, h, coef = mean / invstd / scale / shift."""
    h = _rand(R, C, seed=seed)
    mean, var = h.mean(0), h.var(0, unbiased=False)
    gamma = _rand(C, seed=seed + 1) + 1.5
    invstd = 1 / (var + 1e-5).sqrt()
    coef = torch.stack([mean, invstd, gamma * invstd, _rand(C, seed=seed + 2) - mean * gamma * invstd])
    dy = _rand(R, C + 8, seed=seed + 3)[:, 4:4 + C]
    return dy, dy.stride(0), _rand(R, K, seed=seed + 4), h, coef, True, gamma, 0.2, _rand(C, K, seed=seed + 5)


def test_pairable_product_behind_a_full_finaliser_queue():
    """Inside one fin_batch(): four deferred BatchNorm-backward reductions fill the finaliser queue, then a forward product with
    statistics of the pairable kind (weight-plane path, whole tiles) asks to be deferred too.  Its finaliser finds no room and runs
    at once -- so the product must run at once as well, not wait in the product queue behind it.  All five coefficient sets
    against the unbatched calls' bits, and the product's statistics against float64."""
    from deltaconv_amd.nn import fused
    assert fused.USE_FIN_BATCH[0] and fused.USE_GEMM_PAIR[0]
    fused._planes_reset()
    M, N, K = 4096, 128, 128
    x = _rand(M, K, seed=70)
    w = torch.nn.Parameter(_rand(N, K, seed=71) / K ** 0.5)
    bn = torch.nn.BatchNorm1d(N).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(_rand(N, seed=72) + 1.5)
        bn.bias.copy_(_rand(N, seed=73))
    bn_ref = copy.deepcopy(bn)
    blocks = [_bn_block(100 + 10 * j) for j in range(4)]
    fused.mm_nt(x, w)                                       # planes of w cut (outside the batch)
    poison = [torch.full((1 << 14,), float("nan"), device=DEV) for _ in range(64)]
    del poison                                              # stale workspace memory reads as NaN
    with fused.fin_batch():
        states = [fused.bn_block_reduce(*blk, defer_final=True) for blk in blocks]
        h, coef, _ = fused.linear_stats(x, w, bn, bn.weight, bn.bias, defer_final=True)
    torch.cuda.synchronize()
    ref_states = [fused.bn_block_reduce(*blk) for blk in blocks]
    h_ref, coef_ref, _ = fused.linear_stats(x, w, bn_ref, bn_ref.weight, bn_ref.bias)
    torch.cuda.synchronize()
    for j, (s, r) in enumerate(zip(states, ref_states)):
        for k in (4, 7, 8):                                 # coefs, dgamma, dbeta
            assert torch.equal(s[k], r[k]), (j, k)
    assert torch.equal(h, h_ref)
    hd = h.double()
    mean, var = hd.mean(0), hd.var(0, unbiased=False)
    invstd = 1 / (var + bn.eps).sqrt()
    want = torch.stack([mean, invstd, bn.weight.double() * invstd, bn.bias.double() - mean * bn.weight.double() * invstd])
    for k, name in enumerate(("mean", "invstd", "scale", "shift")):
        assert rel_err(coef[k], want[k]) < 1e-5, (name, rel_err(coef[k], want[k]))
    assert torch.equal(coef, coef_ref)
    assert torch.equal(bn.running_mean, bn_ref.running_mean) and torch.equal(bn.running_var, bn_ref.running_var)
