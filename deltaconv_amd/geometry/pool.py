"""Scalar features from a cloud DOWN to a sampled one on the device (csrc/pool.hip: ``dc_knn_pool``, ``dc_knn_pool_backward``):
the set-abstraction step of PointNet++ -- every sampled point takes the maximum, minimum, sum or mean over its k nearest points
of the full cloud -- what a ``torch_cluster.knn`` search followed by ``torch_scatter.scatter(x[col], row, reduce=...)`` does,
without the ``[Nq, k, C]`` intermediate.  ``knn_interpolate`` is the scalar stream's way up between two resolutions, this is its
way down; ``CloudPair`` (resample.py) holds both for a pair of clouds.  The reference has no such call site.

The search is ``knn_cross`` with the sampled cloud as the query.  The gradient w.r.t. the FEATURES is opt-in
(``knn_pool(..., differentiable=True)``): an ordered, atomics-free sum over the transposed lists of the search
(``knn_cross_transpose``), bit-reproducible.  There is NO gradient for positions.  There is no CPU path."""
import torch

from . import _cross
from ._cross import MAX_K
from .interpolate import knn_cross, knn_cross_transpose

__all__ = ["pool_rows", "pool_rows_backward", "knn_pool"]

_MODES = {"max": 0, "min": 1, "sum": 2, "add": 2, "mean": 3}    # the codes of dc_seg_reduce
NO_ARG = 255


def _mode(fn, reduce):
    if reduce not in _MODES:
        raise ValueError(f"{fn}: reduce must be one of 'max', 'min', 'sum', 'add', 'mean', got {reduce!r}")
    return _MODES[reduce]


def pool_rows(x, qptr, rptr, idx, max_query_cloud, reduce="max", n_query=None, out=None):
    """The arithmetic half of ``knn_pool`` on a search result (``dc_knn_pool``): x ``[Nr,C]`` DEVICE fp32 (rows may be strided) ->
    ``(out fp32 [n_query,C], arg uint8 [n_query,C] or None, cnt uint8 [n_query])``; row ``qptr[b] + i`` of out is the `reduce` over
    rows ``rptr[b] + idx[qptr[b] + i, s]`` of x for the valid slots s (csrc/pool_math.h: the first valid slot is copied, a later
    one taken iff strictly larger / smaller, or added in order; mean divides once by the count; no valid slot: zeros).  ``arg``
    (max / min only): the slot every channel came from, 255 without one; ``cnt``: the valid slots of every query.  Rows outside
    every pair keep what ``out`` held (zeros / 255 / 0 when allocated here).  Not recorded by autograd; ``pool_rows_backward`` is
    its gradient w.r.t. x.  One launch per 65 535 pairs, no synchronise."""
    from .._lib import lib
    fn = "pool_rows"
    mode = _mode(fn, reduce)
    x, c, ldx = _cross.values(fn, "x", x)
    nq, k = _cross.search(fn, idx)
    qptr, rptr = _cross.offsets(fn, x.device, qptr=qptr, rptr=rptr)
    n_query = nq if n_query is None else int(n_query)
    out, ldo = _cross.out_rows(fn, out, n_query, c, x.device, on_device=True)
    lda = (c + 3) // 4 * 4                     # rows of arg a multiple of 4 bytes apart: one 32-bit store per channel group
    arg = torch.full((n_query, lda), NO_ARG, dtype=torch.uint8, device=x.device)[:, :c] if mode <= 1 else None
    cnt = torch.zeros(n_query, dtype=torch.uint8, device=x.device)
    b = int(qptr.numel()) - 1
    if n_query == 0 or nq == 0:
        return out, arg, cnt
    if x.shape[0] == 0:                        # no reference row at all: every slot is invalid, a row that is never read stands in
        x, ldx = x.new_zeros((1, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_pool", x, ldx, c, qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, int(max_query_cloud), k, idx, mode, out, ldo,
                 arg, lda if arg is not None else 0, cnt)
    return out, arg, cnt


def pool_rows_backward(g, rptr, tptr, tedge, arg, cnt, k, max_ref_cloud, reduce="max", n_ref=None, out=None):
    """The gradient of ``pool_rows`` w.r.t. x on the lists of ``knn_cross_transpose`` (``dc_knn_pool_backward``): g ``[n_query,C]``
    DEVICE fp32 (rows may be strided), ``arg`` / ``cnt`` what the forward returned (``arg`` may be None for sum / mean) -> fp32
    ``[n_ref,C]``: for reference row r and its in-edges ``e = q * k + s`` in ascending order, max / min add ``g[q]`` where
    ``arg[q] == s``, sum adds ``g[q]``, mean adds ``g[q] / cnt[q]``, every quotient and sum rounded on its own: no atomics, the
    same bits on every run.  Every reference row of every pair is written (zeros without in-edges); rows of ``out`` outside every
    pair keep what they held (zeros when allocated here).  One launch per 65 535 pairs, no synchronise."""
    from .._lib import lib
    fn = "pool_rows_backward"
    mode = _mode(fn, reduce)
    g, c, ldg = _cross.values(fn, "g", g)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{fn}: k = {k} outside [1, {MAX_K}]")
    rows = int(g.shape[0])
    rptr = _cross.offsets(fn, g.device, rptr=rptr)
    for name, t in (("tptr", tptr), ("tedge", tedge)):
        _cross.device(fn, name, t)
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous int64 (knn_cross_transpose)")
    _cross.device(fn, "cnt", cnt)
    if cnt.dtype != torch.uint8 or tuple(cnt.shape) != (rows,) or not cnt.is_contiguous():
        raise ValueError(f"{fn}: cnt must be contiguous uint8 [{rows}] (pool_rows)")
    if arg is None and mode <= 1:
        raise ValueError(f"{fn}: reduce = {reduce!r} needs the arg of the forward")
    lda = 0
    if arg is not None:
        _cross.device(fn, "arg", arg)
        if arg.dtype != torch.uint8 or tuple(arg.shape) != (rows, c) or (c > 1 and arg.stride(1) != 1) or \
                (rows > 1 and arg.stride(0) < c):
            raise ValueError(f"{fn}: arg must be uint8 [{rows}, {c}] with unit stride along the channels (pool_rows)")
        lda = int(arg.stride(0)) if rows > 1 else c
    n_ref = int(tptr.numel()) - 1 if n_ref is None else int(n_ref)
    out, ldo = _cross.out_rows(fn, out, n_ref, c, g.device, on_device=True)
    b = int(rptr.numel()) - 1
    if n_ref == 0:
        return out
    if rows == 0:                              # no query row at all: every edge is skipped, rows that are never read stand in
        g, ldg, cnt = g.new_zeros((1, c)), c, cnt.new_zeros(1)
        arg, lda = (None, 0) if arg is None else (arg.new_zeros((1, c)), c)
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_pool_backward", g, ldg, rows, c, rptr[lo:hi + 1], hi - lo, int(max_ref_cloud), k, tptr, tedge,
                 int(tedge.numel()), mode, arg, lda, cnt, out, ldo)
    return out


def knn_pool(x, pos_x, pos_y, batch_x=None, batch_y=None, k=16, reduce="max", ptr_x=None, ptr_y=None, differentiable=False,
             max_query_cloud=None, max_ref_cloud=None):
    """The features ``x [len(pos_x), C]`` at ``pos_x`` pooled DOWN to ``pos_y``: for every target its k nearest sources (of the
    same cloud, ``torch_cluster.knn``), reduced by ``reduce`` = ``"max" | "min" | "sum" | "add" | "mean"``
    (``torch_scatter.scatter``) -- PointNet++ set abstraction.  -> fp32 ``[len(pos_y), C]``.  A target whose cloud has fewer than
    k sources reduces what there is; one without any gets zeros.  ``pos_y`` is the caller's (for instance
    ``pos_x[geodesic_fps_batch(...)]``) and need not be a subset of ``pos_x``.  ``ptr_x`` / ``ptr_y`` (int64 [B+1] row offsets)
    stand in for the sorted ``batch`` vectors where the offsets are at hand.

    ``differentiable=False`` (the default) is INFERENCE ONLY: ``x.requires_grad`` while grad mode is on raises ``RuntimeError``
    instead of cutting the graph silently -- call it under ``torch.no_grad()``, pass ``x.detach()``, or ask for the gradient:

    ``differentiable=True``: an ``x`` that requires grad gives a result on the autograd graph (the same forward bits).  The
    forward also builds the transposed lists of the search (``knn_cross_transpose``), so that the backward is one launch of an
    ordered sum: no floating-point atomics, the same gradient bits on every run; a maximum / minimum sends its gradient to the
    nearest of the sources that share it.  Once differentiable; NO gradient for ``pos_x`` / ``pos_y``: one that requires grad
    raises.  ``max_query_cloud`` / ``max_ref_cloud``: the largest target / source cloud where the host knows them; with both and
    ``ptr_x`` / ``ptr_y`` given nothing synchronises and forward + backward can be captured in a ``torch.cuda.graph``.

    Non-HIP tensors raise: there is no CPU path."""
    fn = "knn_pool"
    _mode(fn, reduce)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{fn}: k = {k} outside [1, {MAX_K}]")
    needs_grad = torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled()
    if needs_grad and not differentiable:
        raise RuntimeError(f"{fn}: x requires grad, but the device pooling is inference-only by default; call it under "
                           "torch.no_grad(), pass x.detach() or differentiable=True")
    _cross.device(fn, "x", x)
    _cross.no_grad_inputs(fn, pos_x=pos_x, pos_y=pos_y)
    pos_x, pos_y = _cross.rows3(fn, "pos_x", pos_x), _cross.rows3(fn, "pos_y", pos_y)
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[0] != pos_x.shape[0]:
        raise ValueError(f"{fn}: x must hold one row per point of pos_x, got {tuple(x.shape)} for {pos_x.shape[0]} points")
    with torch.no_grad():
        qptr, rptr, b, mq = _cross.pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, fn, max_query_cloud)
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
        if not needs_grad:
            return pool_rows(x.detach(), qptr, rptr, idx, mq, reduce, n_query=pos_y.shape[0])[0]
        mr = _cross.largest_cloud(rptr, max_ref_cloud)
        tptr, tedge, _ = knn_cross_transpose(idx, d2, qptr, rptr, num_ref=pos_x.shape[0])
    # offsets given by the caller may leave rows of x outside every cloud: their gradient is zero, filled by the backward
    return _cross.Pool.apply(x, pool_rows, pool_rows_backward, reduce, qptr, rptr, idx, tptr, tedge, mq, mr, pos_y.shape[0],
                             ptr_x is None)
