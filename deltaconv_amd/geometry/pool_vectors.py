"""Tangent-vector features from a cloud DOWN to a sampled one on the device (csrc/pool_vectors.hip: ``dc_knn_cross_rotation``,
``dc_knn_pool_vectors``, ``dc_knn_pool_vectors_backward``): the vector stream's set-abstraction step, the sibling of ``knn_pool``.
Every sampled point carries the vectors of its k nearest points of the full cloud into its own frame by parallel transport
(reference: deltaconv/geometry/connection.py:6-47) and keeps the one of largest norm per channel (``"max"``), their sum or
their mean.  The reference has no such call site.

Why not ``knn_interpolate_vectors`` with the roles swapped: its weights are ``1 / max(d^2, 1e-16)``, and a coarse cloud that is a
SUBSET of the fine one (every cloud ``geodesic_fps_batch`` / ``geodesic_subsample`` / ``T.GeodesicFPS`` produce) has a fine point
at ``d^2 = 0`` under every coarse point: that slot's coefficient is exactly 1.0 in fp32, the others' about 1e-13, and the
"pooling" is a gather of the coarse point's own vector.  It is a correct interpolation and stays; this is the pooling.

The per-slot rotations are stored once per search (``knn_cross_rotation``: 16 k bytes per target row) and the apply kernels are
pure gathers over them.  The gradient w.r.t. the VALUES is opt-in (``differentiable=True``): an ordered, atomics-free sum over
the transposed lists of the search (``knn_cross_transpose``), bit-reproducible.  None of the geometry is differentiable.  There
is no CPU path."""
import torch

from . import _cross
from ._cross import MAX_K
from .interpolate import knn_cross, knn_cross_transpose
from .pool import NO_ARG
from .vector_interpolate import _table

__all__ = ["knn_cross_rotation", "pool_vectors", "pool_vectors_backward", "knn_pool_vectors"]

_MODES = {"max": 0, "sum": 2, "add": 2, "mean": 3}    # the codes of dc_seg_reduce; min has no vector analogue


def _mode(fn, reduce):
    if reduce not in _MODES:
        raise ValueError(f"{fn}: reduce must be one of 'max', 'sum', 'add', 'mean', got {reduce!r}")
    return _MODES[reduce]


def knn_cross_rotation(idx, qptr, rptr, query_frames, ref_frames, non_oriented=True, max_query_cloud=None):
    """The table of per-slot rotations of a ``knn_cross`` result (``dc_knn_cross_rotation``) -> fp32 ``[Nq*k, 4]``, row-major
    2 x 2: entry ``q*k + s`` is ``R = build_transport(query frame of q, reference frame of rptr[b] + idx[q, s])`` -- the matrix
    alone, without the interpolation coefficient ``knn_cross_transport`` multiplies in.  Invalid slots and rows outside every pair
    hold zeros.  The arguments are those of ``knn_cross_transport`` without ``d2``.  Nothing here is differentiable: an input that
    requires grad while grad mode is on raises ``RuntimeError``."""
    from .._lib import lib
    fn = "knn_cross_rotation"
    nq, k = _cross.search(fn, idx)
    if len(query_frames) != 3 or len(ref_frames) not in (2, 3):
        raise ValueError(f"{fn}: query_frames = (normal, x_basis, y_basis), ref_frames = (normal, x_basis[, y_basis])")
    _cross.no_grad_inputs(fn, query_normal=query_frames[0], query_x_basis=query_frames[1], query_y_basis=query_frames[2],
                          ref_normal=ref_frames[0], ref_x_basis=ref_frames[1])
    tn = _cross.rows3(fn, "query normal", query_frames[0], nq)
    tx, ty = _cross.rows3(fn, "query x_basis", query_frames[1], nq), _cross.rows3(fn, "query y_basis", query_frames[2], nq)
    sn = _cross.rows3(fn, "ref normal", ref_frames[0])
    sx = _cross.rows3(fn, "ref x_basis", ref_frames[1], sn.shape[0])
    dev = idx.device
    qptr, rptr = _cross.offsets(fn, dev, qptr=qptr, rptr=rptr)
    b = int(qptr.numel()) - 1
    mq = _cross.largest_cloud(qptr, max_query_cloud)
    with torch.no_grad():
        rmat = torch.zeros((nq * k, 4), dtype=torch.float32, device=dev)
        if nq == 0 or mq == 0:
            return rmat
        if sn.shape[0] == 0:                   # every reference cloud is empty: rows that are never read stand in for the null pointers
            sn, sx = sn.new_zeros((1, 3)), sx.new_zeros((1, 3))
        for lo, hi in _cross.launches(b):
            lib.call("dc_knn_cross_rotation", qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, nq, mq, k, idx, tn, tx, ty, sn, sx,
                     int(bool(non_oriented)), rmat)
    return rmat


def pool_vectors(v, qptr, rptr, idx, rmat, max_query_cloud, reduce="max", n_query=None, out=None):
    """The arithmetic half of ``knn_pool_vectors`` on a search result and its rotation table (``dc_knn_pool_vectors``):
    v ``[2*Nr, C]`` DEVICE fp32 (rows may be strided) -> ``(out fp32 [2*n_query, C], arg uint8 [n_query, C] or None, cnt uint8
    [n_query])``; rows ``2q, 2q+1`` of query ``q = qptr[b] + i`` are the `reduce` over the valid slots s of the vectors of rows
    ``rptr[b] + idx[q, s]`` carried into q's frame by ``rmat[q*k + s]`` (csrc/pool_vectors_math.h): ``"sum"`` is
    ``interpolate_vectors`` on ``rmat`` bit for bit, ``"mean"`` divides it once by the count, ``"max"`` keeps per channel the
    transported vector of the slot whose squared norm is largest (the first valid slot, a later one iff strictly larger).  No
    valid slot: zeros.  ``arg`` (max only): the slot every channel came from, 255 without one; ``cnt``: the valid slots of every
    query.  Rows outside every pair keep what ``out`` held (zeros / 255 / 0 when allocated here).  Not recorded by autograd;
    ``pool_vectors_backward`` is its gradient w.r.t. v.  One launch per 65 535 pairs, no synchronise."""
    from .._lib import lib
    fn = "pool_vectors"
    mode = _mode(fn, reduce)
    v, c, ldv = _cross.values(fn, "v", v, per_point=2)
    nq, k = _cross.search(fn, idx)
    rmat = _table(fn, rmat, nq * k)
    qptr, rptr = _cross.offsets(fn, v.device, qptr=qptr, rptr=rptr)
    n_query = nq if n_query is None else int(n_query)
    out, ldo = _cross.out_rows(fn, out, 2 * n_query, c, v.device, on_device=True)
    lda = (c + 3) // 4 * 4                     # rows of arg a multiple of 4 bytes apart: one 32-bit store per channel group
    arg = torch.full((n_query, lda), NO_ARG, dtype=torch.uint8, device=v.device)[:, :c] if mode == 0 else None
    cnt = torch.zeros(n_query, dtype=torch.uint8, device=v.device)
    b = int(qptr.numel()) - 1
    if n_query == 0 or nq == 0:
        return out, arg, cnt
    if v.shape[0] == 0:                        # no reference row at all: every slot is invalid, rows that are never read stand in
        v, ldv = v.new_zeros((2, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_pool_vectors", v, ldv, c, qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, int(max_query_cloud), k, idx, rmat,
                 mode, out, ldo, arg, lda if arg is not None else 0, cnt)
    return out, arg, cnt


def pool_vectors_backward(g, rptr, tptr, tedge, rmat, arg, cnt, k, max_ref_cloud, reduce="max", n_ref=None, out=None):
    """The gradient of ``pool_vectors`` w.r.t. v on the lists of ``knn_cross_transpose`` (``dc_knn_pool_vectors_backward``):
    g ``[2*n_query, C]`` DEVICE fp32 (rows may be strided), ``rmat`` the forward's table, ``arg`` / ``cnt`` what the forward
    returned (``arg`` may be None for sum / mean) -> fp32 ``[2*n_ref, C]``: for reference row r and its in-edges ``e = q*k + s``
    in ascending order, ``R = rmat[e]``: ``du = (du + R00*g[2q]) + R10*g[2q+1]``, ``dw = (dw + R01*g[2q]) + R11*g[2q+1]`` -- for
    every edge (sum), with ``g`` first divided by ``cnt[q]`` (mean) or where ``arg[q] == s`` (max) --, every product, quotient and
    sum rounded on its own: no atomics, the same bits on every run.  Every reference row of every pair is written (zeros without
    in-edges); rows of ``out`` outside every pair keep what they held (zeros when allocated here).  One launch per 65 535 pairs,
    no synchronise."""
    from .._lib import lib
    fn = "pool_vectors_backward"
    mode = _mode(fn, reduce)
    g, c, ldg = _cross.values(fn, "g", g, per_point=2)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{fn}: k = {k} outside [1, {MAX_K}]")
    rows = int(g.shape[0]) // 2
    rmat = _table(fn, rmat, rows * k)
    rptr = _cross.offsets(fn, g.device, rptr=rptr)
    for name, t in (("tptr", tptr), ("tedge", tedge)):
        _cross.device(fn, name, t)
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous int64 (knn_cross_transpose)")
    _cross.device(fn, "cnt", cnt)
    if cnt.dtype != torch.uint8 or tuple(cnt.shape) != (rows,) or not cnt.is_contiguous():
        raise ValueError(f"{fn}: cnt must be contiguous uint8 [{rows}] (pool_vectors)")
    if arg is None and mode == 0:
        raise ValueError(f"{fn}: reduce = {reduce!r} needs the arg of the forward")
    lda = 0
    if arg is not None:
        _cross.device(fn, "arg", arg)
        if arg.dtype != torch.uint8 or tuple(arg.shape) != (rows, c) or (c > 1 and arg.stride(1) != 1) or \
                (rows > 1 and arg.stride(0) < c):
            raise ValueError(f"{fn}: arg must be uint8 [{rows}, {c}] with unit stride along the channels (pool_vectors)")
        lda = int(arg.stride(0)) if rows > 1 else c
    n_ref = int(tptr.numel()) - 1 if n_ref is None else int(n_ref)
    out, ldo = _cross.out_rows(fn, out, 2 * n_ref, c, g.device, on_device=True)
    b = int(rptr.numel()) - 1
    if n_ref == 0:
        return out
    if rows == 0:                              # no query row at all: every edge is skipped, rows that are never read stand in
        g, ldg, cnt, rmat = g.new_zeros((2, c)), c, cnt.new_zeros(1), rmat.new_zeros((1, 4))
        arg, lda = (None, 0) if arg is None else (arg.new_zeros((1, c)), c)
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_pool_vectors_backward", g, ldg, rows, c, rptr[lo:hi + 1], hi - lo, int(max_ref_cloud), k, tptr, tedge,
                 int(tedge.numel()), rmat, mode, arg, lda, cnt, out, ldo)
    return out


def knn_pool_vectors(v, pos_x, pos_y, frames_x, frames_y, batch_x=None, batch_y=None, k=16, reduce="max", ptr_x=None, ptr_y=None,
                     differentiable=False, max_query_cloud=None, max_ref_cloud=None, non_oriented=True):
    """``knn_pool`` for tangent-vector features: ``v [2*len(pos_x), C]`` (rows 2i, 2i+1 = the coefficients at point i in ITS
    frame) at ``pos_x`` pooled DOWN to ``pos_y`` -> fp32 ``[2*len(pos_y), C]`` in the frames of ``pos_y``: for every target its k
    nearest sources (of the same cloud), each carried into the target's frame by parallel transport, reduced by ``reduce`` =
    ``"max"`` (per channel the transported vector of largest norm) ``| "sum" | "add" | "mean"``.  ``frames_x = (normal,
    x_basis[, y_basis])`` of the sources, ``frames_y = (normal, x_basis, y_basis)`` of the targets.  A target whose cloud has
    fewer than k sources reduces what there is; one without any gets zeros.  Search + table + apply; keep the pieces
    (``knn_cross``, ``knn_cross_rotation``, ``pool_vectors``) where the search serves more than one call (``CloudPair`` does).

    ``differentiable=False`` (the default) is INFERENCE ONLY: ``v.requires_grad`` while grad mode is on raises ``RuntimeError``
    instead of cutting the graph silently.  ``differentiable=True``: a ``v`` that requires grad gives a result on the autograd
    graph (the same forward bits) with the gradient w.r.t. ``v`` ONLY -- one launch of an ordered sum over the transposed lists
    of the search, no floating-point atomics, the same bits on every run; a maximum sends its gradient to the nearest of the
    sources that share it.  Frames, normals and positions are never differentiated: one that requires grad raises.  With
    ``ptr_x`` / ``ptr_y``, ``max_query_cloud`` and ``max_ref_cloud`` given nothing synchronises and forward + backward can be
    captured in a ``torch.cuda.graph``.

    Non-HIP tensors raise: there is no CPU path."""
    fn = "knn_pool_vectors"
    _mode(fn, reduce)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{fn}: k = {k} outside [1, {MAX_K}]")
    needs_grad = torch.is_tensor(v) and v.requires_grad and torch.is_grad_enabled()
    if needs_grad and not differentiable:
        raise RuntimeError(f"{fn}: v requires grad, but the device pooling is inference-only by default; call it under "
                           "torch.no_grad(), pass v.detach() or differentiable=True")
    _cross.device(fn, "v", v)
    _cross.no_grad_inputs(fn, pos_x=pos_x, pos_y=pos_y)
    pos_x, pos_y = _cross.rows3(fn, "pos_x", pos_x), _cross.rows3(fn, "pos_y", pos_y)
    if v.dim() != 2 or v.shape[0] != 2 * pos_x.shape[0]:
        raise ValueError(f"{fn}: v must hold two rows per point of pos_x, got {tuple(v.shape)} for {pos_x.shape[0]} points")
    with torch.no_grad():
        qptr, rptr, b, mq = _cross.pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, fn, max_query_cloud)
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
    rmat = knn_cross_rotation(idx, qptr, rptr, frames_y, frames_x, non_oriented, max_query_cloud=mq)
    with torch.no_grad():
        if not needs_grad:
            return pool_vectors(v.detach(), qptr, rptr, idx, rmat, mq, reduce, n_query=pos_y.shape[0])[0]
        mr = _cross.largest_cloud(rptr, max_ref_cloud)
        tptr, tedge, _ = knn_cross_transpose(idx, d2, qptr, rptr, num_ref=pos_x.shape[0])
    # offsets given by the caller may leave rows of v outside every cloud: their gradient is zero, filled by the backward
    return _cross.PoolVectors.apply(v, pool_vectors, pool_vectors_backward, reduce, qptr, rptr, idx, rmat, tptr, tedge, mq, mr,
                                    pos_y.shape[0], ptr_x is None)
