"""Tangent-vector features between two clouds by parallel transport on the device (csrc/interp_transport.hip:
``dc_knn_cross_transport``, ``dc_knn_interpolate_vectors``, ``dc_knn_interpolate_vectors_backward``): the vector stream's
counterpart of ``knn_interpolate``.  A vector feature is a pair of coefficients in the tangent frame of its own point (``[2N, C]``,
rows 2i, 2i+1); ``build_tangent_basis`` frames are not continuous over a surface, so the coefficients of a neighbour are first
carried into the target point's frame (reference: deltaconv/geometry/connection.py:6-47, ``dcconn::transport``) and then weighted
as ``knn_interpolate`` weights scalars.  With the roles swapped (the sampled cloud is the query, the full cloud the reference) the
same call is a transported, distance-weighted pooling down to the sampled cloud.  ``deltaconv_amd.Propagator(frames=...)`` is the
dataset-level form.

The per-slot matrices ``M = c * R`` are stored once per search (``knn_cross_transport``: 16 k bytes per target row) and the
apply kernels are pure gathers over them.  The gradient w.r.t. the VALUES is opt-in (``differentiable=True``): an ordered,
atomics-free sum over the transposed lists of the search (``knn_cross_transpose``), bit-reproducible.  None of the geometry is
differentiable: frames, normals and positions are constants.  There is no CPU path."""
import torch

from . import _cross
from ._cross import MAX_K
from .interpolate import knn_cross, knn_cross_transpose

__all__ = ["knn_cross_transport", "interpolate_vectors", "interpolate_vectors_backward", "knn_interpolate_vectors"]


def _table(fn, tmat, rows=None):
    _cross.device(fn, "tmat", tmat)
    if tmat.dtype != torch.float32 or tmat.dim() != 2 or tmat.shape[1] != 4 or not tmat.is_contiguous() or \
            (rows is not None and tmat.shape[0] != rows):
        raise ValueError(f"{fn}: tmat must be contiguous float32 [{'Nq*k' if rows is None else rows}, 4] (knn_cross_transport), got "
                         f"{tuple(tmat.shape)}")
    if tmat.data_ptr() % 16:
        raise ValueError(f"{fn}: tmat must be 16-byte aligned (one 16-byte load per slot)")
    return tmat


def knn_cross_transport(idx, d2, qptr, rptr, query_frames, ref_frames, non_oriented=True, max_query_cloud=None):
    """The table of per-slot matrices of a ``knn_cross`` result (``dc_knn_cross_transport``) -> fp32 ``[Nq*k, 4]``, row-major
    2 x 2: entry ``q*k + s`` is ``c * R`` with ``c`` the interpolation coefficient of the slot (``w_s / den``; exactly 1 for the
    only valid slot of a query) and ``R = build_transport(query frame of q, reference frame of rptr[b] + idx[q, s])``.  Invalid
    slots and rows outside every pair hold zeros.

    idx int32 / d2 fp32 ``[Nq, k]`` on the DEVICE, qptr / rptr int64 ``[B+1]`` ABSOLUTE offsets.  ``query_frames = (normal,
    x_basis, y_basis)`` over the rows of idx, ``ref_frames = (normal, x_basis)`` over the rows rptr names (a third entry is accepted
    and ignored): ``[rows, 3]`` device tensors.  ``max_query_cloud``: the largest query cloud where the host knows it (otherwise
    read from the offsets: one synchronise).  Nothing here is differentiable: an input that requires grad while grad mode is on
    raises ``RuntimeError``."""
    from .._lib import lib
    fn = "knn_cross_transport"
    nq, k = _cross.search(fn, idx, d2)
    if len(query_frames) != 3 or len(ref_frames) not in (2, 3):
        raise ValueError(f"{fn}: query_frames = (normal, x_basis, y_basis), ref_frames = (normal, x_basis[, y_basis])")
    _cross.no_grad_inputs(fn, query_normal=query_frames[0], query_x_basis=query_frames[1], query_y_basis=query_frames[2],
                           ref_normal=ref_frames[0], ref_x_basis=ref_frames[1], d2=d2)
    tn = _cross.rows3(fn, "query normal", query_frames[0], nq)
    tx, ty = _cross.rows3(fn, "query x_basis", query_frames[1], nq), _cross.rows3(fn, "query y_basis", query_frames[2], nq)
    sn = _cross.rows3(fn, "ref normal", ref_frames[0])
    sx = _cross.rows3(fn, "ref x_basis", ref_frames[1], sn.shape[0])
    dev = idx.device
    qptr, rptr = _cross.offsets(fn, dev, qptr=qptr, rptr=rptr)
    b = int(qptr.numel()) - 1
    mq = _cross.largest_cloud(qptr, max_query_cloud)
    with torch.no_grad():
        tmat = torch.zeros((nq * k, 4), dtype=torch.float32, device=dev)
        if nq == 0 or mq == 0:
            return tmat
        if sn.shape[0] == 0:                   # every reference cloud is empty: rows that are never read stand in for the null pointers
            sn, sx = sn.new_zeros((1, 3)), sx.new_zeros((1, 3))
        for lo, hi in _cross.launches(b):
            lib.call("dc_knn_cross_transport", qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, nq, mq, k, idx, d2, tn, tx, ty, sn, sx,
                     int(bool(non_oriented)), tmat)
    return tmat


def interpolate_vectors(v, qptr, rptr, idx, tmat, max_query_cloud, n_query=None, out=None):
    """The arithmetic half of ``knn_interpolate_vectors`` on a search result and its table (``dc_knn_interpolate_vectors``):
    v ``[2*Nr, C]`` DEVICE fp32 (rows may be strided) -> ``[2*n_query, C]``; rows ``2q, 2q+1`` of query ``q = qptr[b] + i`` are
    ``(au, av)`` with ``au = (au + M00*v[2j]) + M01*v[2j+1]``, ``av = (av + M10*v[2j]) + M11*v[2j+1]`` over the valid slots in
    order, ``j = rptr[b] + idx[q, s]``, ``M = tmat[q*k + s]`` (csrc/interp_transport_math.h); a query without a valid slot gets
    zeros.  Not recorded by autograd; ``interpolate_vectors_backward`` is its gradient w.r.t. v."""
    from .._lib import lib
    fn = "interpolate_vectors"
    v, c, ldv = _cross.values(fn, "v", v, per_point=2)
    nq, k = _cross.search(fn, idx)
    tmat = _table(fn, tmat, nq * k)
    qptr, rptr = _cross.offsets(fn, v.device, qptr=qptr, rptr=rptr)
    n_query = nq if n_query is None else int(n_query)
    out, ldo = _cross.out_rows(fn, out, 2 * n_query, c, v.device, on_device=True)
    b = int(qptr.numel()) - 1
    if n_query == 0 or nq == 0:
        return out
    if v.shape[0] == 0:                        # no reference row at all: every slot is invalid, rows that are never read stand in
        v, ldv = v.new_zeros((2, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_interpolate_vectors", v, ldv, c, qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, int(max_query_cloud), k, idx,
                 tmat, out, ldo)
    return out


def interpolate_vectors_backward(g, rptr, tptr, tedge, tmat, k, max_ref_cloud, n_ref=None, edge_base=0, out=None):
    """The gradient of ``interpolate_vectors`` w.r.t. v on the lists of ``knn_cross_transpose``
    (``dc_knn_interpolate_vectors_backward``): g ``[2*n_query, C]`` DEVICE fp32 (rows may be strided) -> fp32 ``[2*n_ref, C]``
    with, for reference row r and its in-edges e in ascending order, ``i = e // k - edge_base``, ``M = tmat[e - edge_base*k]``:
    ``du = (du + M00*g[2i]) + M10*g[2i+1]``, ``dw = (dw + M01*g[2i]) + M11*g[2i+1]``, every product and sum rounded on its own: no
    atomics, the same bits on every run.  Every reference row of every pair is written (zeros without in-edges); rows of ``out``
    outside every pair keep what they held (zeros when allocated here).  ``tptr`` is indexed by the rows ``rptr`` names, ``tmat``
    starts at the call's first query row; ``edge_base``: see ``dc_knn_interpolate_backward``.  One launch per 65 535 pairs."""
    from .._lib import lib
    fn = "interpolate_vectors_backward"
    g, c, ldg = _cross.values(fn, "g", g, per_point=2)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{fn}: k = {k} outside [1, {MAX_K}]")
    tmat = _table(fn, tmat)
    rptr = _cross.offsets(fn, g.device, rptr=rptr)
    for name, t in (("tptr", tptr), ("tedge", tedge)):
        _cross.device(fn, name, t)
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous int64 (knn_cross_transpose)")
    n_ref = int(tptr.numel()) - 1 if n_ref is None else int(n_ref)
    out, ldo = _cross.out_rows(fn, out, 2 * n_ref, c, g.device, on_device=True)
    b = int(rptr.numel()) - 1
    if n_ref == 0:
        return out
    rows = int(g.shape[0]) // 2
    if rows == 0:                              # no query row at all: every edge is skipped, rows that are never read stand in
        g, ldg = g.new_zeros((2, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_interpolate_vectors_backward", g, ldg, rows, c, rptr[lo:hi + 1], hi - lo, int(max_ref_cloud), k, tptr,
                 tedge, int(tedge.numel()), int(edge_base), tmat, int(tmat.shape[0]), out, ldo)
    return out


def knn_interpolate_vectors(v, pos_x, pos_y, frames_x, frames_y, batch_x=None, batch_y=None, k=3, ptr_x=None, ptr_y=None,
                            non_oriented=True, differentiable=False, max_query_cloud=None, max_ref_cloud=None):
    """``knn_interpolate`` for tangent-vector features: ``v [2*len(pos_x), C]`` (rows 2i, 2i+1 = the coefficients at point i in
    ITS frame) at ``pos_x`` -> fp32 ``[2*len(pos_y), C]`` in the frames of ``pos_y``: for every target its k nearest sources (of
    the same cloud), each carried into the target's frame by parallel transport (connection.py:6-47) and weighted by
    ``1 / clamp(d^2, min=1e-16)``.  ``frames_x = (normal, x_basis[, y_basis])`` of the sources, ``frames_y = (normal, x_basis,
    y_basis)`` of the targets, as ``build_tangent_basis`` returns them.  Search + table + apply; keep the pieces
    (``knn_cross``, ``knn_cross_transport``, ``interpolate_vectors``) where the search serves more than one call.

    ``differentiable=False`` (the default) is INFERENCE ONLY: ``v.requires_grad`` while grad mode is on raises ``RuntimeError``
    instead of cutting the graph silently.  ``differentiable=True``: a ``v`` that requires grad gives a result on the autograd
    graph (the same forward bits) with the gradient w.r.t. ``v`` ONLY -- one launch of an ordered sum over the transposed lists
    of the search, no floating-point atomics, the same bits on every run.  Frames, normals and positions are never differentiated:
    one that requires grad raises.  With ``ptr_x`` / ``ptr_y``, ``max_query_cloud`` and ``max_ref_cloud`` given nothing
    synchronises and forward + backward can be captured in a ``torch.cuda.graph``.

    Non-HIP tensors raise: there is no CPU path."""
    fn = "knn_interpolate_vectors"
    needs_grad = torch.is_tensor(v) and v.requires_grad and torch.is_grad_enabled()
    if needs_grad and not differentiable:
        raise RuntimeError(f"{fn}: v requires grad, but the device interpolation is inference-only by default; call it under "
                           "torch.no_grad(), pass v.detach() or differentiable=True")
    _cross.device(fn, "v", v)
    _cross.no_grad_inputs(fn, pos_x=pos_x, pos_y=pos_y)
    pos_x, pos_y = _cross.rows3(fn, "pos_x", pos_x), _cross.rows3(fn, "pos_y", pos_y)
    if v.dim() != 2 or v.shape[0] != 2 * pos_x.shape[0]:
        raise ValueError(f"{fn}: v must hold two rows per point of pos_x, got {tuple(v.shape)} for {pos_x.shape[0]} points")
    with torch.no_grad():
        qptr, rptr, b, mq = _cross.pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, fn, max_query_cloud)
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
    tmat = knn_cross_transport(idx, d2, qptr, rptr, frames_y, frames_x, non_oriented, max_query_cloud=mq)
    with torch.no_grad():
        if not needs_grad:
            return interpolate_vectors(v.detach(), qptr, rptr, idx, tmat, mq, n_query=pos_y.shape[0])
        mr = _cross.largest_cloud(rptr, max_ref_cloud)
        tptr, tedge, _ = knn_cross_transpose(idx, d2, qptr, rptr, num_ref=pos_x.shape[0])
    # offsets given by the caller may leave rows of v outside every cloud: their gradient is zero, filled by the backward
    return _cross.Interpolate.apply(v, interpolate_vectors, interpolate_vectors_backward, 2, qptr, rptr, idx, tmat, tptr, tedge, tmat,
                                    mq, mr, pos_y.shape[0], 0, ptr_x is None)
