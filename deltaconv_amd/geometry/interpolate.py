"""Two-set nearest neighbours and inverse-squared-distance interpolation on the device (csrc/interp.hip: ``dc_knn_cross``,
``dc_knn_interpolate``): PointNet++ feature propagation, what ``torch_cluster.knn`` and ``torch_geometric.nn.knn_interpolate``
do -- the way back up from a sampled cloud to the points or vertices it was sampled from.  ``deltaconv_amd.Propagator``
(propagate.py) is the dataset-level form.

The gradient w.r.t. the interpolated FEATURES is opt-in (``knn_interpolate(..., differentiable=True)``): the transposed lists of
the search (``knn_cross_transpose``: ``dc_knn_cross_transpose``) and an ordered, atomics-free sum over them
(``interpolate_rows_backward``: ``dc_knn_interpolate_backward``), bit-reproducible.  There is NO gradient for positions or
distances (PyG's op is differentiable through the weights; this one is not).  There is no CPU path."""
import torch

from . import _cross
from ._cross import MAX_K

__all__ = ["knn_cross", "knn_cross_transpose", "knn_interpolate", "interpolate_rows", "interpolate_rows_backward", "MAX_K"]


def knn_cross(pos_query, pos_ref, k, ptr_query=None, ptr_ref=None, batch_query=None, batch_ref=None, max_query_cloud=None,
              out=None, method=None, grid_target=None):
    """The k nearest points of ``pos_ref`` for every point of ``pos_query``, cloud pair by cloud pair (``torch_cluster.knn``).

    pos_query [Nq,3], pos_ref [Nr,3]: DEVICE fp32.  The clouds are given as ``ptr_*`` (int64 [B+1] ABSOLUTE row offsets; a slice
    of a store's ``ptr`` serves) or as sorted ``batch_*`` vectors; with neither, one cloud pair.  Differing cloud counts raise
    ``ValueError``.  ``max_query_cloud``: the largest query cloud where the host knows it (otherwise read from the offsets: one
    synchronise).  ``out``: preallocated ``(idx, d2)`` to write into.
    -> ``(idx int32 [Nq,k], d2 fp32 [Nq,k])``: reference ids LOCAL to the pair's reference cloud in ascending fp32 squared
    distance, ties by the lower id (the order contract of ``knn_graph``); ``-1`` / ``+inf`` where a reference cloud has fewer
    than k points.  A point with a NaN coordinate is never picked.  Rows of ``pos_query`` outside every cloud keep what the
    buffers held (``-1`` / ``+inf`` when allocated here).  The result carries no autograd graph: positions are not differentiated.

    ``method``: "brute" (``dc_knn_cross``: Nq x Nr distances per pair) or "grid" (``dc_knn_cross_grid``: the same ``idx`` and ``d2``
    bit for bit through a uniform cell grid over each reference cloud, for large reference clouds), None = the switch
    ``geometry.graph.KNN_METHOD[0]`` (``DC_KNN``, default "brute").  ``grid_target``: the grid's mean points per cell (None =
    ``geometry.graph.GRID_TARGET``); it cannot change the result."""
    from .._lib import lib
    from . import graph as _graph
    method = _graph.knn_method("knn_cross", method)
    pos_query, pos_ref = _cross.rows3("knn_cross", "pos_query", pos_query), _cross.rows3("knn_cross", "pos_ref", pos_ref)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn_cross: k = {k} outside [1, {MAX_K}]")
    qptr, rptr, b, mq = _cross.pairs(pos_query, pos_ref, ptr_query, ptr_ref, batch_query, batch_ref, "knn_cross", max_query_cloud)
    nq, dev = pos_query.shape[0], pos_query.device
    if out is None:
        idx = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
        d2 = torch.full((nq, k), float("inf"), dtype=torch.float32, device=dev)
    else:
        idx, d2 = out
        for t, dt in ((idx, torch.int32), (d2, torch.float32)):
            if t.dtype != dt or tuple(t.shape) != (nq, k) or not t.is_contiguous():
                raise ValueError(f"knn_cross: out must be contiguous (int32, float32) [{nq}, {k}]")
    if nq == 0:
        return idx, d2
    if pos_ref.shape[0] == 0:                  # every reference cloud is empty: a row that is never read stands in for the null pointer
        pos_ref = pos_ref.new_zeros((1, 3))
    if method == "grid" and b > 0:
        target = float(_graph.GRID_TARGET if grid_target is None else grid_target)
        # the offsets may be a slice of a store's: the reference rows of the call are at most those of pos_ref
        work, nbytes = _graph.grid_workspace(pos_ref.shape[0], min(b, _cross.MAX_PAIRS), dev)
    for lo, hi in _cross.launches(b):
        if method == "grid":
            lib.call("dc_knn_cross_grid", pos_query, qptr[lo:hi + 1], pos_ref, rptr[lo:hi + 1], hi - lo, mq, k, target, idx, d2,
                     work, nbytes)
        else:
            lib.call("dc_knn_cross", pos_query, qptr[lo:hi + 1], pos_ref, rptr[lo:hi + 1], hi - lo, mq, k, idx, d2)
    return idx, d2


def interpolate_rows(x, qptr, rptr, idx, d2, max_query_cloud, n_query=None, out=None):
    """The arithmetic half of ``knn_interpolate`` on a search result: x [Nr,C] DEVICE fp32 (rows may be strided) -> [n_query,C]
    with row ``qptr[b] + i`` = the inverse-squared-distance mean of rows ``rptr[b] + idx[qptr[b] + i]`` of x
    (csrc/interp_math.h: ``w = 1 / max(d2, 1e-16)``; one valid slot is an exact copy, none a row of zeros).  Not recorded by
    autograd; ``interpolate_rows_backward`` is its gradient w.r.t. x."""
    from .._lib import lib
    x, c, ldx = _cross.values("interpolate_rows", "x", x)
    k = int(idx.shape[1])
    n_query = int(idx.shape[0]) if n_query is None else int(n_query)
    out, ldo = _cross.out_rows("interpolate_rows", out, n_query, c, x.device)
    b = int(qptr.numel()) - 1
    if n_query == 0 or idx.shape[0] == 0:
        return out
    if x.shape[0] == 0:                        # no reference row at all: every slot is invalid, a row that is never read stands in
        x, ldx = x.new_zeros((1, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_interpolate", x, ldx, c, qptr[lo:hi + 1], rptr[lo:hi + 1], hi - lo, int(max_query_cloud), k, idx, d2, out,
                 ldo)
    return out


def knn_cross_transpose(idx, d2, qptr, rptr, num_ref=None):
    """The transposed lists of a ``knn_cross`` result (``dc_knn_cross_transpose``): for every reference row its in-edges, i.e. the
    valid slots ``(q, s)`` that picked it, as edge ids ``e = q * k + s`` (q: the row of ``idx``) in ASCENDING order, with the
    coefficient of each (csrc/interp_math.h: 1 for the only valid slot of a query, else ``w_s / den``).

    idx int32 / d2 fp32 ``[Nq,k]`` on the DEVICE, qptr / rptr int64 ``[B+1]`` ABSOLUTE offsets (any B).  ``num_ref``: the rows of
    the reference tensor (``tptr`` is indexed like it); where it is not given it is read from ``rptr[-1]`` (one synchronise).
    -> ``(tptr int64 [num_ref+1], tedge int64 [Nq*k], tcoef fp32 [Nq*k])``: the list of row r is ``[tptr[r], tptr[r+1])``; the
    first ``tptr[-1]`` entries of tedge / tcoef are written, the rest is zero.  A function of the inputs only (integer atomics,
    then a ranking pass); no synchronise with ``num_ref`` given, capturable.  No gradient flows into ``d2``."""
    from .._lib import lib
    nq, k = _cross.search("knn_cross_transpose", idx, d2)
    dev = idx.device
    qptr, rptr = _cross.offsets("knn_cross_transpose", dev, qptr=qptr, rptr=rptr)
    num_ref = int(rptr[-1]) if num_ref is None else int(num_ref)
    with torch.no_grad():
        tptr = torch.empty(num_ref + 1, dtype=torch.int64, device=dev)
        tedge = torch.zeros(nq * k, dtype=torch.int64, device=dev)
        tcoef = torch.zeros(nq * k, dtype=torch.float32, device=dev)
        nbytes = int(lib.raw("dc_knn_cross_transpose_workspace_bytes")(nq, num_ref, k))
        work = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
        lib.call("dc_knn_cross_transpose", qptr, rptr, int(qptr.numel()) - 1, nq, num_ref, k, idx, d2, tptr, tedge, tcoef, work,
                 work.numel() * 8)
    return tptr, tedge, tcoef


def interpolate_rows_backward(g, rptr, tptr, tedge, tcoef, k, max_ref_cloud, n_ref=None, edge_base=0, out=None):
    """The gradient of ``interpolate_rows`` w.r.t. x on the lists of ``knn_cross_transpose`` (``dc_knn_interpolate_backward``):
    g ``[n_query,C]`` DEVICE fp32 (rows may be strided) -> fp32 ``[n_ref,C]`` with
    ``dx[r] = sum over the in-edges of r, in ascending order, of tcoef * g[e // k - edge_base]``, every product and sum rounded on
    its own: no atomics, the same bits on every run.  Every reference row of every pair is written (zeros without in-edges); rows
    of ``out`` outside every pair keep what they held (zeros when allocated here).  ``tptr`` is indexed by the rows ``rptr``
    names; ``edge_base``: see ``dc_knn_interpolate_backward``.  One launch per 65 535 pairs, no synchronise."""
    from .._lib import lib
    g, c, ldg = _cross.values("interpolate_rows_backward", "g", g)
    k = int(k)
    n_ref = int(tptr.numel()) - 1 if n_ref is None else int(n_ref)
    out, ldo = _cross.out_rows("interpolate_rows_backward", out, n_ref, c, g.device)
    b = int(rptr.numel()) - 1
    if n_ref == 0:
        return out
    if g.shape[0] == 0:                        # no query row at all: every edge is skipped, a row that is never read stands in
        g, ldg = g.new_zeros((1, c)), c
    for lo, hi in _cross.launches(b):
        lib.call("dc_knn_interpolate_backward", g, ldg, int(g.shape[0]), c, rptr[lo:hi + 1], hi - lo, int(max_ref_cloud), k, tptr,
                 tedge, tcoef, int(tedge.numel()), int(edge_base), out, ldo)
    return out


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, ptr_x=None, ptr_y=None, differentiable=False,
                    max_query_cloud=None, max_ref_cloud=None):
    """``torch_geometric.nn.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k)``: the features ``x [len(pos_x), C]`` at
    ``pos_x`` interpolated to ``pos_y`` -- for every target its k nearest sources (of the same cloud), weighted by
    ``1 / clamp(d^2, min=1e-16)``.  -> fp32 ``[len(pos_y), C]``.  ``ptr_x`` / ``ptr_y`` (int64 [B+1] row offsets) stand in for
    the sorted ``batch`` vectors where the offsets are at hand.

    ``differentiable=False`` (the default) is INFERENCE ONLY: ``x.requires_grad`` while grad mode is on raises ``RuntimeError``
    instead of cutting the graph silently -- call it under ``torch.no_grad()``, pass ``x.detach()``, or ask for the gradient:

    ``differentiable=True``: an ``x`` that requires grad gives a result on the autograd graph (the same forward bits).  The
    forward also builds the transposed lists of the search (``knn_cross_transpose``), so that the backward is one launch of an
    ordered sum: no floating-point atomics, the same gradient bits on every run; it is a contiguous fp32-computed tensor of x's
    shape, also for a strided or 1-D x.  Once differentiable; NO gradient for ``pos_x`` / ``pos_y`` (PyG's op has one through the
    weights).  ``max_query_cloud`` / ``max_ref_cloud``: the largest target / source cloud where the host knows them; with both
    and ``ptr_x`` / ``ptr_y`` given nothing synchronises and forward + backward can be captured in a ``torch.cuda.graph``.

    Non-HIP tensors raise: there is no CPU path."""
    needs_grad = torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled()
    if needs_grad and not differentiable:
        raise RuntimeError("knn_interpolate: x requires grad, but the device interpolation is inference-only by default; call it "
                           "under torch.no_grad(), pass x.detach() or differentiable=True")
    _cross.device("knn_interpolate", "x", x)
    pos_x, pos_y = _cross.rows3("knn_interpolate", "pos_x", pos_x), _cross.rows3("knn_interpolate", "pos_y", pos_y)
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[0] != pos_x.shape[0]:
        raise ValueError(f"knn_interpolate: x must hold one row per point of pos_x, got {tuple(x.shape)} for {pos_x.shape[0]} points")
    with torch.no_grad():
        qptr, rptr, b, mq = _cross.pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, "knn_interpolate", max_query_cloud)
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
        if not needs_grad:
            return interpolate_rows(x.detach(), qptr, rptr, idx, d2, mq, n_query=pos_y.shape[0])
        mr = _cross.largest_cloud(rptr, max_ref_cloud)
        tptr, tedge, tcoef = knn_cross_transpose(idx, d2, qptr, rptr, num_ref=pos_x.shape[0])
    # offsets given by the caller may leave rows of x outside every cloud: their gradient is zero, filled by the backward
    return _cross.Interpolate.apply(x, interpolate_rows, interpolate_rows_backward, 1, qptr, rptr, idx, d2, tptr, tedge, tcoef, mq, mr,
                                    pos_y.shape[0], 0, ptr_x is None)
