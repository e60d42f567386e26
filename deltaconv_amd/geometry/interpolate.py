"""Two-set nearest neighbours and inverse-squared-distance interpolation on the device (csrc/interp.hip: ``dc_knn_cross``,
``dc_knn_interpolate``): PointNet++ feature propagation, what ``torch_cluster.knn`` and ``torch_geometric.nn.knn_interpolate``
do -- the way back up from a sampled cloud to the points or vertices it was sampled from.  ``deltaconv_amd.Propagator``
(propagate.py) is the dataset-level form.

The gradient w.r.t. the interpolated FEATURES is opt-in (``knn_interpolate(..., differentiable=True)``): the transposed lists of
the search (``knn_cross_transpose``: ``dc_knn_cross_transpose``) and an ordered, atomics-free sum over them
(``interpolate_rows_backward``: ``dc_knn_interpolate_backward``), bit-reproducible.  There is NO gradient for positions or
distances (PyG's op is differentiable through the weights; this one is not).  There is no CPU path."""
import torch
from torch.autograd.function import once_differentiable

__all__ = ["knn_cross", "knn_cross_transpose", "knn_interpolate", "interpolate_rows", "interpolate_rows_backward", "MAX_K"]

MAX_K = 16                 # csrc/interp_math.h: MAX_K
MAX_PAIRS = 65535          # cloud pairs per launch (the grid's second dimension)


def _device_f32(name, t, cols=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on a HIP device (there is no CPU path)")
    if t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"{name} must be [n, {cols or 'C'}], got {tuple(t.shape)}")
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.contiguous().float()


def _offsets(n, ptr, batch, device, what, known_max=None):
    """-> (ptr int64 [B+1] on the device, B, largest cloud): from `ptr`, from a sorted `batch` vector (one host read, as
    graph._ptr_from_batch), or one cloud of n rows.  known_max: the largest cloud where the caller knows it (no host read of ptr)."""
    if ptr is not None and batch is not None:
        raise ValueError(f"{what}: give ptr or batch, not both")
    if ptr is not None:
        ptr = torch.as_tensor(ptr).to(device=device, dtype=torch.int64).contiguous()
        if ptr.dim() != 1 or ptr.numel() < 1:
            raise ValueError(f"{what}: ptr must hold B+1 offsets")
        b = int(ptr.numel()) - 1
        if known_max is not None:
            return ptr, b, int(known_max)
        return ptr, b, (int((ptr[1:] - ptr[:-1]).max()) if b else 0)
    if batch is None:
        return torch.tensor([0, n], dtype=torch.int64).to(device), 1, n
    if batch.dim() != 1 or batch.shape[0] != n:
        raise ValueError(f"{what}: batch must hold one cloud id per row")
    if n == 0:
        return torch.zeros(1, dtype=torch.int64, device=device), 0, 0
    counts = torch.bincount(batch.to(device))
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=device)
    ptr[1:] = torch.cumsum(counts, 0)
    return ptr, int(counts.numel()), int(counts.max())


def _pairs(pos_query, pos_ref, ptr_query, ptr_ref, batch_query, batch_ref, what, max_query_cloud=None):
    dev = pos_query.device
    qptr, bq, mq = _offsets(pos_query.shape[0], ptr_query, batch_query, dev, what, max_query_cloud)
    rptr, br, _ = _offsets(pos_ref.shape[0], ptr_ref, batch_ref, dev, what, 0)
    mq = mq if max_query_cloud is None else int(max_query_cloud)
    if bq != br:
        raise ValueError(f"{what}: {bq} query clouds but {br} reference clouds")
    return qptr, rptr, bq, mq


def _launches(b):
    return [(lo, min(b, lo + MAX_PAIRS)) for lo in range(0, b, MAX_PAIRS)]


def knn_cross(pos_query, pos_ref, k, ptr_query=None, ptr_ref=None, batch_query=None, batch_ref=None, max_query_cloud=None,
              out=None):
    """The k nearest points of ``pos_ref`` for every point of ``pos_query``, cloud pair by cloud pair (``torch_cluster.knn``).

    pos_query [Nq,3], pos_ref [Nr,3]: DEVICE fp32.  The clouds are given as ``ptr_*`` (int64 [B+1] ABSOLUTE row offsets; a slice
    of a store's ``ptr`` serves) or as sorted ``batch_*`` vectors; with neither, one cloud pair.  Differing cloud counts raise
    ``ValueError``.  ``max_query_cloud``: the largest query cloud where the host knows it (otherwise read from the offsets: one
    synchronise).  ``out``: preallocated ``(idx, d2)`` to write into.
    -> ``(idx int32 [Nq,k], d2 fp32 [Nq,k])``: reference ids LOCAL to the pair's reference cloud in ascending fp32 squared
    distance, ties by the lower id (the order contract of ``knn_graph``); ``-1`` / ``+inf`` where a reference cloud has fewer
    than k points.  A point with a NaN coordinate is never picked.  Rows of ``pos_query`` outside every cloud keep what the
    buffers held (``-1`` / ``+inf`` when allocated here).  The result carries no autograd graph: positions are not differentiated."""
    from .._lib import lib
    pos_query, pos_ref = _device_f32("knn_cross: pos_query", pos_query, 3), _device_f32("knn_cross: pos_ref", pos_ref, 3)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"knn_cross: k = {k} outside [1, {MAX_K}]")
    qptr, rptr, b, mq = _pairs(pos_query, pos_ref, ptr_query, ptr_ref, batch_query, batch_ref, "knn_cross", max_query_cloud)
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
    for lo, hi in _launches(b):
        lib.call("dc_knn_cross", pos_query, qptr[lo:hi + 1], pos_ref, rptr[lo:hi + 1], hi - lo, mq, k, idx, d2)
    return idx, d2


def interpolate_rows(x, qptr, rptr, idx, d2, max_query_cloud, n_query=None, out=None):
    """The arithmetic half of ``knn_interpolate`` on a search result: x [Nr,C] DEVICE fp32 (rows may be strided) -> [n_query,C]
    with row ``qptr[b] + i`` = the inverse-squared-distance mean of rows ``rptr[b] + idx[qptr[b] + i]`` of x
    (csrc/interp_math.h: ``w = 1 / max(d2, 1e-16)``; one valid slot is an exact copy, none a row of zeros).  Not recorded by
    autograd; ``interpolate_rows_backward`` is its gradient w.r.t. x."""
    from .._lib import lib
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("interpolate_rows: x must be a tensor on a HIP device (there is no CPU path)")
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"interpolate_rows: x must be [n, C] with C >= 1, got {tuple(x.shape)}")
    # the kernel reads channels at unit stride and rows ldx >= C apart: anything else (a channel slice such as t[:, ::2], also
    # of ONE row; an expanded row) is copied.  One channel has no channel stride, one row no row stride.
    if x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.float().contiguous()
    c, k = int(x.shape[1]), int(idx.shape[1])
    ldx = int(x.stride(0)) if x.shape[0] > 1 else c
    n_query = int(idx.shape[0]) if n_query is None else int(n_query)
    if out is None:
        out = torch.zeros((n_query, c), dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n_query, c) or (c > 1 and out.stride(1) != 1) or \
            (n_query > 1 and out.stride(0) < c):
        raise ValueError(f"interpolate_rows: out must be float32 [{n_query}, {c}] with unit stride along the channels and rows "
                         "that do not overlap")
    ldo = int(out.stride(0)) if n_query > 1 else c
    b = int(qptr.numel()) - 1
    if n_query == 0 or idx.shape[0] == 0:
        return out
    if x.shape[0] == 0:                        # no reference row at all: every slot is invalid, a row that is never read stands in
        x = x.new_zeros((1, c))
    for lo, hi in _launches(b):
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
    for name, t, dt in (("idx", idx, torch.int32), ("d2", d2, torch.float32)):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"knn_cross_transpose: {name} must be a tensor on a HIP device (there is no CPU path)")
        if t.dtype != dt or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"knn_cross_transpose: {name} must be contiguous {dt} [Nq, k]")
    if idx.shape != d2.shape or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError(f"knn_cross_transpose: idx {tuple(idx.shape)} and d2 {tuple(d2.shape)} must agree, k in [1, {MAX_K}]")
    dev = idx.device
    qptr = torch.as_tensor(qptr).to(device=dev, dtype=torch.int64).contiguous()
    rptr = torch.as_tensor(rptr).to(device=dev, dtype=torch.int64).contiguous()
    if qptr.dim() != 1 or qptr.shape != rptr.shape or qptr.numel() < 1:
        raise ValueError("knn_cross_transpose: qptr and rptr must hold B+1 offsets each")
    nq, k = int(idx.shape[0]), int(idx.shape[1])
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
    if not torch.is_tensor(g) or not g.is_cuda:
        raise RuntimeError("interpolate_rows_backward: g must be a tensor on a HIP device (there is no CPU path)")
    if g.dim() != 2 or g.shape[1] < 1:
        raise ValueError(f"interpolate_rows_backward: g must be [n, C] with C >= 1, got {tuple(g.shape)}")
    if g.dtype != torch.float32 or (g.shape[1] > 1 and g.stride(1) != 1) or (g.shape[0] > 1 and g.stride(0) < g.shape[1]):
        g = g.float().contiguous()
    c, k = int(g.shape[1]), int(k)
    ldg = int(g.stride(0)) if g.shape[0] > 1 else c
    n_ref = int(tptr.numel()) - 1 if n_ref is None else int(n_ref)
    if out is None:
        out = torch.zeros((n_ref, c), dtype=torch.float32, device=g.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (n_ref, c) or (c > 1 and out.stride(1) != 1) or \
            (n_ref > 1 and out.stride(0) < c):
        raise ValueError(f"interpolate_rows_backward: out must be float32 [{n_ref}, {c}] with unit stride along the channels and "
                         "rows that do not overlap")
    ldo = int(out.stride(0)) if n_ref > 1 else c
    b = int(rptr.numel()) - 1
    if n_ref == 0:
        return out
    if g.shape[0] == 0:                        # no query row at all: every edge is skipped, a row that is never read stands in
        g = g.new_zeros((1, c))
    for lo, hi in _launches(b):
        lib.call("dc_knn_interpolate_backward", g, ldg, int(g.shape[0]), c, rptr[lo:hi + 1], hi - lo, int(max_ref_cloud), k, tptr,
                 tedge, tcoef, int(tedge.numel()), int(edge_base), out, ldo)
    return out


class _InterpolateRows(torch.autograd.Function):
    """``interpolate_rows`` on the autograd graph: the forward is the inference kernel (the same bits), the backward ONE launch on
    transposed lists built beforehand.  ``covered``: every row of x lies in a pair, so the backward writes all of dx itself."""

    @staticmethod
    def forward(ctx, x, qptr, rptr, idx, d2, tptr, tedge, tcoef, mq, mr, n_query, edge_base, covered):
        ctx.save_for_backward(rptr, tptr, tedge, tcoef)
        ctx.meta = (tuple(x.shape), x.dtype, int(idx.shape[1]), int(mr), int(edge_base), bool(covered))
        return interpolate_rows(x.detach(), qptr, rptr, idx, d2, mq, n_query=n_query)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rptr, tptr, tedge, tcoef = ctx.saved_tensors
        shape, dtype, k, mr, edge_base, covered = ctx.meta
        out = torch.empty(shape, dtype=torch.float32, device=g.device) if covered else None
        dx = interpolate_rows_backward(g, rptr, tptr, tedge, tcoef, k, mr, n_ref=shape[0], edge_base=edge_base, out=out)
        return (dx.to(dtype),) + (None,) * 12


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
        raise RuntimeError("knn_interpolate: x requires grad, but the device interpolation is inference-only (no backward kernel); "
                           "call it under torch.no_grad() or pass x.detach()")
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("knn_interpolate: x must be a tensor on a HIP device (there is no CPU path)")
    pos_x, pos_y = _device_f32("knn_interpolate: pos_x", pos_x, 3), _device_f32("knn_interpolate: pos_y", pos_y, 3)
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[0] != pos_x.shape[0]:
        raise ValueError(f"knn_interpolate: x must hold one row per point of pos_x, got {tuple(x.shape)} for {pos_x.shape[0]} points")
    with torch.no_grad():
        qptr, rptr, b, mq = _pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, "knn_interpolate", max_query_cloud)
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
        if not needs_grad:
            return interpolate_rows(x.detach(), qptr, rptr, idx, d2, mq, n_query=pos_y.shape[0])
        mr = int(max_ref_cloud) if max_ref_cloud is not None else (int((rptr[1:] - rptr[:-1]).max()) if b else 0)
        tptr, tedge, tcoef = knn_cross_transpose(idx, d2, qptr, rptr, num_ref=pos_x.shape[0])
    # offsets given by the caller may leave rows of x outside every cloud: their gradient is zero, filled by the backward
    return _InterpolateRows.apply(x, qptr, rptr, idx, d2, tptr, tedge, tcoef, mq, mr, pos_y.shape[0], 0, ptr_x is None)
