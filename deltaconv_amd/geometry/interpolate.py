"""Two-set nearest neighbours and inverse-squared-distance interpolation on the device (csrc/interp.hip: ``dc_knn_cross``,
``dc_knn_interpolate``): PointNet++ feature propagation, what ``torch_cluster.knn`` and ``torch_geometric.nn.knn_interpolate``
do -- the way back up from a sampled cloud to the points or vertices it was sampled from.  ``deltaconv_amd.Propagator``
(propagate.py) is the dataset-level form.

Inference only: nothing here is recorded by autograd and there is no backward kernel.  There is no CPU path."""
import torch

__all__ = ["knn_cross", "knn_interpolate", "interpolate_rows", "MAX_K"]

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
    buffers held (``-1`` / ``+inf`` when allocated here).  Inference only: the result carries no autograd graph."""
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
    (csrc/interp_math.h: ``w = 1 / max(d2, 1e-16)``; one valid slot is an exact copy, none a row of zeros).  Inference only."""
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


def knn_interpolate(x, pos_x, pos_y, batch_x=None, batch_y=None, k=3, ptr_x=None, ptr_y=None):
    """``torch_geometric.nn.knn_interpolate(x, pos_x, pos_y, batch_x, batch_y, k)``: the features ``x [len(pos_x), C]`` at
    ``pos_x`` interpolated to ``pos_y`` -- for every target its k nearest sources (of the same cloud), weighted by
    ``1 / clamp(d^2, min=1e-16)``.  -> fp32 ``[len(pos_y), C]``.  ``ptr_x`` / ``ptr_y`` (int64 [B+1] row offsets) stand in for
    the sorted ``batch`` vectors where the offsets are at hand.

    INFERENCE ONLY: there is no backward kernel.  ``x.requires_grad`` while grad mode is on raises ``RuntimeError`` instead of
    cutting the graph silently -- call it under ``torch.no_grad()`` or pass ``x.detach()``.  Non-HIP tensors raise: there is no
    CPU path."""
    if torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled():
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
        qptr, rptr, b, mq = _pairs(pos_y, pos_x, ptr_y, ptr_x, batch_y, batch_x, "knn_interpolate")
        idx, d2 = knn_cross(pos_y, pos_x, k, ptr_query=qptr, ptr_ref=rptr, max_query_cloud=mq)
        return interpolate_rows(x.detach(), qptr, rptr, idx, d2, mq, n_query=pos_y.shape[0])
