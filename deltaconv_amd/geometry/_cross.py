"""What the cross-cloud functions share (interpolate.py, vector_interpolate.py, pool.py, pool_vectors.py, resample.py,
connection.py, propagate.py): their argument checks, each written once -- `fn` is the public function the message names, every
check returns what the kernels take -- and the autograd nodes of the two interpolations and of the two poolings."""
import torch
from torch.autograd.function import once_differentiable

MAX_K = 16                 # csrc/interp_math.h: MAX_K
MAX_PAIRS = 65535          # cloud pairs per launch (the grid's second dimension)


def device(fn, name, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{fn}: {name} must be a tensor on a HIP device (there is no CPU path)")
    return t


def no_grad_inputs(fn, **tensors):
    """The geometry is not differentiable: an input that requires grad while grad mode is on raises."""
    if torch.is_grad_enabled():
        for name, t in tensors.items():
            if torch.is_tensor(t) and t.requires_grad:
                raise RuntimeError(f"{fn}: {name} requires grad, but the device {fn} is not differentiable (no backward kernel); "
                                   f"call it under torch.no_grad() or pass {name}.detach()")


def rows3(fn, name, t, m=None):
    """[M,3] rows (m: how many) -> detached, fp32, contiguous."""
    device(fn, name, t)
    if t.dim() != 2 or t.shape[1] != 3 or (m is not None and t.shape[0] != m):
        want = "[M,3]" if m is None else f"[{m},3]"
        raise ValueError(f"{fn}: {name} must be {want}, got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def values(fn, name, t, per_point=1):
    """[per_point * n, C] DEVICE rows for the kernels -> (t, C, ld): fp32, unit stride along the channels, rows ld >= C apart.
    Anything else (a channel slice such as t[:, ::2], also of ONE row; an expanded row) is copied.  One channel has no channel
    stride, one row no row stride."""
    device(fn, name, t)
    if per_point == 2 and (t.dim() != 2 or t.shape[1] < 1 or t.shape[0] % 2):
        raise ValueError(f"{fn}: {name} must be [2n, C] with C >= 1 (rows 2i, 2i+1 = the two coefficients at point i), got "
                         f"{tuple(t.shape)}")
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"{fn}: {name} must be [n, C] with C >= 1, got {tuple(t.shape)}")
    if t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.float().contiguous()
    return t, int(t.shape[1]), (int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]))


def out_rows(fn, out, rows, c, dev, on_device=False):
    """`out` or a new zero tensor, fp32 [rows, c] -> (out, ld).  on_device: a given `out` off the device is refused here."""
    if out is None:
        out = torch.zeros((rows, c), dtype=torch.float32, device=dev)
    elif on_device:
        device(fn, "out", out)
    if out.dtype != torch.float32 or tuple(out.shape) != (rows, c) or (c > 1 and out.stride(1) != 1) or \
            (rows > 1 and out.stride(0) < c):
        raise ValueError(f"{fn}: out must be float32 [{rows}, {c}] with unit stride along the channels and rows that do not overlap")
    return out, (int(out.stride(0)) if rows > 1 else c)


def offsets(fn, dev, **ptrs):
    """int64 [B+1] offsets on the device, each: a list or a host tensor is brought over."""
    out = [torch.as_tensor(t).to(device=dev, dtype=torch.int64).contiguous() for t in ptrs.values()]
    if any(t.dim() != 1 or t.numel() < 1 or t.shape != out[0].shape for t in out):
        raise ValueError(f"{fn}: {' and '.join(ptrs)} must hold B+1 offsets each")
    return out if len(out) > 1 else out[0]


def largest_cloud(ptr, known=None):
    """The largest cloud of the offsets: `known` where the host has it, otherwise read from the device (one synchronise)."""
    if known is not None:
        return int(known)
    return int((ptr[1:] - ptr[:-1]).max()) if ptr.numel() > 1 else 0


def cloud_offsets(n, ptr, batch, device, what, known_max=None):
    """-> (ptr int64 [B+1] on the device, B, largest cloud): from `ptr`, from a sorted `batch` vector (one host read, as
    graph._ptr_from_batch), or one cloud of n rows.  known_max: the largest cloud where the caller knows it (no host read of ptr)."""
    if ptr is not None and batch is not None:
        raise ValueError(f"{what}: give ptr or batch, not both")
    if ptr is not None:
        ptr = torch.as_tensor(ptr).to(device=device, dtype=torch.int64).contiguous()
        if ptr.dim() != 1 or ptr.numel() < 1:
            raise ValueError(f"{what}: ptr must hold B+1 offsets")
        return ptr, int(ptr.numel()) - 1, largest_cloud(ptr, known_max)
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


def pairs(pos_query, pos_ref, ptr_query, ptr_ref, batch_query, batch_ref, what, max_query_cloud=None):
    """The cloud pairs of two point sets -> (qptr, rptr, B, largest query cloud); differing cloud counts raise."""
    dev = pos_query.device
    qptr, bq, mq = cloud_offsets(pos_query.shape[0], ptr_query, batch_query, dev, what, max_query_cloud)
    rptr, br, _ = cloud_offsets(pos_ref.shape[0], ptr_ref, batch_ref, dev, what, 0)
    mq = mq if max_query_cloud is None else int(max_query_cloud)
    if bq != br:
        raise ValueError(f"{what}: {bq} query clouds but {br} reference clouds")
    return qptr, rptr, bq, mq


def search(fn, idx, d2=None):
    """The (idx, d2) pair of a search, or idx alone -> (Nq, k)."""
    for name, t, dt in (("idx", idx, torch.int32), ("d2", d2, torch.float32)):
        if t is None:
            continue
        device(fn, name, t)
        if t.dtype != dt or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous {dt} [Nq, k]")
    if (d2 is not None and idx.shape != d2.shape) or not 1 <= idx.shape[1] <= MAX_K:
        raise ValueError(f"{fn}: idx {tuple(idx.shape)}" + (f" and d2 {tuple(d2.shape)} must agree," if d2 is not None else ":") +
                         f" k in [1, {MAX_K}]")
    return int(idx.shape[0]), int(idx.shape[1])


def launches(b):
    """The pair ranges of the launches: at most 65 535 pairs each."""
    return [(lo, min(b, lo + MAX_PAIRS)) for lo in range(0, b, MAX_PAIRS)]


class Interpolate(torch.autograd.Function):
    """An interpolation on the autograd graph: the forward is the inference kernel (the same bits), the backward ONE launch on
    transposed lists built beforehand.  `fwd` / `bwd`: ``interpolate_rows`` / ``interpolate_rows_backward`` with `per` = 1 row
    per point and the weights (d2, tcoef), or ``interpolate_vectors`` / ``interpolate_vectors_backward`` with `per` = 2 and
    (tmat, tmat).  ``covered``: every row of x lies in a pair, so the backward writes all of dx itself."""

    @staticmethod
    def forward(ctx, x, fwd, bwd, per, qptr, rptr, idx, w_fwd, tptr, tedge, w_bwd, mq, mr, n_query, edge_base, covered):
        ctx.save_for_backward(rptr, tptr, tedge, w_bwd)
        ctx.meta = (bwd, int(per), tuple(x.shape), x.dtype, int(idx.shape[1]), int(mr), int(edge_base), bool(covered))
        return fwd(x.detach(), qptr, rptr, idx, w_fwd, mq, n_query=n_query)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rptr, tptr, tedge, w_bwd = ctx.saved_tensors
        bwd, per, shape, dtype, k, mr, edge_base, covered = ctx.meta
        out = torch.empty(shape, dtype=torch.float32, device=g.device) if covered else None
        dx = bwd(g, rptr, tptr, tedge, w_bwd, k, mr, n_ref=shape[0] // per, edge_base=edge_base, out=out)
        return (dx.to(dtype),) + (None,) * 15


class Pool(torch.autograd.Function):
    """The cross-cloud pooling on the autograd graph, the sibling of ``Interpolate``: the forward is the inference kernel (the same
    bits) and keeps what it recorded (``arg``: the slot every maximum / minimum came from, ``cnt``: the valid slots of every query),
    the backward ONE launch on transposed lists built beforehand.  `fwd` / `bwd`: ``pool_rows`` / ``pool_rows_backward``.
    ``covered``: every row of x lies in a pair, so the backward writes all of dx itself."""

    @staticmethod
    def forward(ctx, x, fwd, bwd, reduce, qptr, rptr, idx, tptr, tedge, mq, mr, n_query, covered):
        out, arg, cnt = fwd(x.detach(), qptr, rptr, idx, mq, reduce, n_query=n_query)
        ctx.save_for_backward(rptr, tptr, tedge, cnt, *(() if arg is None else (arg,)))
        ctx.meta = (bwd, reduce, tuple(x.shape), x.dtype, int(idx.shape[1]), int(mr), bool(covered))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rptr, tptr, tedge, cnt, *arg = ctx.saved_tensors
        bwd, reduce, shape, dtype, k, mr, covered = ctx.meta
        out = torch.empty(shape, dtype=torch.float32, device=g.device) if covered else None
        dx = bwd(g, rptr, tptr, tedge, arg[0] if arg else None, cnt, k, mr, reduce, n_ref=shape[0], out=out)
        return (dx.to(dtype),) + (None,) * 12


class PoolVectors(torch.autograd.Function):
    """``Pool`` for tangent-vector features (two rows per point): `fwd` / `bwd`: ``pool_vectors`` / ``pool_vectors_backward``,
    ``rmat`` the rotation table of the search, read by both."""

    @staticmethod
    def forward(ctx, v, fwd, bwd, reduce, qptr, rptr, idx, rmat, tptr, tedge, mq, mr, n_query, covered):
        out, arg, cnt = fwd(v.detach(), qptr, rptr, idx, rmat, mq, reduce, n_query=n_query)
        ctx.save_for_backward(rptr, tptr, tedge, rmat, cnt, *(() if arg is None else (arg,)))
        ctx.meta = (bwd, reduce, tuple(v.shape), v.dtype, int(idx.shape[1]), int(mr), bool(covered))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        rptr, tptr, tedge, rmat, cnt, *arg = ctx.saved_tensors
        bwd, reduce, shape, dtype, k, mr, covered = ctx.meta
        out = torch.empty(shape, dtype=torch.float32, device=g.device) if covered else None
        dv = bwd(g, rptr, tptr, tedge, rmat, arg[0] if arg else None, cnt, k, mr, reduce, n_ref=shape[0] // 2, out=out)
        return (dv.to(dtype),) + (None,) * 13
