"""Pooling of per-point data over the cells of a cluster vector on the device (csrc/cluster.hip: ``dc_cluster_lists``,
``dc_cluster_pool``, ``dc_cluster_pool_backward``, ``dc_cluster_gather``, ``dc_cluster_mean3``, ``dc_cluster_majority``): what
``torch_geometric``'s ``voxel_grid`` + ``max_pool`` / ``avg_pool_x`` / ``pool_pos`` keep of a thinned cloud, that is
``torch_scatter.scatter(x, cluster, reduce=...)`` -- the LINEAR-time way down between resolutions, next to ``knn_pool``.  The cluster
vector is int64 ``[N]``: values in ``[0, M)`` name the output row, anything else (``-1``: ``voxel_subsample``'s "no cell") belongs
to no cell; ``voxel_subsample``'s third result is one, any other is taken as well.

Every sum is ordered (the members of a cell in ascending row order), the gradient w.r.t. the FEATURES is opt-in
(``differentiable=True``) and atomics-free: the same bits on every run.  ``cluster`` and positions are never differentiated.  The
rules are csrc/cluster_math.h.  There is no CPU path."""
import torch
from torch.autograd.function import once_differentiable

from . import _cross
from .pool import _mode

__all__ = ["cluster_lists", "cluster_pool_rows", "cluster_pool_rows_backward", "cluster_pool", "cluster_unpool", "cluster_mean_pos",
           "cluster_majority"]

MAX_ROWS = 2 ** 31 - 1     # csrc/cluster_math.h: MAX_ROWS (arg holds rows of x as int32)
MAX_CLASSES = 1024         # csrc/cluster_math.h: MAX_CLASSES


def _ids(fn, name, t, n=None):
    """An int64 vector on the device ([n] where given) -> contiguous."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{fn}: `{name}` must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.int64 or t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise TypeError(f"{fn}: `{name}` must be int64 [{'N' if n is None else n}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous() if t.numel() else t.new_empty(t.shape)


def _count(fn, name, v):
    v = int(v)
    if not 0 <= v <= MAX_ROWS:
        raise ValueError(f"{fn}: {name} = {v} outside [0, 2^31)")
    return v


def _lists(fn, cptr, members):
    """-> (cptr, members, M, N) of a ``cluster_lists`` result."""
    cptr, members = _ids(fn, "cptr", cptr), _ids(fn, "members", members)
    if cptr.numel() < 1:
        raise ValueError(f"{fn}: `cptr` must hold M+1 offsets")
    return cptr, members, int(cptr.numel()) - 1, int(members.numel())


def _features(fn, name, t):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{fn}: `{name}` must be a tensor on a HIP device (there is no CPU path)")
    if not t.is_floating_point():
        raise TypeError(f"{fn}: `{name}` must be a floating-point tensor, got {t.dtype}")
    return _cross.values(fn, name, t if t.numel() else t.new_empty(t.shape))      # (no element: whatever strides it came with)


def cluster_lists(cluster, num_clusters):
    """The member lists of a cluster vector (``dc_cluster_lists``): cluster DEVICE int64 ``[N]``, ``num_clusters`` = M (a host
    number) -> ``(cptr int64 [M+1], members int64 [N])``: the rows of cell j are ``members[cptr[j]:cptr[j+1]]``, ASCENDING; the
    first ``cptr[M]`` entries of ``members`` are written, the rest are -1.  A row whose id lies outside ``[0, M)`` is in no list.
    Count, scan, unordered fill and a ranking pass with one thread per fill position: six launches sized by N and M, nothing
    synchronises, capturable; a function of the inputs only.  The ranking is quadratic in a list's length -- a single cell that
    holds every row of a call (up to 262 144) is slow, not a hang."""
    from .._lib import lib
    fn = "cluster_lists"
    cluster = _ids(fn, "cluster", cluster)
    n, m = _count(fn, "N", cluster.numel()), _count(fn, "num_clusters", num_clusters)
    need = int(lib.raw("dc_cluster_lists_workspace_bytes")(n, m))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=cluster.device)
    cptr = torch.empty(m + 1, dtype=torch.int64, device=cluster.device)
    members = torch.empty(n, dtype=torch.int64, device=cluster.device)
    lib.call("dc_cluster_lists", cluster, n, m, cptr, members, ws, need)
    return cptr, members


def cluster_pool_rows(x, cptr, members, reduce="max"):
    """The arithmetic half of ``cluster_pool`` on finished lists (``dc_cluster_pool``): x ``[N,C]`` DEVICE fp32 (rows may be
    strided) -> ``(out fp32 [M,C], arg int32 [M,C] or None)``: row j of out is the `reduce` over the rows ``members[cptr[j]:
    cptr[j+1]]`` of x in that order (csrc/cluster_math.h: the first member is copied, a later one taken iff strictly larger /
    smaller, or added in order; mean divides once by the count; an empty cell gives zeros).  ``arg`` (max / min only): the row of
    x every channel came from, -1 for an empty cell.  Not recorded by autograd; ``cluster_pool_rows_backward`` is its gradient.
    One launch, no synchronise."""
    from .._lib import lib
    fn = "cluster_pool_rows"
    mode = _mode(fn, reduce)
    x, c, ldx = _features(fn, "x", x)
    cptr, members, m, n = _lists(fn, cptr, members)
    if x.shape[0] != n:
        raise ValueError(f"{fn}: x holds {x.shape[0]} rows, the lists {n}")
    _count(fn, "N", n)
    out = torch.empty((m, c), dtype=torch.float32, device=x.device)             # every row is written
    lda = (c + 3) // 4 * 4                    # rows of arg a multiple of 16 bytes apart: one 128-bit store per channel group
    arg = torch.empty((m, lda), dtype=torch.int32, device=x.device)[:, :c] if mode <= 1 else None
    lib.call("dc_cluster_pool", x, ldx, n, c, cptr, members, m, mode, out, c, arg, lda if arg is not None else 0)
    return out, arg


def cluster_pool_rows_backward(g, cluster, cptr, arg, reduce="max", out=None):
    """The gradient of ``cluster_pool_rows`` w.r.t. x (``dc_cluster_pool_backward``): g ``[M,C]`` DEVICE fp32 (rows may be
    strided), ``cluster`` int64 ``[N]``, ``cptr`` what ``cluster_lists`` returned (read by the mean), ``arg`` what the forward
    returned (may be None for sum / mean) -> fp32 ``[N,C]``.  Every point belongs to one cell, so this is a gather: max / min
    ``g[cl]`` where ``arg[cl]`` names the point, sum ``g[cl]``, mean ``g[cl] / cnt[cl]``; a point without a cell gets zeros.
    Every row is written.  One launch, no atomics, no synchronise."""
    from .._lib import lib
    fn = "cluster_pool_rows_backward"
    mode = _mode(fn, reduce)
    g, c, ldg = _features(fn, "g", g)
    cluster = _ids(fn, "cluster", cluster)
    m, n = int(g.shape[0]), _count(fn, "N", cluster.numel())
    cptr = _ids(fn, "cptr", cptr, m + 1)
    if arg is None and mode <= 1:
        raise ValueError(f"{fn}: reduce = {reduce!r} needs the arg of the forward")
    lda = 0
    if arg is not None:
        _cross.device(fn, "arg", arg)
        if arg.dtype != torch.int32 or tuple(arg.shape) != (m, c) or (c > 1 and arg.stride(1) != 1) or (m > 1 and arg.stride(0) < c):
            raise ValueError(f"{fn}: arg must be int32 [{m}, {c}] with unit stride along the channels (cluster_pool_rows)")
        lda = int(arg.stride(0)) if m > 1 else c
    out, ldo = _cross.out_rows(fn, torch.empty((n, c), dtype=torch.float32, device=g.device) if out is None else out, n, c,
                               g.device, on_device=True)
    lib.call("dc_cluster_pool_backward", g, ldg, m, c, cluster, n, cptr, arg if mode <= 1 else None, lda, mode, out, ldo)
    return out


def _gather_rows(fn, x, cluster):
    from .._lib import lib
    x, c, ldx = _features(fn, "x", x)
    n = _count(fn, "N", cluster.numel())
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    lib.call("dc_cluster_gather", x, ldx, int(x.shape[0]), c, cluster, n, out, c)
    return out


class _Pool(torch.autograd.Function):
    """``cluster_pool`` on the autograd graph: the forward is the inference kernel (the same bits) and keeps ``arg``, the backward
    ONE launch of the gather."""

    @staticmethod
    def forward(ctx, x, cluster, cptr, members, reduce):
        out, arg = cluster_pool_rows(x.detach(), cptr, members, reduce)
        ctx.save_for_backward(cluster, cptr, *(() if arg is None else (arg,)))
        ctx.meta = (reduce, x.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cluster, cptr, *arg = ctx.saved_tensors
        reduce, dtype = ctx.meta
        dx = cluster_pool_rows_backward(g, cluster, cptr, arg[0] if arg else None, reduce)
        return dx.to(dtype), None, None, None, None


class _Unpool(torch.autograd.Function):
    """``cluster_unpool`` on the autograd graph: a gather forward, the ordered sum over the member lists backward."""

    @staticmethod
    def forward(ctx, x, cluster, cptr, members):
        ctx.save_for_backward(cptr, members)
        ctx.meta = x.dtype
        return _gather_rows("cluster_unpool", x.detach(), cluster)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cptr, members = ctx.saved_tensors
        return cluster_pool_rows(g, cptr, members, "sum")[0].to(ctx.meta), None, None, None


def _needs_grad(fn, x, differentiable):
    needs = torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled()
    if needs and not differentiable:
        raise RuntimeError(f"{fn}: x requires grad, but the device pooling is inference-only by default; call it under "
                           "torch.no_grad(), pass x.detach() or differentiable=True")
    return needs


def cluster_pool(x, cluster, num_clusters=None, reduce="max", lists=None, differentiable=False):
    """The features ``x [N,C]`` pooled over the cells of ``cluster`` (int64 ``[N]``, values in ``[0, num_clusters)``; anything
    else belongs to no cell) by ``reduce`` = ``"max" | "min" | "sum" | "add" | "mean"`` -> fp32 ``[num_clusters, C]``;
    ``torch_scatter.scatter(x, cluster, dim=0, reduce=...)`` / ``torch_geometric.nn.max_pool`` / ``avg_pool_x`` with ordered sums:
    the members of a cell in ascending row order, ties of a maximum to the lower row, an empty cell zeros.  With the third result
    of ``voxel_subsample`` and ``num_clusters = len(rows)`` the result lines up with the thinned cloud.

    ``lists``: the ``(cptr, members)`` of ``cluster_lists(cluster, num_clusters)`` where they are at hand (they are built once per
    thinning and serve every pooling over it).  ``num_clusters=None`` reads it from the device (``cluster.max() + 1``, or from
    ``lists``); given, nothing reads the device and lists + pool + backward can be captured in a ``torch.cuda.graph``.

    ``differentiable=False`` (the default) is INFERENCE ONLY: an ``x`` that requires grad while grad mode is on raises
    ``RuntimeError``.  ``differentiable=True`` puts the op on the autograd graph (the same forward bits); the backward is one
    gather launch -- a maximum sends its gradient to the lowest of the rows that share it.  Once differentiable; NO gradient for
    ``cluster``.  Non-HIP tensors raise: there is no CPU path."""
    fn = "cluster_pool"
    _mode(fn, reduce)
    needs_grad = _needs_grad(fn, x, differentiable)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError(f"{fn}: `x` must be a tensor on a HIP device (there is no CPU path)")
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"{fn}: x must be [N, C] with C >= 1, got {tuple(x.shape)}")
    if not x.is_floating_point():
        raise TypeError(f"{fn}: `x` must be a floating-point tensor, got {x.dtype}")
    cluster = _ids(fn, "cluster", cluster, x.shape[0])
    with torch.no_grad():
        if lists is not None:
            cptr, members, m, n = _lists(fn, *lists)
            if n != cluster.numel() or (num_clusters is not None and int(num_clusters) != m):
                raise ValueError(f"{fn}: `lists` of {n} rows in {m} cells do not belong to {cluster.numel()} rows in {num_clusters} cells")
        else:
            if num_clusters is None:           # the one read
                num_clusters = max(int(cluster.max()) + 1, 0) if cluster.numel() else 0
            cptr, members = cluster_lists(cluster, num_clusters)
        if not needs_grad:
            return cluster_pool_rows(x.detach(), cptr, members, reduce)[0]
    return _Pool.apply(x, cluster, cptr, members, reduce)


def cluster_unpool(x, cluster, lists=None, differentiable=False):
    """The pooled rows ``x [M,C]`` back on the points: ``out[i] = x[cluster[i]]``, zeros for a point without a cell -> fp32
    ``[N,C]`` (``dc_cluster_gather``).  ``differentiable=True``: the backward is the ordered sum of ``g`` over every cell's member
    list (``dc_cluster_pool`` in sum mode; ``lists``: the ``(cptr, members)`` of ``cluster_lists(cluster, M)``, built here where
    not given) -- the atomics-free ``index_add_``.  Inference only by default, as ``cluster_pool``."""
    fn = "cluster_unpool"
    needs_grad = _needs_grad(fn, x, differentiable)
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ValueError(f"{fn}: `x` must be a tensor on a HIP device (there is no CPU path)")
    if x.dim() == 1:
        x = x[:, None]
    cluster = _ids(fn, "cluster", cluster)
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"{fn}: x must be [M, C] with C >= 1, got {tuple(x.shape)}")
    if not needs_grad:
        return _gather_rows(fn, x.detach(), cluster)
    with torch.no_grad():
        if lists is not None:
            cptr, members, m, n = _lists(fn, *lists)
            if n != cluster.numel() or m != x.shape[0]:
                raise ValueError(f"{fn}: `lists` of {n} rows in {m} cells do not belong to {cluster.numel()} rows in {x.shape[0]} cells")
        else:
            cptr, members = cluster_lists(cluster, int(x.shape[0]))
    return _Unpool.apply(x, cluster, cptr, members)


def cluster_mean_pos(p, cptr, members, normalize=False):
    """The barycentre of every cell (``torch_geometric``'s ``pool_pos``; ``dc_cluster_mean3``): p DEVICE fp32 ``[N,3]`` -> fp32
    ``[M,3]``.  Per cell an fp64 sum in member order, one fp64 division by the count, one rounding to fp32 -- an fp32 chain loses
    the low bits of a cloud far from the origin.  ``normalize=True`` (normals): the fp64 sum divided by its fp64 norm; zeros where
    that norm is zero or not finite.  An empty cell gives zeros.  Never differentiated: a ``p`` that requires grad raises."""
    from .._lib import lib
    fn = "cluster_mean_pos"
    if not torch.is_tensor(p) or not p.is_cuda:
        raise ValueError(f"{fn}: `p` must be a tensor on a HIP device (there is no CPU path)")
    if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32:
        raise TypeError(f"{fn}: `p` must be float32 [N,3], got {p.dtype} {tuple(p.shape)}")
    _cross.no_grad_inputs(fn, p=p)
    cptr, members, m, n = _lists(fn, cptr, members)
    if p.shape[0] != n:
        raise ValueError(f"{fn}: p holds {p.shape[0]} rows, the lists {n}")
    _count(fn, "N", n)
    out = torch.empty((m, 3), dtype=torch.float32, device=p.device)
    p = p.detach().contiguous() if n else p.new_empty((0, 3))
    lib.call("dc_cluster_mean3", p, n, cptr, members, m, 1 if normalize else 0, out)
    return out


def cluster_majority(labels, cptr, members, num_classes):
    """The most frequent label of every cell (``dc_cluster_majority``): labels DEVICE int64 ``[N]``, ``num_classes`` in
    ``[1, 1024]`` -> int64 ``[M]``.  Ties go to the lowest label; labels outside ``[0, num_classes)`` are ignored; a cell without
    a valid label gets -1.  Integer counting only."""
    from .._lib import lib
    fn = "cluster_majority"
    labels = _ids(fn, "labels", labels)
    cptr, members, m, n = _lists(fn, cptr, members)
    if labels.shape[0] != n:
        raise ValueError(f"{fn}: labels holds {labels.shape[0]} rows, the lists {n}")
    num_classes = int(num_classes)
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f"{fn}: num_classes = {num_classes} outside [1, {MAX_CLASSES}]")
    _count(fn, "N", n)
    out = torch.empty(m, dtype=torch.int64, device=labels.device)
    lib.call("dc_cluster_majority", labels, n, cptr, members, m, num_classes, out)
    return out
