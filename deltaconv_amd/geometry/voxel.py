"""Voxel-grid subsampling of clouds that live on the device (csrc/voxel.hip behind ``dc_voxel_subsample``): one representative
per occupied cell of edge ``size`` and, for every point, the output row of its cell -- ``torch_cluster.grid_cluster`` /
``torch_geometric.nn.voxel_grid`` followed by ``consecutive_cluster``.  Linear in the points, order-free, a function of the
geometry and ``size`` alone; the rules are csrc/voxel_math.h."""
import numpy as np

PICKS = {"centre": 0, "first": 1}
CELL_LIMIT = 1 << 20          # |cell index| per axis stays below it: three axes pack into 63 bits (csrc/voxel_math.h)


def _edges(fn, size):
    try:
        s = np.asarray(size, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: size must be a positive finite float or three of them, got {size!r}") from None
    if s.size not in (1, 3) or np.ndim(size) > 1:
        raise ValueError(f"{fn}: size must be a positive finite float or three of them, got {size!r}")
    with np.errstate(over="ignore"):
        s = np.broadcast_to(s.astype(np.float32), (3,))
    if not (np.isfinite(s).all() and (s > 0).all()):
        raise ValueError(f"{fn}: size must be positive and finite in float32, got {size!r}")
    return [float(v) for v in s]


def _origins(fn, origin, b, dev):
    import torch
    if origin is None:
        return None
    o = origin if torch.is_tensor(origin) else torch.as_tensor(np.asarray(origin, dtype=np.float32))
    if o.dim() not in (1, 2) or o.shape[-1] != 3 or (o.dim() == 2 and o.shape[0] != b):
        raise ValueError(f"{fn}: origin must be [3] or [{b},3], got {tuple(o.shape)}")
    if not o.is_cuda and not bool(torch.isfinite(o.float()).all()):
        raise ValueError(f"{fn}: origin must be finite")
    o = o.detach().to(device=dev, dtype=torch.float32)
    return (o[None, :].expand(b, 3) if o.dim() == 1 else o).contiguous()


def voxel_subsample(pos, size, ptr=None, batch=None, ptr_info=None, origin=None, pick="centre"):
    """One representative per occupied grid cell of every cloud of a batch on the device (``torch_cluster.grid_cluster`` /
    ``torch_geometric.nn.voxel_grid`` + ``consecutive_cluster``; csrc/voxel.hip behind ``dc_voxel_subsample``).

    pos: DEVICE float32 [N,3].  The clouds: ``ptr_info`` (a ``PtrInfo``), or ``ptr`` (B+1 row offsets), or a sorted ``batch``
    vector (one more read, for its offsets), or one cloud of N rows; empty clouds are allowed and give zero rows.  ``size``: the
    edge length of a cell, a positive finite float or three of them (per axis).  ``origin``: where the grid starts -- ``None``
    for every cloud's OWN fp32 minimum over its finite points (a cloud's result does not depend on its batch-mates), or ``[3]``
    for all clouds, or ``[B,3]``.  ``pick``: ``"centre"`` keeps of every cell the member nearest the cell centre (ties: the lower
    row), ``"first"`` the member with the lowest row.
    -> ``(rows int64 [N_out], optr int64 [B+1], cluster int64 [N])``: ``rows[optr[b]:optr[b+1]]`` are cloud b's representatives
    as rows of ``pos``, ASCENDING (a stable subset: file order survives); ``cluster[i]`` is the output row of point i's cell, so
    ``rows[cluster[i]]`` is i's representative and ``cluster`` indexes a pooled ``[N_out, C]`` tensor directly
    (``cluster_pool(x, cluster, len(rows), ...)`` pools onto it, ``cluster_unpool`` brings rows back).  A point with a
    non-finite coordinate, or outside every cloud of ``ptr``, belongs to no cell, is never picked and gets cluster -1.

    The rules (csrc/voxel_math.h; tests/voxel_restate.py restates them in numpy, bit for bit): per axis the cell is
    ``floorf(fl(fl(p - o) / s))``; the representative has the smallest key ``(bits(d2) << 32) | local row`` with ``d2`` the fp32
    ``(dx*dx + dy*dy) + dz*dz`` to the centre ``fl(fl(fl(t + 0.5) * s) + o)``.  The result is a function of the inputs only: the
    same bits on every run, whatever the batch.  A finite point whose cell index reaches 2^20 in magnitude on some axis raises
    ``ValueError`` naming the first such cloud (a larger ``size``, or an ``origin`` nearer the cloud, helps); so do host tensors,
    anything but float32 [N,3], a bad ``size`` / ``origin`` / ``pick`` / ``ptr``; a ``pos`` that requires grad raises (nothing
    here is differentiable).  NOT capturable by ``torch.cuda.graph``: the number of output rows depends on the data, and the
    call reads it from the device -- ONE read, the total and the status words together."""
    import torch
    from . import _cross
    from .._lib import lib
    from .graph import _ptr_from_batch
    fn = "voxel_subsample"
    if not torch.is_tensor(pos) or not pos.is_cuda:
        raise ValueError(f"{fn}: `pos` must be a tensor on a HIP device (there is no CPU path)")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
        raise ValueError(f"{fn}: `pos` must be float32 [N,3], got {pos.dtype} {tuple(pos.shape)}")
    _cross.no_grad_inputs(fn, pos=pos)
    if pick not in PICKS:
        raise ValueError(f"{fn}: pick must be 'centre' or 'first', got {pick!r}")
    sx, sy, sz = _edges(fn, size)
    if sum(a is not None for a in (ptr, batch, ptr_info)) > 1:
        raise ValueError(f"{fn}: give one of ptr, batch and ptr_info")
    n, dev = int(pos.shape[0]), pos.device
    if ptr_info is not None:
        ptr = ptr_info[0]
    elif ptr is None:
        if batch is not None and (not torch.is_tensor(batch) or batch.dim() != 1 or batch.shape[0] != n):
            raise ValueError(f"{fn}: `batch` must hold one cloud id per row")
        ptr = (_ptr_from_batch(batch.to(dev), n, dev)[0] if batch is not None and n else
               torch.tensor([0, n], dtype=torch.int64, device=dev))
    ptr = torch.as_tensor(ptr).to(device=dev, dtype=torch.int64).contiguous()
    if ptr.dim() != 1 or ptr.numel() < 1:
        raise ValueError(f"{fn}: `ptr` must hold B+1 offsets")
    b = int(ptr.numel()) - 1
    if ptr_info is not None and int(ptr_info[1]) != b:
        raise ValueError(f"{fn}: {int(ptr_info[1])} clouds need {int(ptr_info[1]) + 1} offsets, got {ptr.numel()}")
    origin = _origins(fn, origin, b, dev)
    need = int(lib.raw("dc_voxel_subsample_workspace_bytes")(n, b))
    if need == 0:
        raise ValueError(f"{fn}: {n} points in {b} clouds are more than one call takes")
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    rows = torch.empty(n, dtype=torch.int64, device=dev)
    cluster = torch.empty(n, dtype=torch.int64, device=dev)
    optr = torch.empty(b + 1, dtype=torch.int64, device=dev)
    info = torch.empty(4, dtype=torch.int64, device=dev)
    lib.call("dc_voxel_subsample", pos.detach().contiguous(), ptr, b, n, sx, sy, sz, origin, PICKS[pick], rows, optr, cluster, info,
             ws, need)
    # the one read: the total and the status words, with what is needed to judge the offsets (the kernels keep to the rows of
    # `pos` whatever the offsets hold)
    steps = ptr[1:] - ptr[:-1]
    least = steps.min() if b else ptr.new_zeros(())
    total, overflow, full, _, lo, hi, least = torch.cat([info, torch.stack([ptr[0], ptr[-1], least])]).tolist()
    if lo < 0 or hi > n or least < 0:
        raise ValueError(f"{fn}: `ptr` must ascend inside the {n} rows of `pos` (it runs from {lo} to {hi})")
    if overflow >= 0:
        raise ValueError(f"{fn}: cloud {overflow} has a point whose cell index reaches 2^20 = {CELL_LIMIT} on some axis with the edge "
                         f"length ({sx:g}, {sy:g}, {sz:g}); use a larger size or an origin nearer the cloud")
    if full:
        raise RuntimeError(f"{fn}: a cloud's slice of the cell table ran out (offsets that do not ascend?)")
    return rows[:total].clone(), optr, cluster
