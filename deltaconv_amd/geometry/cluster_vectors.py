"""Pooling of tangent-vector features over the cells of a cluster vector on the device (csrc/cluster_vectors.hip:
``dc_cluster_rotation``, ``dc_cluster_pool_vectors``, ``dc_cluster_pool_vectors_backward``, ``dc_cluster_unpool_vectors``,
``dc_cluster_unpool_vectors_backward``): the VECTOR stream's way across the boundary ``cluster_pool`` / ``cluster_unpool`` carry
scalar features over -- the linear-time sibling of ``knn_pool_vectors``.  Vector features ``[2N, C]`` are coefficients in every
point's own frame (rows 2i, 2i+1 = point i), so each member of a cell is first carried into the cell's frame by parallel transport
(reference: deltaconv/geometry/connection.py:6-47) and then reduced: per channel the transported vector of largest norm
(``"max"``), the sum or the mean.  On the way up the cell's vector is carried into every member's frame.  The reference has no such
call site.

Every point belongs to one cell, so the rotations are stored per POINT (``cluster_rotation``: 16 N bytes per direction), the way
down is a walk over the member lists of ``cluster_lists`` with a gather as its backward, the way up a gather with a walk as its
backward.  Every sum is ordered (the members of a cell in ascending row order) and atomics-free: the same bits on every run.  The
gradient w.r.t. the VALUES is opt-in (``differentiable=True``); frames, normals and ``cluster`` are never differentiated.  The
rules are csrc/cluster_vectors_math.h.  There is no CPU path."""
import torch
from torch.autograd.function import once_differentiable

from . import _cross
from .cluster import _count, _ids, _lists, cluster_lists, cluster_pool, cluster_unpool
from .pool_vectors import _mode

__all__ = ["cluster_rotation", "cluster_pool_vectors_rows", "cluster_pool_vectors_rows_backward", "cluster_unpool_vectors_rows",
           "cluster_unpool_vectors_rows_backward", "cluster_pool_vectors", "cluster_unpool_vectors", "ClusterPair"]

_DIRECTIONS = ("down", "up")


def _vectors(fn, name, t):
    """[2n, C] DEVICE rows -> (t, C, ld) as the kernels take them."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{fn}: `{name}` must be a tensor on a HIP device (there is no CPU path)")
    if not t.is_floating_point():
        raise TypeError(f"{fn}: `{name}` must be a floating-point tensor, got {t.dtype}")
    return _cross.values(fn, name, t if t.numel() else t.new_empty(t.shape), per_point=2)      # (no element: whatever strides it came with)


def _table(fn, rotation, n):
    if not torch.is_tensor(rotation) or not rotation.is_cuda:
        raise ValueError(f"{fn}: `rotation` must be a tensor on a HIP device (there is no CPU path)")
    if rotation.dtype != torch.float32 or tuple(rotation.shape) != (n, 4) or not rotation.is_contiguous():
        raise ValueError(f"{fn}: rotation must be contiguous float32 [{n}, 4] (cluster_rotation), got {rotation.dtype} "
                         f"{tuple(rotation.shape)}")
    if n and rotation.data_ptr() % 16:
        raise ValueError(f"{fn}: rotation must be 16-byte aligned (one 16-byte load per point)")
    return rotation


def _frames(fn, name, frames, rows, need_y):
    """(normal, x_basis[, y_basis]) over `rows` rows -> three contiguous fp32 tensors, the last None where it is absent."""
    if frames is None or not 2 <= len(frames) <= 3 or not all(torch.is_tensor(t) for t in frames) or (need_y and len(frames) < 3):
        raise ValueError(f"{fn}: {name} = (normal, x_basis, y_basis) over its {rows} rows" +
                         ("" if need_y else " (y_basis may be left out on the source side)"))
    _cross.no_grad_inputs(fn, **{f"{name}[{i}]": t for i, t in enumerate(frames)})
    out = [_cross.rows3(fn, f"{name}[{i}]", t, rows) for i, t in enumerate(frames)]
    return out + [None] * (3 - len(out))


def cluster_rotation(cluster, num_clusters, frames_fine, frames_coarse, direction="down", non_oriented=True):
    """The per-POINT table of parallel transports of a cluster vector (``dc_cluster_rotation``) -> fp32 ``[N, 4]``, row-major
    2 x 2.  ``direction="down"``: entry i is ``build_transport`` INTO the frame of cell ``cluster[i]`` FROM the frame of point i
    (what ``cluster_pool_vectors`` reduces through); ``"up"``: into the frame of point i from the frame of its cell (what
    ``cluster_unpool_vectors`` reads).  The up table is built, not taken as the transpose of the down table.  A point whose id lies
    outside ``[0, num_clusters)`` holds zeros; a member whose frame equals its cell's bit for bit holds the identity.

    ``cluster``: DEVICE int64 ``[N]``; ``frames_fine = (normal, x_basis, y_basis)`` over the N points, ``frames_coarse`` the same
    over the ``num_clusters`` cells (the y-axes of the SOURCE side are not read and may be left out).  Nothing here is
    differentiable: a frame that requires grad while grad mode is on raises ``RuntimeError``.  One launch, no synchronise."""
    from .._lib import lib
    fn = "cluster_rotation"
    if direction not in _DIRECTIONS:
        raise ValueError(f"{fn}: direction must be 'down' or 'up', got {direction!r}")
    cluster = _ids(fn, "cluster", cluster)
    n, m = _count(fn, "N", cluster.numel()), _count(fn, "num_clusters", num_clusters)
    down = direction == "down"
    fine = _frames(fn, "frames_fine", frames_fine, n, not down)
    coarse = _frames(fn, "frames_coarse", frames_coarse, m, down)
    with torch.no_grad():
        rmat = torch.empty((n, 4), dtype=torch.float32, device=cluster.device)     # every entry is written
        if n:
            if m == 0:                        # no cell: every entry is zero and no frame is read
                fine, coarse = [None] * 3, [None] * 3
            lib.call("dc_cluster_rotation", cluster, n, m, *fine, *coarse, int(down), int(bool(non_oriented)), rmat)
    return rmat


def cluster_pool_vectors_rows(v, cptr, members, rotation, reduce="max"):
    """The arithmetic half of ``cluster_pool_vectors`` on finished lists and a finished DOWN table (``dc_cluster_pool_vectors``):
    v ``[2N,C]`` DEVICE fp32 (rows may be strided) -> ``(out fp32 [2M,C], arg int32 [M,C] or None)``: rows ``2j, 2j+1`` of out are
    the `reduce` over the members ``members[cptr[j]:cptr[j+1]]`` in that order, each carried into the cell's frame by
    ``rotation[i]`` (csrc/cluster_vectors_math.h: ``"sum"`` from zero, ``"mean"`` the sum divided once by the count, ``"max"``
    per channel the transported vector of the member whose squared norm is largest -- the first member, a later one iff strictly
    larger); an empty cell gives zeros.  ``arg`` (max only): the row every channel came from, -1 for an empty cell.  Not
    recorded by autograd; ``cluster_pool_vectors_rows_backward`` is its gradient.  One launch, no synchronise."""
    from .._lib import lib
    fn = "cluster_pool_vectors_rows"
    mode = _mode(fn, reduce)
    v, c, ldv = _vectors(fn, "v", v)
    cptr, members, m, n = _lists(fn, cptr, members)
    if v.shape[0] != 2 * n:
        raise ValueError(f"{fn}: v holds {v.shape[0]} rows, the lists {n} points (two rows each)")
    _count(fn, "N", n)
    rotation = _table(fn, rotation, n)
    out = torch.empty((2 * m, c), dtype=torch.float32, device=v.device)         # every row is written
    lda = (c + 3) // 4 * 4                    # rows of arg a multiple of 16 bytes apart: one 128-bit store per channel group
    arg = torch.empty((m, lda), dtype=torch.int32, device=v.device)[:, :c] if mode == 0 else None
    lib.call("dc_cluster_pool_vectors", v, ldv, n, c, cptr, members, m, rotation, mode, out, c, arg, lda if arg is not None else 0)
    return out, arg


def _arg(fn, arg, m, c):
    _cross.device(fn, "arg", arg)
    if arg.dtype != torch.int32 or tuple(arg.shape) != (m, c) or (c > 1 and arg.stride(1) != 1) or (m > 1 and arg.stride(0) < c):
        raise ValueError(f"{fn}: arg must be int32 [{m}, {c}] with unit stride along the channels (cluster_pool_vectors_rows)")
    return int(arg.stride(0)) if m > 1 else c


def cluster_pool_vectors_rows_backward(g, cluster, cptr, rotation, arg, reduce="max", out=None):
    """The gradient of ``cluster_pool_vectors_rows`` w.r.t. v (``dc_cluster_pool_vectors_backward``): g ``[2M,C]`` DEVICE fp32
    (rows may be strided), ``cluster`` int64 ``[N]``, ``cptr`` what ``cluster_lists`` returned (read by the mean), ``rotation`` the
    forward's DOWN table, ``arg`` what the forward returned (may be None for sum / mean) -> fp32 ``[2N,C]``.  A gather, one term
    per point: ``R^T`` applied to the two rows of the point's cell -- always (sum), divided by the cell's count first (mean), or
    where ``arg`` names the point (max); a point without a cell gets zeros.  Every row is written.  One launch, no atomics."""
    from .._lib import lib
    fn = "cluster_pool_vectors_rows_backward"
    mode = _mode(fn, reduce)
    g, c, ldg = _vectors(fn, "g", g)
    cluster = _ids(fn, "cluster", cluster)
    m, n = int(g.shape[0]) // 2, _count(fn, "N", cluster.numel())
    cptr = _ids(fn, "cptr", cptr, m + 1)
    rotation = _table(fn, rotation, n)
    if arg is None and mode == 0:
        raise ValueError(f"{fn}: reduce = {reduce!r} needs the arg of the forward")
    lda = _arg(fn, arg, m, c) if arg is not None else 0
    out, ldo = _cross.out_rows(fn, torch.empty((2 * n, c), dtype=torch.float32, device=g.device) if out is None else out, 2 * n, c,
                               g.device, on_device=True)
    lib.call("dc_cluster_pool_vectors_backward", g, ldg, m, c, cluster, n, cptr, rotation, arg if mode == 0 else None, lda, mode, out,
             ldo)
    return out


def cluster_unpool_vectors_rows(x, cluster, rotation):
    """The arithmetic half of ``cluster_unpool_vectors`` on a finished UP table (``dc_cluster_unpool_vectors``): x ``[2M,C]``
    DEVICE fp32 (rows may be strided) -> fp32 ``[2N,C]``: rows ``2i, 2i+1`` are the vector of cell ``cluster[i]`` carried into
    the frame of point i by ``rotation[i]``; zeros for a point without a cell.  One launch."""
    from .._lib import lib
    fn = "cluster_unpool_vectors_rows"
    x, c, ldx = _vectors(fn, "x", x)
    cluster = _ids(fn, "cluster", cluster)
    n = _count(fn, "N", cluster.numel())
    rotation = _table(fn, rotation, n)
    out = torch.empty((2 * n, c), dtype=torch.float32, device=x.device)         # every row is written
    lib.call("dc_cluster_unpool_vectors", x, ldx, int(x.shape[0]) // 2, c, cluster, n, rotation, out, c)
    return out


def cluster_unpool_vectors_rows_backward(g, cptr, members, rotation):
    """The gradient of ``cluster_unpool_vectors_rows`` w.r.t. x (``dc_cluster_unpool_vectors_backward``): g ``[2N,C]`` DEVICE
    fp32, the lists of ``cluster_lists`` and the forward's UP table -> fp32 ``[2M,C]``: per cell the ordered sum over its members
    of ``R^T`` applied to the member's two rows of g -- the atomics-free ``index_add_``; an empty cell gets zeros.  One launch."""
    from .._lib import lib
    fn = "cluster_unpool_vectors_rows_backward"
    g, c, ldg = _vectors(fn, "g", g)
    cptr, members, m, n = _lists(fn, cptr, members)
    if g.shape[0] != 2 * n:
        raise ValueError(f"{fn}: g holds {g.shape[0]} rows, the lists {n} points (two rows each)")
    _count(fn, "N", n)
    rotation = _table(fn, rotation, n)
    out = torch.empty((2 * m, c), dtype=torch.float32, device=g.device)         # every row is written
    lib.call("dc_cluster_unpool_vectors_backward", g, ldg, n, c, cptr, members, m, rotation, out, c)
    return out


class _PoolVectors(torch.autograd.Function):
    """``cluster_pool_vectors`` on the autograd graph: the forward is the inference kernel (the same bits) and keeps ``arg``, the
    backward ONE launch of the gather."""

    @staticmethod
    def forward(ctx, v, cluster, cptr, members, rotation, reduce):
        out, arg = cluster_pool_vectors_rows(v.detach(), cptr, members, rotation, reduce)
        ctx.save_for_backward(cluster, cptr, rotation, *(() if arg is None else (arg,)))
        ctx.meta = (reduce, v.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cluster, cptr, rotation, *arg = ctx.saved_tensors
        reduce, dtype = ctx.meta
        dv = cluster_pool_vectors_rows_backward(g, cluster, cptr, rotation, arg[0] if arg else None, reduce)
        return dv.to(dtype), None, None, None, None, None


class _UnpoolVectors(torch.autograd.Function):
    """``cluster_unpool_vectors`` on the autograd graph: a gather forward, the ordered walk over the member lists backward."""

    @staticmethod
    def forward(ctx, x, cluster, cptr, members, rotation):
        ctx.save_for_backward(cptr, members, rotation)
        ctx.meta = x.dtype
        return cluster_unpool_vectors_rows(x.detach(), cluster, rotation)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        cptr, members, rotation = ctx.saved_tensors
        return cluster_unpool_vectors_rows_backward(g, cptr, members, rotation).to(ctx.meta), None, None, None, None


def _needs_grad(fn, v, differentiable):
    needs = torch.is_tensor(v) and v.requires_grad and torch.is_grad_enabled()
    if needs and not differentiable:
        raise RuntimeError(f"{fn}: v requires grad, but the device pooling is inference-only by default; call it under "
                           "torch.no_grad(), pass v.detach() or differentiable=True")
    return needs


def _values(fn, v):
    if not torch.is_tensor(v) or not v.is_cuda:
        raise ValueError(f"{fn}: `v` must be a tensor on a HIP device (there is no CPU path)")
    if v.dim() != 2 or v.shape[1] < 1 or v.shape[0] % 2:
        raise ValueError(f"{fn}: v must be [2n, C] with C >= 1 (rows 2i, 2i+1 = the two coefficients at point i), got {tuple(v.shape)}")
    if not v.is_floating_point():
        raise TypeError(f"{fn}: `v` must be a floating-point tensor, got {v.dtype}")


def _own_lists(fn, lists, n, m):
    cptr, members, lm, ln = _lists(fn, *lists)
    if ln != n or (m is not None and lm != m):
        raise ValueError(f"{fn}: `lists` of {ln} rows in {lm} cells do not belong to {n} rows in {m} cells")
    return cptr, members, lm


def cluster_pool_vectors(v, cluster, frames_fine=None, frames_coarse=None, num_clusters=None, reduce="max", lists=None, rotation=None,
                         differentiable=False, non_oriented=True):
    """``cluster_pool`` for tangent-vector features: ``v [2N,C]`` (rows 2i, 2i+1 = the coefficients at point i in ITS frame)
    pooled over the cells of ``cluster`` (int64 ``[N]``, values in ``[0, num_clusters)``; anything else belongs to no cell) ->
    fp32 ``[2*num_clusters, C]`` in the frames of the cells: every member carried into its cell's frame by parallel transport,
    then ``reduce`` = ``"max"`` (per channel the transported vector of largest norm; ties to the lower row) ``| "sum" | "add" |
    "mean"``.  ``frames_fine = (normal, x_basis[, y_basis])`` of the points, ``frames_coarse = (normal, x_basis, y_basis)`` of the
    cells -- with ``voxel_subsample``'s ``(rows, optr, cluster)``: ``num_clusters = len(rows)`` and ``frames_coarse =
    frames_fine[rows]`` (every representative's own entry is then the identity).

    ``lists``: the ``(cptr, members)`` of ``cluster_lists(cluster, num_clusters)``; ``rotation``: the table of
    ``cluster_rotation(..., direction="down")`` -- where they are at hand (``ClusterPair`` holds them); with ``rotation`` the
    frames are not looked at.  ``num_clusters=None`` takes it from ``lists``, else from ``frames_coarse``, else reads the device
    (``cluster.max() + 1``); given, nothing reads the device and lists + table + pool + backward can be captured.

    ``differentiable=False`` (the default) is INFERENCE ONLY: a ``v`` that requires grad while grad mode is on raises
    ``RuntimeError``.  ``differentiable=True`` puts the op on the autograd graph (the same forward bits); the backward is one
    gather launch.  The gradient is w.r.t. ``v`` ONLY: a frame that requires grad raises.  Non-HIP tensors raise."""
    fn = "cluster_pool_vectors"
    _mode(fn, reduce)
    needs_grad = _needs_grad(fn, v, differentiable)
    _values(fn, v)
    cluster = _ids(fn, "cluster", cluster, v.shape[0] // 2)
    n = cluster.numel()
    with torch.no_grad():
        if num_clusters is None and lists is None:
            if frames_coarse is not None and len(frames_coarse) and torch.is_tensor(frames_coarse[0]):
                num_clusters = int(frames_coarse[0].shape[0])
            else:                             # the one read
                num_clusters = max(int(cluster.max()) + 1, 0) if n else 0
        if lists is not None:
            cptr, members, m = _own_lists(fn, lists, n, None if num_clusters is None else int(num_clusters))
        else:
            m = _count(fn, "num_clusters", num_clusters)
            cptr, members = cluster_lists(cluster, m)
    if rotation is None:
        rotation = cluster_rotation(cluster, m, frames_fine, frames_coarse, "down", non_oriented)
    with torch.no_grad():
        if not needs_grad:
            return cluster_pool_vectors_rows(v.detach(), cptr, members, rotation, reduce)[0]
    return _PoolVectors.apply(v, cluster, cptr, members, _table(fn, rotation, n), reduce)


def cluster_unpool_vectors(v, cluster, frames_fine=None, frames_coarse=None, lists=None, rotation=None, differentiable=False,
                           non_oriented=True):
    """``cluster_unpool`` for tangent-vector features: the cells' vectors ``v [2M,C]`` (in the cells' frames) back on the points
    -> fp32 ``[2N,C]`` in the points' frames: rows ``2i, 2i+1`` are the vector of cell ``cluster[i]`` carried into the frame of
    point i by parallel transport; zeros for a point without a cell.  ``frames_fine = (normal, x_basis, y_basis)``,
    ``frames_coarse = (normal, x_basis[, y_basis])``; ``rotation``: the table of ``cluster_rotation(..., direction="up")`` where it
    is at hand (the frames are then not looked at).  ``differentiable=True``: the backward is the ordered sum over every cell's
    member list through the transposed rotations (``lists``: the ``(cptr, members)`` of ``cluster_lists(cluster, M)``, built here
    where not given).  Inference only by default, as ``cluster_pool_vectors``."""
    fn = "cluster_unpool_vectors"
    needs_grad = _needs_grad(fn, v, differentiable)
    _values(fn, v)
    cluster = _ids(fn, "cluster", cluster)
    n, m = cluster.numel(), int(v.shape[0]) // 2
    if rotation is None:
        rotation = cluster_rotation(cluster, m, frames_fine, frames_coarse, "up", non_oriented)
    if not needs_grad:
        with torch.no_grad():
            return cluster_unpool_vectors_rows(v.detach(), cluster, rotation)
    with torch.no_grad():
        if lists is not None:
            cptr, members, _ = _own_lists(fn, lists, n, m)
        else:
            cptr, members = cluster_lists(cluster, m)
    return _UnpoolVectors.apply(v, cluster, cptr, members, _table(fn, rotation, n))


class ClusterPair:
    """A cloud and its thinning by a cluster vector, both directions and both feature streams in one object: the linear-time
    sibling of ``CloudPair``, which searches.

    ``cluster``: DEVICE int64 ``[N]`` (``voxel_subsample``'s third result, or any vector with values in ``[0, num_clusters)``;
    anything else belongs to no cell); ``num_clusters`` = M, a host number.  ``frames_fine`` / ``frames_coarse``: ``(normal,
    x_basis, y_basis)`` over the N points / the M cells; without them the vector methods raise ``ValueError``.  With
    ``voxel_subsample``'s ``(rows, optr, cluster)`` and ``frames_coarse = frames_fine[rows]``, ``ClusterPair(cluster, len(rows),
    ...)`` is the pair of a thinned cloud; a store thinned with ``reduce="mean"`` builds its coarse frames from the pooled normals.

    Held, each built on first use and once: the member lists (``lists()``) and the two per-point rotation tables
    (``rotation("down" | "up")``).  ``prepare()`` builds all of them ahead of a ``torch.cuda.graph`` capture.

    Every method is on the autograd graph when ``differentiable`` is set and its input requires grad (grad mode on) -- the same
    forward bits, every backward one ordered, atomics-free launch; otherwise nothing is recorded and the inference bits are
    returned.  ``cluster`` and the frames are never differentiated: a frame that requires grad raises ``RuntimeError``."""

    def __init__(self, cluster, num_clusters, frames_fine=None, frames_coarse=None, differentiable=True, non_oriented=True):
        fn = "ClusterPair"
        self.cluster = _ids(fn, "cluster", cluster)
        self.n, self.m = _count(fn, "N", self.cluster.numel()), _count(fn, "num_clusters", num_clusters)
        self.frames = {"fine": None if frames_fine is None else _frames(fn, "frames_fine", frames_fine, self.n, True),
                       "coarse": None if frames_coarse is None else _frames(fn, "frames_coarse", frames_coarse, self.m, True)}
        self.differentiable, self.non_oriented = bool(differentiable), bool(non_oriented)
        self._built = {}

    def _once(self, key, build):
        if key not in self._built:
            with torch.no_grad():
                self._built[key] = build()
        return self._built[key]

    def lists(self):
        """-> ``(cptr, members)`` of ``cluster_lists``."""
        return self._once("lists", lambda: cluster_lists(self.cluster, self.m))

    def rotation(self, direction):
        """-> the ``cluster_rotation`` table of ``direction`` = ``"down" | "up"``; ``ValueError`` without frames."""
        if direction not in _DIRECTIONS:
            raise ValueError(f"ClusterPair.rotation: direction must be 'down' or 'up', got {direction!r}")
        if self.frames["fine"] is None or self.frames["coarse"] is None:
            raise ValueError(f"ClusterPair.{direction}_vectors: this pair was built without frames_fine= / frames_coarse= "
                             "(no rotation table)")
        return self._once(("rotation", direction), lambda: cluster_rotation(self.cluster, self.m, self.frames["fine"],
                                                                            self.frames["coarse"], direction, self.non_oriented))

    def prepare(self):
        """Builds every piece the four methods can need, so that nothing is left to build inside a capture."""
        self.lists()
        if self.frames["fine"] is not None and self.frames["coarse"] is not None:
            for direction in _DIRECTIONS:
                self.rotation(direction)
        return self

    def _recorded(self, t):
        return self.differentiable and torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled()

    @staticmethod
    def _input(t, recorded):
        return t if recorded or not torch.is_tensor(t) else t.detach()

    def down(self, x, reduce="max"):
        """Scalar features ``[N,C]`` pooled over the cells -> ``[M,C]`` (``cluster_pool``: ``"max" | "min" | "sum" | "add" |
        "mean"``)."""
        rec = self._recorded(x)
        return cluster_pool(self._input(x, rec), self.cluster, self.m, reduce, lists=self.lists(), differentiable=rec)

    def up(self, x):
        """Scalar features ``[M,C]`` back on the points -> ``[N,C]`` (``cluster_unpool``)."""
        rec = self._recorded(x)
        if torch.is_tensor(x) and x.dim() >= 1 and x.shape[0] != self.m:
            raise ValueError(f"ClusterPair.up: the input must hold one row per cell ([{self.m}, C]), got {tuple(x.shape)}")
        return cluster_unpool(self._input(x, rec), self.cluster, lists=self.lists() if rec else None, differentiable=rec)

    def down_vectors(self, v, reduce="max"):
        """Tangent-vector features ``[2N,C]`` in the points' frames -> ``[2M,C]`` in the cells' frames (``cluster_pool_vectors``:
        ``"max" | "sum" | "add" | "mean"``)."""
        _mode("ClusterPair.down_vectors", reduce)
        rotation = self.rotation("down")
        rec = self._recorded(v)
        return cluster_pool_vectors(self._input(v, rec), self.cluster, num_clusters=self.m, reduce=reduce, lists=self.lists(),
                                    rotation=rotation, differentiable=rec)

    def up_vectors(self, v):
        """Tangent-vector features ``[2M,C]`` in the cells' frames -> ``[2N,C]`` in the points' frames
        (``cluster_unpool_vectors``)."""
        rotation = self.rotation("up")
        rec = self._recorded(v)
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] != 2 * self.m:
            raise ValueError(f"ClusterPair.up_vectors: the input must hold two rows per cell ([{2 * self.m}, C]), got {tuple(v.shape)}")
        return cluster_unpool_vectors(self._input(v, rec), self.cluster, lists=self.lists() if rec else None, rotation=rotation,
                                      differentiable=rec)
