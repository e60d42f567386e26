"""Both directions between two resolutions of the same clouds in one object: ``CloudPair`` holds the searches, transposed lists and
transport tables of a fine and a coarse cloud set, each built once, and carries both feature streams across them --

    scalars   down: ``pool_rows`` (max / min / sum / mean over the k_down nearest fine points; csrc/pool.hip)
              up:   ``interpolate_rows`` (inverse-squared-distance mean of the k_up nearest coarse points; csrc/interp.hip)
    vectors   down / up: ``interpolate_vectors`` on the respective search and table (parallel transport into the target's frame,
              then the distance weights; csrc/interp_transport.hip)
              down, pooled: ``pool_vectors`` on the down search and its rotation table (parallel transport, then the vector of
              largest norm / the mean / the sum over the k_down nearest fine points; csrc/pool_vectors.hip)

-- what a multi-resolution DeltaConv network needs inside a training step (the reference points at it: "GeodesicFPS is used in the
multiscale architecture", train_shapenet.py:32).  Every backward is an ordered, atomics-free sum: bit-reproducible.  Nothing of the
geometry is differentiated.  There is no CPU path."""
import torch

from . import _cross
from .interpolate import interpolate_rows, interpolate_rows_backward, knn_cross, knn_cross_transpose
from .graph import PtrInfo
from .pool import _mode, pool_rows, pool_rows_backward
from .pool_vectors import knn_cross_rotation, pool_vectors, pool_vectors_backward
from .vector_interpolate import interpolate_vectors, interpolate_vectors_backward, knn_cross_transport

__all__ = ["CloudPair", "fps_levels", "prefix_levels"]


class CloudPair:
    """A fine and a coarse set of clouds, cloud b of one belonging to cloud b of the other.

    ``pos_fine [Nf,3]``, ``pos_coarse [Nc,3]``: DEVICE fp32; ``ptr_fine`` / ``ptr_coarse``: int64 ``[B+1]`` ABSOLUTE row offsets.
    The coarse cloud is the CALLER's -- for instance ``pos_fine[geodesic_fps_batch(...)]`` -- and need not be a subset of the fine
    one.  ``k_down``: the fine neighbours a coarse point pools over; ``k_up``: the coarse neighbours a fine point interpolates
    from.  ``frames_fine`` / ``frames_coarse``: ``(normal, x_basis, y_basis)`` over the rows of the respective cloud, as
    ``build_tangent_basis`` returns them behind the normal; without them the vector methods raise ``ValueError``.
    ``max_fine_cloud`` / ``max_coarse_cloud``: the largest cloud of each set where the host knows it; with both given nothing
    here synchronises (otherwise the constructor reads them from the offsets, once).  ``search_method``: the ``method`` of both
    searches (``knn_cross``: "brute" | "grid", None = the ``DC_KNN`` switch); it cannot change a bit of anything held here.

    Held, each built on first use and once: the down search (coarse queries into fine references, ``k_down``), the up search
    (fine queries into coarse references, ``k_up``), their transposed lists when ``differentiable`` is set, and the two transport
    tables when frames are given.  ``prepare()`` builds all of them ahead of a ``torch.cuda.graph`` capture; after it a forward +
    backward through any composition of the four methods can be captured.  The down ROTATION table, which only
    ``down_vectors(v, reduce="max" | "mean" | "sum")`` reads, is built on its first use, or by ``prepare(vector_pool=True)``.

    Every method is on the autograd graph when ``differentiable`` is set and its input requires grad (grad mode on) -- the same
    forward bits, the backward one launch over the transposed lists; otherwise nothing is recorded and the inference bits are
    returned.  Positions and frames are never differentiated: one that requires grad raises ``RuntimeError``."""

    def __init__(self, pos_fine, pos_coarse, ptr_fine, ptr_coarse, k_down=16, k_up=3, frames_fine=None, frames_coarse=None,
                 differentiable=True, max_fine_cloud=None, max_coarse_cloud=None, non_oriented=True, search_method=None):
        fn = "CloudPair"
        self.search_method = search_method
        self.k = {"down": int(k_down), "up": int(k_up)}
        for name, k in self.k.items():
            if not 1 <= k <= _cross.MAX_K:
                raise ValueError(f"{fn}: k_{name} = {k} outside [1, {_cross.MAX_K}]")
        self.frames = {"fine": self._frames(fn, "frames_fine", frames_fine), "coarse": self._frames(fn, "frames_coarse", frames_coarse)}
        _cross.no_grad_inputs(fn, pos_fine=pos_fine, pos_coarse=pos_coarse,
                              **{f"frames_{side}[{i}]": t for side, fr in self.frames.items() if fr for i, t in enumerate(fr)})
        self.pos = {"fine": _cross.rows3(fn, "pos_fine", pos_fine), "coarse": _cross.rows3(fn, "pos_coarse", pos_coarse)}
        fptr, cptr = _cross.offsets(fn, self.pos["fine"].device, ptr_fine=ptr_fine, ptr_coarse=ptr_coarse)
        self.ptr = {"fine": fptr, "coarse": cptr}
        self.largest = {"fine": _cross.largest_cloud(fptr, max_fine_cloud), "coarse": _cross.largest_cloud(cptr, max_coarse_cloud)}
        self.differentiable, self.non_oriented = bool(differentiable), bool(non_oriented)
        self._built = {}

    @staticmethod
    def _frames(fn, name, frames):
        if frames is None:
            return None
        frames = tuple(frames)
        if len(frames) != 3 or not all(torch.is_tensor(t) for t in frames):
            raise ValueError(f"{fn}: {name} = (normal, x_basis, y_basis)")
        return frames

    # ---- the lazily built pieces; a direction is named by its target: "down" queries coarse -> fine, "up" fine -> coarse ----------
    @staticmethod
    def _sides(direction):
        return ("coarse", "fine") if direction == "down" else ("fine", "coarse")        # (query, reference)

    def _once(self, key, build):
        if key not in self._built:
            with torch.no_grad():
                self._built[key] = build()
        return self._built[key]

    def search(self, direction):
        """-> ``(idx int32 [Nq,k], d2 fp32 [Nq,k])`` of the direction's ``knn_cross``."""
        q, r = self._sides(direction)
        return self._once(("search", direction), lambda: knn_cross(self.pos[q], self.pos[r], self.k[direction], ptr_query=self.ptr[q],
                                                                   ptr_ref=self.ptr[r], max_query_cloud=self.largest[q],
                                                                   method=self.search_method))

    def lists(self, direction):
        """-> ``(tptr, tedge, tcoef)`` of the direction's ``knn_cross_transpose``."""
        q, r = self._sides(direction)
        return self._once(("lists", direction), lambda: knn_cross_transpose(*self.search(direction), self.ptr[q], self.ptr[r],
                                                                            num_ref=self.pos[r].shape[0]))

    def table(self, direction):
        """-> the direction's ``knn_cross_transport`` table; ``ValueError`` without frames."""
        q, r = self._sides(direction)
        if self.frames[q] is None or self.frames[r] is None:
            raise ValueError(f"CloudPair.{direction}_vectors: this pair was built without frames_fine= / frames_coarse= "
                             "(no transport table)")
        return self._once(("table", direction), lambda: knn_cross_transport(*self.search(direction), self.ptr[q], self.ptr[r],
                                                                            self.frames[q], self.frames[r], self.non_oriented,
                                                                            max_query_cloud=self.largest[q]))

    def rotation(self, direction):
        """-> the direction's ``knn_cross_rotation`` table (the transport matrices alone, what ``down_vectors(v, reduce=...)``
        pools through); ``ValueError`` without frames."""
        q, r = self._sides(direction)
        if self.frames[q] is None or self.frames[r] is None:
            raise ValueError(f"CloudPair.{direction}_vectors: this pair was built without frames_fine= / frames_coarse= "
                             "(no rotation table)")
        return self._once(("rotation", direction), lambda: knn_cross_rotation(self.search(direction)[0], self.ptr[q], self.ptr[r],
                                                                              self.frames[q], self.frames[r], self.non_oriented,
                                                                              max_query_cloud=self.largest[q]))

    def prepare(self, vector_pool=False):
        """Builds every piece the four methods can need, so that nothing is left to build inside a capture.  ``vector_pool``:
        also the down rotation table, which only ``down_vectors(v, reduce="max" | "mean" | "sum")`` reads."""
        for direction in ("down", "up"):
            self.search(direction)
            if self.differentiable:
                self.lists(direction)
            if self.frames["fine"] is not None and self.frames["coarse"] is not None:
                self.table(direction)
        if vector_pool:
            self.rotation("down")
        return self

    # ---- the four methods -----------------------------------------------------------------------------------------------------
    def _recorded(self, t):
        return self.differentiable and torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled()

    def _rows(self, what, t, side, per=1):
        _cross.device(f"CloudPair.{what}", "the input", t)
        n = self.pos[side].shape[0]
        if t.dim() != 2 or t.shape[0] != per * n:
            raise ValueError(f"CloudPair.{what}: the input must hold {'two rows' if per == 2 else 'one row'} per {side} point "
                             f"([{per * n}, C]), got {tuple(t.shape)}")

    def down(self, x, reduce="max"):
        """Scalar features ``[Nf,C]`` pooled to the coarse clouds -> ``[Nc,C]``: ``reduce`` over the ``k_down`` nearest fine points
        (``"max" | "min" | "sum" | "add" | "mean"``, ``knn_pool``)."""
        _mode("CloudPair.down", reduce)
        self._rows("down", x, "fine")
        idx, _ = self.search("down")
        q, r = self.ptr["coarse"], self.ptr["fine"]
        mq, n = self.largest["coarse"], self.pos["coarse"].shape[0]
        if self._recorded(x):
            tptr, tedge, _ = self.lists("down")
            return _cross.Pool.apply(x, pool_rows, pool_rows_backward, reduce, q, r, idx, tptr, tedge, mq, self.largest["fine"], n, False)
        with torch.no_grad():
            return pool_rows(x.detach(), q, r, idx, mq, reduce, n_query=n)[0]

    def _interpolate(self, direction, per, fwd, bwd, t, w_fwd, w_bwd):
        qs, rs = self._sides(direction)
        idx, _ = self.search(direction)
        q, r = self.ptr[qs], self.ptr[rs]
        mq, n = self.largest[qs], self.pos[qs].shape[0]
        if self._recorded(t):
            tptr, tedge, tcoef = self.lists(direction)
            return _cross.Interpolate.apply(t, fwd, bwd, per, q, r, idx, w_fwd, tptr, tedge, tcoef if w_bwd is None else w_bwd, mq,
                                            self.largest[rs], n, 0, False)
        with torch.no_grad():
            return fwd(t.detach(), q, r, idx, w_fwd, mq, n_query=n)

    def up(self, x):
        """Scalar features ``[Nc,C]`` interpolated to the fine clouds -> ``[Nf,C]`` (``knn_interpolate`` over ``k_up``)."""
        self._rows("up", x, "coarse")
        return self._interpolate("up", 1, interpolate_rows, interpolate_rows_backward, x, self.search("up")[1], None)

    def down_vectors(self, v, reduce="interpolate"):
        """Tangent-vector features ``[2*Nf,C]`` in the fine frames -> ``[2*Nc,C]`` in the coarse frames, over the ``k_down``
        nearest fine points of every coarse point, each carried into the coarse point's frame by parallel transport.

        ``reduce="interpolate"`` (the default): the distance-weighted mean of ``knn_interpolate_vectors`` with the coarse cloud
        as the target.  On a coarse cloud that is a SUBSET of the fine one -- every cloud ``geodesic_fps_batch``,
        ``geodesic_subsample`` and ``T.GeodesicFPS`` produce -- it DEGENERATES: the coincident fine point has ``d^2 = 0``, weight
        ``1e16`` and coefficient exactly 1.0 in fp32, the other neighbours about 1e-13, so the result is the gather of the coarse
        points' own vectors and the other ``k_down - 1`` neighbours contribute nothing.  It is a correct interpolation.

        ``reduce="max" | "mean" | "sum" | "add"``: the pooling of ``knn_pool_vectors`` (csrc/pool_vectors.hip) -- per channel the
        transported vector of largest norm, or the unweighted mean / sum.  Its rotation table is built on first use and once
        (``rotation("down")``; ahead of a capture: ``prepare(vector_pool=True)``)."""
        if reduce == "interpolate":
            tmat = self.table("down")
            self._rows("down_vectors", v, "fine", 2)
            return self._interpolate("down", 2, interpolate_vectors, interpolate_vectors_backward, v, tmat, tmat)
        if reduce not in ("max", "mean", "sum", "add"):
            raise ValueError(f"CloudPair.down_vectors: reduce must be one of 'interpolate', 'max', 'mean', 'sum', 'add', got {reduce!r}")
        rmat = self.rotation("down")
        self._rows("down_vectors", v, "fine", 2)
        idx, _ = self.search("down")
        q, r = self.ptr["coarse"], self.ptr["fine"]
        mq, n = self.largest["coarse"], self.pos["coarse"].shape[0]
        if self._recorded(v):
            tptr, tedge, _ = self.lists("down")
            return _cross.PoolVectors.apply(v, pool_vectors, pool_vectors_backward, reduce, q, r, idx, rmat, tptr, tedge, mq,
                                            self.largest["fine"], n, False)
        with torch.no_grad():
            return pool_vectors(v.detach(), q, r, idx, rmat, mq, reduce, n_query=n)[0]

    def up_vectors(self, v):
        """Tangent-vector features ``[2*Nc,C]`` in the coarse frames -> ``[2*Nf,C]`` in the fine frames
        (``knn_interpolate_vectors`` over ``k_up``)."""
        tmat = self.table("up")
        self._rows("up_vectors", v, "coarse", 2)
        return self._interpolate("up", 2, interpolate_vectors, interpolate_vectors_backward, v, tmat, tmat)


def prefix_levels(ptr_info, ratios):
    """The levels of a multi-resolution network whose coarser clouds are PREFIXES of the finer ones: level ``l + 1`` keeps the
    first ``ceil(n_b / ratios[l])`` rows of every cloud b of level l.  -> a list of ``(rows, ptr, info)``, one per level, level 0
    first: ``rows`` int64 ``[N_l]`` on the device, the level's rows as row ids into LEVEL 0 (None at level 0: every row); ``ptr``
    int64 ``[B+1]`` the level's row offsets (what ``CloudPair`` takes); ``info`` a ``PtrInfo`` (int32 offsets, B, largest cloud)
    whose ``min_cloud`` is set -- largest and smallest cloud are derived on the host, ``ceil`` is monotone.

    The hierarchy is a farthest-point-sampling hierarchy EXACTLY WHEN the rows of every cloud are in FPS pick order: FPS is greedy,
    so the first m picks of an n-point sample are the m-point sample from the same start (tests/test_fps_prefix_host.py).
    ``geodesic_subsample`` (the dataset recipes) writes its rows in pick order, and so puts them there; on clouds in any other
    order the prefixes are still valid levels, but arbitrary subsets.

    ``ptr_info``: the ``PtrInfo`` of level 0 (``(ptr, B, largest cloud)`` with ``min_cloud``; a plain tuple or a missing
    ``min_cloud`` costs one read of the offsets).  A UNIFORM batch (largest == smallest cloud: what ``DeviceLoader`` feeds a
    captured step) synchronises nothing: level l has ``B * n_l`` rows.  A ragged batch reads its coarse total once per level."""
    from .graph import _min_cloud
    ptr0, b, mx = ptr_info[0], int(ptr_info[1]), int(ptr_info[2])
    mn = _min_cloud(ptr_info)
    ratios = [int(r) for r in ratios]
    if any(r < 1 for r in ratios):
        raise ValueError(f"prefix_levels: ratios must be integers >= 1, got {ratios}")
    dev = ptr0.device
    levels = [(None, ptr0.to(torch.int64), PtrInfo(ptr0.to(torch.int32), b, mx, mn))]
    uniform = mx == mn
    sizes = None if uniform else (ptr0[1:] - ptr0[:-1]).to(torch.int64)
    cloud = torch.arange(b, dtype=torch.int64, device=dev)
    for r in ratios:
        mx, mn = -(-mx // r), -(-mn // r)
        if uniform:
            ptr = torch.arange(b + 1, dtype=torch.int64, device=dev) * mx
            rows = (levels[0][1][:-1, None] + torch.arange(mx, dtype=torch.int64, device=dev)[None, :]).reshape(-1)
        else:
            sizes = (sizes + (r - 1)) // r
            ptr = torch.zeros(b + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(sizes, 0)
            total = int(ptr[-1])                       # the one host read of the level
            of = torch.repeat_interleave(cloud, sizes, output_size=total)
            rows = torch.arange(total, dtype=torch.int64, device=dev) - ptr[of] + levels[0][1][of]
        levels.append((rows, ptr, PtrInfo(ptr.to(torch.int32), b, mx, mn)))
    return levels


def fps_levels(pos, ptr_info, ratios, start=None, method=None, grid_target=None):
    """``prefix_levels`` for clouds whose rows are in ANY order: the same list of ``(rows, ptr, info)`` with identical ``ptr`` and
    ``info``, but level 1's ``rows`` are the picks of ONE Euclidean farthest-point sampling launch (``geometry.fps`` with
    ``ratios[0]``, from ``start`` or every cloud's row 0), in pick order, and the ``rows`` of every deeper level are the prefix of
    level 1's rows per cloud -- FPS is greedy, so those ARE the coarser samples from the same start.  On clouds already in that
    pick order the result equals ``prefix_levels``; with no ratios it is ``prefix_levels``.  ``pos``: DEVICE float32 [N,3], the
    rows of level 0.  A uniform batch synchronises nothing and can be captured.  ``method`` / ``grid_target``: the sampler, as in
    ``geometry.fps`` ("brute" | "grid", None = ``FPS_METHOD[0]``; the same rows either way, "grid" takes larger clouds)."""
    from .fps import fps_grid_launch, fps_launch, fps_method
    method = fps_method("fps_levels", method)
    if method != "grid" and grid_target is not None:
        raise ValueError("fps_levels: grid_target sizes the cells of method='grid'; it cannot be combined with method='brute'")
    levels = prefix_levels(ptr_info, ratios)
    if len(levels) == 1:
        return levels
    if not torch.is_tensor(pos) or not pos.is_cuda or pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
        raise ValueError("fps_levels: `pos` must be a device float32 [N,3] tensor")
    _cross.no_grad_inputs("fps_levels", pos=pos)
    if levels[0][2].min_cloud < 1:
        raise ValueError("fps_levels: empty cloud")
    prefix1, ptr1, info1 = levels[1]
    launch = fps_launch if method == "brute" else (lambda *a: fps_grid_launch(*a, grid_target=grid_target))
    picks = launch(pos.detach().contiguous(), levels[0][1].contiguous(), ptr1.contiguous(), int(ptr_info[1]), levels[0][2][2],
                   info1[2], int(prefix1.shape[0]), start)
    # level 1's row of every prefix row: pick r of cloud b stands where the prefix hierarchy has row r of cloud b
    slot = torch.empty(pos.shape[0], dtype=torch.int64, device=pos.device)
    slot[prefix1] = torch.arange(prefix1.shape[0], dtype=torch.int64, device=pos.device)
    return [levels[0], (picks, ptr1, info1)] + [(picks[slot[rows]], ptr, info) for rows, ptr, info in levels[2:]]
