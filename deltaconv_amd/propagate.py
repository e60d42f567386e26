"""Propagation of per-point values from a sampled, device-resident dataset back to the points or vertices it was sampled from
(csrc/interp.hip: ``dc_knn_cross`` once per dataset, ``dc_knn_interpolate`` per use; with ``differentiable=True`` also
``dc_knn_cross_transpose`` once and ``dc_knn_interpolate_backward`` per backward) -- PointNet++-style feature propagation,
``torch_geometric.nn.knn_interpolate`` for a whole store.

What it closes: every stage of the device pipeline (``DeviceMeshDataset.sample_points``, ``DeviceDataset.geodesic_subsample``)
reduces resolution, and ``DeviceEvaluator`` scored the sampled points only; the part-segmentation benchmarks are defined on all
points of a shape, or on a mesh's vertices.

    full = DeviceDataset.from_dataset(test_set, device)                 # every point of every shape, with its labels
    test = full.geodesic_subsample(2048, seed=1)                         # what the network sees
    result = DeviceEvaluator(model, DeviceLoader(test, 16), num_votes=10, propagate_to=full).run()
    result["mean_iou"], result["sampled"]["mean_iou"]                   # at full resolution / at the sampled points

    prop = Propagator(test, meshes, k=3)                                 # target: a DeviceMeshDataset (its vertices)
    vertex_logits = prop.apply(logits, (0, len(test)))

    prop = Propagator(train, full, k=3, differentiable=True)            # a loss on ALL points of a shape trains the network
    loss = F.cross_entropy(prop.apply(logits, (c0, c1)), full.y_point[t0:t1])

    prop = Propagator(test, full, k=3, frames="normals")                 # the vector stream: tangent-vector features [2N, C]
    full_vectors = prop.apply_vectors(vectors)                           # carried into every target point's own frame

Inference only by default; ``differentiable=True`` adds the gradient w.r.t. the propagated VALUES (an ordered, atomics-free sum:
bit-reproducible).  Positions are never differentiated.  There is no CPU path.

``frames=`` adds the vector stream (csrc/interp_transport.hip: ``dc_knn_cross_transport`` once per dataset,
``dc_knn_interpolate_vectors`` per use, ``dc_knn_interpolate_vectors_backward`` per backward): tangent-vector features are carried
into the target point's frame by parallel transport before they are weighted (``geometry.vector_interpolate``).
"""
import numpy as np
import torch

from .geometry._cross import Interpolate
from .geometry.interpolate import MAX_K, interpolate_rows, interpolate_rows_backward, knn_cross, knn_cross_transpose
from .geometry.vector_interpolate import interpolate_vectors, interpolate_vectors_backward, knn_cross_transport

__all__ = ["Propagator", "target_view"]


def target_view(target):
    """-> (pos [rows,3], ptr int64 [S+1] on the device, sizes on the host, per-row labels or None) of a ``DeviceDataset`` (its
    points) or a ``DeviceMeshDataset`` (its vertices)."""
    if hasattr(target, "vert") and hasattr(target, "vptr"):
        return target.vert, target.vptr, np.asarray(target.n_verts, dtype=np.int64), target.y_vert
    if hasattr(target, "pos") and hasattr(target, "ptr") and hasattr(target, "sizes"):
        return target.pos, target.ptr, np.asarray(target.sizes, dtype=np.int64), target.y_point
    raise TypeError(f"Propagator: the target must be a DeviceDataset or a DeviceMeshDataset, got {type(target).__name__}")


def _host_offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    return off


class Propagator:
    """The k nearest SOURCE points of every TARGET row, found once for the whole set, and the interpolation from them.

    `source`: a ``DeviceDataset`` (the sampled clouds the network runs on).  `target`: a ``DeviceDataset`` (its ``pos``) or a
    ``DeviceMeshDataset`` (its ``vert``) with the same number of clouds in the same order.  The constructor runs
    ``dc_knn_cross`` over the set in groups of ``clouds_per_launch`` clouds, in STORE coordinates -- the loader's per-cloud
    augmentations do not enter -- and keeps ``idx`` (int32, local to the source cloud, -1 = no such neighbour) and ``d2`` (fp32):
    8 k bytes per target row.  No synchronise: the sizes are the stores' host arrays.

    ``apply(values, clouds)`` interpolates source-resolution rows to target rows (``w = 1 / max(d^2, 1e-16)``, PyG's
    ``knn_interpolate``); ``labels(pred)`` is the k = 1 label transfer, a gather.

    ``differentiable=False`` (the default) is inference only: no autograd, no backward.  With ``True`` the constructor also builds
    the store-wide transposed lists once (``knn_cross_transpose``: per valid slot an int64 edge id and an fp32 coefficient, i.e.
    at most 12 k further bytes per target row, plus 8 bytes per source row of list offsets), and ``apply`` joins the autograd
    graph when ``values`` requires grad and grad mode is on: the backward is one launch of an ordered sum over those lists, no
    atomics, the same bits on every run.  There is no gradient for positions.

    ``frames`` (keyword only; default ``None``: nothing further is allocated or launched, and ``apply_vectors`` raises) adds the
    vector stream.  Either a pair ``(source_frames, target_frames)`` over the stores' rows -- ``source_frames = (normal,
    x_basis[, y_basis])``, ``target_frames = (normal, x_basis, y_basis)`` -- or ``"normals"``: both derived from the stores'
    normals through ``build_tangent_basis`` (``source.norm``; ``target.norm`` of a ``DeviceDataset``, ``target.vertex_normals()``
    of a mesh store; ``ValueError`` where a store has none).  The constructor then builds the store-wide table of per-slot
    matrices once (``knn_cross_transport``: 16 k bytes per target row), and ``apply_vectors(values, clouds)`` interpolates
    ``[2 x source rows, C]`` tangent-vector features to ``[2 x target rows, C]``, every neighbour's vector carried into the
    target's frame first.  The table is built from STORE frames: it matches a network that was fed the store's un-augmented
    normals.  A rotated or jittered batch has other frames and needs the tensor-level call
    (``geometry.knn_interpolate_vectors``) with the batch's own.  Frames are never differentiated."""

    def __init__(self, source, target, k=3, clouds_per_launch=4096, differentiable=False, *, frames=None):
        k, per = int(k), int(clouds_per_launch)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"Propagator: k = {k} outside [1, {MAX_K}]")
        if not 1 <= per <= 65535:
            raise ValueError("Propagator: 1 <= clouds_per_launch <= 65535")
        if not (hasattr(source, "pos") and hasattr(source, "ptr") and hasattr(source, "sizes")):
            raise TypeError(f"Propagator: the source must be a DeviceDataset, got {type(source).__name__}")
        tpos, tptr, tsizes, _ = target_view(target)
        if len(tsizes) != len(source):
            raise ValueError(f"Propagator: {len(source)} source clouds but {len(tsizes)} target clouds (same clouds, same order)")
        if tpos.device != source.pos.device:
            raise ValueError("Propagator: source and target live on different devices")
        self.source, self.target, self.k = source, target, k
        self.device = tpos.device
        self.tptr, self.sptr = tptr, source.ptr
        self.tsizes, self.ssizes = tsizes, np.asarray(source.sizes, dtype=np.int64)
        self.toff, self.soff = _host_offsets(self.tsizes), _host_offsets(self.ssizes)     # host copies of the offsets
        rows, s = int(self.toff[-1]), len(source)
        # every target row lies in exactly one cloud of the store, so the search writes every entry: no fill pass
        self.idx = torch.empty((rows, k), dtype=torch.int32, device=self.device)
        self.d2 = torch.empty((rows, k), dtype=torch.float32, device=self.device)
        with torch.no_grad():
            for lo in range(0, s, per):
                hi = min(s, lo + per)
                mq = int(self.tsizes[lo:hi].max())
                if mq:
                    knn_cross(tpos, source.pos, k, ptr_query=tptr[lo:hi + 1], ptr_ref=self.sptr[lo:hi + 1], max_query_cloud=mq,
                              out=(self.idx, self.d2))
            self.differentiable = bool(differentiable)
            self.lists = knn_cross_transpose(self.idx, self.d2, tptr, self.sptr, num_ref=int(self.soff[-1])) \
                if self.differentiable else None
        # (outside no_grad: a frame that requires grad raises, as everywhere in geometry.connection)
        self.tmat = None if frames is None else self._build_table(frames)
        self._ranges = {}

    def _build_table(self, frames):
        """The store-wide table of ``c * R`` per slot (``knn_cross_transport``)."""
        from .geometry import build_tangent_basis
        if isinstance(frames, str):
            if frames != "normals":
                raise ValueError(f"Propagator: frames must be (source_frames, target_frames) or 'normals', got {frames!r}")
            tnorm = self.target.vertex_normals() if hasattr(self.target, "vertex_normals") else getattr(self.target, "norm", None)
            snorm = getattr(self.source, "norm", None)
            if snorm is None or tnorm is None:
                raise ValueError("Propagator: frames='normals' needs normals on both stores; the "
                                 f"{'source' if snorm is None else 'target'} has none")
            sframes, tframes = (snorm,) + tuple(build_tangent_basis(snorm)), (tnorm,) + tuple(build_tangent_basis(tnorm))
        else:
            try:
                sframes, tframes = frames
                sframes, tframes = tuple(sframes), tuple(tframes)
            except (TypeError, ValueError):
                raise ValueError("Propagator: frames must be (source_frames, target_frames) or 'normals'") from None
        rows, srows = int(self.toff[-1]), int(self.soff[-1])
        if len(tframes) != 3 or len(sframes) not in (2, 3):
            raise ValueError("Propagator: source_frames = (normal, x_basis[, y_basis]), target_frames = (normal, x_basis, y_basis)")
        for name, fr, n in (("source", sframes[:2], srows), ("target", tframes, rows)):
            for t in fr:
                if not torch.is_tensor(t) or tuple(t.shape) != (n, 3):
                    got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                    raise ValueError(f"Propagator: every {name} frame tensor must be [{n}, 3] (the store's rows), got {got}")
        # one call for the store (a launch per 65 535 clouds): the grid is sized by the largest target cloud, workgroups past a
        # cloud's end return at once
        mq = int(self.tsizes.max()) if len(self) else 0
        return knn_cross_transport(self.idx, self.d2, self.tptr, self.sptr, tframes, sframes, max_query_cloud=mq)

    def __len__(self):
        return len(self.tsizes)

    def cloud_range(self, clouds):
        """The offsets of the contiguous cloud range ``(c0, c1)`` RELATIVE to its first row, built on the device from the stores'
        offsets and kept: ``(target ptr int64, source ptr int64, target ptr int32, target rows (t0, t1), source rows (s0, s1))``."""
        c0, c1 = int(clouds[0]), int(clouds[1])
        if not 0 <= c0 <= c1 <= len(self):
            raise ValueError(f"Propagator: clouds ({c0}, {c1}) outside [0, {len(self)}]")
        r = self._ranges.get((c0, c1))
        if r is None:
            q = (self.tptr[c0:c1 + 1] - self.tptr[c0:c0 + 1]).contiguous()
            s = (self.sptr[c0:c1 + 1] - self.sptr[c0:c0 + 1]).contiguous()
            r = self._ranges[(c0, c1)] = (q, s, q.to(torch.int32), (int(self.toff[c0]), int(self.toff[c1])),
                                          (int(self.soff[c0]), int(self.soff[c1])))
        return r

    def _apply(self, what, per, rows_text, fwd, bwd, weights, values, clouds, out):
        """The body of ``apply`` (per = 1 row per point) and ``apply_vectors`` (per = 2): ``weights(t0, t1)`` gives what `fwd` and
        `bwd` weight the target rows [t0, t1) of the store with."""
        clouds = (0, len(self)) if clouds is None else clouds
        c0, c1 = int(clouds[0]), int(clouds[1])
        q, s, _, (t0, t1), (s0, s1) = self.cloud_range((c0, c1))
        if values.dim() != 2 or values.shape[0] != per * (s1 - s0):
            raise ValueError(f"Propagator.{what}: values must hold {rows_text} {s1 - s0} source rows of clouds {(c0, c1)}, got "
                             f"{tuple(values.shape)}")
        mq = int(self.tsizes[c0:c1].max()) if c1 > c0 else 0
        w_fwd, w_bwd = weights(t0, t1)
        if self.differentiable and values.requires_grad and torch.is_grad_enabled():
            if out is not None:
                raise ValueError(f"Propagator.{what}: out= cannot receive a result that is recorded by autograd")
            mr = int(self.ssizes[c0:c1].max()) if c1 > c0 else 0
            tptr, tedge, _ = self.lists
            # the store-wide lists name target rows of the STORE: the range's first row is subtracted (edge_base; edge e of the
            # store is entry e - t0 * k of a slice of the table); every source row of the range lies in one of its clouds, so the
            # backward writes the whole gradient
            return Interpolate.apply(values, fwd, bwd, per, q, s, self.idx[t0:t1], w_fwd, tptr[s0:s1 + 1], tedge, w_bwd, mq, mr,
                                     t1 - t0, t0, True)
        with torch.no_grad():
            return fwd(values, q, s, self.idx[t0:t1], w_fwd, mq, n_query=t1 - t0, out=out)

    def apply(self, values, clouds=None, out=None):
        """values: DEVICE fp32 ``[source rows of the clouds, C]`` (rows may be strided), the clouds ``(c0, c1)`` a contiguous range
        of the set (default: all) -> fp32 ``[target rows of those clouds, C]``.  One launch; no synchronise.  On a
        ``differentiable`` propagator a ``values`` that requires grad (grad mode on) gives a result on the autograd graph -- the
        same forward bits; ``out`` cannot be combined with that.  Otherwise nothing is recorded."""
        return self._apply("apply", 1, "the", interpolate_rows, interpolate_rows_backward,
                           lambda t0, t1: (self.d2[t0:t1], self.lists[2] if self.lists else None), values, clouds, out)

    def apply_vectors(self, values, clouds=None, out=None):
        """Tangent-vector features: values DEVICE fp32 ``[2 x source rows of the clouds, C]`` (rows 2i, 2i+1 = the coefficients at
        source point i in ITS frame; rows may be strided) -> fp32 ``[2 x target rows of those clouds, C]`` in the targets' frames.
        Needs ``frames=`` at construction.  One launch; no synchronise.  On a ``differentiable`` propagator a ``values`` that
        requires grad (grad mode on) gives a result on the autograd graph exactly as ``apply`` does -- the same forward bits, the
        backward one launch over the store-wide lists; ``out`` cannot be combined with that."""
        if self.tmat is None:
            raise RuntimeError("Propagator.apply_vectors: this propagator was built without frames= (no transport table)")
        return self._apply("apply_vectors", 2, "two rows for each of the", interpolate_vectors, interpolate_vectors_backward,
                           lambda t0, t1: (self.tmat[t0 * self.k:t1 * self.k],) * 2, values, clouds, out)

    @torch.no_grad()
    def labels(self, pred, clouds=None):
        """The k = 1 label transfer: every target row takes the entry of `pred` (DEVICE ``[source rows of the clouds]``, any
        dtype) of its NEAREST source point -- a gather by the first neighbour slot.  A target row without a neighbour (an empty
        source cloud) gets -1."""
        clouds = (0, len(self)) if clouds is None else clouds
        c0, c1 = int(clouds[0]), int(clouds[1])
        q, s, _, (t0, t1), (s0, s1) = self.cloud_range((c0, c1))
        if pred.dim() != 1 or pred.shape[0] != s1 - s0:
            raise ValueError(f"Propagator.labels: pred must hold the {s1 - s0} source rows of clouds {(c0, c1)}")
        if not pred.is_cuda:
            raise RuntimeError("Propagator.labels: pred must live on the HIP device (there is no CPU path)")
        sizes = torch.from_numpy(self.tsizes[c0:c1]).to(self.device)
        base = torch.repeat_interleave(s[:-1], sizes, output_size=t1 - t0)          # first source row of every target row's cloud
        near = self.idx[t0:t1, 0].long()
        out = pred[(base + near.clamp(min=0)).clamp(max=max(s1 - s0 - 1, 0))] if s1 > s0 else pred.new_zeros(t1 - t0)
        return torch.where(near >= 0, out, torch.full_like(out, -1))
