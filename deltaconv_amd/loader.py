"""Device-resident datasets: the prepared dataset lives in HBM, ONE kernel launch builds a training batch from it --
gather of the chosen clouds, augmentation with on-device draws, ``pos / norm / x / batch / ptr / y / category`` written
straight into the batch's tensors (csrc/batch.hip: ``dc_batch_assemble``).

What it replaces: the host side of the reference's input pipelines (experiments/train_modelnet.py:37-50,99,
train_shapenet.py:36-50, train_scanobjectnn.py:47-62, train_shapeseg.py:37-61, train_shrec.py:37-52) -- a Python
``transform`` per shape, a Python collate per batch, an upload from pageable memory per batch.  Every dataset of those
scripts fits in HBM many times over (ModelNet40 at 1024 points with normals: 242 MB).

    store = DeviceDataset.from_dataset(train_dataset, device)          # ds.transform is NOT run; the loader's is
    loader = DeviceLoader(store, 32, shuffle=True, drop_last=True,
                          transform=[T.RandomScale((4 / 5, 5 / 4)), T.RandomTranslateGlobal(0.1)], seed=1)
    for epoch in range(epochs):
        loader.set_epoch(epoch)
        for batch in loader: ...                                        # deltaconv_amd.Batch on the device, no host sync
    step = GraphedTrainStep(model, loss_fn, loader.static_batch(), opt)
    for _ in loader.into(step.static): step()                           # assembled in place, then the replay

The permutation of an epoch is a function of ``(seed, epoch)``, drawn on the host and uploaded once per epoch; the
augmentation draws are a function of ``(seed, step = epoch * len(loader) + i, dataset index of the cloud, op, point)``
(csrc/batch_math.h), so a run is reproducible from ``(seed, epoch)`` and a cloud's augmented rows do not depend on the
batch it lands in.  There is no CPU path: a transform the kernel does not implement raises ``ValueError``.
"""
import ctypes
import numbers

import numpy as np
import torch

from . import transforms as T
from ._lib import lib
from .data import Batch
from .geometry.graph import PtrInfo

__all__ = ["DeviceDataset", "DeviceLoader", "RandomJitter", "translate_transforms", "translate_normalize", "random_split",
           "OP_SCALE", "OP_ROTATE", "OP_TRANSLATE", "OP_NORMAL_JITTER", "OP_POINT_JITTER", "MAX_OPS"]

# op codes of csrc/batch_math.h
OP_SCALE, OP_ROTATE, OP_TRANSLATE, OP_NORMAL_JITTER, OP_POINT_JITTER = 1, 2, 3, 4, 5
MAX_OPS = 8


class RandomJitter:
    """Per-point, per-axis offsets uniform in ``(-translate, translate)`` added to ``pos``: torch_geometric's
    ``RandomTranslate`` (the jitter of experiments/train_scanobjectnn.py:49), with its random-number consumption -- one
    ``uniform_`` of n values per axis, in axis order."""

    def __init__(self, translate):
        self.translate = translate

    def __call__(self, data):
        n, dim = data.pos.size()
        t = [self.translate] * dim if isinstance(self.translate, numbers.Number) else list(self.translate)
        assert len(t) == dim
        ts = [data.pos.new_empty(n).uniform_(-abs(a), abs(a)) for a in t]
        data.pos = data.pos + torch.stack(ts, dim=-1)
        return data

    def __repr__(self):
        return f"{self.__class__.__name__}({self.translate})"


def _three(t, what):
    t = [t] * 3 if isinstance(t, numbers.Number) else list(t)
    if len(t) != 3:
        raise ValueError(f"{what}: one value or one per axis of a 3-D cloud, got {t}")
    return tuple(abs(float(a)) for a in t)


def translate_transforms(transform, has_norm=True):
    """``None`` | a transform | a ``Compose`` / list / tuple of them -> the kernel's op list ``[(code, (p0, p1, p2)), ...]``,
    in order.  Anything but RandomScale / RandomRotate / RandomTranslateGlobal / RandomNormals / RandomJitter raises
    ``ValueError`` naming it; so does RandomNormals on a store without normals."""
    if transform is None:
        seq = []
    elif isinstance(transform, (list, tuple)):
        seq = list(transform)
    elif hasattr(transform, "transforms"):
        seq = list(transform.transforms)
    else:
        seq = [transform]
    ops = []
    for t in seq:
        if type(t) is T.RandomScale:
            ops.append((OP_SCALE, (float(t.scales[0]), float(t.scales[1]), 0.0)))
        elif type(t) is T.RandomRotate:
            if t.axis not in (0, 1, 2):
                raise ValueError(f"{t!r}: axis must be 0, 1 or 2")
            ops.append((OP_ROTATE, (float(t.degrees[0]), float(t.degrees[1]), float(t.axis))))
        elif type(t) is T.RandomTranslateGlobal:
            ops.append((OP_TRANSLATE, _three(t.translate, repr(t))))
        elif type(t) is T.RandomNormals:
            if not has_norm:
                raise ValueError(f"{t!r}: the store has no normals")
            ops.append((OP_NORMAL_JITTER, _three(t.translate, repr(t))))
        elif type(t) is RandomJitter:
            ops.append((OP_POINT_JITTER, _three(t.translate, repr(t))))
        else:
            raise ValueError(f"DeviceLoader: no device form of transform {t!r} ({type(t).__name__}); it takes RandomScale, "
                             "RandomRotate, RandomTranslateGlobal, RandomNormals and RandomJitter (there is no CPU fallback)")
    if len(ops) > MAX_OPS:
        raise ValueError(f"DeviceLoader: at most {MAX_OPS} augmentation ops, got {len(ops)}")
    return ops


def _sequence(transform):
    if transform is None:
        return []
    if isinstance(transform, (list, tuple)):
        return list(transform)
    return list(transform.transforms) if hasattr(transform, "transforms") else [transform]


def translate_normalize(transform, has_face=False):
    """A transform | a ``Compose`` / list / tuple of them -> the op list ``[(code, p0, p1), ...]`` of csrc/shape_norm.hip, in order.
    ``NormalizeScale(norm_ord 2 | inf, scaling_factor)``, ``NormalizeArea()`` (a mesh store only) and ``NormalizeAxes()`` (its
    ``max_points`` is accepted and ignored, as the reference ignores it); anything else, an empty chain or more than 4 ops raises
    ``ValueError``."""
    from .geometry.shape_norm import MAX_NORM_OPS, OP_NORM_AREA, OP_NORM_AXES, OP_NORM_SCALE
    ops = []
    for t in _sequence(transform):
        if type(t) is T.NormalizeScale:
            if t.norm_ord not in (2, float("inf")) or isinstance(t.norm_ord, bool):
                raise ValueError(f"normalize: NormalizeScale(norm_ord={t.norm_ord!r}): the device op takes 2 and inf")
            factor = float("nan") if t.scaling_factor is None else float(t.scaling_factor)
            if t.scaling_factor is not None and factor != factor:
                raise ValueError("normalize: NormalizeScale(scaling_factor=nan)")
            ops.append((OP_NORM_SCALE, float(t.norm_ord), factor))
        elif type(t) is T.NormalizeArea:
            if not has_face:
                raise ValueError("normalize: NormalizeArea needs faces: it runs on a DeviceMeshDataset, not on a point store")
            ops.append((OP_NORM_AREA, 0.0, 0.0))
        elif type(t) is T.NormalizeAxes:
            ops.append((OP_NORM_AXES, 0.0, 0.0))
        else:
            raise ValueError(f"normalize: no device form of transform {t!r} ({type(t).__name__}); it takes NormalizeScale, "
                             "NormalizeArea and NormalizeAxes (there is no CPU fallback)")
    if not 1 <= len(ops) <= MAX_NORM_OPS:
        raise ValueError(f"normalize: 1 .. {MAX_NORM_OPS} normalisation ops, got {len(ops)}")
    return ops


def shape_rows(sizes, indices):
    """Host int64 array of the store rows of the shapes ``indices`` (in that order), from the host sizes."""
    sizes = np.asarray(sizes, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < 0 or idx.max() >= sizes.shape[0]):
        raise ValueError(f"subset: indices must lie in [0, {sizes.shape[0]})")
    n = sizes[idx]
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    return (np.repeat(start[idx] - first, n) + np.arange(int(n.sum()), dtype=np.int64)).astype(np.int64), idx, n


def random_split(store, lengths, seed):
    """The seeded split of experiments/train_shapeseg.py:46-50 for a device store: subsets whose indices are those of
    ``torch.utils.data.random_split(range(len(store)), lengths, generator=torch.Generator().manual_seed(seed))``, in its order
    (``lengths``: counts, or fractions that sum to 1, as torch takes them).  Pure indexing: no kernel, any device."""
    parts = torch.utils.data.random_split(range(len(store)), lengths, generator=torch.Generator().manual_seed(int(seed)))
    return [store.subset(list(p.indices)) for p in parts]


class DeviceDataset:
    """All clouds of a dataset concatenated on the device (the "store") + their sizes on the host."""

    def __init__(self, pos, ptr, sizes, norm=None, x=None, y_point=None, y_cloud=None, category=None):
        self.pos, self.norm, self.x, self.y_point, self.y_cloud, self.category = pos, norm, x, y_point, y_cloud, category
        self.ptr = ptr                                   # int64 [S+1], device
        self.sizes = np.asarray(sizes, dtype=np.int64)   # host
        self.device = pos.device
        self.norm_stats = self.degenerate = None         # of the normalize pass that made this store

    def __len__(self):
        return int(self.sizes.shape[0])

    @classmethod
    def from_dataset(cls, ds, device, fps=None, fps_seed=None, normalize=None, fps_large="host"):
        """ds: a dataset with ``.items`` (ModelNet / ScanObjectNN / ShapeNet / ShapeSeg; its ``transform`` is not run) or any
        sequence of ``Data``.  Attributes taken: ``pos``, ``norm`` (or ``normal``), ``x``, ``y`` (one per cloud or one per
        point), ``category`` -- each either on every item or on none, as ``collate`` treats them.  ``fps``: reduce every cloud to
        that many points with ``geodesic_subsample(fps, seed=fps_seed, large=fps_large)`` once it is on the device (``None``: the
        clouds as they are).
        ``normalize``: NormalizeScale / NormalizeAxes transforms run on the device by ``normalize`` below, before ``fps``."""
        items = list(ds.items if hasattr(ds, "items") and not callable(ds.items) else ds)
        if not items:
            raise ValueError("DeviceDataset: empty dataset")

        def column(name):
            vals = [getattr(d, name, None) for d in items]
            return vals if all(v is not None for v in vals) else None

        pos = [d.pos for d in items]
        sizes = [int(p.shape[0]) for p in pos]
        for p in pos:
            if p.dim() != 2 or p.shape[1] != 3:
                raise ValueError(f"DeviceDataset: pos must be [n, 3], got {tuple(p.shape)}")
        norm = column("norm") or column("normal")
        x = column("x")
        if x is not None:
            x = [v.reshape(v.shape[0], -1) for v in x]
        ys, y_point, y_cloud = column("y"), None, None
        if ys is not None:
            ys = [(v if torch.is_tensor(v) else torch.tensor([v])).reshape(-1) for v in ys]
            if any(v.is_floating_point() for v in ys):
                raise ValueError("DeviceDataset: labels must be integers")
            if all(v.numel() == 1 for v in ys):
                y_cloud = torch.cat(ys).long()
            elif all(v.numel() == n for v, n in zip(ys, sizes)):
                y_point = torch.cat(ys).long()
            else:
                raise ValueError("DeviceDataset: y must hold one label per cloud or one per point")
        cats = column("category")
        category = torch.stack([c.reshape(-1) for c in cats]).float() if cats is not None else None
        for name, col in (("norm", norm), ("x", x)):
            if col is not None and any(v.shape[0] != n for v, n in zip(col, sizes)):
                raise ValueError(f"DeviceDataset: {name} must have one row per point")
        ptr = torch.zeros(len(items) + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
        up = lambda t: None if t is None else t.contiguous().to(device)
        f32 = lambda col: None if col is None else torch.cat(col).float()
        store = cls(up(f32(pos)), up(ptr), sizes, up(f32(norm)), up(f32(x)), up(y_point), up(y_cloud), up(category))
        if normalize is not None:
            store.normalize(normalize, out=store)
        return store if fps is None else store.geodesic_subsample(fps, seed=fps_seed, large=fps_large)

    def normalize(self, transforms, shapes_per_launch=4096, out=None):
        """``T.NormalizeScale(norm_ord=, scaling_factor=)`` / ``T.NormalizeAxes()`` (one of them or a list / ``Compose`` of up to 4)
        for every cloud of the store on the device: two launches per group of ``shapes_per_launch`` clouds (csrc/shape_norm.hip),
        the same bits whatever the grouping.  -> a new store that shares every tensor with this one but ``pos`` (and ``norm``
        where NormalizeAxes permuted its columns as it permutes the positions); ``out=store`` (this store, typically) is
        normalised in place and returned.  The result carries ``norm_stats`` (device [S, n_ops, 8]: centre, scale, permutation per
        op) and ``degenerate`` (host bool array: a centre or scale that is not finite or a scale <= 0) -- one synchronise at the
        end of the pass.  ``NormalizeArea`` needs faces and raises ``ValueError`` here; so does any other transform."""
        from .geometry.shape_norm import OP_NORM_AXES, normalize_store_rows
        ops = translate_normalize(transforms, has_face=False)
        res = out if out is not None else DeviceDataset(self.pos, self.ptr, self.sizes, self.norm, self.x, self.y_point, self.y_cloud,
                                                        self.category)
        if out is not None and (out.pos.shape != self.pos.shape or not np.array_equal(out.sizes, self.sizes)):
            raise ValueError("normalize: `out` must be a store of the same clouds")
        permutes = self.norm is not None and any(o[0] == OP_NORM_AXES for o in ops)
        if permutes:
            res.norm = self.norm.clone() if out is None else out.norm.copy_(self.norm)
        res.pos, res.norm_stats, res.degenerate = normalize_store_rows(
            self.pos, self.ptr, self.sizes, ops, shapes_per_launch, norm=res.norm if permutes else None,
            out=None if out is None else out.pos)
        return res

    def subset(self, indices):
        """A new store of the clouds ``indices`` (host sequence of dataset indices, kept in that order): rows, offsets, host sizes,
        labels and categories follow.  Pure tensor indexing: no kernel, and it works on CPU tensors."""
        rows, idx, n = shape_rows(self.sizes, indices)
        dev = self.pos.device
        rows_d, idx_d = torch.from_numpy(rows).to(dev), torch.from_numpy(idx).to(dev)
        ptr = torch.zeros(idx.shape[0] + 1, dtype=torch.int64)
        ptr[1:] = torch.from_numpy(np.cumsum(n))
        take = lambda t, i: None if t is None else t[i].contiguous()
        sub = DeviceDataset(take(self.pos, rows_d), ptr.to(dev), n, take(self.norm, rows_d), take(self.x, rows_d),
                            take(self.y_point, rows_d), take(self.y_cloud, idx_d), take(self.category, idx_d))
        sub.norm_stats = take(self.norm_stats, idx_d)
        sub.degenerate = None if self.degenerate is None else np.asarray(self.degenerate)[idx]
        return sub

    def geodesic_subsample(self, n_samples, start=None, seed=None, clouds_per_launch=1024, large="host"):
        """A new store whose clouds each hold ``n_samples`` geodesic-farthest points of this one's: ``T.GeodesicFPS(n_samples)``
        (reference: transforms/geodesic_fps.py:14-43) for the whole dataset on the device -- ``geometry.geodesic_fps_batch`` over
        groups of ``clouds_per_launch`` clouds, then ``pos``, ``norm``, ``x`` and per-point ``y`` gathered by the sample ids.  A
        cloud of n < n_samples points is tiled as the transform tiles it (``idx[:n].repeat(ceil(n_samples / n))[:n_samples]``).
        ``start``: the first sample of every cloud (host sequence of ids local to the cloud); otherwise drawn per cloud from
        ``(seed, dataset index)`` (``geometry.fps.fps_starts``; ``seed=None``: at random), whatever ``clouds_per_launch`` is.
        A cloud above the device sampler's cap of 16 384 points goes through the host library (``geometry.geodesic_fps``, which
        derives its start from a seed: an explicit ``start`` for such a cloud raises ``ValueError``) and its ids are uploaded.
        ``large="device"``: such a cloud is sampled on the device as well (``dc_geodesic_fps_large``, up to 262 144 points; above
        that, or for a store on the CPU, ``ValueError``), from the same ``start`` / ``fps_starts`` point as any other cloud --
        the picks do not depend on which side of the cap a cloud falls, nor on ``clouds_per_launch``."""
        from .geometry.fps import (FPS_LARGE_MAX_POINTS, FPS_MAX_POINTS, _fps_by_size_class, _fps_launches, fps_starts,
                                   geodesic_fps)
        m, s, dev = int(n_samples), len(self), self.device
        if m < 1 or int(clouds_per_launch) < 1:
            raise ValueError("geodesic_subsample: n_samples >= 1 and clouds_per_launch >= 1")
        if large not in ("host", "device"):
            raise ValueError(f"geodesic_subsample: large must be 'host' or 'device', got {large!r}")
        if large == "device" and not self.pos.is_cuda:
            raise ValueError("geodesic_subsample: large='device' needs a store on a HIP device")
        if large == "device" and s and self.sizes.max() > FPS_LARGE_MAX_POINTS:
            raise ValueError(f"geodesic_subsample: a cloud of {int(self.sizes.max())} points; the device sampler for large clouds "
                             f"takes at most {FPS_LARGE_MAX_POINTS} per cloud")
        sizes = self.sizes
        if start is None:
            starts = fps_starts(sizes, seed)
        else:
            starts = np.asarray(start, dtype=np.int64).reshape(-1)
            if starts.shape != sizes.shape or (starts < 0).any() or (starts >= sizes).any():
                raise ValueError("geodesic_subsample: `start` must hold one point of every cloud (ids local to the cloud)")
        ptr_host = np.zeros(s + 1, dtype=np.int64)
        ptr_host[1:] = np.cumsum(sizes)
        small = np.flatnonzero(sizes <= FPS_MAX_POINTS)
        ids = torch.empty((s, m), dtype=torch.int64, device=dev)
        if small.size == s:
            ids = _fps_launches(self.pos, ptr_host, m, starts, int(clouds_per_launch)).long()
        elif large == "device":
            ids = _fps_by_size_class(self.pos, ptr_host, m, starts, int(clouds_per_launch))
        else:
            if start is not None:
                raise ValueError(f"geodesic_subsample: a cloud above {FPS_MAX_POINTS} points is sampled by the host library, which "
                                 "takes a seed, not a start point")
            if small.size:
                rows = torch.from_numpy(np.concatenate([np.arange(ptr_host[i], ptr_host[i + 1]) for i in small])).to(dev)
                ptr_small = np.zeros(small.size + 1, dtype=np.int64)
                ptr_small[1:] = np.cumsum(sizes[small])
                ids[torch.from_numpy(small).to(dev)] = _fps_launches(self.pos[rows], ptr_small, m, starts[small],
                                                                     int(clouds_per_launch)).long()
            for i in np.flatnonzero(sizes > FPS_MAX_POINTS):
                pts = self.pos[int(ptr_host[i]):int(ptr_host[i + 1])].cpu().numpy()
                host_seed = None if seed is None else int(np.random.Generator(np.random.Philox(key=[int(seed), int(i)])).integers(0, 2 ** 31))
                ids[i] = torch.from_numpy(np.atleast_1d(geodesic_fps(pts, m, seed=host_seed)).astype(np.int64)).to(dev)
        # the tiling rule of T.GeodesicFPS: column j of a cloud of n < m points is sample j mod n
        n_dev = torch.from_numpy(np.minimum(sizes, m)).to(dev)
        cols = torch.arange(m, device=dev)[None, :] % n_dev[:, None]
        rows = (ids.gather(1, cols) + torch.from_numpy(ptr_host[:-1]).to(dev)[:, None]).reshape(-1)
        take = lambda t: None if t is None else t[rows].contiguous()
        ptr = torch.arange(s + 1, dtype=torch.int64, device=dev) * m
        return DeviceDataset(take(self.pos), ptr, np.full(s, m, dtype=np.int64), take(self.norm), take(self.x), take(self.y_point),
                             self.y_cloud, self.category)

    def fps_subsample(self, n_samples, start=None, seed=None, method=None):
        """The Euclidean sibling of ``geodesic_subsample``: a new store whose clouds each hold the ``n_samples`` Euclidean
        farthest points of this one's (``geometry.fps``, one call for the whole store), rows in PICK order -- so ``prefix_levels``
        on the new store is a farthest-point hierarchy.  ``start``: the first pick of every cloud (host sequence of ids local to
        the cloud); otherwise drawn per cloud from ``(seed, dataset index)`` (``geometry.fps.fps_starts``; ``seed=None``: at
        random).  ``method``: the sampler, as in ``geometry.fps`` ("brute": clouds up to 16 384 points; "grid": up to 262 144;
        None: its switch) -- the same rows either way.  ``pos``, ``norm``, ``x`` and per-point ``y`` are gathered by the picks;
        ``source_rows`` (int64 [S * n_samples]: the picked rows of THIS store) is set as ``voxel_subsample`` sets it, so
        ``Propagator(sub, parent)`` is the way back.  A cloud of fewer than ``n_samples`` points raises ``ValueError`` naming it:
        there is no tiling."""
        from .geometry.fps import fps, fps_starts
        from .geometry.graph import PtrInfo
        m, s, dev, sizes = int(n_samples), len(self), self.device, self.sizes
        if m < 1:
            raise ValueError("fps_subsample: n_samples >= 1")
        if s and sizes.min() < m:
            i = int(np.argmin(sizes))
            raise ValueError(f"fps_subsample: cloud {i} has {int(sizes[i])} points, fewer than n_samples = {m}")
        if start is None:
            starts = fps_starts(sizes, seed)
        else:
            starts = np.asarray(start, dtype=np.int64).reshape(-1)
            if starts.shape != sizes.shape or (starts < 0).any() or (starts >= sizes).any():
                raise ValueError("fps_subsample: `start` must hold one point of every cloud (ids local to the cloud)")
        ptr = torch.arange(s + 1, dtype=torch.int64, device=dev) * m
        if s:
            info = PtrInfo(self.ptr, s, int(sizes.max()), int(sizes.min()))
            rows, _ = fps(self.pos, ptr_info=info, n_samples=m, start=torch.from_numpy(starts.astype(np.int32)).to(dev), method=method)
        else:
            rows = torch.empty(0, dtype=torch.int64, device=dev)
        take = lambda t: None if t is None else t[rows].contiguous()
        sub = DeviceDataset(take(self.pos), ptr, np.full(s, m, dtype=np.int64), take(self.norm), take(self.x), take(self.y_point),
                            self.y_cloud, self.category)
        sub.source_rows = rows
        return sub

    def voxel_subsample(self, size, origin=None, pick="centre", reduce=None, num_classes=None):
        """A new store that keeps of every cloud one point per occupied grid cell of edge ``size`` (``geometry.voxel_subsample``:
        the member nearest the cell centre, or with ``pick="first"`` the first one; ``origin=None``: every cloud's grid starts at
        its own minimum, so a cloud thins the same way in any store).  ``pos``, ``norm``, ``x`` and per-point ``y`` are gathered by
        the kept rows, which stay in their order; ``y_cloud`` and ``category`` are shared; the ragged host ``sizes`` come from the
        output offsets.  Two more attributes: ``source_rows`` (int64 [N_out]: the kept rows of THIS store) and ``cluster`` (int64
        [N]: for every row of this store the row of the new one that stands for it, -1 for a row with a non-finite coordinate) --
        ``Propagator(sub, parent)`` interpolates predictions back, ``cluster`` pools onto the thinned store.  Linear in the
        points: it evens out a scan or an over-tessellated mesh before ``geodesic_subsample``.  Two device reads: the call's own and the output offsets.

        ``reduce=None`` (the default): every attribute is the representative's.  ``reduce="mean"``: the attributes are pooled over
        the cells instead (``geometry.cluster_lists`` once, then one launch each) -- ``pos`` the cell barycentre and ``norm`` the
        normalised mean normal (``cluster_mean_pos``: fp64 sums in row order; a cell whose normals cancel keeps its representative's
        normal), ``x`` the fp32 mean (``cluster_pool_rows``), ``y_point`` the majority label (``cluster_majority``, ties to the
        lowest label; ``num_classes``: the number of labels, read once from the store's labels -- one more device read -- where not
        given).  ``source_rows``, ``cluster`` and the row order are the same in both modes."""
        from .geometry.voxel import voxel_subsample
        if reduce not in (None, "mean"):
            raise ValueError(f"voxel_subsample: reduce must be None or 'mean', got {reduce!r}")
        rows, optr, cluster = voxel_subsample(self.pos, size, ptr=self.ptr, origin=origin, pick=pick)
        take = lambda t: None if t is None else t[rows].contiguous()
        optr_host = optr.cpu().numpy()
        if reduce is None:
            sub = DeviceDataset(take(self.pos), optr, optr_host[1:] - optr_host[:-1], take(self.norm), take(self.x),
                                take(self.y_point), self.y_cloud, self.category)
        else:
            from .geometry.cluster import MAX_CLASSES, cluster_lists, cluster_majority, cluster_mean_pos, cluster_pool_rows
            cptr, members = cluster_lists(cluster, int(rows.numel()))
            norm = x = y_point = None
            if self.norm is not None:
                norm = cluster_mean_pos(self.norm, cptr, members, normalize=True)
                norm = torch.where((norm == 0).all(1, keepdim=True), take(self.norm), norm)
            if self.x is not None:
                x = cluster_pool_rows(self.x, cptr, members, "mean")[0]
            if self.y_point is not None:
                if num_classes is None:
                    num_classes = max(int(self.y_point.max()) + 1, 1) if self.y_point.numel() else 1
                if not 1 <= int(num_classes) <= MAX_CLASSES:
                    raise ValueError(f"voxel_subsample: num_classes = {int(num_classes)} outside [1, {MAX_CLASSES}]")
                y_point = cluster_majority(self.y_point, cptr, members, int(num_classes))
            sub = DeviceDataset(cluster_mean_pos(self.pos, cptr, members), optr, optr_host[1:] - optr_host[:-1], norm, x, y_point,
                                self.y_cloud, self.category)
        sub.source_rows, sub.cluster = rows, cluster
        return sub


def epoch_permutation(n, seed, epoch, shuffle=True):
    """The order of the n clouds in `epoch`: a function of (seed, epoch) only; ``arange`` without shuffling."""
    if not shuffle:
        return np.arange(n, dtype=np.int64)
    return np.random.Generator(np.random.Philox(key=[int(seed), int(epoch)])).permutation(n).astype(np.int64)


class DeviceLoader:
    def __init__(self, store, batch_size, shuffle=False, drop_last=False, transform=None, seed=0, rank=0, world=1):
        if batch_size < 1 or not 0 <= rank < world:
            raise ValueError("DeviceLoader: batch_size >= 1 and 0 <= rank < world")
        if not 0 <= int(seed) < 2 ** 32:
            raise ValueError("DeviceLoader: seed in [0, 2^32)")
        self.store, self.batch_size, self.shuffle, self.drop_last = store, int(batch_size), shuffle, drop_last
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.ops = translate_transforms(transform, has_norm=getattr(store, "norm", None) is not None)
        n = len(self.ops)
        self._codes = (ctypes.c_int32 * max(n, 1))(*[c for c, _ in self.ops])
        self._params = (ctypes.c_float * max(3 * n, 1))(*[v for _, p in self.ops for v in p])
        self.share = len(store) // self.world            # clouds per rank and epoch: equally long shares
        self._perm_dev = (None, None)                    # (epoch, this rank's share of its permutation on the device)

    def __len__(self):
        return self.share // self.batch_size if self.drop_last else -(-self.share // self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def rank_share(self, epoch, rank=None):
        """Host index array of one rank's share of the epoch: the permutation is the same on every rank, cut to a multiple
        of `world` (the last ``len(store) % world`` clouds of the epoch's order sit out), rank r takes every world-th."""
        perm = epoch_permutation(len(self.store), self.seed, epoch, self.shuffle)
        return perm[:self.share * self.world][(self.rank if rank is None else rank)::self.world]

    def batch_indices(self, epoch=None):
        """The dataset indices of every batch of `epoch` (default: the current one) on this rank, as host lists."""
        share = self.rank_share(self.epoch if epoch is None else epoch)
        bs = self.batch_size
        return [share[i * bs:(i + 1) * bs].tolist() for i in range(len(self))]

    # ---- the launch -----------------------------------------------------------------------------------------------------
    def _shape(self, sizes):
        st = self.store
        nt, b = int(sizes.sum()), int(sizes.shape[0])
        return {"pos": (nt, 3), "norm": None if st.norm is None else (nt, 3),
                "x": None if st.x is None else (nt, st.x.shape[1]),
                "y": (nt,) if st.y_point is not None else ((b,) if st.y_cloud is not None else None),
                "category": None if st.category is None else (b, st.category.shape[1])}

    def _new_batch(self, sizes):
        dev, sh = self.store.device, self._shape(sizes)
        mk = lambda s, dt: None if s is None else torch.empty(s, dtype=dt, device=dev)
        out = Batch(mk(sh["pos"], torch.float32), torch.empty(sh["pos"][0], dtype=torch.int64, device=dev),
                    mk(sh["norm"], torch.float32), mk(sh["x"], torch.float32), mk(sh["y"], torch.int64),
                    mk(sh["category"], torch.float32), num_graphs=sizes.shape[0])
        out._ptr = torch.empty(sizes.shape[0] + 1, dtype=torch.int32, device=dev)
        return out

    def _assemble(self, out, idx_dev, sizes, step):
        """One launch: the clouds idx_dev (device int64 [B], sizes known on the host) into the tensors of `out`."""
        st = self.store
        b, nt, mx = int(sizes.shape[0]), int(sizes.sum()), int(sizes.max())
        lib.call("dc_batch_assemble", st.pos, st.norm, st.x, 0 if st.x is None else st.x.shape[1], st.y_point, st.y_cloud,
                 st.category, 0 if st.category is None else st.category.shape[1], st.ptr, len(st), idx_dev, b, nt, mx,
                 self._codes, self._params, len(self.ops), self.seed, int(step), out.pos, out.norm, out.x, out.batch, out._ptr,
                 out.y, out.category)
        out._ptr_info = PtrInfo(out._ptr, b, mx, int(sizes.min()))     # the host knows the sizes: no sync in the model
        return out

    def assemble(self, indices, step=0, out=None):
        """The batch of the clouds `indices` (host list / array of dataset indices) at augmentation step `step`."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.min() < 0 or idx.max() >= len(self.store):
            raise ValueError("DeviceLoader.assemble: indices must be a non-empty list of dataset indices")
        sizes = self.store.sizes[idx]
        out = self._new_batch(sizes) if out is None else out
        return self._assemble(out, torch.from_numpy(idx).to(self.store.device), sizes, step)

    def _epoch(self, target=None, fresh_tail=False):
        epoch = self.epoch
        share = self.rank_share(epoch)
        if self._perm_dev[0] != (epoch, self.shuffle):
            self._perm_dev = ((epoch, self.shuffle), torch.from_numpy(np.ascontiguousarray(share)).to(self.store.device))
        perm_dev, bs, nb = self._perm_dev[1], self.batch_size, len(self)
        want = None if target is None else self._batch_shape(target)
        for i in range(nb):
            sizes = self.store.sizes[share[i * bs:(i + 1) * bs]]
            into = target
            if target is not None:
                sh = dict(self._shape(sizes), batch=(int(sizes.sum()),), ptr=(sizes.shape[0] + 1,))
                if fresh_tail and i == nb - 1 and sizes.shape[0] < bs:
                    into = None                 # the short last batch of an evaluation pass: a batch of its own
                elif sh != want or not np.array_equal(sizes, self._static_sizes(target)):
                    raise ValueError(f"DeviceLoader.into: batch {i} of epoch {epoch} does not have the shape of the static batch "
                                     f"({sh} vs {want}, or other cloud sizes); in-place assembly needs equal shapes "
                                     "(equal-size clouds, drop_last=True)")
            out = self._new_batch(sizes) if into is None else into
            yield self._assemble(out, perm_dev[i * bs:(i + 1) * bs], sizes, epoch * nb + i)
        self.epoch = epoch + 1

    def __iter__(self):
        return self._epoch()

    # ---- in place, in front of a captured step ---------------------------------------------------------------------------
    @staticmethod
    def _batch_shape(batch):
        sh = lambda t: None if t is None else tuple(t.shape)
        return {"pos": sh(batch.pos), "norm": sh(batch.norm), "x": sh(batch.x), "y": sh(batch.y),
                "category": sh(batch.category), "batch": sh(batch.batch), "ptr": sh(batch.ptr)}

    @staticmethod
    def _static_sizes(batch):
        sizes = getattr(batch, "_dc_sizes", None)
        if sizes is None:                       # a batch from elsewhere: one host read, once
            ptr = batch.ptr.cpu().numpy().astype(np.int64)
            sizes = batch._dc_sizes = ptr[1:] - ptr[:-1]
        return sizes

    def static_batch(self):
        """A batch of the loader's full shape (the first batch of epoch 0, unaugmented order does not matter: it is
        overwritten by ``into``), to hand to ``GraphedTrainStep`` as its sample batch."""
        if len(self) == 0:
            raise ValueError("DeviceLoader.static_batch: the loader has no full batch")
        idx = self.rank_share(0)[:self.batch_size]
        out = self.assemble(idx, step=0)
        out._dc_sizes = self.store.sizes[idx].copy()
        return out

    def into(self, static, fresh_tail=False):
        """Iterate the current epoch while assembling IN PLACE into the tensors of `static` (``step.static`` of a
        GraphedTrainStep): one launch per batch in place of the copy launch of ``GraphedTrainStep.load``, every ``data_ptr``
        unchanged.  Yields `static` itself; call the step without a batch.  Raises when a batch of the epoch has another
        shape or other cloud sizes than `static` (the captured step holds its cloud offsets).  fresh_tail: a last batch with
        fewer clouds than ``batch_size`` (``drop_last=False``) is yielded as a NEW batch instead of raising -- the
        evaluation passes of deltaconv_amd.evaluate run it eagerly."""
        if static.pos.device != self.store.device:
            raise ValueError("DeviceLoader.into: the static batch lives on another device than the store")
        for name, dt in (("pos", torch.float32), ("norm", torch.float32), ("x", torch.float32), ("y", torch.int64),
                         ("category", torch.float32), ("batch", torch.int64)):
            t = getattr(static, name, None)
            if t is not None and (t.dtype != dt or not t.is_contiguous()):
                raise ValueError(f"DeviceLoader.into: static.{name} must be contiguous {dt}")
        static.ptr                               # materialised once (a batch from elsewhere computes it here)
        return self._epoch(target=static, fresh_tail=fresh_tail)
