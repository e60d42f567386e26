"""Device-resident triangle meshes and their surface sampling: all meshes of a dataset concatenated in HBM, ``num`` points
drawn on every one of them in two launches per group of meshes (csrc/mesh.hip: ``dc_mesh_sample``), after their normalisation
in two more (csrc/shape_norm.hip: ``dc_shape_normalize``), with ``subset`` for the seeded splits of ``loader.random_split``; and
the meshes' own vertices as clouds, with per-vertex normals (csrc/mesh_normal.hip: ``vertex_normals``, ``vertex_cloud``).

What it replaces: the ``SamplePoints`` step of the reference's data preparation (deltaconv/transforms/sample_points.py:22-59,
called per shape from the ``pre_transform`` of experiments/train_modelnet.py:30-34, train_shrec.py:30-34 and
train_shapeseg.py:28-34) -- a ``torch.multinomial`` over the faces and a handful of small ATen calls per shape.

    meshes = DeviceMeshDataset.from_dataset(ModelNet(root, None, "40", True), device, normalize=T.NormalizeScale())
    store = meshes.sample_points(num_points * sampling_margin, seed=1).geodesic_subsample(num_points, seed=1)
    loader = DeviceLoader(store, 32, shuffle=True, drop_last=True, transform=aug, seed=1)

A mesh's sample is a function of ``(mesh, seed, round, dataset index)`` only (csrc/mesh_math.h): it does not depend on how
meshes are grouped into launches, and another ``round`` gives a fresh sample of the same store.  There is no CPU path.
"""
import numpy as np
import torch

from .geometry.mesh_normals import vertex_face_lists, vertex_normals_batch, weighting_code
from .geometry.mesh_sample import sample_points_batch
from .loader import DeviceDataset, shape_rows, translate_normalize

__all__ = ["DeviceMeshDataset", "sample_points_batch", "MESH_MAX_FACES"]

MESH_MAX_FACES = 1 << 24          # faces per mesh (csrc/mesh_math.h: the sum of the integer face weights stays below 2^57)


def _offsets(counts):
    ptr = np.zeros(len(counts) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.asarray(counts, dtype=np.int64))
    return ptr


class DeviceMeshDataset:
    """All meshes of a dataset concatenated on the device + their vertex and face counts on the host."""

    def __init__(self, vert, face, vptr, fptr, n_verts, n_faces, y_vert=None, y_cloud=None, category=None):
        self.vert, self.face, self.vptr, self.fptr = vert, face, vptr, fptr      # [Vs,3] f32, [Fs,3] i32 (local ids), [S+1] i64 x 2
        self.n_verts = np.asarray(n_verts, dtype=np.int64)                        # host
        self.n_faces = np.asarray(n_faces, dtype=np.int64)                        # host
        self.y_vert, self.y_cloud, self.category = y_vert, y_cloud, category
        self.device = vert.device
        self.total = self.degenerate = None                                       # of the last sample_points pass
        self.norm_stats = None                                                    # of the normalize pass that made this store
        self.vertex_lists = None                                                  # (vf_ptr, vf_edge) once vertex_normals built them

    def __len__(self):
        return int(self.n_faces.shape[0])

    @classmethod
    def from_dataset(cls, ds, device, normalize=None):
        """ds: a dataset with ``.items`` (ModelNet / ShapeSeg read with a ``pre_transform`` that keeps the faces; its
        ``transform`` is not run) or any sequence of items with ``pos [V,3]`` and ``face [3,F]`` as the OFF / PLY / OBJ readers
        give them.  Optional ``y`` (one per vertex or one per cloud) and ``category``, each on every item or on none.  Raises
        ``ValueError`` unless every mesh has ``V >= 1``, ``1 <= F <= 2^24`` and every face id in ``[0, V)``.  ``normalize``: NormalizeScale /
        NormalizeArea / NormalizeAxes transforms run on the device by ``normalize`` below once the meshes are there, so the
        dataset's ``pre_transform`` need not normalise on the host."""
        items = list(ds.items if hasattr(ds, "items") and not callable(ds.items) else ds)
        if not items:
            raise ValueError("DeviceMeshDataset: empty dataset")
        verts, faces = [], []
        for i, d in enumerate(items):
            p, f = getattr(d, "pos", None), getattr(d, "face", None)
            if p is None or f is None:
                raise ValueError(f"DeviceMeshDataset: item {i} has no pos / face (was SamplePoints already run in pre_transform?)")
            if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
                raise ValueError(f"DeviceMeshDataset: item {i}: pos must be [V,3] with V >= 1, got {tuple(p.shape)}")
            if f.dim() != 2 or f.shape[0] != 3 or f.is_floating_point():
                raise ValueError(f"DeviceMeshDataset: item {i}: face must be integer [3,F], got {f.dtype} {tuple(f.shape)}")
            if not 1 <= f.shape[1] <= MESH_MAX_FACES:
                raise ValueError(f"DeviceMeshDataset: item {i} has {f.shape[1]} faces, supported: 1 .. 2^24")
            if int(f.min()) < 0 or int(f.max()) >= p.shape[0]:
                raise ValueError(f"DeviceMeshDataset: item {i}: face ids {int(f.min())} .. {int(f.max())} outside its "
                                 f"{p.shape[0]} vertices")
            verts.append(p.float())
            faces.append(f.t().to(torch.int32))
        n_verts, n_faces = [int(p.shape[0]) for p in verts], [int(f.shape[0]) for f in faces]

        def column(name):
            vals = [getattr(d, name, None) for d in items]
            return vals if all(v is not None for v in vals) else None

        ys, y_vert, y_cloud = column("y"), None, None
        if ys is not None:
            ys = [(v if torch.is_tensor(v) else torch.tensor([v])).reshape(-1) for v in ys]
            if any(v.is_floating_point() for v in ys):
                raise ValueError("DeviceMeshDataset: labels must be integers")
            if all(v.numel() == 1 for v in ys):
                y_cloud = torch.cat(ys).long()
            elif all(v.numel() == n for v, n in zip(ys, n_verts)):
                y_vert = torch.cat(ys).long()
            else:
                raise ValueError("DeviceMeshDataset: y must hold one label per cloud or one per vertex")
        cats = column("category")
        category = torch.stack([c.reshape(-1) for c in cats]).float() if cats is not None else None
        up = lambda t: None if t is None else t.contiguous().to(device)
        store = cls(up(torch.cat(verts)), up(torch.cat(faces)), up(torch.from_numpy(_offsets(n_verts))),
                    up(torch.from_numpy(_offsets(n_faces))), n_verts, n_faces, up(y_vert), up(y_cloud), up(category))
        return store if normalize is None else store.normalize(normalize, out=store)

    def normalize(self, transforms, shapes_per_launch=4096, out=None):
        """``T.NormalizeScale(...)`` / ``T.NormalizeArea()`` / ``T.NormalizeAxes()`` (one of them or a list / ``Compose`` of up to 4,
        e.g. the ``[T.NormalizeArea(), T.NormalizeAxes()]`` of experiments/train_shapeseg.py:28-30) for every mesh of the store on
        the device: two launches per group of ``shapes_per_launch`` meshes (csrc/shape_norm.hip), the same bits whatever the
        grouping.  NormalizeArea is the surface area over the face rows (``T.NormalizeArea`` on ``Data(pos, face=[F,3])``).
        -> a new store that shares every tensor with this one but ``vert``; ``out=store`` (this store, typically) is normalised
        in place and returned.  The result carries ``norm_stats`` (device [S, n_ops, 8]: centre, scale, permutation per op) and
        ``degenerate`` (host bool array: a centre or scale that is not finite or a scale <= 0, e.g. a mesh without area under
        NormalizeArea) -- one synchronise at the end of the pass.  Any other transform raises ``ValueError``."""
        from .geometry.shape_norm import normalize_store_rows
        ops = translate_normalize(transforms, has_face=True)
        res = out if out is not None else DeviceMeshDataset(self.vert, self.face, self.vptr, self.fptr, self.n_verts, self.n_faces,
                                                            self.y_vert, self.y_cloud, self.category)
        if out is not None and (out.vert.shape != self.vert.shape or not np.array_equal(out.n_verts, self.n_verts)):
            raise ValueError("normalize: `out` must be a store of the same meshes")
        res.vert, res.norm_stats, res.degenerate = normalize_store_rows(
            self.vert, self.vptr, self.n_verts, ops, shapes_per_launch, face=self.face, fptr=self.fptr,
            out=None if out is None else out.vert)
        return res

    def subset(self, indices):
        """A new store of the meshes ``indices`` (host sequence of dataset indices, kept in that order): vertex and face rows (face
        ids are local to the mesh), offsets, host counts, labels and categories follow.  Pure tensor indexing: no kernel, and it
        works on CPU tensors."""
        vrows, idx, nv = shape_rows(self.n_verts, indices)
        frows, _, nf = shape_rows(self.n_faces, indices)
        dev = self.vert.device
        up = lambda a: torch.from_numpy(a).to(dev)
        vrows, frows, idx_d = up(vrows), up(frows), up(idx)
        take = lambda t, i: None if t is None else t[i].contiguous()
        sub = DeviceMeshDataset(take(self.vert, vrows), take(self.face, frows), up(_offsets(nv)), up(_offsets(nf)), nv, nf,
                                take(self.y_vert, vrows), take(self.y_cloud, idx_d), take(self.category, idx_d))
        sub.norm_stats = take(self.norm_stats, idx_d)
        return sub

    def sample_points(self, num, include_normals=True, include_labels=False, seed=0, round=0, meshes_per_launch=4096):
        """``T.SamplePoints(num, include_normals=, include_labels=)`` for the whole store on the device -> a ``DeviceDataset`` whose
        clouds each hold ``num`` points (``geodesic_subsample`` takes it from there).  ``norm`` is set with ``include_normals``;
        ``y_point`` from the per-vertex labels (corner 0 of the picked face) with ``include_labels``, otherwise ``y_cloud`` and
        ``category`` pass through.  Draws are a function of ``(seed, round, dataset index, sample index)``, whatever
        ``meshes_per_launch`` is (the workspace holds 8 bytes per face of a group).  The per-mesh sums of the face weights are
        kept as ``total`` (device) and ``degenerate`` (host bool array, ``total == 0``: every face of that mesh has zero area
        and it was sampled uniformly by face index) on this store and on the result -- one synchronise at the end of the pass."""
        num, s, dev, per = int(num), len(self), self.device, int(meshes_per_launch)
        if num < 1 or not 1 <= per <= 65535:
            raise ValueError("sample_points: num >= 1 and 1 <= meshes_per_launch <= 65535")
        if not 0 <= int(seed) < 2 ** 32 or int(round) < 0:
            raise ValueError("sample_points: seed in [0, 2^32) and round >= 0")
        if include_labels and self.y_vert is None:
            raise ValueError("sample_points: include_labels needs one label per vertex on every mesh")
        pos = torch.empty((s * num, 3), dtype=torch.float32, device=dev)
        norm = torch.empty((s * num, 3), dtype=torch.float32, device=dev) if include_normals else None
        y = torch.empty(s * num, dtype=torch.int64, device=dev) if include_labels else None
        total = torch.empty(s, dtype=torch.int64, device=dev)
        fhost = _offsets(self.n_faces)
        for lo in range(0, s, per):
            hi = min(s, lo + per)
            cut = lambda t: None if t is None else t[lo * num:hi * num]
            out = {"pos": cut(pos), "total": total[lo:hi]}
            if include_normals:
                out["norm"] = cut(norm)
            if include_labels:
                out["y"] = cut(y)
            sample_points_batch(self.vert, self.face, self.vptr[lo:hi + 1], self.fptr[lo:hi + 1], num, first_mesh_index=lo,
                                seed=seed, round=round, y_vert=self.y_vert if include_labels else None, normals=include_normals,
                                labels=include_labels, n_faces=int(fhost[hi] - fhost[lo]), out=out)
        ptr = torch.arange(s + 1, dtype=torch.int64, device=dev) * num
        store = DeviceDataset(pos, ptr, np.full(s, num, dtype=np.int64), norm, None, y,
                              None if include_labels else self.y_cloud, self.category)
        self.total = store.total = total
        self.degenerate = store.degenerate = total.cpu().numpy() == 0             # the one synchronise of the pass
        return store

    def vertex_normals(self, weighting="uniform", zero_count=None):
        """``GenerateMeshNormals()`` (torch_geometric's, train_shapeseg.py:31) for the whole store on the device -> float32 [Vs,3],
        one unit normal per vertex row: per face ``c = (p1 - p0) x (p2 - p0)``, which gives ``c / max(|c|, 1e-12)``
        (``weighting="uniform"``, PyG's) or ``c`` (``"area"``) to each of its corners, summed per vertex in a fixed order and
        normalised (``geometry.vertex_normals_batch``; no floating-point atomics, the same bits on every run).  A vertex without
        incident face, or whose contributions cancel exactly, gets the zero vector; ``zero_count`` (device int32 [S]) receives
        their number per mesh.  The face winding decides the sign: inconsistent winding is not repaired.  A vertex's normal is a
        function of its mesh alone; permuting the faces of a mesh may change the last bits.  The vertex-to-corner lists are built
        once and kept on the store as ``vertex_lists`` (a normalisation in place keeps them: they hold no coordinates; ``subset``
        and a ``normalize`` that makes a new store start without)."""
        weighting_code(weighting)
        if self.vertex_lists is None:
            self.vertex_lists = vertex_face_lists(self.face, self.vptr, self.fptr, int(self.vert.shape[0]))
        return vertex_normals_batch(self.vert, self.face, self.vptr, self.fptr, self.vertex_lists, weighting, zero_count=zero_count)

    @staticmethod
    def _refuse_zero_normals(counts):
        bad = np.flatnonzero(np.asarray(counts) != 0)
        if bad.size:
            first = ", ".join(f"mesh {int(i)}: {int(counts[i])}" for i in bad[:5])
            raise ValueError(f"vertex_cloud: {bad.size} of {len(counts)} meshes have vertices with a zero normal (no incident face, or "
                             f"face normals that cancel) -- {first}{', ...' if bad.size > 5 else ''}; pass allow_zero_normals=True "
                             "to keep them")

    def vertex_cloud(self, include_normals=True, include_labels=True, weighting="uniform", allow_zero_normals=False):
        """The meshes' own vertices as a ``DeviceDataset`` -- what the human-body segmentation benchmark is scored on: ``pos`` IS
        ``vert`` (shared, not copied), ``ptr`` / ``sizes`` the vertex offsets and counts, ``norm`` the ``vertex_normals(weighting)``
        with ``include_normals``, ``y_point`` the per-vertex labels with ``include_labels`` (otherwise ``y_cloud`` passes through);
        ``category`` and ``norm_stats`` carry over.  The result runs through ``normalize``, ``geodesic_subsample``, ``DeviceLoader``
        (variable-size clouds are assembled eagerly), ``DeviceEvaluator``, ``DeviceTrainer`` and, with this store as target,
        ``Propagator``.  With ``include_normals`` the per-mesh counts of zero normals are read back -- the one synchronise of the
        pass -- and kept on the result as ``zero_normals`` (host int array); any non-zero count raises ``ValueError`` naming the
        first few meshes unless ``allow_zero_normals``."""
        weighting_code(weighting)
        if include_labels and self.y_vert is None:
            raise ValueError("vertex_cloud: include_labels needs one label per vertex on every mesh")
        norm = counts = None
        if include_normals:
            zero = torch.empty(len(self), dtype=torch.int32, device=self.device)
            norm = self.vertex_normals(weighting, zero_count=zero)
            counts = zero.cpu().numpy().astype(np.int64)                          # the one synchronise of the pass
            if not allow_zero_normals:
                self._refuse_zero_normals(counts)
        store = DeviceDataset(self.vert, self.vptr, self.n_verts, norm, None, self.y_vert if include_labels else None,
                              None if include_labels else self.y_cloud, self.category)
        store.norm_stats, store.zero_normals = self.norm_stats, counts
        return store
