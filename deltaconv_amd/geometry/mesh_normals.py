"""Per-vertex normals of a batch of device-resident triangle meshes (reference: ``GenerateMeshNormals()`` of torch_geometric in the
ShapeSeg ``pre_transform``, experiments/train_shapeseg.py:31, one host call per shape): the tensor-level form of
csrc/mesh_normal.hip behind ``dc_mesh_vertex_faces`` and ``dc_mesh_vertex_normals``.  ``DeviceMeshDataset.vertex_normals`` and
``vertex_cloud`` (meshes.py) are the dataset-level forms; ``transforms.GenerateMeshNormals`` is the host transform."""
import torch

WEIGHTINGS = {"uniform": 0, "area": 1}           # csrc/mesh_normal_math.h


def weighting_code(weighting):
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting must be one of {sorted(WEIGHTINGS)}, got {weighting!r}")
    return WEIGHTINGS[weighting]


def _check(fn, tensors, face, vptr, fptr):
    for name, t, dt in tensors:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{fn}: `{name}` must be a contiguous {dt} tensor on a HIP device")
    if face.dim() != 2 or face.shape[1] != 3:
        raise ValueError(f"{fn}: face must be [Fs,3] (one row per triangle)")
    if vptr.dim() != 1 or vptr.shape != fptr.shape or vptr.shape[0] < 1:
        raise ValueError(f"{fn}: vptr and fptr must both hold B+1 offsets")


def vertex_face_lists(face, vptr, fptr, num_verts):
    """The vertex-to-incident-corner lists of a whole store, built once on the device.

    face: DEVICE int32 [Fs,3], vertex ids LOCAL to the mesh; vptr, fptr: DEVICE int64 [B+1] ABSOLUTE row offsets of the B meshes
    into the vertex rows / face; num_verts: the vertex rows of the store (host).
    -> ``(vf_ptr int64 [num_verts+1], vf_edge int64 [3*Fs])``: the list of vertex row v is ``vf_edge[vf_ptr[v]:vf_ptr[v+1]]``, its
    entries ``3 * face_row + corner`` in ascending order.  A face row with an id outside its mesh is in no list (``vf_edge`` is then
    written up to ``vf_ptr[-1]`` only)."""
    from .._lib import lib
    _check("vertex_face_lists", (("face", face, torch.int32), ("vptr", vptr, torch.int64), ("fptr", fptr, torch.int64)),
           face, vptr, fptr)
    nv, nf, dev = int(num_verts), int(face.shape[0]), face.device
    if nv < 0:
        raise ValueError("vertex_face_lists: num_verts >= 0")
    vf_ptr = torch.empty(nv + 1, dtype=torch.int64, device=dev)
    vf_edge = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    need = int(lib.raw("dc_mesh_vertex_faces_workspace_bytes")(nv, nf))
    ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
    lib.call("dc_mesh_vertex_faces", face, vptr, fptr, int(vptr.shape[0]) - 1, nv, nf, vf_ptr, vf_edge, ws, need)
    return vf_ptr, vf_edge


def vertex_normals_batch(vert, face, vptr, fptr, lists=None, weighting="uniform", out=None, zero_count=None):
    """``GenerateMeshNormals()`` for every mesh of a batch on the device: per face ``c = (p1 - p0) x (p2 - p0)``, which gives
    ``c / max(|c|, 1e-12)`` (``weighting="uniform"``, torch_geometric's) or ``c`` itself (``"area"``) to each of its corners; the
    normal of a vertex is ``s / max(|s|, 1e-12)`` with ``s`` the sum over its incident corners, taken sequentially in ascending
    ``3 * face_row + corner`` -- no floating-point atomics, the same bits on every run (csrc/mesh_normal_math.h).

    vert: DEVICE float32 [Vs,3]; face, vptr, fptr as in ``vertex_face_lists``; lists: its result for the same store (built here
    when ``None``); out: float32 [Vs,3] to write into (rows outside every mesh of the call keep their values; a fresh ``out``
    starts as zeros); zero_count: int32 [B] to receive per mesh the number of vertices that got the zero vector (no incident
    face, or a sum that is exactly zero).
    The face winding decides the sign of a normal: inconsistent winding is not repaired.  A vertex's normal is a function of its
    mesh alone, whatever the grouping into calls; permuting the faces of a mesh may change the last bits.
    -> ``out``."""
    from .._lib import lib
    code = weighting_code(weighting)
    checks = [("vert", vert, torch.float32), ("face", face, torch.int32), ("vptr", vptr, torch.int64), ("fptr", fptr, torch.int64)]
    if lists is not None:
        checks += [("lists[0]", lists[0], torch.int64), ("lists[1]", lists[1], torch.int64)]
    if out is not None:
        checks.append(("out", out, torch.float32))
    if zero_count is not None:
        checks.append(("zero_count", zero_count, torch.int32))
    _check("vertex_normals_batch", checks, face, vptr, fptr)
    if vert.dim() != 2 or vert.shape[1] != 3:
        raise ValueError("vertex_normals_batch: vert must be [Vs,3]")
    nv, nf, b = int(vert.shape[0]), int(face.shape[0]), int(vptr.shape[0]) - 1
    if out is not None and out.shape != vert.shape:
        raise ValueError("vertex_normals_batch: `out` must have the shape of vert")
    if zero_count is not None and tuple(zero_count.shape) != (b,):
        raise ValueError("vertex_normals_batch: `zero_count` must hold one count per mesh")
    if lists is None:
        lists = vertex_face_lists(face, vptr, fptr, nv)
    elif tuple(lists[0].shape) != (nv + 1,) or tuple(lists[1].shape) != (3 * nf,):
        raise ValueError("vertex_normals_batch: `lists` must be (vf_ptr [Vs+1], vf_edge [3*Fs]) of this store")
    out = torch.zeros_like(vert) if out is None else out
    lib.call("dc_mesh_vertex_normals", vert, face, vptr, fptr, b, nv, nf, lists[0], lists[1], code, out, zero_count)
    return out
