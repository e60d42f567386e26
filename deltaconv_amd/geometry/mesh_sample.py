"""Surface sampling of a batch of device-resident triangle meshes (reference: deltaconv/transforms/sample_points.py:22-59, one
host call per shape): the tensor-level form of csrc/mesh.hip behind ``dc_mesh_sample``.  ``deltaconv_amd.DeviceMeshDataset``
(meshes.py) is the dataset-level form."""
import torch


def sample_points_batch(vert, face, vptr, fptr, num, first_mesh_index=0, seed=0, round=0, y_vert=None, normals=True,
                        labels=False, face_ids=False, return_cdf=False, n_faces=None, out=None):
    """``num`` surface points of every mesh of a batch on the device (reference: transforms/sample_points.py:22-59, one host call
    per shape).

    vert: DEVICE float32 [Vs,3]; face: DEVICE int32 [Fs,3], vertex ids LOCAL to the mesh; vptr, fptr: DEVICE int64 [B+1]
    ABSOLUTE row offsets of the B meshes into vert / face (a slice of a store's offset arrays serves).  Mesh b draws as
    dataset index ``first_mesh_index + b``.  ``n_faces``: ``fptr[B] - fptr[0]`` where the host knows it (otherwise it is read
    from the device: one synchronise).  ``out``: a dict of preallocated ``pos / norm / y / face_id / total`` to write into.
    -> ``(pos [B*num,3], norm [B*num,3] | None, y [B*num] | None, face_id [B*num] | None, total [B])`` and, with
    ``return_cdf``, the uint64 cdf as int64 ``[n_faces]``.  ``total[b] == 0``: every face of mesh b is degenerate and it was
    sampled uniformly by face index."""
    from .._lib import lib
    for name, t, dt in (("vert", vert, torch.float32), ("face", face, torch.int32), ("vptr", vptr, torch.int64),
                        ("fptr", fptr, torch.int64)):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"sample_points_batch: `{name}` must be a contiguous {dt} tensor on a HIP device")
    if vert.dim() != 2 or vert.shape[1] != 3 or face.dim() != 2 or face.shape[1] != 3:
        raise ValueError("sample_points_batch: vert must be [Vs,3] and face [Fs,3] (one row per triangle)")
    if vptr.dim() != 1 or vptr.shape != fptr.shape or vptr.shape[0] < 1:
        raise ValueError("sample_points_batch: vptr and fptr must both hold B+1 offsets")
    b, num = int(vptr.shape[0]) - 1, int(num)
    if labels and y_vert is None:
        raise ValueError("sample_points_batch: labels need the per-vertex labels y_vert")
    if y_vert is not None and (y_vert.dtype != torch.int64 or y_vert.shape != (vert.shape[0],)):
        raise ValueError("sample_points_batch: y_vert must be int64 [Vs]")
    if num < 1:
        raise ValueError("sample_points_batch: num >= 1")
    dev = vert.device
    out = out or {}
    mk = lambda key, shape, dt, want: (out[key] if key in out else torch.empty(shape, dtype=dt, device=dev)) if want else None
    pos = mk("pos", (b * num, 3), torch.float32, True)
    norm = mk("norm", (b * num, 3), torch.float32, normals)
    y = mk("y", (b * num,), torch.int64, labels)
    fid = mk("face_id", (b * num,), torch.int32, face_ids)
    total = mk("total", (b,), torch.int64, True)
    for t, shape in ((pos, (b * num, 3)), (norm, (b * num, 3)), (y, (b * num,)), (fid, (b * num,)), (total, (b,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"sample_points_batch: an output of shape {tuple(t.shape)}, expected contiguous {shape}")
    if n_faces is None:
        n_faces = int(fptr[-1] - fptr[0]) if b else 0
    need = int(lib.raw("dc_mesh_sample_workspace_bytes")(int(n_faces)))
    ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
    lib.call("dc_mesh_sample", vert, face, vptr, fptr, b, int(first_mesh_index), num, int(seed), int(round), y_vert, pos, norm, y,
             fid, total, ws, need)
    res = (pos, norm, y, fid, total)
    return res + (ws[:int(n_faces)],) if return_cdf else res
