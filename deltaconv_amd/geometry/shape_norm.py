"""Per-shape normalisation of a batch of device-resident clouds or meshes (reference: deltaconv/transforms/normalize_scale.py:12-21,
normalize_area.py:12-20, normalize_axes.py:17-26, one host call per shape): the tensor-level form of csrc/shape_norm.hip behind
``dc_shape_normalize``.  ``DeviceDataset.normalize`` and ``DeviceMeshDataset.normalize`` are the dataset-level forms."""
import ctypes

import numpy as np
import torch

# op codes of csrc/shape_norm_math.h; an op is ``(code, p0, p1)``: OP_NORM_SCALE takes (norm_ord 2 | inf, scaling_factor | NaN for none)
OP_NORM_SCALE, OP_NORM_AREA, OP_NORM_AXES = 1, 2, 3
MAX_NORM_OPS = 4
STAT_WORDS = 8


def normalize_shapes_batch(pos, ptr, ops, face=None, fptr=None, norm=None, out=None, n_rows=None):
    """A chain of 1 to 4 normalisation ops on every shape of a batch, two launches.

    pos: DEVICE float32 [N,3]; ptr: DEVICE int64 [B+1] ABSOLUTE row offsets of the B shapes into pos (a slice of a store's offsets
    serves); ops: ``[(code, p0, p1), ...]`` as ``loader.translate_normalize`` gives them; face: DEVICE int32 [Fs,3] ids LOCAL to the
    shape with fptr [B+1], needed by an area op; norm: DEVICE float32 [N,3], permuted IN PLACE where an axes op permutes the
    columns (an extension: the reference has no normals at this point; uniform scaling leaves unit normals alone); out: the
    tensor the rows are written to (``out=pos``: in place; default: a clone of pos, so rows outside the call keep their values);
    ``n_rows``: ``ptr[B] - ptr[0]`` where the host knows it (otherwise read from the device: one synchronise).
    -> ``(pos, norm, stats [B, n_ops, 8])``: per shape and op the centre (3), the scale, the permutation (3, as floats), 0."""
    from .._lib import lib
    ops = list(ops)
    need_face = any(o[0] == OP_NORM_AREA for o in ops)
    checks = [("pos", pos, torch.float32), ("ptr", ptr, torch.int64)]
    if face is not None or fptr is not None or need_face:
        checks += [("face", face, torch.int32), ("fptr", fptr, torch.int64)]
    if norm is not None:
        checks.append(("norm", norm, torch.float32))
    if out is not None:
        checks.append(("out", out, torch.float32))
    for name, t, dt in checks:
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"normalize_shapes_batch: `{name}` must be a contiguous {dt} tensor on a HIP device")
    if pos.dim() != 2 or pos.shape[1] != 3 or ptr.dim() != 1 or ptr.shape[0] < 1:
        raise ValueError("normalize_shapes_batch: pos must be [N,3] and ptr hold B+1 offsets")
    if face is not None and (face.dim() != 2 or face.shape[1] != 3 or fptr.shape != ptr.shape):
        raise ValueError("normalize_shapes_batch: face must be [Fs,3] (one row per triangle) and fptr hold B+1 offsets")
    for name, t in (("norm", norm), ("out", out)):
        if t is not None and t.shape != pos.shape:
            raise ValueError(f"normalize_shapes_batch: `{name}` must have the shape of pos")
    if not 1 <= len(ops) <= MAX_NORM_OPS:
        raise ValueError(f"normalize_shapes_batch: 1 .. {MAX_NORM_OPS} ops, got {len(ops)}")
    b = int(ptr.shape[0]) - 1
    if n_rows is None:
        n_rows = int(ptr[-1] - ptr[0]) if b else 0
    out = pos.clone() if out is None else out
    stats = torch.empty((b, len(ops), STAT_WORDS), dtype=torch.float32, device=pos.device)
    codes = (ctypes.c_int32 * len(ops))(*[int(o[0]) for o in ops])
    params = (ctypes.c_float * (2 * len(ops)))(*[float(v) for o in ops for v in (o[1], o[2])])
    lib.call("dc_shape_normalize", pos, ptr, face, fptr, b, int(n_rows), codes, params, len(ops), out, norm, stats, None, 0)
    return out, norm, stats


def degenerate_from_stats(stats):
    """stats [S, n_ops, 8] (numpy) -> bool [S]: a centre or scale that is not finite, or a scale <= 0, in any op."""
    head = np.asarray(stats)[:, :, :4]
    return ~(np.isfinite(head).all(axis=(1, 2)) & (head[:, :, 3] > 0).all(axis=1))


def normalize_store_rows(pos, ptr, sizes, ops, per, face=None, fptr=None, norm=None, out=None):
    """The rows of a whole store in groups of ``per`` shapes (what both stores' ``normalize`` run) -> ``(pos, stats [S,n_ops,8],
    degenerate host bool [S])``.  ``degenerate``: a centre or scale that is not finite, or a scale <= 0, in any op -- read back with
    the one synchronise of the pass."""
    s, per = int(len(sizes)), int(per)
    if not 1 <= per <= 65535:
        raise ValueError("normalize: 1 <= shapes_per_launch <= 65535")
    off = np.zeros(s + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(sizes, dtype=np.int64))
    out = pos.clone() if out is None else out
    parts = []
    for lo in range(0, s, per):
        hi = min(s, lo + per)
        parts.append(normalize_shapes_batch(pos, ptr[lo:hi + 1], ops, face, None if fptr is None else fptr[lo:hi + 1], norm, out,
                                            n_rows=int(off[hi] - off[lo]))[2])
    stats = parts[0] if len(parts) == 1 else torch.cat(parts)
    return out, stats, degenerate_from_stats(stats.cpu().numpy())                 # the one synchronise of the pass
