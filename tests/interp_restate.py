"""Numpy restatement of deltaconv_amd/csrc/interp_math.h: the two-set nearest-neighbour search as a brute-force STABLE sort on the
fp32 squared distance, and the inverse-squared-distance interpolation op by op in fp32.  tests/test_interp_host.py holds it to
a g++ build of the header bit for bit and to fp64 (``cKDTree``, the PyG formula); tests/test_gpu_interp.py holds the kernels
of csrc/interp.hip to it bit for bit."""
import numpy as np

D2_CLAMP = np.float32(1e-16)
F32 = np.float32


def dist2(q, r):
    """fp32 [Nq, Nr]: dx = q - r per axis, ((dx*dx + dy*dy) + dz*dz), every operation rounded on its own."""
    q, r = np.asarray(q, dtype=F32).reshape(-1, 3), np.asarray(r, dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = (q[:, None, :] - r[None, :, :]).astype(F32)
        sq = (d * d).astype(F32)
        return ((sq[..., 0] + sq[..., 1]).astype(F32) + sq[..., 2]).astype(F32)


def knn_cross(q, r, k):
    """-> (idx int32 [Nq,k] local to r, d2 fp32 [Nq,k]): ascending distance, ties by the lower index; only candidates with a
    distance BELOW +inf (NaN and +inf are never picked); empty slots are -1 / +inf."""
    d = dist2(q, r)
    nq, nr = d.shape
    idx = np.full((nq, k), -1, dtype=np.int32)
    out = np.full((nq, k), np.inf, dtype=F32)
    if nr == 0 or nq == 0:
        return idx, out
    with np.errstate(invalid="ignore"):
        ok = d < np.inf
    key = np.where(ok, d, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    picked_ok = np.take_along_axis(ok, order, axis=1)
    idx[:, :m] = np.where(picked_ok, order, -1)
    out[:, :m] = np.where(picked_ok, np.take_along_axis(d, order, axis=1), np.inf)
    return idx, out


def interpolate(x, idx, d2):
    """x [Nr, C] fp32, idx / d2 [Nq, k] -> fp32 [Nq, C]: w = 1 / fmax(d2, 1e-16); slots in order, a slot with idx outside
    [0, Nr) skipped; num += w * x, den += w (each rounded); num / den; ONE valid slot: the row itself; none: zeros."""
    x = np.asarray(x, dtype=F32)
    nr, c = x.shape
    nq, k = idx.shape
    num, den = np.zeros((nq, c), dtype=F32), np.zeros(nq, dtype=F32)
    only, valid = np.zeros((nq, c), dtype=F32), np.zeros(nq, dtype=np.int64)
    for s in range(k):
        j = idx[:, s].astype(np.int64)
        ok = (j >= 0) & (j < nr)
        if not ok.any():
            continue
        w = (F32(1.0) / np.fmax(d2[ok, s].astype(F32), D2_CLAMP)).astype(F32)
        rows = x[j[ok]]
        num[ok] = (num[ok] + (w[:, None] * rows).astype(F32)).astype(F32)
        den[ok] = (den[ok] + w).astype(F32)
        only[ok] = rows
        valid[ok] += 1
    with np.errstate(all="ignore"):
        out = (num / np.where(valid > 1, den, F32(1.0))[:, None]).astype(F32)
    out[valid == 1] = only[valid == 1]
    out[valid == 0] = 0
    return out


def knn_cross_batched(q, qptr, r, rptr, k):
    """The B pairs of absolute offsets qptr / rptr [B+1] -> idx / d2 [len(q), k]; rows outside every pair stay -9 / -9."""
    q, r = np.asarray(q, dtype=F32), np.asarray(r, dtype=F32)
    idx, d2 = np.full((q.shape[0], k), -9, dtype=np.int32), np.full((q.shape[0], k), -9, dtype=F32)
    for b in range(len(qptr) - 1):
        i, d = knn_cross(q[qptr[b]:qptr[b + 1]], r[rptr[b]:rptr[b + 1]], k)
        idx[qptr[b]:qptr[b + 1]], d2[qptr[b]:qptr[b + 1]] = i, d
    return idx, d2


def interpolate_batched(x, qptr, rptr, idx, d2):
    x = np.asarray(x, dtype=F32)
    out = np.zeros((idx.shape[0], x.shape[1]), dtype=F32)
    for b in range(len(qptr) - 1):
        rows = slice(qptr[b], qptr[b + 1])
        out[rows] = interpolate(x[rptr[b]:rptr[b + 1]], idx[rows], d2[rows])
    return out


def knn_interpolate(x, pos_x, pos_y, k=3, ptr_x=None, ptr_y=None):
    """``torch_geometric.nn.knn_interpolate`` restated: features x at pos_x -> rows at pos_y."""
    ptr_x = [0, len(pos_x)] if ptr_x is None else ptr_x
    ptr_y = [0, len(pos_y)] if ptr_y is None else ptr_y
    idx, d2 = knn_cross_batched(pos_y, ptr_y, pos_x, ptr_x, k)
    return interpolate_batched(x, ptr_y, ptr_x, idx, d2)
