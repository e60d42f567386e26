"""numpy restatement of deltaconv_amd/csrc/voxel_math.h: which points take part, the origin, the cell of a point, the range, the
64-bit key of a representative and the output order, every fp32 operation rounded on its own.  Written from the header's rules,
not from its code; tests/test_voxel_host.py holds the g++ build of the header to it bit for bit, tests/test_gpu_voxel.py the device."""
import numpy as np

F = np.float32
LIMIT = F(2.0 ** 20)
BIAS = 1 << 20


def finite_rows(p):
    return np.isfinite(np.asarray(p, dtype=F).reshape(-1, 3)).all(1)


def edges(size):
    return np.broadcast_to(np.asarray(size, dtype=F).reshape(-1), (3,)).copy()


def origin_of(pos):
    """The default origin of one cloud: the fp32 minimum per axis over its finite points (zeros where it has none)."""
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    fin = pos[finite_rows(pos)]
    return fin.min(0).astype(F) if fin.shape[0] else np.zeros(3, F)


def cells(pos, o, s):
    """-> t fp32 [n,3]: floorf(fl(fl(p - o) / s)) (rows with a non-finite coordinate give whatever comes out)."""
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = (pos - o[None, :].astype(F)).astype(F)
        return np.floor((d / s[None, :].astype(F)).astype(F)).astype(F)


def centres(t, o, s):
    with np.errstate(all="ignore"):
        return (((t + F(0.5)).astype(F) * s[None, :]).astype(F) + o[None, :]).astype(F)


def dist2(p, c):
    with np.errstate(all="ignore"):
        d = (p - c).astype(F)
        sq = (d * d).astype(F)
        return ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)


def key(d2, idx):
    """(bits(d2) << 32) | index as uint64."""
    bits = np.ascontiguousarray(d2, dtype=F).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def pack(t):
    """In-range cells [m,3] fp32 -> the 63-bit packed cell (x lowest)."""
    c = (t.astype(np.int64) + BIAS).astype(np.uint64)
    return (c[:, 2] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 0]


def cloud(pos, size, origin=None, pick="centre"):
    """One cloud -> dict(rows int64 ascending local ids, cluster int64 [n] rank or -1, overflow bool, cell uint64 [n] (all ones:
    none), key uint64 [n])."""
    pos = np.asarray(pos, dtype=F).reshape(-1, 3)
    n = pos.shape[0]
    s = edges(size)
    o = origin_of(pos) if origin is None else np.asarray(origin, dtype=F).reshape(3)
    fin = finite_rows(pos)
    t = cells(pos, o, s)
    with np.errstate(all="ignore"):
        inside = (np.abs(t) < LIMIT).all(1)
    overflow = bool((fin & ~inside).any())
    part = fin & inside
    ids = np.flatnonzero(part)
    cell = np.full(n, ~np.uint64(0), np.uint64)
    keys = np.full(n, ~np.uint64(0), np.uint64)
    cell[ids] = pack(t[ids])
    d2 = dist2(pos[ids], centres(t[ids], o, s)) if pick == "centre" else np.zeros(ids.size, F)
    assert pick in ("centre", "first")
    keys[ids] = key(d2, ids)
    # per cell the smallest key; its low word is the representative
    order = ids[np.lexsort((keys[ids], cell[ids]))]
    head = np.ones(order.size, bool)
    head[1:] = cell[order[1:]] != cell[order[:-1]]
    reps = np.sort(order[head])                                        # ascending rows
    cluster = np.full(n, -1, np.int64)
    if ids.size:
        group = np.cumsum(head) - 1                                    # of order[j]
        rep_of = np.empty(n, np.int64)
        rep_of[order] = order[head][group]
        cluster[ids] = np.searchsorted(reps, rep_of[ids])
    return dict(rows=reps.astype(np.int64), cluster=cluster, overflow=overflow, cell=cell, key=keys)


def batch(clouds, size, origin=None, pick="centre"):
    """A batch -> (rows int64 global, optr int64 [B+1], cluster int64 [N] global output rows or -1, first overflowing cloud or -1).
    ``origin``: None, [3] for all clouds, or [B,3]."""
    b = len(clouds)
    if origin is not None:
        origin = np.asarray(origin, dtype=F)
        origin = np.broadcast_to(origin.reshape(-1, 3), (b, 3)) if b else origin.reshape(0, 3)
    rows, cluster, optr, base, over = [], [], [0], 0, -1
    for i, pos in enumerate(clouds):
        r = cloud(pos, size, None if origin is None else origin[i], pick)
        if r["overflow"] and over < 0:
            over = i
        rows.append(r["rows"] + base)
        cluster.append(np.where(r["cluster"] >= 0, r["cluster"] + optr[-1], -1))
        optr.append(optr[-1] + r["rows"].size)
        base += np.asarray(pos).reshape(-1, 3).shape[0]
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    return cat(rows), np.asarray(optr, np.int64), cat(cluster), over
