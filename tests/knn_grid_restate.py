"""numpy restatement of deltaconv_amd/csrc/knn_grid_math.h: the grid rule (fp64 operations that IEEE rounds the same everywhere), the
cell of a point, the stopping bound and the ring search, every fp32 operation rounded on its own.  Written from the header's
rules, not from its code; tests/test_knn_grid_host.py holds the g++ build of the header to it bit for bit."""
import numpy as np

F = np.float32
MAX_AXIS = 1024
SLACK = F(1.0 - 2.0 ** -10)
B2_MIN, B2_MAX = F(1e-30), F(1e37)
FLT_MAX = F(3.4028234663852886e38)


def finite_rows(p):
    return np.isfinite(np.asarray(p, dtype=F)).all(1)


def dist2(q, r):
    """q [3], r [M,3] fp32 -> [M]: ((dx*dx + dy*dy) + dz*dz), every operation rounded to fp32."""
    with np.errstate(all="ignore"):
        d = (q[None, :].astype(F) - r.astype(F)).astype(F)
        sq = (d * d).astype(F)
        return ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)


def make_grid(m, lo, hi, target):
    """-> dict(lo [3] f32, inv_h [3] f32, g [3] int, min_h f32, m, cells)"""
    G = dict(lo=np.zeros(3, F), inv_h=np.zeros(3, F), g=np.ones(3, np.int64), min_h=F(0), m=max(int(m), 0), cells=1)
    if m <= 0:
        return G
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    G["lo"] = lo.copy()
    want = np.floor(np.float64(m) / np.float64(F(target)))
    want = min(max(want, 1.0), 2.0 * m)
    with np.errstate(all="ignore"):
        ext32 = (hi - lo).astype(F)
    act = np.isfinite(ext32) & (ext32 > 0)
    ext = ext32.astype(np.float64)
    if not act.any():
        return G
    ext_max = ext[act].max()
    ratio = np.where(act, ext / ext_max, 0.0)

    def cells_at(s):
        g = np.where(act, np.clip(np.ceil(ratio * np.float64(s)), 1, MAX_AXIS), 1).astype(np.int64)
        return g, int(g[0]) * int(g[1]) * int(g[2])

    s = max(t for t in range(1, MAX_AXIS + 1) if cells_at(t)[1] <= want)       # (one cell, s = 1, is always allowed)
    g, _ = cells_at(s)
    min_h = F(0)
    for a in range(3):
        if g[a] <= 1:
            continue
        ih = np.float64(g[a]) / ext[a]
        if not (1e-30 <= ih <= 3e38):
            continue
        G["g"][a] = g[a]
        G["inv_h"][a] = F(ih)
        h = F(1.0) / G["inv_h"][a]
        min_h = h if (min_h == 0 or h < min_h) else min_h
    G["min_h"] = F(min_h)
    G["cells"] = int(np.prod(G["g"]))
    return G


def grid_of(ref, target):
    ref = np.asarray(ref, dtype=F).reshape(-1, 3)
    fin = ref[finite_rows(ref)]
    if fin.shape[0] == 0:
        return make_grid(0, np.zeros(3), np.zeros(3), target)
    return make_grid(fin.shape[0], fin.min(0), fin.max(0), target)


def words(G):
    """The 12 words of the header's Grid record."""
    out = np.zeros(12, np.uint32)
    out[0:3] = G["lo"].view(np.uint32)
    out[3:6] = G["inv_h"].view(np.uint32)
    out[6:9] = G["g"].astype(np.uint32)
    out[9] = np.array([G["min_h"]], F).view(np.uint32)[0]
    out[10], out[11] = G["m"], G["cells"]
    return out


def cells(G, p):
    """p [N,3] finite fp32 -> per-axis cells [N,3]"""
    p = np.asarray(p, dtype=F).reshape(-1, 3)
    out = np.zeros(p.shape, np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            g = int(G["g"][a])
            if g <= 1:
                continue
            t = np.floor(((p[:, a] - G["lo"][a]).astype(F) * G["inv_h"][a]).astype(F))
            out[:, a] = np.where(t >= F(g - 1), g - 1, np.where(t > 0, np.minimum(t, F(g - 1)), 0)).astype(np.int64)
    return out


def bound2(r, min_h):
    with np.errstate(all="ignore"):
        b = ((np.asarray(r).astype(F) * F(min_h)).astype(F) * SLACK).astype(F)
        b2 = (b * b).astype(F)
    return np.where(b2 >= B2_MIN, np.minimum(b2, B2_MAX), F(0)).astype(F)


def search(query, ref, k, target):
    """One cloud pair by the ring walk -> (idx int32 [Nq,k], d2 fp32 [Nq,k]); -1 / +inf where nothing fills a slot."""
    query, ref = np.asarray(query, dtype=F).reshape(-1, 3), np.asarray(ref, dtype=F).reshape(-1, 3)
    G = grid_of(ref, target)
    ids = np.nonzero(finite_rows(ref))[0]
    rc = cells(G, ref[ids])
    qc = cells(G, np.where(np.isfinite(query), query, 0))
    idx = np.full((query.shape[0], k), -1, np.int32)
    d2 = np.full((query.shape[0], k), np.inf, F)
    for q in range(query.shape[0]):
        if not np.isfinite(query[q]).all():
            continue
        cheb = np.abs(rc - qc[q]).max(1) if ids.size else np.zeros(0, np.int64)
        rmax = int(np.maximum(qc[q], G["g"] - 1 - qc[q]).max())
        kd, ki = np.zeros(0, F), np.zeros(0, np.int64)
        for r in range(rmax + 1):
            ring = ids[cheb == r]
            d = dist2(query[q], ref[ring])
            keep = d < np.inf
            kd, ki = np.concatenate([kd, d[keep]]), np.concatenate([ki, ring[keep]])
            order = np.lexsort((ki, kd.view(np.uint32)))[:k]
            kd, ki = kd[order], ki[order]
            if kd.size == k and kd[-1] < bound2(r, G["min_h"]):
                break
        idx[q, :kd.size], d2[q, :kd.size] = ki, kd
    return idx, d2
