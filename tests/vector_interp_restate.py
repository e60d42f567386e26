"""Numpy restatement of deltaconv_amd/csrc/interp_transport_math.h: the table of per-slot matrices ``M = c * R`` of a two-set
search, the transported interpolation over it and its transpose, op by op.  Built from the existing restatements: the connection is
``tests/connection_restate.transport``, the coefficient the weight / ``den`` order of tests/interp_restate.py as
``tests/interp_grad_restate.coefficients`` states it, the lists ``tests/interp_grad_restate.transpose``.  ``dtype=np.float32`` is the
bit-for-bit twin of the g++ build (tests/hostcheck_vector_interp) and of the kernels (csrc/interp_transport.hip); ``np.float64`` is
the same formulas in fp64 from the fp32 search result, the yardstick of the bounds."""
import numpy as np

from tests import connection_restate as CR
from tests import interp_grad_restate as G
from tests import interp_restate as IR

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24


def slots(idx, d2, qptr, rptr, dtype=F32):
    """-> (coef [Nq,k] in `dtype`, 0 where invalid; ok bool [Nq,k]; src int64 [Nq,k] ABSOLUTE source row, 0 where invalid).  Rows
    outside every pair have no valid slot."""
    nq, k = idx.shape
    coef, ok, src = np.zeros((nq, k), dtype=dtype), np.zeros((nq, k), dtype=bool), np.zeros((nq, k), dtype=np.int64)
    for b in range(len(qptr) - 1):
        rows = slice(int(qptr[b]), int(qptr[b + 1]))
        c, good = G.coefficients(idx[rows], d2[rows], int(rptr[b + 1] - rptr[b]), dtype)
        coef[rows], ok[rows] = c, good
        src[rows] = np.where(good, int(rptr[b]) + idx[rows].astype(np.int64), 0)
    return coef, ok, src


def connection(ok, src, tframes, sframes, non_oriented=True, dtype=F32, details=False):
    """R [Nq,k,4] of every valid slot (zeros elsewhere): transport(target frame of q, source frame of src[q,s])."""
    nq, k = ok.shape
    tn, tx, ty = (np.asarray(a) for a in tframes[:3])
    sn, sx = (np.asarray(a) for a in sframes[:2])
    q, s = np.nonzero(ok)
    R = np.zeros((nq, k, 4), dtype=dtype)
    j = src[q, s]
    res = CR.transport(tn[q], tx[q], ty[q], sn[j], sx[j], non_oriented, dtype, details=details)
    R[q, s] = res[0] if details else res
    return (R, res[1], (q, s)) if details else R


def table(idx, d2, qptr, rptr, tframes, sframes, non_oriented=True, dtype=F32):
    """-> M [Nq*k, 4]: c * R, one product per entry; four +0 for an invalid slot and for a row outside every pair."""
    coef, ok, src = slots(idx, d2, qptr, rptr, dtype)
    R = connection(ok, src, tframes, sframes, non_oriented, dtype)
    M = (coef[:, :, None] * R).astype(dtype)
    M[~ok] = 0
    return M.reshape(-1, 4)


def forward(v, idx, d2, qptr, rptr, tmat, dtype=F32):
    """v [2 Nr, C] -> out [2 Nq, C]: slots in order, invalid ones skipped, au = (au + M00*v0) + M01*v1, av = (av + M10*v0) + M11*v1."""
    v = np.asarray(v).astype(dtype)
    nq, k = idx.shape
    _, ok, src = slots(idx, d2, qptr, rptr, dtype)
    M = np.asarray(tmat).astype(dtype).reshape(nq, k, 4)
    v0, v1 = v[0::2], v[1::2]
    au, av = np.zeros((nq, v.shape[1]), dtype=dtype), np.zeros((nq, v.shape[1]), dtype=dtype)
    for s in range(k):
        q = np.nonzero(ok[:, s])[0]
        j = src[q, s]
        au[q] = (au[q] + M[q, s, 0, None] * v0[j]) + M[q, s, 1, None] * v1[j]
        av[q] = (av[q] + M[q, s, 2, None] * v0[j]) + M[q, s, 3, None] * v1[j]
    out = np.zeros((2 * nq, v.shape[1]), dtype=dtype)
    out[0::2], out[1::2] = au, av
    return out


def backward(g, tptr, tedge, tmat, k, edge_base=0, dtype=F32):
    """g [2 rows, C] -> dv [2 num_ref, C]: per source row its in-edges in list order, du = (du + M00*g0) + M10*g1,
    dw = (dw + M01*g0) + M11*g1 with M = tmat[e - edge_base*k], g0 / g1 rows 2 (e // k - edge_base) and the next; an edge whose row
    falls outside g or whose entry falls outside tmat is skipped."""
    g = np.asarray(g).astype(dtype)
    M = np.asarray(tmat).astype(dtype).reshape(-1, 4)
    g0, g1 = g[0::2], g[1::2]
    num_ref = len(tptr) - 1
    du, dw = np.zeros((num_ref, g.shape[1]), dtype=dtype), np.zeros((num_ref, g.shape[1]), dtype=dtype)
    length = np.diff(tptr)
    by_length = np.argsort(-length, kind="stable")
    rows, at = tedge // k - edge_base, tedge - edge_base * k
    inside = (rows >= 0) & (rows < g0.shape[0]) & (at >= 0) & (at < M.shape[0])
    for p in range(int(length.max()) if num_ref else 0):
        live = by_length[:int((length > p).sum())]
        t = tptr[live] + p
        live, t = live[inside[t]], t[inside[t]]
        m, i = M[at[t]], rows[t]
        du[live] = (du[live] + m[:, 0, None] * g0[i]) + m[:, 2, None] * g1[i]
        dw[live] = (dw[live] + m[:, 1, None] * g0[i]) + m[:, 3, None] * g1[i]
    dv = np.zeros((2 * num_ref, g.shape[1]), dtype=dtype)
    dv[0::2], dv[1::2] = du, dw
    return dv


def lists(idx, d2, qptr, rptr, num_ref):
    """(tptr, tedge) of the search: the lists of dc_knn_cross_transpose (its tcoef is not needed)."""
    tptr, tedge, _ = G.transpose(idx, d2, qptr, rptr, num_ref)
    return tptr, tedge


# ---- shared inputs of the host and the device tests ---------------------------------------------------------------------------
SETS = ((1, 2048, 256, 3), (2, 1500, 64, 5), (3, 700, 700, 1), (4, 513, 40, 16))      # (seed, target rows, source rows, k)
# ragged batches (target sizes, source sizes) at k = 3: the last pair of the first has invalid slots and its boundaries fall inside
# a 256-chunk; the second has an empty query cloud between two non-empty ones
BATCHES = {"three_pairs": ((300, 1, 257), (40, 1, 2)), "empty_middle": ((300, 0, 257), (40, 7, 2))}
_cache = {}


def input_set(seed, nt, ns, k):
    """One pair: the target a bumpy sphere (connection_restate.cloud), the source a sorted random subset of it with the SAME frames
    -> dict(pos_t, tframes, pos_s, sframes, keep, qptr, rptr, idx, d2, k)."""
    key = ("set", seed, nt, ns, k)
    if key not in _cache:
        pos, nrm, xb, yb = CR.cloud(nt, seed)
        keep = np.sort(np.random.default_rng(1000 + seed).permutation(nt)[:ns])
        qptr, rptr = np.array([0, nt], dtype=np.int64), np.array([0, ns], dtype=np.int64)
        idx, d2 = IR.knn_cross_batched(pos, qptr, pos[keep], rptr, k)
        _cache[key] = dict(pos_t=pos, tframes=(nrm, xb, yb), pos_s=pos[keep], sframes=(nrm[keep], xb[keep], yb[keep]), keep=keep,
                           qptr=qptr, rptr=rptr, idx=idx, d2=d2, k=k)
    return _cache[key]


def batch_set(name, k=3, seed=7):
    """A ragged batch of BATCHES: every pair a cloud of its own, the source a sorted random subset of the target where it is smaller,
    the whole target otherwise."""
    key = ("batch", name, k, seed)
    if key not in _cache:
        tsizes, ssizes = BATCHES[name]
        rng = np.random.default_rng(seed)
        parts_t, parts_s = [], []
        for b, (nt, ns) in enumerate(zip(tsizes, ssizes)):
            big = CR.cloud(max(nt, ns), 100 * seed + b)
            tsel = np.arange(nt)
            ssel = np.sort(rng.permutation(max(nt, ns))[:ns])
            parts_t.append([a[tsel] for a in big])
            parts_s.append([a[ssel] for a in big])
        cat = lambda parts, i: np.concatenate([p[i] for p in parts]).astype(F32)
        qptr = np.concatenate([[0], np.cumsum(tsizes)]).astype(np.int64)
        rptr = np.concatenate([[0], np.cumsum(ssizes)]).astype(np.int64)
        pos_t, pos_s = cat(parts_t, 0), cat(parts_s, 0)
        idx, d2 = IR.knn_cross_batched(pos_t, qptr, pos_s, rptr, k)
        _cache[key] = dict(pos_t=pos_t, tframes=tuple(cat(parts_t, i) for i in (1, 2, 3)), pos_s=pos_s,
                           sframes=tuple(cat(parts_s, i) for i in (1, 2, 3)), qptr=qptr, rptr=rptr, idx=idx, d2=d2, k=k)
    return _cache[key]


def hub_set():
    """One pair at k = 2: 14 targets crowd around sources 0 and 1, sources 2 and 3 lie far away -- two in-lists of 14 entries (more
    than the backward keeps in flight) with true divisions, and two source rows without any in-edge."""
    if "hub" not in _cache:
        rng = np.random.default_rng(5)
        _, tn, tx, ty = CR.cloud(14, 31)
        _, sn, sx, sy = CR.cloud(4, 32)
        pos_t = (rng.random((14, 3), dtype=F32) * F32(0.05)).astype(F32)
        pos_s = np.array([[0, 0, 0], [0.1, 0, 0], [50, 0, 0], [0, 50, 0]], dtype=F32)
        qptr, rptr = np.array([0, 14], dtype=np.int64), np.array([0, 4], dtype=np.int64)
        idx, d2 = IR.knn_cross_batched(pos_t, qptr, pos_s, rptr, 2)
        _cache["hub"] = dict(pos_t=pos_t, tframes=(tn, tx, ty), pos_s=pos_s, sframes=(sn, sx, sy), qptr=qptr, rptr=rptr, idx=idx,
                             d2=d2, k=2)
    return _cache["hub"]


def values(rows, c, seed):
    return (np.random.default_rng(seed).standard_normal((rows, c)) * 3).astype(F32)
