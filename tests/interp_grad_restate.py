"""Numpy restatement of the backward rules of deltaconv_amd/csrc/interp_math.h (coef / pick / bwd4): the coefficient of every
slot, the transposed lists of a two-set search (the in-edges of every reference row in ascending edge id) and the ordered sum
``dx = dx + c_e * g_e``, op by op in fp32 -- or, with ``dtype=np.float64``, the SAME lists and sum in fp64 from the fp32 search
result, which is what the fp32 result is held to.  tests/test_interp_grad_host.py holds it to a g++ build of the header bit for
bit and to fp64; tests/test_gpu_interp_grad.py holds the kernels of csrc/interp.hip to it bit for bit.

There is no gradient for positions or distances: the weights are constants of the backward."""
import numpy as np

F32 = np.float32
D2_CLAMP = np.float32(1e-16)
EPS = 2.0 ** -24


def coefficients(idx, d2, nr, dtype=F32):
    """One cloud pair: idx / d2 [Nq,k], nr reference points -> (coef [Nq,k], 0 where the slot is invalid; valid bool [Nq,k]).
    Slots in order: w_s = 1 / fmax(d2_s, 1e-16), den = den + w_s (each rounded); ONE valid slot: 1; otherwise w_s / den."""
    idx, d2 = np.asarray(idx), np.asarray(d2, dtype=F32)
    nq, k = idx.shape
    ok = (idx >= 0) & (idx < nr)
    den, w = np.zeros(nq, dtype=dtype), np.zeros((nq, k), dtype=dtype)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for s in range(k):
            ws = (one / np.fmax(d2[:, s], D2_CLAMP).astype(dtype)).astype(dtype)
            w[:, s] = np.where(ok[:, s], ws, 0)
            den = np.where(ok[:, s], (den + ws).astype(dtype), den)
        n = ok.sum(axis=1)
        c = (w / np.where(n > 1, den, one)[:, None]).astype(dtype)
    c[(n == 1)[:, None] & ok] = one
    c[~ok] = 0
    return c, ok


def transpose(idx, d2, qptr, rptr, num_ref, dtype=F32):
    """-> (tptr int64 [num_ref+1], tedge int64 [valid slots], tcoef [valid slots]): the in-edges e = q * k + s (q the ABSOLUTE
    query row) of every ABSOLUTE reference row, ascending within each list."""
    k = idx.shape[1]
    es, rs, cs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=dtype)]
    for b in range(len(qptr) - 1):
        rows = slice(int(qptr[b]), int(qptr[b + 1]))
        c, ok = coefficients(idx[rows], d2[rows], int(rptr[b + 1] - rptr[b]), dtype)
        q, s = np.nonzero(ok)
        es.append((int(qptr[b]) + q.astype(np.int64)) * k + s)
        rs.append(int(rptr[b]) + idx[rows][q, s].astype(np.int64))
        cs.append(c[q, s])
    e, r, c = np.concatenate(es), np.concatenate(rs), np.concatenate(cs)
    order = np.lexsort((e, r))
    tptr = np.zeros(num_ref + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(r, minlength=num_ref))
    return tptr, e[order], c[order].astype(dtype)


def backward(g, tptr, tedge, tcoef, k, edge_base=0, dtype=F32):
    """g [rows, C] -> dx [num_ref, C]: per reference row the sequential sum over its list, ``dx = dx + c_e * g[e // k - edge_base]``,
    the product and the sum each rounded to `dtype`; an edge whose row falls outside g is skipped."""
    g = np.asarray(g).astype(dtype)
    num_ref = len(tptr) - 1
    dx = np.zeros((num_ref, g.shape[1]), dtype=dtype)
    length = np.diff(tptr)
    by_length = np.argsort(-length, kind="stable")
    rows = tedge // k - edge_base
    inside = (rows >= 0) & (rows < g.shape[0])
    for p in range(int(length.max()) if num_ref else 0):
        live = by_length[:int((length > p).sum())]
        t = tptr[live] + p
        live, t = live[inside[t]], t[inside[t]]
        prod = (tcoef[t].astype(dtype)[:, None] * g[rows[t]]).astype(dtype)
        dx[live] = (dx[live] + prod).astype(dtype)
    return dx


def bound(g, tptr, tedge, tcoef64, k, edge_base=0):
    """(L_j + k + 8) * 2^-24 * sum_e |c_e| |g_e| per entry of dx, the sum formed in fp64: the first-order bound of an L-term
    sequential sum whose coefficients come from at most k positive additions and two divisions; 8 covers the second order."""
    mag = backward(np.abs(np.asarray(g, dtype=np.float64)), tptr, tedge, np.abs(tcoef64), k, edge_base, np.float64)
    return (np.diff(tptr) + k + 8)[:, None] * EPS * mag


# ---- the ragged call both test files run -------------------------------------------------------------------------------------
# (query points, reference points): the ragged set of tests/test_gpu_interp.py, then one list of 2 100 entries (a one-point
# reference cloud: past every 64- and 256-wide seam of the ranking and of the sum, every coefficient 1) and two lists of about
# 65 k entries with true divisions
PAIRS = [(700, 2049), (257, 2048), (256, 5), (1, 1), (0, 300), (40, 0), (2100, 1), (130, 2)]
KS = (1, 3, 8, 16)
CHANNELS = (1, 3, 50, 64, 65)
_cache = {}


def ragged_clouds():
    """-> (query [Nq,3], qptr, ref [Nr,3], rptr) of PAIRS: uniform in the unit cube; pair 0 has 40 duplicated reference points and
    one query equal to a reference point (ties: the lower id takes the in-edge)."""
    if "clouds" not in _cache:
        rng = np.random.default_rng(0)
        qptr = np.concatenate([[0], np.cumsum([p[0] for p in PAIRS])]).astype(np.int64)
        rptr = np.concatenate([[0], np.cumsum([p[1] for p in PAIRS])]).astype(np.int64)
        qry, ref = rng.random((qptr[-1], 3), dtype=np.float32), rng.random((rptr[-1], 3), dtype=np.float32)
        ref[100:140] = ref[0:40]
        qry[5] = ref[17]
        _cache["clouds"] = (qry, qptr, ref, rptr)
    return _cache["clouds"]


def ragged_search(k):
    """The restated search of the ragged call (tests/interp_restate.py), once per k."""
    from tests import interp_restate as R
    if ("search", k) not in _cache:
        qry, qptr, ref, rptr = ragged_clouds()
        _cache["search", k] = R.knn_cross_batched(qry, qptr, ref, rptr, k)
    return _cache["search", k]


def ragged_lists(k, dtype=F32):
    """The restated transposed lists of the ragged call, once per (k, dtype)."""
    if ("lists", k, dtype) not in _cache:
        _, qptr, _, rptr = ragged_clouds()
        idx, d2 = ragged_search(k)
        _cache["lists", k, dtype] = transpose(idx, d2, qptr, rptr, int(rptr[-1]), dtype)
    return _cache["lists", k, dtype]


def ragged_gradient(c, seed=0):
    qptr = ragged_clouds()[1]
    return (np.random.default_rng(100 + c + seed).standard_normal((int(qptr[-1]), c)) * 10).astype(F32)
