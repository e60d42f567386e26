"""Numpy restatement of deltaconv_amd/csrc/pool_math.h: the pooling of scalar features over the slots of a two-set search
(``forward``: values, ``arg`` and ``cnt``) and its gradient w.r.t. the features over the transposed lists (``backward``), op by
op in fp32 -- and an fp64 form of both (``forward64`` / ``backward64``) written another way (a dense [Nq,k,C] gather with
argmax / argmin / sum, and an unordered scatter-add), which is what the fp32 results are held to.
tests/test_pool_host.py holds the restatement to a g++ build of the header bit for bit and to the fp64 form;
tests/test_gpu_pool.py holds the kernels of csrc/pool.hip to it bit for bit.

The rules (csrc/pool_math.h): a slot is valid iff 0 <= idx < nr; the FIRST valid slot is copied; max / min take a later slot iff
it is strictly larger / smaller (ties keep the earlier slot, a later NaN is never taken, a first NaN stays) and record the slot in
``arg``; sum / mean add the later slots in order, every addition rounded, mean divides once by ``(float)cnt``; no valid slot:
zeros, arg 255, cnt 0.  Backward: per reference row its in-edges in ascending ``e = q * k + s`` from dx = 0; max / min add
``g[q]`` iff ``arg[q] == s``, sum adds ``g[q]``, mean adds ``g[q] / (float)cnt[q]`` (rounded on its own).

The ragged clouds and searches are those of tests/interp_grad_restate.py (a reference cloud smaller than k, an empty pair, query
clouds of more than 256 rows)."""
import numpy as np

from tests.interp_grad_restate import KS, PAIRS, ragged_clouds, ragged_lists, ragged_search  # noqa: F401  (shared with the tests)

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
MODES = {"max": 0, "min": 1, "sum": 2, "mean": 3}
NO_ARG = 255
_cache = {}


def forward(x, qptr, rptr, idx, mode, dtype=F32):
    """x [Nr,C], idx [Nq,k] (local to the pair's reference cloud) -> (out [Nq,C] `dtype`, arg uint8 [Nq,C] -- 255 everywhere for
    sum / mean, which store none --, cnt uint8 [Nq]).  Rows outside every pair: zeros, 255, 0."""
    x = np.asarray(x).astype(dtype)
    nq, k = idx.shape
    c = x.shape[1]
    out, arg, cnt = np.zeros((nq, c), dtype=dtype), np.full((nq, c), NO_ARG, dtype=np.uint8), np.zeros(nq, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for b in range(len(qptr) - 1):
            q0, q1, r0, nr = int(qptr[b]), int(qptr[b + 1]), int(rptr[b]), int(rptr[b + 1] - rptr[b])
            if q1 <= q0:
                continue
            ids = idx[q0:q1]
            ok = (ids >= 0) & (ids < nr)
            acc, at, n = np.zeros((q1 - q0, c), dtype=dtype), np.full((q1 - q0, c), NO_ARG, dtype=np.uint8), np.zeros(q1 - q0, dtype=np.int64)
            for s in range(k):
                live = ok[:, s]
                if not live.any():
                    continue
                v = np.zeros_like(acc)
                v[live] = x[r0 + ids[live, s]]
                first = (live & (n == 0))[:, None]
                later = (live & (n > 0))[:, None]
                if mode <= 1:
                    take = first | (later & ((v > acc) if mode == 0 else (v < acc)))
                    acc = np.where(take, v, acc)
                    at = np.where(take, np.uint8(s), at)
                else:
                    acc = np.where(first, v, np.where(later, (acc + v).astype(dtype), acc))
                n += live
            if mode == 3:
                acc = np.where((n > 0)[:, None], (acc / np.maximum(n, 1).astype(dtype)[:, None]).astype(dtype), acc)
            out[q0:q1], arg[q0:q1], cnt[q0:q1] = acc, at, n
    return out, arg, cnt


def backward(g, tptr, tedge, k, mode, arg, cnt, dtype=F32):
    """g [rows,C] -> dx [num_ref,C]: per reference row the sequential sum over its list, in list order, of the terms of
    csrc/pool_math.h; an edge whose query row falls outside g is skipped, an edge that lost a max / min adds nothing (restated as
    adding -0.0, which leaves every value's bits as they are).  ``np.add.accumulate`` is the sequential sum, rounded per step."""
    g = np.asarray(g).astype(dtype)
    num_ref, c = len(tptr) - 1, g.shape[1]
    dx = np.zeros((num_ref, c), dtype=dtype)
    q = tedge // k
    s = tedge - q * k
    inside = (q >= 0) & (q < g.shape[0])
    for j in np.nonzero(np.diff(tptr))[0]:
        t = np.arange(tptr[j], tptr[j + 1])
        t = t[inside[t]]
        term = g[q[t]]
        if mode == 3:
            with np.errstate(all="ignore"):
                term = (term / cnt[q[t]].astype(dtype)[:, None]).astype(dtype)
        if mode <= 1:
            term = np.where(arg[q[t]] == s[t][:, None], term, dtype(-0.0))
        dx[j] = np.add.accumulate(np.concatenate([np.zeros((1, c), dtype=dtype), term]), axis=0, dtype=dtype)[-1]
    return dx


def _gathered(x, qptr, rptr, idx):
    """-> (rows int64 [Nq,k] absolute, 0 where invalid; ok bool [Nq,k])."""
    rows, ok = np.zeros(idx.shape, dtype=np.int64), np.zeros(idx.shape, dtype=bool)
    for b in range(len(qptr) - 1):
        s = slice(int(qptr[b]), int(qptr[b + 1]))
        ok[s] = (idx[s] >= 0) & (idx[s] < int(rptr[b + 1] - rptr[b]))
        rows[s] = np.where(ok[s], int(rptr[b]) + idx[s], 0)
    return rows, ok


def forward64(x, qptr, rptr, idx, mode):
    """The fp64 form on the SAME fp32 inputs, written densely: -> (out64 [Nq,C], arg [Nq,C] (the LOWEST slot that holds the
    extreme value; 255 without a valid slot and for sum / mean), cnt [Nq], sum over the valid slots of |x| [Nq,C])."""
    x64 = np.asarray(x, dtype=F32).astype(F64)
    rows, ok = _gathered(x, qptr, rptr, idx)
    cnt = ok.sum(axis=1)
    near = x64[rows] if x64.shape[0] else np.zeros(idx.shape + (x64.shape[1],))
    mag = np.where(ok[:, :, None], np.abs(near), 0.0).sum(axis=1)
    arg = np.full((idx.shape[0], x64.shape[1]), NO_ARG, dtype=np.uint8)
    if mode <= 1:
        pad = -np.inf if mode == 0 else np.inf
        masked = np.where(ok[:, :, None], near, pad)
        at = masked.argmax(axis=1) if mode == 0 else masked.argmin(axis=1)       # the first occurrence: the lowest slot
        out = np.take_along_axis(masked, at[:, None, :], axis=1)[:, 0, :]
        arg[cnt > 0] = at[cnt > 0].astype(np.uint8)
    else:
        out = np.where(ok[:, :, None], near, 0.0).sum(axis=1)
        if mode == 3:
            out = out / np.maximum(cnt, 1)[:, None]
    out = np.where((cnt > 0)[:, None], out, 0.0)
    return out, arg, cnt.astype(np.uint8), mag


def backward64(g, qptr, rptr, idx, mode, arg, cnt, num_ref):
    """The fp64 gradient as an unordered scatter-add over the valid slots -> (dx64 [num_ref,C], sum of |term| [num_ref,C], the
    number of terms added L [num_ref,C])."""
    g64 = np.asarray(g, dtype=F32).astype(F64)
    rows, ok = _gathered(g, qptr, rptr, idx)
    c = g64.shape[1]
    dx, mag, terms = np.zeros((num_ref, c)), np.zeros((num_ref, c)), np.zeros((num_ref, c), dtype=np.int64)
    for s in range(idx.shape[1]):
        live = ok[:, s]
        if not live.any():
            continue
        w = (arg[live] == s).astype(F64) if mode <= 1 else np.ones((int(live.sum()), c))
        if mode == 3:
            w = w / cnt[live].astype(F64)[:, None]
        np.add.at(dx, rows[live, s], w * g64[live])
        np.add.at(mag, rows[live, s], np.abs(w * g64[live]))
        np.add.at(terms, rows[live, s], (w != 0).astype(np.int64))
    return dx, mag, terms


def forward_bound(mode, cnt, mag):
    """|out - out64| per entry: nothing for a selection; sum: cnt * 2^-24 * sum|x_s| (at most cnt - 1 additions pass over a term);
    mean: (cnt + 1) * 2^-24 * sum|x_s| / cnt (the division and the second order on top)."""
    n = cnt.astype(F64)[:, None]
    if mode <= 1:
        return np.zeros_like(mag)
    return n * EPS * mag if mode == 2 else (n + 1) * EPS * mag / np.maximum(n, 1)


def backward_bound(mag, terms):
    """(L_j + 2) * 2^-24 * sum_e |term_e|: a term passes through at most L - 1 additions and one division; 2 covers the second
    order."""
    return (terms + 2) * EPS * mag


# ---- the ragged call the test files run ---------------------------------------------------------------------------------------------
# A channel never looks at its neighbours, so every case is restated ONCE at WIDTH channels and a test of C channels takes the
# first C columns of the inputs and of the results.
WIDTH = 67


def ragged_features(kind="ties"):
    """x [Nr, WIDTH] over the reference rows of the ragged call.  "ties": multiples of 0.25 in about [-4, 4], equal values among a
    query's neighbours on purpose; "distinct": every column a permutation of the multiples of 1/64, no two rows equal (a selection
    has ONE winner); "gauss": 10 * standard normal (sums that round)."""
    n = int(ragged_clouds()[3][-1])
    rng = np.random.default_rng(300)
    if kind == "ties":
        return (np.round(rng.standard_normal((n, WIDTH)) * 4) / 4).astype(F32)
    if kind == "distinct":
        return ((np.stack([rng.permutation(n) for _ in range(WIDTH)], axis=1) - n // 2) / 64).astype(F32)
    return (rng.standard_normal((n, WIDTH)) * 10).astype(F32)


def ragged_gradient():
    qptr = ragged_clouds()[1]
    return (np.random.default_rng(400).standard_normal((int(qptr[-1]), WIDTH)) * 10).astype(F32)


def ragged_case(k, mode, kind="ties"):
    """-> (x, g, out, arg, cnt, dx) of the ragged call at WIDTH channels, restated once per case."""
    key = (k, mode, kind)
    if key not in _cache:
        _, qptr, _, rptr = ragged_clouds()
        idx, _ = ragged_search(k)
        tptr, tedge, _ = ragged_lists(k)
        x, g = ragged_features(kind), ragged_gradient()
        out, arg, cnt = forward(x, qptr, rptr, idx, mode)
        _cache[key] = (x, g, out, arg, cnt, backward(g, tptr, tedge, k, mode, arg, cnt))
    return _cache[key]
