"""Numpy restatement of the rules of deltaconv_amd/csrc/pool_vectors_math.h, written from the rules and not from the header: the
rotation table of a two-set search (``table``), the pooling of tangent-vector features over it (``forward``: values, ``arg`` and
``cnt``) and its gradient w.r.t. the values over the transposed lists (``backward``), op by op in fp32 -- and an fp64 form of
both (``forward64`` / ``backward64``) written another way (a dense [Nq,k,C] gather with argmax / sum, and an unordered
scatter-add), which is what the fp32 results are held to.  tests/test_pool_vectors_host.py holds the restatement to a g++ build
of the header bit for bit and to the fp64 form; tests/test_gpu_pool_vectors.py holds the kernels of csrc/pool_vectors.hip to it.

The rules: a slot is valid iff 0 <= idx < nr.  Table entry q*k + s = transport(target frame of q, source frame of rptr[b] + idx)
(tests/connection_restate.transport, itself held to the reference's connection), zeros for invalid slots and rows in no pair.
sum: au = av = 0, valid slots in order, au = (au + R00*v0) + R01*v1, av = (av + R10*v0) + R11*v1.  mean: the sum, one division by
(float)cnt.  max, per channel: key v0*v0 + v1*v1; the first valid slot is taken, a later one iff its key is strictly larger (a
later NaN never, a first NaN stays); the value is (R00*v0 + R01*v1, R10*v0 + R11*v1) of the winner, arg its slot.  No valid slot:
zeros, arg 255, cnt 0.  Backward: per source row its in-edges in ascending e = q*k + s from du = dw = 0,
du = (du + R00*g0) + R10*g1, dw = (dw + R01*g0) + R11*g1 -- always (sum), with g0, g1 first divided by (float)cnt[q] (mean), or iff
arg[q] == s (max; a loser adds nothing).  Every product, sum and quotient is rounded on its own.

The ragged clouds and searches are those of tests/interp_grad_restate.py (a reference cloud smaller than k, an empty pair, query
clouds of more than 256 rows, one in-edge list of about 2 100); the frames are random unit normals with build_tangent_basis frames."""
import numpy as np

from tests import connection_restate as CR
from tests import vector_interp_restate as V
from tests.interp_grad_restate import PAIRS, ragged_clouds, ragged_lists, ragged_search  # noqa: F401  (shared with the tests)

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
MODES = {"max": 0, "sum": 2, "mean": 3}
MODE_CODES = (0, 2, 3)
NO_ARG = 255
KS = (1, 3, 16)
CHANNELS = (1, 3, 4, 6, 64)
WIDTH = 64            # a channel never looks at its neighbours: every case is restated ONCE at WIDTH channels
_cache = {}


def slots(idx, qptr, rptr):
    """-> (ok bool [Nq,k]; src int64 [Nq,k] ABSOLUTE source row, 0 where invalid).  Rows outside every pair have no valid slot."""
    ok, src = np.zeros(idx.shape, dtype=bool), np.zeros(idx.shape, dtype=np.int64)
    for b in range(len(qptr) - 1):
        s = slice(int(qptr[b]), int(qptr[b + 1]))
        ok[s] = (idx[s] >= 0) & (idx[s] < int(rptr[b + 1] - rptr[b]))
        src[s] = np.where(ok[s], int(rptr[b]) + idx[s].astype(np.int64), 0)
    return ok, src


def table(idx, qptr, rptr, tframes, sframes, non_oriented=True, dtype=F32):
    """-> R [Nq*k, 4]: the transport alone; four +0 for an invalid slot and for a row outside every pair."""
    ok, src = slots(idx, qptr, rptr)
    return V.connection(ok, src, tframes, sframes, non_oriented, dtype).reshape(-1, 4)


def forward(v, idx, qptr, rptr, rmat, mode, dtype=F32):
    """v [2 Nr, C] -> (out [2 Nq, C] `dtype`, arg uint8 [Nq, C] -- 255 everywhere for sum / mean --, cnt uint8 [Nq])."""
    v = np.asarray(v).astype(dtype)
    nq, k = idx.shape
    c = v.shape[1]
    ok, src = slots(idx, qptr, rptr)
    R = np.asarray(rmat).astype(dtype).reshape(nq, k, 4)
    v0, v1 = v[0::2], v[1::2]
    au, av, key = (np.zeros((nq, c), dtype=dtype) for _ in range(3))
    at, n = np.full((nq, c), NO_ARG, dtype=np.uint8), np.zeros(nq, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(k):
            q = np.nonzero(ok[:, s])[0]
            if not len(q):
                continue
            a, b = v0[src[q, s]], v1[src[q, s]]
            r00, r01, r10, r11 = (R[q, s, i, None] for i in range(4))
            if mode == 0:
                norm = a * a + b * b
                take = (n[q] == 0)[:, None] | (norm > key[q])
                key[q] = np.where(take, norm, key[q])
                au[q] = np.where(take, r00 * a + r01 * b, au[q])
                av[q] = np.where(take, r10 * a + r11 * b, av[q])
                at[q] = np.where(take, np.uint8(s), at[q])
            else:
                au[q] = (au[q] + r00 * a) + r01 * b
                av[q] = (av[q] + r10 * a) + r11 * b
            n[q] += 1
        if mode == 3:
            div = np.maximum(n, 1).astype(dtype)[:, None]
            au, av = np.where((n > 0)[:, None], au / div, au), np.where((n > 0)[:, None], av / div, av)
    out = np.zeros((2 * nq, c), dtype=dtype)
    out[0::2], out[1::2] = au, av
    return out, at, n.astype(np.uint8)


def backward(g, tptr, tedge, rmat, k, mode, arg, cnt, dtype=F32):
    """g [2 rows, C] -> dv [2 num_ref, C]: per source row the sequential sum over its list, in list order; the p-th in-edge of
    every row in one vector step.  An edge whose query row falls outside g is skipped."""
    g = np.asarray(g).astype(dtype)
    M = np.asarray(rmat).astype(dtype).reshape(-1, 4)
    g0, g1 = g[0::2], g[1::2]
    num_ref, c = len(tptr) - 1, g.shape[1]
    du, dw = np.zeros((num_ref, c), dtype=dtype), np.zeros((num_ref, c), dtype=dtype)
    length = np.diff(tptr)
    by_length = np.argsort(-length, kind="stable")
    qs = tedge // k
    ss = tedge - qs * k
    inside = (qs >= 0) & (qs < g0.shape[0])
    with np.errstate(all="ignore"):
        for p in range(int(length.max()) if num_ref else 0):
            live = by_length[:int((length > p).sum())]
            t = tptr[live] + p
            live, t = live[inside[t]], t[inside[t]]
            m, q = M[tedge[t]], qs[t]
            a, b = g0[q], g1[q]
            if mode == 3:
                div = cnt[q].astype(dtype)[:, None]
                a, b = (a / div).astype(dtype), (b / div).astype(dtype)
            nu = (du[live] + m[:, 0, None] * a) + m[:, 2, None] * b
            nw = (dw[live] + m[:, 1, None] * a) + m[:, 3, None] * b
            if mode == 0:
                hit = arg[q] == ss[t][:, None].astype(np.uint8)
                nu, nw = np.where(hit, nu, du[live]), np.where(hit, nw, dw[live])
            du[live], dw[live] = nu, nw
    dv = np.zeros((2 * num_ref, c), dtype=dtype)
    dv[0::2], dv[1::2] = du, dw
    return dv


# ---- the fp64 forms, written densely ---------------------------------------------------------------------------------------------------
def transported64(v, idx, qptr, rptr, rmat):
    """-> (tu, tv [Nq,k,C] the transported coefficients of every slot in fp64 from the fp32 inputs; su, sv [Nq,k,C] the magnitudes
    |R00 v0| + |R01 v1| and |R10 v0| + |R11 v1|; key [Nq,k,C] the exact squared norms; ok [Nq,k])."""
    v64 = np.asarray(v, dtype=F32).astype(F64)
    nq, k = idx.shape
    ok, src = slots(idx, qptr, rptr)
    R = np.asarray(rmat, dtype=F32).astype(F64).reshape(nq, k, 4, 1)
    a, b = v64[0::2][src], v64[1::2][src]
    live = ok[:, :, None]
    tu, tv = R[:, :, 0] * a + R[:, :, 1] * b, R[:, :, 2] * a + R[:, :, 3] * b
    su, sv = np.abs(R[:, :, 0] * a) + np.abs(R[:, :, 1] * b), np.abs(R[:, :, 2] * a) + np.abs(R[:, :, 3] * b)
    z = lambda x: np.where(live, x, 0.0)
    return z(tu), z(tv), z(su), z(sv), np.where(live, a * a + b * b, -np.inf), ok


def forward64(v, idx, qptr, rptr, rmat, mode, arg=None):
    """-> (out64 [2 Nq,C], arg [Nq,C] (the LOWEST slot of the largest exact key; 255 without a valid slot and for sum / mean),
    cnt [Nq], mag [2 Nq,C]: the S of the bounds -- the sum over the valid slots for sum / mean, the chosen slot's for max).
    ``arg`` given: max evaluates THAT selection (the value bound is about the transport of the chosen slot)."""
    tu, tv, su, sv, key, ok = transported64(v, idx, qptr, rptr, rmat)
    nq, k, c = tu.shape
    cnt = ok.sum(axis=1)
    at = np.full((nq, c), NO_ARG, dtype=np.uint8)
    if mode == 0:
        pick = key.argmax(axis=1) if arg is None else np.where(arg == NO_ARG, 0, arg).astype(np.int64)
        take = lambda x: np.take_along_axis(x, pick[:, None, :], axis=1)[:, 0, :]
        ou, ov, mu, mv = take(tu), take(tv), take(su), take(sv)
        at[cnt > 0] = pick[cnt > 0].astype(np.uint8)
    else:
        ou, ov, mu, mv = tu.sum(axis=1), tv.sum(axis=1), su.sum(axis=1), sv.sum(axis=1)
        if mode == 3:
            ou, ov = ou / np.maximum(cnt, 1)[:, None], ov / np.maximum(cnt, 1)[:, None]
    some = (cnt > 0)[:, None]
    out, mag = np.zeros((2 * nq, c)), np.zeros((2 * nq, c))
    out[0::2], out[1::2] = np.where(some, ou, 0.0), np.where(some, ov, 0.0)
    mag[0::2], mag[1::2] = np.where(some, mu, 0.0), np.where(some, mv, 0.0)
    return out, at, cnt.astype(np.uint8), mag


def backward64(g, idx, qptr, rptr, rmat, mode, arg, cnt, num_ref):
    """The fp64 gradient as an unordered scatter-add over the valid slots -> (dv64 [2 num_ref,C], T [2 num_ref,C] the sum of
    |R00 g0| + |R10 g1| (|R01 g0| + |R11 g1|) over the terms added, L [num_ref,C] the number of terms added)."""
    g64 = np.asarray(g, dtype=F32).astype(F64)
    nq, k = idx.shape
    ok, src = slots(idx, qptr, rptr)
    R = np.asarray(rmat, dtype=F32).astype(F64).reshape(nq, k, 4)
    c = g64.shape[1]
    du, dw, tu, tw = (np.zeros((num_ref, c)) for _ in range(4))
    terms = np.zeros((num_ref, c), dtype=np.int64)
    for s in range(k):
        q = np.nonzero(ok[:, s])[0]
        if not len(q):
            continue
        w = (arg[q] == s).astype(F64) if mode == 0 else np.ones((len(q), c))
        if mode == 3:
            w = w / cnt[q].astype(F64)[:, None]
        a, b = w * g64[0::2][q], w * g64[1::2][q]
        r = R[q, s]
        j = src[q, s]
        np.add.at(du, j, r[:, 0, None] * a + r[:, 2, None] * b)
        np.add.at(dw, j, r[:, 1, None] * a + r[:, 3, None] * b)
        np.add.at(tu, j, np.abs(r[:, 0, None] * a) + np.abs(r[:, 2, None] * b))
        np.add.at(tw, j, np.abs(r[:, 1, None] * a) + np.abs(r[:, 3, None] * b))
        np.add.at(terms, j, (w != 0).astype(np.int64))
    dv, mag = np.zeros((2 * num_ref, c)), np.zeros((2 * num_ref, c))
    dv[0::2], dv[1::2], mag[0::2], mag[1::2] = du, dw, tu, tw
    return dv, mag, terms


def forward_bound(mode, cnt, mag):
    """|out - out64| per entry (csrc/pool_vectors_math.h): sum 2 cnt u S; mean (2 cnt + 1) u S / cnt; max 3 u S of the chosen slot."""
    n = np.repeat(cnt.astype(F64), 2)[:, None]
    if mode == 0:
        return 3 * EPS * mag
    return 2 * n * EPS * mag if mode == 2 else (2 * n + 1) * EPS * mag / np.maximum(n, 1)


def backward_bound(mode, mag, terms):
    """2 L u T for sum and max, (2 L + 1) u T for mean (one more rounding per term: the quotient)."""
    L = np.repeat(terms, 2, axis=0).astype(F64)
    return (2 * L + (1 if mode == 3 else 0)) * EPS * mag


# ---- the ragged call the test files run -----------------------------------------------------------------------------------------------
def _frames(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3)).astype(F32)
    nrm = (nrm / CR.norm3(nrm)[:, None]).astype(F32)
    xb, yb = CR.tangent_basis(nrm)
    return nrm, xb, yb


def ragged_frames():
    """-> (query frames, reference frames) of the ragged call: (normal, x_basis, y_basis) fp32 each; normals on both hemispheres,
    so the non_oriented reflection is taken on about half of the slots."""
    if "frames" not in _cache:
        _, qptr, _, rptr = ragged_clouds()
        _cache["frames"] = (_frames(int(qptr[-1]), 501), _frames(int(rptr[-1]), 502))
    return _cache["frames"]


def ragged_table(k, non_oriented=True):
    if ("table", k, non_oriented) not in _cache:
        _, qptr, _, rptr = ragged_clouds()
        tf, sf = ragged_frames()
        _cache["table", k, non_oriented] = table(ragged_search(k)[0], qptr, rptr, tf, sf, non_oriented)
    return _cache["table", k, non_oriented]


def ragged_values(kind="ties"):
    """v [2 Nr, WIDTH] over the reference rows of the ragged call.  "ties": multiples of 0.25 in about [-4, 4] -- every key
    v0^2 + v1^2 is exact in fp32 and equal keys among a query's neighbours are common; "gauss": 3 * standard normal."""
    n = int(ragged_clouds()[3][-1])
    rng = np.random.default_rng(300)
    if kind == "ties":
        return (np.round(rng.standard_normal((2 * n, WIDTH)) * 4) / 4).astype(F32)
    return (rng.standard_normal((2 * n, WIDTH)) * 3).astype(F32)


def ragged_gradient():
    qptr = ragged_clouds()[1]
    return (np.random.default_rng(400).standard_normal((2 * int(qptr[-1]), WIDTH)) * 10).astype(F32)


def ragged_case(k, mode, kind="ties"):
    """-> (v, g, rmat, out, arg, cnt, dv) of the ragged call at WIDTH channels, restated once per case."""
    key = ("case", k, mode, kind)
    if key not in _cache:
        _, qptr, _, rptr = ragged_clouds()
        idx, _ = ragged_search(k)
        tptr, tedge, _ = ragged_lists(k)
        v, g, rmat = ragged_values(kind), ragged_gradient(), ragged_table(k)
        out, arg, cnt = forward(v, idx, qptr, rptr, rmat, mode)
        _cache[key] = (v, g, rmat, out, arg, cnt, backward(g, tptr, tedge, rmat, k, mode, arg, cnt))
    return _cache[key]
