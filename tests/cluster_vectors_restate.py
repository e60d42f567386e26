"""numpy restatement of deltaconv_amd/csrc/cluster_vectors_math.h, written from the header's rules and not from its code: the two
per-point transport tables of a cluster vector (``table``), the pooling of tangent-vector features over the member lists
(``pool``: values and ``arg``), its backward (``pool_backward``, a gather), the un-pooling (``unpool``, a gather) and its backward
(``unpool_backward``, a walk).  ``dtype=np.float32`` rounds every product, sum and quotient on its own and gives the bits of the
g++ build (tests/test_cluster_vectors_host.py) and of the kernels (tests/test_gpu_cluster_vectors.py); ``dtype=np.float64`` is the
same formulas in fp64 on the fp32 inputs, the yardstick of the bounds.  Built on tests/connection_restate.transport (held to the
reference's connection) and the list helpers of tests/cluster_restate.py.

The rules: row i belongs to cell cl = cluster[i] iff 0 <= cl < m.  rdown[i] = transport(target: frame of cell cl, source: frame of
point i), rup[i] = transport(target: frame of point i, source: frame of cell cl), zeros without a cell.  Members in ascending row
order; one outside [0, n) is skipped and not counted.  sum: au = av = 0, au = (au + R00*v0) + R01*v1, av = (av + R10*v0) + R11*v1.
mean: the sum, one division by (float)cnt.  max, per channel: key v0*v0 + v1*v1; the first member is taken, a later one iff its
key is strictly larger (a later NaN never, a first NaN stays); the value is (R00*v0 + R01*v1, R10*v0 + R11*v1) of the winner, arg
its row.  Empty cell: zeros, arg -1.  Pool backward, per point: du = R00*g0 + R10*g1, dw = R01*g0 + R11*g1 -- always (sum), g0 / g1
first divided by (float)(cptr[cl+1] - cptr[cl]) (mean), where arg[cl] == i and +0 elsewhere (max).  Un-pooling: out = R x with R =
rup[i].  Its backward: per cell from 0 in member order du = (du + R00*g0) + R10*g1, dw = (dw + R01*g0) + R11*g1."""
import numpy as np

from tests import cluster_restate as CL
from tests import connection_restate as CR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
MODES = {"max": 0, "sum": 2, "mean": 3}
NO_ARG = -1
MARGIN = 1.0 - 2.0 ** -22             # the winner's exact key against the largest (the header's max rule)


def gamma(k):
    """k roundings of relative size u compound to at most k u / (1 - k u)."""
    k = np.asarray(k, dtype=F64)
    return k * U / (1.0 - k * U)


def table(cluster, m, fine, coarse, direction, non_oriented=True, dtype=F32):
    """fine = (normal, x, y) [n,3] each, coarse = (normal, x, y) [m,3] each -> R [n,4] of ``direction`` = "down" | "up"."""
    cluster = np.asarray(cluster, dtype=np.int64)
    out = np.zeros((cluster.size, 4), dtype=dtype)
    ok = CL.valid(cluster, m)
    if not ok.any():
        return out
    i, cl = np.flatnonzero(ok), cluster[ok]
    f, c = [np.asarray(a) for a in fine], [np.asarray(a) for a in coarse]     # (transport brings them to `dtype`)
    if direction == "down":
        out[i] = CR.transport(c[0][cl], c[1][cl], c[2][cl], f[0][i], f[1][i], non_oriented, dtype)
    else:
        out[i] = CR.transport(f[0][i], f[1][i], f[2][i], c[0][cl], c[1][cl], non_oriented, dtype)
    return out


def _walk(v, cptr, members, rmat, mode, transposed, dtype):
    """Member t of every cell at once, t ascending -> (out [2m,C], arg int32 [m,C], cnt [m] the members taken)."""
    v = np.asarray(v).astype(dtype)
    R = np.asarray(rmat).astype(dtype).reshape(-1, 4)
    m, c, n = cptr.size - 1, v.shape[1], v.shape[0] // 2
    v0, v1 = v[0::2], v[1::2]
    length = cptr[1:] - cptr[:-1]
    au, av, key = (np.zeros((m, c), dtype=dtype) for _ in range(3))
    at, cnt = np.full((m, c), NO_ARG, np.int32), np.zeros(m, np.int64)
    i01, i10 = (2, 1) if transposed else (1, 2)
    with np.errstate(all="ignore"):
        for t in range(int(length.max()) if m else 0):
            cells = np.flatnonzero(length > t)
            rows = members[cptr[cells] + t]
            inside = (rows >= 0) & (rows < n)
            cells, rows = cells[inside], rows[inside]
            a, b = v0[rows], v1[rows]
            r00, r01, r10, r11 = R[rows, 0, None], R[rows, i01, None], R[rows, i10, None], R[rows, 3, None]
            if mode == 0:
                k = a * a + b * b
                take = (cnt[cells] == 0)[:, None] | (k > key[cells])
                key[cells] = np.where(take, k, key[cells])
                au[cells] = np.where(take, r00 * a + r01 * b, au[cells])
                av[cells] = np.where(take, r10 * a + r11 * b, av[cells])
                at[cells] = np.where(take, rows[:, None].astype(np.int32), at[cells])
            else:
                au[cells] = (au[cells] + r00 * a) + r01 * b
                av[cells] = (av[cells] + r10 * a) + r11 * b
            cnt[cells] += 1
        if mode == 3:
            full = cnt > 0
            div = cnt[full].astype(dtype)[:, None]
            au[full], av[full] = au[full] / div, av[full] / div
    out = np.zeros((2 * m, c), dtype=dtype)
    out[0::2], out[1::2] = au, av
    return out, at, cnt


def pool(v, cptr, members, rdown, reduce, dtype=F32):
    """v [2n,C] -> (out [2m,C] `dtype`, arg int32 [m,C] for max or None)."""
    out, at, _ = _walk(v, cptr, members, rdown, MODES[reduce], False, dtype)
    return out, (at if reduce == "max" else None)


def unpool_backward(g, cptr, members, rup, dtype=F32):
    """g [2n,C] -> dx [2m,C]: the ordered sum through the transposed matrices."""
    return _walk(g, cptr, members, rup, MODES["sum"], True, dtype)[0]


def _gather(g, cluster, rmat, transposed, dtype, cptr=None, arg=None, mode=2):
    g = np.asarray(g).astype(dtype)
    cluster = np.asarray(cluster, dtype=np.int64)
    R = np.asarray(rmat).astype(dtype).reshape(-1, 4)
    m, c, n = g.shape[0] // 2, g.shape[1], cluster.size
    out = np.zeros((2 * n, c), dtype=dtype)
    ok = CL.valid(cluster, m)
    if not ok.any():
        return out
    i, cl = np.flatnonzero(ok), cluster[ok]
    g0, g1 = g[0::2][cl], g[1::2][cl]
    i01, i10 = (2, 1) if transposed else (1, 2)
    with np.errstate(all="ignore"):
        if mode == 3:
            div = (cptr[cl + 1] - cptr[cl]).astype(dtype)[:, None]
            g0, g1 = g0 / div, g1 / div
        o0 = R[i, 0, None] * g0 + R[i, i01, None] * g1
        o1 = R[i, i10, None] * g0 + R[i, 3, None] * g1
    if mode == 0:
        hit = arg[cl] == i[:, None]
        o0, o1 = np.where(hit, o0, dtype(0)), np.where(hit, o1, dtype(0))
    out[2 * i], out[2 * i + 1] = o0, o1
    return out


def pool_backward(g, cluster, cptr, rdown, arg, reduce, dtype=F32):
    """g [2m,C] -> dv [2n,C]: one term per point, through the transposed rdown."""
    return _gather(g, cluster, rdown, True, dtype, cptr, arg, MODES[reduce])


def unpool(x, cluster, rup, dtype=F32):
    """x [2m,C] -> out [2n,C]: the cell's vector in every member's frame."""
    return _gather(x, cluster, rup, False, dtype)


# ---- the magnitudes of the bounds, in fp64 ----------------------------------------------------------------------------------------------
def pool_magnitude(v, cptr, members, rmat, transposed=False):
    """-> S [2m,C]: the sum over a cell's members of |R00 v0| + |R01 v1| (|R10 v0| + |R11 v1|), and cnt [m]."""
    out, _, cnt = _walk(np.abs(np.asarray(v, dtype=F32).astype(F64)), cptr, members, np.abs(np.asarray(rmat, dtype=F32).astype(F64)), 2,
                        transposed, F64)
    return out, cnt


def gather_magnitude(g, cluster, rmat, transposed, cptr=None, mean=False):
    """-> T [2n,C]: |a00 g0| + |a01 g1| per point (on the exact quotients for the mean)."""
    return _gather(np.abs(np.asarray(g, dtype=F32).astype(F64)), cluster, np.abs(np.asarray(rmat, dtype=F32).astype(F64)), transposed, F64,
                   cptr, None, 3 if mean else 2)


def exact_keys(v):
    """-> [n,C] the squared norms of the fp32 vectors in fp64."""
    v = np.asarray(v, dtype=F32).astype(F64)
    return v[0::2] * v[0::2] + v[1::2] * v[1::2]
