"""numpy restatement of deltaconv_amd/csrc/cluster_math.h: the member lists of a cluster vector, the pooling of features over them
(max / min / sum / mean, with the row every maximum came from), its backward, the un-pooling and its backward, the fp64
barycentres and the majority labels -- every fp32 operation rounded on its own, every sum in ASCENDING row order.  Written from the
header's rules, not from its code; tests/test_cluster_host.py holds the g++ build of the header to it bit for bit,
tests/test_gpu_cluster.py the device.  The fp64 sums are np.add.at (sequential, unbuffered), never the pairwise np.sum."""
import math

import numpy as np

F = np.float32
MODES = {"max": 0, "min": 1, "sum": 2, "mean": 3}


def valid(cluster, m):
    cluster = np.asarray(cluster, dtype=np.int64)
    return (cluster >= 0) & (cluster < m)


def lists(cluster, m):
    """-> (cptr int64 [m+1], members int64 [n]: ascending rows per cell, -1 from cptr[m] on)."""
    cluster = np.asarray(cluster, dtype=np.int64)
    rows = np.flatnonzero(valid(cluster, m))
    order = rows[np.argsort(cluster[rows], kind="stable")]                 # by cell, rows ascending inside a cell
    cptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(cluster[rows], minlength=m)[:m], out=cptr[1:])
    members = np.full(cluster.size, -1, np.int64)
    members[:order.size] = order
    return cptr, members


def pool(x, cptr, members, reduce):
    """x fp32 [n,C] -> (out fp32 [m,C], arg int32 [m,C] (max / min) or None).  Member t of every cell at once, t ascending."""
    x = np.asarray(x, dtype=F)
    m, c = cptr.size - 1, x.shape[1]
    cnt = cptr[1:] - cptr[:-1]
    out, arg = np.zeros((m, c), F), np.full((m, c), -1, np.int32)
    with np.errstate(all="ignore"):
        for t in range(int(cnt.max()) if m else 0):
            cells = np.flatnonzero(cnt > t)
            rows = members[cptr[cells] + t]
            v = x[rows]
            if t == 0:
                out[cells], arg[cells] = v, rows[:, None].astype(np.int32)
            elif reduce in ("max", "min"):
                take = v > out[cells] if reduce == "max" else v < out[cells]
                out[cells] = np.where(take, v, out[cells])
                arg[cells] = np.where(take, rows[:, None].astype(np.int32), arg[cells])
            else:
                out[cells] = (out[cells] + v).astype(F)
        if reduce == "mean":
            full = cnt > 0
            out[full] = (out[full] / cnt[full].astype(F)[:, None]).astype(F)
    return out, (arg if reduce in ("max", "min") else None)


def pool_backward(g, cluster, cptr, arg, reduce):
    """g fp32 [m,C] -> dx fp32 [n,C]: a gather from every point's cell."""
    g, cluster = np.asarray(g, dtype=F), np.asarray(cluster, dtype=np.int64)
    m = g.shape[0]
    ok = valid(cluster, m)
    cl = np.where(ok, cluster, 0)
    dx = np.zeros((cluster.size, g.shape[1]), F)
    if m == 0 or cluster.size == 0:
        return dx
    if reduce in ("max", "min"):
        term = np.where(arg[cl] == np.arange(cluster.size)[:, None], g[cl], F(0))
    elif reduce == "sum":
        term = g[cl]
    else:
        with np.errstate(all="ignore"):
            term = (g[cl] / (cptr[cl + 1] - cptr[cl]).astype(F)[:, None]).astype(F)
    dx[ok] = term[ok]
    return dx


def gather(x, cluster):
    """The un-pooling out[i] = x[cluster[i]], zeros without a cell."""
    return pool_backward(x, cluster, None, None, "sum")


def gather_backward(g, cptr, members):
    """Its gradient w.r.t. x: the ordered sum of g over every cell's members."""
    return pool(g, cptr, members, "sum")[0]


def mean3(p, cluster, m, normalize=False):
    """p fp32 [n,3] -> fp32 [m,3]: fp64 sums in ascending row order, one fp64 division, one rounding."""
    p, cluster = np.asarray(p, dtype=F).reshape(-1, 3), np.asarray(cluster, dtype=np.int64)
    rows = np.flatnonzero(valid(cluster, m))
    s = np.zeros((m, 3), np.float64)
    with np.errstate(all="ignore"):
        np.add.at(s, cluster[rows], p[rows].astype(np.float64))                # sequential: row order
        cnt = np.bincount(cluster[rows], minlength=m)[:m]
        if normalize:
            sq = s * s
            div = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
            ok = (cnt > 0) & (div > 0) & np.isfinite(div)
        else:
            div, ok = cnt.astype(np.float64), cnt > 0
        out = np.zeros((m, 3), F)
        out[ok] = (s[ok] / div[ok][:, None]).astype(F)
    return out


def majority(labels, cluster, m, num_classes):
    labels, cluster = np.asarray(labels, dtype=np.int64), np.asarray(cluster, dtype=np.int64)
    ok = valid(cluster, m) & (labels >= 0) & (labels < num_classes)
    table = np.zeros((m, num_classes), np.int64)
    np.add.at(table, (cluster[ok], labels[ok]), 1)
    return np.where(table.max(1, initial=0) > 0, table.argmax(1) if m else np.zeros(0, np.int64), -1).astype(np.int64)  # argmax: the lowest


# ---- fp64 truth and the derived bounds ------------------------------------------------------------------------------------------------
U32, U64 = 2.0 ** -24, 2.0 ** -53


def exact_sums(x, cptr, members):
    """-> (sum [m,C], sum of magnitudes [m,C]) as fp64, by math.fsum (exact, then rounded once)."""
    x = np.asarray(x, dtype=np.float64)
    m, c = cptr.size - 1, x.shape[1]
    s, a = np.zeros((m, c)), np.zeros((m, c))
    for j in range(m):
        rows = members[cptr[j]:cptr[j + 1]]
        for ch in range(c):
            s[j, ch] = math.fsum(x[rows, ch])
            a[j, ch] = math.fsum(np.abs(x[rows, ch]))
    return s, a


def bounds(x, cptr, members):
    """-> dict(sum, mean, bary): the per-element bounds on the fp32 sum / mean and the fp64-held barycentre against fp64, with the
    truth they are about.  sum: a chain of cnt - 1 rounded additions, each off by at most 2^-24 of a partial sum that Σ|x| bounds:
    cnt * 2^-24 * Σ|x|.  mean: the same over cnt plus the quotient's own rounding (2^-24 |mean| <= 2^-24 Σ|x| / cnt):
    (cnt + 1) * 2^-24 * Σ|x| / cnt.  bary: the one rounding to fp32, 2^-24 |mean|, plus the fp64 chain and quotient,
    (cnt + 1) * 2^-53 * Σ|p| / cnt."""
    s, a = exact_sums(x, cptr, members)
    cnt = np.maximum(cptr[1:] - cptr[:-1], 1).astype(np.float64)[:, None]
    mean = s / cnt
    return dict(true_sum=s, true_mean=mean, sum=cnt * U32 * a, mean=(cnt + 1) * U32 * a / cnt,
                bary=U32 * np.abs(mean) + (cnt + 1) * U64 * a / cnt)
