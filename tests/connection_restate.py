"""numpy restatement of deltaconv_amd/csrc/connection_math.h: ``transport`` operation by operation (every product, sum, quotient
and square root one rounding of ``dtype``, in the header's order), ``transport_sum`` and its transpose in the stated slot / edge
order, and the helpers ``angle_in_plane`` / ``rotate_around``.  ``dtype=np.float32`` is the bit-for-bit twin of the g++ build
(tests/hostcheck_connection) and of the kernels (csrc/connection.hip); ``dtype=np.float64`` is the same formulas in fp64, the
yardstick of the bounds.  The helpers use numpy's arctan2 / cos / sin and are held to a tolerance only."""
import numpy as np

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24
AXIS_EPS, NORM_CLAMP = 1e-6, 1e-8


def _c(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def norm3(a):
    return np.sqrt(dot3(a, a))


def normalize_clamped(a, eps):
    return a / np.fmax(norm3(a), a.dtype.type(eps))[:, None]


def plane_coords(u, v, normal):
    up = normalize_clamped(u - normal * dot3(u, normal)[:, None], NORM_CLAMP)
    by = normalize_clamped(cross3(normal, up), NORM_CLAMP)
    return dot3(v, up), dot3(v, by)


def rotate_cs(v, axis, c, s):
    par = axis * dot3(v, axis)[:, None]
    tc = v - par
    tl = np.fmax(norm3(tc), v.dtype.type(NORM_CLAMP))
    bx = tc / tl[:, None]
    by = cross3(axis, bx)
    rot = (bx * c[:, None] + by * s[:, None]) * tl[:, None] + par
    return np.where((tl > 0)[:, None], rot, par)


def transport(tn, tx, ty, sn, sx, non_oriented=True, dtype=F32, details=False):
    """-> [M,4].  details=True also returns (d, an, l): the three quantities whose comparisons pick a branch."""
    tn, tx, ty, sn, sx = (_c(a, dtype).reshape(-1, 3) for a in (tn, tx, ty, sn, sx))
    T = dtype
    same = (sn == tn).all(axis=1) & (sx == tx).all(axis=1)          # a frame seen from itself: the identity, (1, -0, 0, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = dot3(sn, tn)
        inverted = d < 0
        tn = np.where(inverted[:, None], -tn, tn)
        ty = np.where(inverted[:, None], -ty, ty)
        axis = cross3(tn, sn)
        an = norm3(axis)
        axis = np.where((an > T(AXIS_EPS))[:, None], axis / an[:, None], sx)
        xc, yc = plane_coords(sn, tn, axis)
        r = np.sqrt(xc * xc + yc * yc)
        c = np.where(r > 0, xc / r, T(1))
        s = np.where(r > 0, yc / r, T(0))
        rot = rotate_cs(sx, axis, c, s)
        a, b = dot3(rot, tx), dot3(rot, ty)
        l = np.sqrt(a * a + b * b)
        ok = l > T(AXIS_EPS)
        a = np.where(ok, a / l, T(1))
        b = np.where(ok, b / l, T(0))
    conj = np.where(inverted & bool(non_oriented), T(-1), T(1))
    out = np.stack([a, -b, b * conj, a * conj], axis=1).astype(dtype)
    out[same] = np.array([1, -0.0, 0, 1], dtype=dtype)
    return (out, (d, an, l)) if details else out


def graph_transport(normal, xb, yb, nbr, non_oriented=True, dtype=F32):
    """the graph form: target = row m // k, source = row nbr[m]."""
    n, k = nbr.shape
    t, s = np.repeat(np.arange(n), k), nbr.reshape(-1)
    return transport(normal[t], xb[t], yb[t], normal[s], xb[s], non_oriented, dtype)


def angle_in_plane(u, v, normal, dtype=F64):
    u, v, normal = (_c(a, dtype).reshape(-1, 3) for a in (u, v, normal))
    xc, yc = plane_coords(u, v, normal)
    return np.arctan2(yc, xc)


def rotate_around(v, axis, angle, dtype=F64):
    v, axis = (_c(a, dtype).reshape(-1, 3) for a in (v, axis))
    angle = _c(angle, dtype).reshape(-1)
    return rotate_cs(v, axis, np.cos(angle), np.sin(angle))


# ---- the sums -----------------------------------------------------------------------------------------------------------------
def csc(nbr):
    """(tptr [n+1], tedge [n*k]): the in-edges e = i*k + s of every point, ascending (Graph.csc())."""
    n, k = nbr.shape
    flat = nbr.reshape(-1).astype(np.int64)
    tedge = np.argsort(flat, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))])
    return tptr.astype(np.int32), tedge.astype(np.int32)


def fold_weights(connection, weights, dtype=F32):
    """coef = w * R: one rounding per entry."""
    connection = _c(connection, dtype)
    return connection if weights is None else (_c(weights, dtype)[:, None] * connection).astype(dtype)


def transport_sum(v, coef, nbr, scale=1.0, dtype=F32):
    """v [2n,C], coef [n*k,4], nbr [n,k] -> out [2n,C]; slots ascending, vectorised over points and channels."""
    n, k = nbr.shape
    v, R = _c(v, dtype), _c(coef, dtype).reshape(n, k, 4)
    v0, v1 = v[0::2], v[1::2]
    au, av = np.zeros((n, v.shape[1]), dtype=dtype), np.zeros((n, v.shape[1]), dtype=dtype)
    for s in range(k):
        j = nbr[:, s]
        au = (au + R[:, s, 0, None] * v0[j]) + R[:, s, 1, None] * v1[j]
        av = (av + R[:, s, 2, None] * v0[j]) + R[:, s, 3, None] * v1[j]
    out = np.empty_like(v)
    out[0::2], out[1::2] = dtype(scale) * au, dtype(scale) * av
    return out


def transport_sum_backward(g, coef, nbr, scale=1.0, dtype=F32, into=None):
    """g [2n,C] -> dv [2n,C]: per point the in-edges in ascending edge id; the p-th in-edge of every point in one vector step.
    into: accumulate = 1, dv = into + scale * acc."""
    n, k = nbr.shape
    g, R = _c(g, dtype), _c(coef, dtype).reshape(n * k, 4)
    g0, g1 = g[0::2], g[1::2]
    tptr, tedge = csc(nbr)
    deg = np.diff(tptr)
    au, av = np.zeros((n, g.shape[1]), dtype=dtype), np.zeros((n, g.shape[1]), dtype=dtype)
    for p in range(int(deg.max()) if n else 0):
        js = np.nonzero(deg > p)[0]
        e = tedge[tptr[js] + p]
        i = e // k
        au[js] = (au[js] + R[e, 0, None] * g0[i]) + R[e, 2, None] * g1[i]
        av[js] = (av[js] + R[e, 1, None] * g0[i]) + R[e, 3, None] * g1[i]
    dv = np.empty_like(g)
    dv[0::2], dv[1::2] = dtype(scale) * au, dtype(scale) * av
    return dv if into is None else (_c(into, dtype) + dv).astype(dtype)


def sum_bound(v, coef, nbr, scale, extra=0):
    """(2k + 3 + extra) * 2^-24 * |scale| * sum_s sum_b |coef_ab| |v_b| per output entry, in fp64."""
    n, k = nbr.shape
    mag = transport_sum(np.abs(_c(v, F64)), np.abs(_c(coef, F64)), nbr, 1.0, F64)
    return (2 * k + 3 + extra) * EPS * abs(float(scale)) * mag


def backward_bound(g, coef, nbr, scale, extra=0):
    """(2 L_j + 3 + extra) * 2^-24 * |scale| * sum_e sum_a |coef_ab| |g_a|, L_j the in-list length of the point."""
    mag = transport_sum_backward(np.abs(_c(g, F64)), np.abs(_c(coef, F64)), nbr, 1.0, F64)
    L = np.repeat(np.diff(csc(nbr)[0]), 2).astype(F64)
    return (2 * L[:, None] + 3 + extra) * EPS * abs(float(scale)) * mag


# ---- shared inputs of the host and the device tests ---------------------------------------------------------------------------
def tangent_basis(n):
    """fp32 restatement of build_tangent_basis (csrc/point_math.h: tangent_basis_point), good enough to make frames for tests."""
    n = _c(n, F32)
    alt = np.abs(n[:, 0]) > F32(0.9)
    t = np.zeros_like(n)
    t[:, 0], t[:, 1] = np.where(alt, 0, 1), np.where(alt, 1, 0)
    x = cross3(t, n)
    x = x * (F32(1) / np.fmax(norm3(x), F32(1e-5)))[:, None]
    y = cross3(n, x)
    y = y * (F32(1) / np.fmax(norm3(y), F32(1e-5)))[:, None]
    return x.astype(F32), y.astype(F32)


def random_pairs(m, seed):
    """m pairs of unit normals with frames -> (tn, tx, ty, sn, sx) fp32."""
    rng = np.random.default_rng(seed)
    tn = rng.standard_normal((m, 3)).astype(F32)
    sn = rng.standard_normal((m, 3)).astype(F32)
    tn, sn = tn / norm3(tn)[:, None], sn / norm3(sn)[:, None]
    tx, ty = tangent_basis(tn)
    sx, _ = tangent_basis(sn)
    return tn, tx, ty, sn, sx


def cloud(n, seed):
    """a bumpy sphere: positions, outward unit normals, frames."""
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3)).astype(F32)
    nrm = nrm / norm3(nrm)[:, None]
    pos = (nrm * (1 + 0.1 * rng.random((n, 1), dtype=F32))).astype(F32)
    xb, yb = tangent_basis(nrm)
    return pos, nrm.astype(F32), xb, yb


def hand_table(n=300, k=5, seed=11):
    """nbr [n,k] of one cloud: slot 0 the point itself, slot 1 point 0 (ONE in-list of n + entries), the other slots random
    points among 1 .. n - 2: the last point has only its self edge."""
    rng = np.random.default_rng(seed)
    nbr = rng.integers(1, n - 1, (n, k)).astype(np.int32)
    nbr[:, 0], nbr[:, 1] = np.arange(n), 0
    return nbr
