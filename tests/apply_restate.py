"""Plain fp64 restatement of the fixed-degree sparse applies and neighbourhood aggregations (the formulas in the comments of
deltaconv_amd/csrc/ell_math.h), for tests/test_gpu_apply_abi.py and tests/test_apply_restate_host.py.

Everything works on nbr [n, k] (int64) and coef [n, k, 2] directly: forward bodies gather, transposed bodies scatter with
index_add_ over nbr.  No CSC arrays are used, so the transposed references do not depend on dc_csc_build.

Every body returns (value, S, m):
  value   the fp64 result (inputs are fp32, so every product is exact in fp64 and the fp64 sum of m terms is within
          m 2^-53 S of the true value: below 1e-5 of any bound here);
  S       per output element, the sum of the magnitudes of the terms that were added (with `prev` -- accumulate = 1 -- also
          |previous content|; for grad_T_sum also |a| and |b|; for the norm term also |d_norm v / |v||);
  m       the number of fma terms of the element's chain (an int, or a tensor that broadcasts against value).

Bounds.  u = 2^-24.  A chain acc = fma(c_i, x_i, acc) of m terms started from 0 returns sum_i c_i x_i (1 + theta_i) with
|theta_i| <= gamma_m = m u / (1 - m u) (the first fma is exact up to its one rounding, every later one adds one factor
(1 + delta)), so the chain is within gamma_m S of the exact sum.  What follows the chain adds at most two more roundings of
a sum whose terms are already in S: `accumulate` (one add), grad_T_sum ((a + b) + chain: two adds), the sum / mean
aggregation (k - 1 adds and one product with the scale: m = k).  Hence
    linear bodies:      gamma_(m + 2) S        = (m + 2) u S to first order; the quotient form is used so that the bound is
                                                 rigorous at m = 4400 (the hub columns), where it is 0.03 % larger
    norm output:        3 u |n|                (n = sqrt(fma(a, a, b b)): product, fma and square root, one rounding each;
                                                 the two under the root count half: 2 u would do)
    div|curl|norm^T:    gamma_(m + 6) S        (the norm term sc v with sc = d_norm / sqrt(...) carries the 2 u of the norm,
                                                 the division, the final fma and the accumulate add: 5 u; the chain's terms see
                                                 that last fma and the accumulate add: m + 2; m + 6 covers both)
    max_affine:         per slot e_s = gamma_2 (|scale h_s| + |shift|), gamma_2 = 2 u / (1 - 2 u) (2 u to first order; the quotient
                        covers the u^2 of two stacked roundings): the fma rounds once (u |z| <= u (|scale h| + |shift|)), the
                        product with the slope once more and slope <= 1.  The maximum of the computed candidates is within
                        max_s e_s of the maximum of the exact ones.
    arg slot:           the winning slot w holds the largest COMPUTED candidate, so its exact value is at least the exact
                        maximum (slot t) minus e_w + e_t: that sum is the bound (one e alone is not implied by the arithmetic).
    residual form:      out = fl(act2(fma(scale2, h2, shift2)) + max): both addends are computed within (1 + u)^2 of terms bounded
                        by B = |scale2 h2| + |shift2| and A = max_s (|scale h_s| + |shift|), and the sum rounds once more on
                        top of them: (1 + u)^3 - 1 <= gamma_3 = 3 u / (1 - 3 u), so gamma_3 (A + B) (3 u (A + B) to first order).
    plain max:          exact value and first maximal slot.
"""
import torch

U = 2.0 ** -24
G2, G3 = 2 * U / (1 - 2 * U), 3 * U / (1 - 3 * U)


def gamma_bound(m, S, extra=2):
    """gamma_(m + extra) S."""
    g = (torch.as_tensor(m, dtype=torch.float64) + extra) * U
    return g / (1 - g) * S


def _uv(t):
    return t[0::2], t[1::2]


def _interleave(u, v):
    return torch.stack([u, v], 1).reshape(2 * u.shape[0], u.shape[1])


def _scatter(nbr, t):
    """t [n, k, ...]: the term of edge (i, s) -> summed at row nbr[i, s]."""
    n, k = nbr.shape
    out = torch.zeros((n,) + tuple(t.shape[2:]), dtype=torch.float64)
    out.index_add_(0, nbr.reshape(-1), t.reshape((n * k,) + tuple(t.shape[2:])))
    return out


def in_degree(nbr):
    return torch.bincount(nbr.reshape(-1), minlength=nbr.shape[0]).double()[:, None]


def _with_prev(val, S, prev):
    if prev is None:
        return val, S
    return val + prev.double(), S + prev.double().abs()


# ---- forward bodies -----------------------------------------------------------------------------------------------------------
def grad(nbr, G, x):
    """out[2i + a, c] = sum_s G[i, s, a] x[nbr[i, s], c]"""
    g, xg = G.double(), x.double()[nbr]                                  # [n, k, 2], [n, k, C]
    tu, tv = g[:, :, 0:1] * xg, g[:, :, 1:2] * xg
    return _interleave(tu.sum(1), tv.sum(1)), _interleave(tu.abs().sum(1), tv.abs().sum(1)), nbr.shape[1]


def div(nbr, D, v):
    """out[i, c] = sum_s D[i, s, 0] v[2j, c] + D[i, s, 1] v[2j + 1, c]"""
    d = D.double()
    vu, vv = (t.double()[nbr] for t in _uv(v))
    t0, t1 = d[:, :, 0:1] * vu, d[:, :, 1:2] * vv
    return (t0 + t1).sum(1), (t0.abs() + t1.abs()).sum(1), 2 * nbr.shape[1]


def curl(nbr, D, v):
    """curl = -div(J v), J(v) = (-v_v, v_u): out[i, c] = sum_s D[i, s, 0] v[2j + 1, c] - D[i, s, 1] v[2j, c]"""
    d = D.double()
    vu, vv = (t.double()[nbr] for t in _uv(v))
    t0, t1 = d[:, :, 0:1] * vv, -d[:, :, 1:2] * vu
    return (t0 + t1).sum(1), (t0.abs() + t1.abs()).sum(1), 2 * nbr.shape[1]


def norm(v):
    vu, vv = (t.double() for t in _uv(v))
    return (vu * vu + vv * vv).sqrt()


def div_curl_norm(nbr, D, v):
    """-> ((value [n, 3C], S [n, 3C], m), norm bound [n, C]); the last C columns of S are unused (the norm has its own bound)."""
    (dv, ds, m), (cv, cs, _) = div(nbr, D, v), curl(nbr, D, v)
    nv = norm(v)
    return (torch.cat([dv, cv, nv], 1), torch.cat([ds, cs, nv], 1), m), 3 * U * nv


def hodge(nbr, G, dc):
    """dc [n, 2C] = [div v | curl v]: h_u = -(sum G_u dv_j - sum G_v cv_j), h_v = -(sum G_v dv_j + sum G_u cv_j); out [2n, C]"""
    g = G.double()
    c = dc.shape[1] // 2
    dv, cv = dc.double()[:, :c][nbr], dc.double()[:, c:][nbr]
    ga, gb = g[:, :, 0:1], g[:, :, 1:2]
    u0, u1, v0, v1 = -ga * dv, gb * cv, -gb * dv, -ga * cv
    return (_interleave((u0 + u1).sum(1), (v0 + v1).sum(1)), _interleave((u0.abs() + u1.abs()).sum(1), (v0.abs() + v1.abs()).sum(1)),
            2 * nbr.shape[1])


# ---- transposed bodies: the term of edge (i, s) lands on j = nbr[i, s] ---------------------------------------------------------
def grad_T(nbr, G, dy, prev=None):
    """dx[j, c] (+)= sum_e G[e, 0] dy[2i, c] + G[e, 1] dy[2i + 1, c]"""
    g = G.double()
    du, dv = (t.double()[:, None, :] for t in _uv(dy))
    t0, t1 = g[:, :, 0:1] * du, g[:, :, 1:2] * dv
    val, S = _with_prev(_scatter(nbr, t0 + t1), _scatter(nbr, t0.abs() + t1.abs()), prev)
    return val, S, 2 * in_degree(nbr)


def grad_T_sum(nbr, G, dy, a, b=None):
    """out[j, c] = a[j, c] (+ b[j, c]) + grad^T dy"""
    val, S, m = grad_T(nbr, G, dy)
    for t in (a, b):
        if t is not None:
            val, S = val + t.double(), S + t.double().abs()
    return val, S, m


def div_T(nbr, D, dy, prev=None):
    """dv[2j + a, c] (+)= sum_e D[e, a] dy[i, c]"""
    d, g = D.double(), dy.double()[:, None, :]
    tu, tv = d[:, :, 0:1] * g, d[:, :, 1:2] * g
    val, S = _with_prev(_interleave(_scatter(nbr, tu), _scatter(nbr, tv)), _interleave(_scatter(nbr, tu.abs()), _scatter(nbr, tv.abs())),
                        prev)
    return val, S, in_degree(nbr).repeat_interleave(2, 0)


def div_curl_norm_T(nbr, D, dout, v, prev=None):
    """dv_u[j] = sum_e (D0 d_div_i - D1 d_curl_i) + d_norm_j v_u[j] / |v_j|,  dv_v[j] = sum_e (D1 d_div_i + D0 d_curl_i) + d_norm_j
    v_v[j] / |v_j|; the norm term is 0 at |v| = 0 (the subgradient torch takes).  Bound: gamma_bound(m, S, extra=6)."""
    d = D.double()
    c = dout.shape[1] // 3
    o = dout.double()
    dd, dcu, dn = o[:, None, :c], o[:, None, c:2 * c], o[:, 2 * c:]
    d0, d1 = d[:, :, 0:1], d[:, :, 1:2]
    u0, u1, v0, v1 = d0 * dd, -d1 * dcu, d1 * dd, d0 * dcu
    vu, vv = (t.double() for t in _uv(v))
    nv = norm(v)
    safe = torch.where(nv > 0, nv, torch.ones_like(nv))
    nu, nw = torch.where(nv > 0, dn * vu / safe, 0.0), torch.where(nv > 0, dn * vv / safe, 0.0)
    val = _interleave(_scatter(nbr, u0 + u1) + nu, _scatter(nbr, v0 + v1) + nw)
    S = _interleave(_scatter(nbr, u0.abs() + u1.abs()) + nu.abs(), _scatter(nbr, v0.abs() + v1.abs()) + nw.abs())
    val, S = _with_prev(val, S, prev)
    return val, S, (2 * in_degree(nbr)).repeat_interleave(2, 0)


def hodge_T(nbr, G, dh, prev=None):
    """ddc[j, 0:C] (+)= -sum_e (G_u dh_u[i] + G_v dh_v[i]),  ddc[j, C:2C] (+)= sum_e (G_v dh_u[i] - G_u dh_v[i])"""
    g = G.double()
    hu, hv = (t.double()[:, None, :] for t in _uv(dh))
    ga, gb = g[:, :, 0:1], g[:, :, 1:2]
    a0, a1, c0, c1 = -ga * hu, -gb * hv, gb * hu, -ga * hv
    val = torch.cat([_scatter(nbr, a0 + a1), _scatter(nbr, c0 + c1)], 1)
    S = torch.cat([_scatter(nbr, a0.abs() + a1.abs()), _scatter(nbr, c0.abs() + c1.abs())], 1)
    val, S = _with_prev(val, S, prev)
    return val, S, 2 * in_degree(nbr)


# ---- aggregations ---------------------------------------------------------------------------------------------------------------
def knn_sum(nbr, h, scale):
    """out[i, c] = scale * sum_s h[nbr[i, s], c]; scale = the fp32 value the entry point is given (1 or fl(1 / k))"""
    hg = h.double()[nbr]
    return scale * hg.sum(1), abs(scale) * hg.abs().sum(1), nbr.shape[1]


def knn_sum_T(nbr, dout, scale, prev=None):
    """dh[j, c] (+)= scale * sum over the in-edges (i, s) of j of dout[i, c]"""
    t = dout.double()[:, None, :].expand(-1, nbr.shape[1], -1)
    val, S = _with_prev(scale * _scatter(nbr, t), abs(scale) * _scatter(nbr, t.abs()), prev)
    return val, S, in_degree(nbr)


def first_max(y):
    """y [n, k, C] -> (maximum [n, C], first maximal slot [n, C])"""
    mx = y.max(1).values
    eq = y == mx[:, None, :]
    first = (eq.long().cumsum(1) == 1) & eq
    return mx, (first.long() * torch.arange(y.shape[1]).view(1, -1, 1)).sum(1)


def knn_max(nbr, h):
    """-> (value, first maximal slot): exact in every format"""
    return first_max(h.double()[nbr])


def affine_candidates(nbr, h, scale, shift, slope):
    """y = leaky_slope(scale_c h + shift_c) per candidate -> (y [n, k, C] fp64, e [n, k, C] = gamma_2 (|scale h| + |shift|))"""
    sh = scale.double() * h.double()
    z = sh + shift.double()
    y = torch.where(z > 0, z, slope * z)
    return y[nbr], (G2 * (sh.abs() + shift.double().abs()))[nbr]


def affine_block(h2, scale2, shift2, slope2):
    """-> (act2(scale2 h2 + shift2), B = |scale2 h2| + |shift2|)"""
    sh = scale2.double() * h2.double()
    z = sh + shift2.double()
    return torch.where(z > 0, z, slope2 * z), sh.abs() + shift2.double().abs()


def knn_max_T(nbr, arg, dout, prev=None):
    """dh[j, c] (+)= sum over in-edges (i, s) of j with arg[i, c] == s of dout[i, c]; m = the number of hits"""
    hit = (arg.long()[:, None, :] == torch.arange(nbr.shape[1]).view(1, -1, 1)).double()
    t = hit * dout.double()[:, None, :]
    val, S = _with_prev(_scatter(nbr, t), _scatter(nbr, t.abs()), prev)
    return val, S, _scatter(nbr, hit)


# ---- data ---------------------------------------------------------------------------------------------------------------------
def make_graph(sizes, k, seed, hub_rows=0):
    """nbr [n, k]: slot 0 = the point itself, the rest random points of its own cloud (repeats allowed: ties for the maximum).
    hub_rows > 0 (one cloud): slots 1.. of that many points all name the same k - 1 targets, whose columns of the transposed
    structure then hold more than hub_rows in-edges each."""
    g = torch.Generator().manual_seed(seed)
    n = sum(sizes)
    nbr = torch.empty(n, k, dtype=torch.int64)
    lo = 0
    for sz in sizes:
        nbr[lo:lo + sz] = lo + torch.randint(0, sz, (sz, k), generator=g)
        lo += sz
    nbr[:, 0] = torch.arange(n)
    if hub_rows:
        assert len(sizes) == 1 and k > 1
        perm = torch.randperm(n, generator=g)
        nbr[perm[:hub_rows], 1:] = torch.randperm(n, generator=g)[:k - 1]
    return nbr


def make_coef(n, k, seed):
    """[n, k, 2] fp32: per-row magnitudes log-uniform over 1e-3 .. 1e3, entries within (0.25 .. 1) of it, random signs"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g) * 6 - 3)
    sign = torch.randint(0, 2, (n, k, 2), generator=g) * 2.0 - 1.0
    return (mag[:, None, None] * (0.25 + 0.75 * torch.rand(n, k, 2, generator=g)) * sign).float()


def make_features(rows, c, seed):
    """[rows, c] fp32: normal draws times column scales log-uniform over 1e-2 .. 1e2 (products with the coefficients stay between
    ~1e-9 and 1e7 in magnitude apart from the tails of the normal: no underflow)"""
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(c, generator=g) * 4 - 2)
    return (scale * torch.randn(rows, c, generator=g)).float()


def make_vectors(n, c, seed):
    """[2n, c] tangent vectors; every 37th point (and point 0) carries exactly zero vectors in all channels, every 11th in channel 0"""
    v = make_features(2 * n, c, seed)
    idx = torch.arange(0, n, 37)
    v[2 * idx] = 0.0
    v[2 * idx + 1] = 0.0
    idx = torch.arange(0, n, 11)
    v[2 * idx, 0] = 0.0
    v[2 * idx + 1, 0] = 0.0
    return v


def make_affine(c, seed):
    """scale (both signs, one exact zero when c > 2) and shift of a folded BatchNorm, fp32"""
    g = torch.Generator().manual_seed(seed)
    scale = (10.0 ** (torch.rand(c, generator=g) * 2 - 1)) * (torch.randint(0, 2, (c,), generator=g) * 2.0 - 1.0)
    if c > 2:
        scale[c // 2] = 0.0
    return scale.float(), torch.randn(c, generator=g).float()
