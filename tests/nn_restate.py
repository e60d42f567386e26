"""An fp64 restatement, in plain torch, of the single-rank entry points of deltaconv_amd/csrc/nn.hip (element formulas:
nn_math.h, reductions and finalisers: colreduce.h) with a per-element bound for every output, the data they are tested on and
one driver per family that runs every call through a `backend` and holds each output to its bound.  No import of the package:
tests/test_nn_restate_host.py passes the CPU build of the same headers (tests/hostcheck), tests/test_gpu_nn_abi.py the C ABI
on the device.

u = 2^-24 is the unit roundoff of fp32; every fp32 operation (+, -, *, /, sqrtf, fmaf) is correctly rounded, so it returns
its exact result times (1 + d), |d| <= u.  A bound below is the first-order sum of those d over the expression as the code
writes it, times O2 = 1 + 2^-20 for the products of at most sixteen such factors (16 u^2 < 2^-20 u).  The inputs are fp32
and enter the fp64 reference exactly.  The reference sums in fp64 in two passes; on these data (column means up to 30
standard deviations, at most 24 000 rows) its own error is below 1e-9 of every bound.  No constant is fitted to an output.

Column sums (colreduce_body, colreduce_final_kernel): the addends are accumulated in fp64 -- per row lane, 16 lanes, per
chunk, 64 finaliser lanes, six butterfly steps -- so a sum of R addends a_r is within N53 sum|a_r|, N53 = (R + 80) 2^-53, of
the exact sum of the addends the kernel formed.  What matters is the error e_r of each addend, formed in fp32.

dc_bn_stats / BnFin (bounds of tests/test_gpu_sync_bn.py, unchanged): addends x and x^2 are exact in fp64, so mean, invstd,
    scale are one rounding of an fp64 value: 2 u |ref| (the factor 2 is the slack that test allows); shift = b - m g invstd
    and the running pair (1 - mom) old + mom new: 2 u (sum of the magnitudes of their terms).  Unbiased variance var R / (R - 1)
    in running_var when R > 1, the biased one when R = 1.  gamma / beta NULL: 1 / 0.
dc_vn_stats: the addends are fp32 norms n = sqrtf(fmaf(yu, yu, yv * yv)) of the combined (yu, yv) = (pu - qv, pv + qu): at most
    3 u relative (one for the combination, one each for the product, the fma and, halved by the root, the root's own), as
    that test counts them.  Hence mean: 2 u |mean| + 3 u E n; var = E n^2 - mean^2 is uncertain by 6 u (E n^2 + mean^2), so
    invstd, scale: rho = 2 u + 6 u (E n^2 + mean^2) / (2 (var + eps)) relative; shift: 2 u (|b| + |mean scale|) + |scale| 3 u E n
    + (rho - 2 u) |mean scale|; running_mean: + mom 3 u E n; running_var: + mom R / (R - 1) 6 u (E n^2 + mean^2).
dc_bn_eval_coeffs (fp32): invstd = 1 / sqrtf(rv + eps): add u, root u / 2 + u, quotient u = 2.5 u -> 3 u |ref|; mean = rm
    exactly; scale = g invstd: 3.5 u -> 4 u |ref|; shift = b - (rm g) invstd: the product term t carries 1 + 2.5 + 1 = 4.5 u, the
    difference one more rounding u (|b| + |t|): u |b| + 6 u |t|.
dc_bn_act / dc_bn_act2, y = act(fmaf(scale, h, shift)) (+ residual), scale / shift as given: the fma rounds once (u |a|,
    a = act(z); rounding keeps the sign, so the branch is the reference's), slope * z once more where z <= 0 and slope != 1,
    the residual add once (u |y|).  act is continuous: no element is excluded.
dc_bn_act_backward_reduce.  The reference takes mean / invstd / scale / shift in fp64 (training: the batch statistics;
    inference: the fp64 map of the running pair); the kernel is given their fp32 values, within km u |mean| and ki u invstd
    (training: one rounding each, km = ki = 1; inference: km = 0, ki = 3 from above).  Per addend (bn_bwd_terms):
      dz = dy act'(z): e0 = u |dz| where act' != 1 (the gate is the reference's: the data keep |z| off 0, below);
      dz xhat, xhat = ((h - mean) invstd): the fp32 mean shifts h - mean by km u |mean|, the difference, the product with
      invstd and the final product round once each, invstd carries ki u: e1 = e0 |xhat| + u |dz| (km |mean| invstd + (3 + ki) |xhat|).
    dbeta = sum dz: u |ref| + E0, E0 = sum e0 + N53 sum|dz|; dgamma = sum dz xhat: u |ref| + E1 likewise.
    coefs (BwdCoefFin, fp64 from fp32 inputs, one rounding): c_sc, c_sh are the given scale / shift bit for bit;
      c_g = gamma invstd: (1 + ki) u |ref|;   c_a = -gi m2 invstd: (1 + 2 ki) u |ref| + |gi| invstd E1 / R;
      c_b = -gi m1 + gi m2 invstd mean, T1 = |gi m1|, T2 = |gi m2 invstd mean|:
            u (T1 + T2) + ki u T1 + (2 ki + km) u T2 + |gi| (E0 + invstd |mean| E1) / R.
      training = 0: c_g = the given scale, c_a = c_b = 0, exactly.
    dh rebuilt in fp64 as c_g dz + c_a h + c_b from the returned rows: within e(c_g) |dz| + e(c_a) |h| + e(c_b) of the fp64 dh.
dc_vn_apply, out = y s, s = relu(fmaf(scale, n, shift)) / max(n, 1e-8), scale / shift as given: n carries 3 u, so
    z is off by 3 u |scale| n + u |z| and relu (1-Lipschitz) passes at most that on; the clamped denominator carries 3 u, the
    quotient u, the combination of y u, the product u: e = |y_comp| ((3 u |scale| n + u |z|) / nc + 6 u s).  A zero vector has
    bound 0: the output is exactly 0.  relu and the clamp are continuous: no element is excluded.
dc_vn_backward (held by tests/test_gpu_sync_bn.py in its split form; here for the layout of d(P, Q): row u = [dy_u | dy_v], row v =
    [dy_v | -dy_u], blocked or interleaved).  Bounds of that test, unchanged: per component
      (8 u + 2 rho) [ |gi| (G / nc + |m1| + (n + |mean|) invstd (|m2| + |nhat| |m1|)) + (|d| + G / nc) Z / nc ],
    G = |y_u d_u| + |y_v d_v|, Z = |scale| (n + |mean|) + |beta|; dbeta: 6 u sum G / nc; dgamma: (8 u + rho) sum (G / nc) (n + |mean|) invstd
    over the points with z > 0.  The gate z > 0 is discontinuous: the generator keeps |z| above (2^-18 + 4 rho) Z (it scales
    a vector that is too near out of the band; where that vector is a zero one, z = shift, it moves the column's beta by 0.07), asserted.
dc_bn_act_pool.  Elements y with their bound e as dc_bn_act.  max: |got - max y| <= max e over the cloud's column.  mean:
    a lane adds ceil(N / 16) terms into 0.f (ceil(N / 16) - 1 roundings), 15 adds join the lanes, one division:
    ((ceil(N / 16) + 15) u sum|y| + sum e) / N.  arg: y at the returned row is within 2 max e of max y; where the runner-up
    (the largest y below the maximum) is more than 2 max e away, the row is the LOWEST row that attains the maximum (rows
    that hold the same fp32 input tie in fp32 as well); otherwise the pair is undecided (share asserted <= 0.1 %).
dc_bn_act_pool_backward.  dy = (arg == row ? dmax : 0) + dmean / N: the division rounds (u |dmean / N|), the add rounds
    where both are non-zero (u |dy|): eg.  dz, the sums, dgamma, dbeta as above with e0 = act' eg + u |dz| [act' != 1].
    dh = gi (dz - m1 - xhat m2) (BnActBwdBody's arithmetic): 8 u |gi| (|dz| + |m1| + (|h| + |mean|) invstd |m2|) as
    tests/test_gpu_sync_bn.py holds it for given m1, m2, plus what reaches it from before: |gi| (act' eg + E0 / R + |xhat| E1 / R).
    training = 0: dh = scale dz, the inference scale carries 4 u, dz and the product one each: 6 u |ref| + |scale| act' eg.
dc_cloud_bias_add: one IEEE add: the bits of torch's fp32 add.  dc_cloud_colsum: fp64 sum, one rounding: u |ref| + N53 sum|x|.

Data (as tests/test_gpu_sync_bn.py): column standard deviations log-uniform over 1e-3 .. 1e3, column means up to 30 standard
deviations of either sign, gamma of both signs, |beta| >= 0.02.  act' jumps at z = 0: the generator keeps |z| above
2^-18 (|scale h| + |mean scale| + |beta|) = 64 u of the magnitudes of z's terms for the batch AND the inference coefficients
(the fp32 coefficients move z by at most 5 u of them) and `RowCase` asserts that on the fp64 data; no element is excluded.
One row (R = 1): h = mean, z = beta up to the cancellation of scale h - mean scale with invstd = eps^-1/2 = 316: the margin
holds only for |h| <= 1, which is what the generator draws there.  Vectors: one exactly-zero vector per 64 points, one with
|y| ~ 1e-9 (clamped denominator; its squares are normal numbers)."""
import functools

import torch

U = 2.0 ** -24
O2 = 1.0 + 2.0 ** -20
_f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
EPS, MOM = _f32(1e-5), _f32(0.1)                     # the ABI takes eps, momentum and slopes as float
SLOPES = (_f32(0.2), 0.0, 1.0)
SLOPE = SLOPES[0]
VEC_EPS = _f32(1e-8)
RT = CT = 16


def n53(rows):
    return (rows + 80) * 2.0 ** -53


# ---- the tilings, restated from colreduce.h / nn.hip (the tests assert the chunk counts they mean to reach) ---------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def rows_per_chunk(R, C, blocks=768):                # colreduce.h: rows_per_chunk
    rpc = cdiv(R * cdiv(C, CT * 4) // blocks, RT) * RT
    return min(max(rpc, RT), 512)


def chunks_of(R, C):
    return cdiv(R, rows_per_chunk(R, C))


def tile_rows(R, C, V):                              # nn.hip: run_tile
    rpc = cdiv(R * cdiv(C, CT * V) // 1024, RT) * RT
    return min(max(rpc, RT), 1024)


def cloud_chunks(B, mx, C):                          # nn.hip: cloud_colsum_chunks, dc_cloud_colsum -> (rows per chunk, chunks used)
    want = max(1, 768 // max(1, B * cdiv(C, CT * 4)))
    chunks = max(1, min(want, cdiv(mx, RT)))
    rpc = cdiv(cdiv(mx, chunks), RT) * RT
    return rpc, cdiv(mx, rpc)


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def stats_ref(v, gamma, beta, mom, rm0, rv0, mut=(), vec=False):
    """Two-pass fp64 statistics of the columns of v [R, C] -> {name: (ref, bound)}; vec: v holds fp32-formed norms."""
    v = v.double()
    R = v.shape[0]
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    invstd = (var + EPS).rsqrt()
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    scale = g * invstd
    ms = mean * scale
    if vec:
        en, en2 = v.abs().mean(0), (v * v).mean(0) + mean * mean
        em, rho, ev = 3 * U * en, 2 * U + 6 * U * en2 / (2 * (var + EPS)), 6 * U * en2
    else:
        em, rho, ev = torch.zeros_like(mean), torch.full_like(mean, 2 * U), torch.zeros_like(mean)
    out = dict(mean=(mean, 2 * U * mean.abs() + em), invstd=(invstd, rho * invstd), scale=(scale, rho * scale.abs()),
               shift=(b - ms, 2 * U * (b.abs() + ms.abs()) + scale.abs() * em + (rho - 2 * U) * ms.abs()), var=(var, None))
    if rm0 is not None:
        k = R / (R - 1) if R > 1 and "biased_running_var" not in mut else 1.0
        a, c = (1 - mom) * rm0.double(), (1 - mom) * rv0.double()
        out["rm"] = (a + mom * mean, 2 * U * (a.abs() + (mom * mean).abs()) + mom * em)
        out["rv"] = (c + mom * k * var, 2 * U * (c.abs() + mom * k * var) + mom * k * ev)
    return out


def eval_ref(gamma, beta, rm, rv):
    rm, rv = rm.double(), rv.double()
    g = gamma.double() if gamma is not None else torch.ones_like(rm)
    b = beta.double() if beta is not None else torch.zeros_like(rm)
    invstd = (rv + EPS).rsqrt()
    t = rm * g * invstd
    return dict(mean=(rm, torch.zeros_like(rm)), invstd=(invstd, 3 * U * O2 * invstd), scale=(g * invstd, 4 * U * O2 * (g * invstd).abs()),
                shift=(b - t, U * O2 * (b.abs() + 6 * t.abs())))


def check_coef(ck, tag, got, ref):
    for name, (val, bound) in ref.items():
        if bound is not None and got.get(name) is not None:
            ck.hold(f"{tag} {name}", got[name], val, bound)


# ---- y = act(scale h + shift) (+ residual) ------------------------------------------------------------------------------------------
def act_ref(x, scale, shift, slope, res=None, mut=()):
    """scale / shift: the fp32 coefficients the call is given.  -> (y, bound, z)"""
    z = scale.double() * x.double() + shift.double()
    if res is not None and "residual_before_act" in mut:
        z = z + res.double()
    a = torch.where(z > 0, z, slope * z)
    e = U * a.abs() * (1.0 + ((z <= 0) & (slope != 1.0)).double())
    y = a
    if res is not None:
        if "residual_before_act" not in mut:
            y = a + res.double()
        e = e + U * y.abs()
    return y, O2 * e, z


# ---- BatchNorm backward: the two column sums and what the finalisers make of them -------------------------------------------------
def bwd_ref(x, dy, st, gamma, slope, training, km, ki, eg=None, mut=()):
    """st: the fp64 coefficients {mean, invstd, scale, shift}; dy: fp64 gradient [R, C] with per-element error eg (None: exact).
    -> dict of (ref, bound) pairs and the pieces the checks need."""
    x, R = x.double(), x.shape[0]
    mean, invstd, scale, shift = st["mean"], st["invstd"], st["scale"], st["shift"]
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    z = scale * x + shift
    da = torch.where(z > 0, 1.0, slope)
    dz = dy * da
    xhat = (x - mean) * invstd
    e0 = U * dz.abs() * (da != 1.0).double() + (da * eg if eg is not None else 0.0)
    e1 = e0 * xhat.abs() + U * dz.abs() * (km * mean.abs() * invstd + (3 + ki) * xhat.abs())
    S0, S1 = dz.sum(0), (dz * xhat).sum(0)
    E0 = O2 * (e0.sum(0) + n53(R) * dz.abs().sum(0))
    E1 = O2 * (e1.sum(0) + n53(R) * (dz * xhat).abs().sum(0))
    gi, m1, m2 = g * invstd, S0 / R, S1 / R
    out = dict(dbeta=(S0, U * S0.abs() + E0), dgamma=(S1, U * S1.abs() + E1))
    zero = torch.zeros_like(mean)
    if training and "eval_in_training" not in mut:
        m2u = zero if "drop_m2" in mut else m2
        ca, t1, t2 = -gi * m2u * invstd, (gi * m1).abs(), (gi * m2u * invstd * mean).abs()
        out["c_g"] = (gi, (1 + ki) * U * O2 * gi.abs())
        out["c_a"] = (ca, (1 + 2 * ki) * U * O2 * ca.abs() + gi.abs() * invstd * E1 / R)
        out["c_b"] = (-gi * m1 + gi * m2u * invstd * mean,
                      U * O2 * ((1 + ki) * t1 + (1 + 2 * ki + km) * t2) + gi.abs() * (E0 + invstd * mean.abs() * E1) / R)
        dh = gi * (dz - m1 - xhat * m2u)
        e_dh = 8 * U * gi.abs() * (dz.abs() + m1.abs() + (x.abs() + mean.abs()) * invstd * m2.abs()) \
            + gi.abs() * ((da * eg if eg is not None else 0.0) + E0 / R + xhat.abs() * E1 / R)
    else:
        out["c_g"], out["c_a"], out["c_b"] = (scale, None), (zero, zero), (zero, zero)
        dh = scale * dz
        e_dh = 6 * U * O2 * dh.abs() + scale.abs() * (da * eg if eg is not None else 0.0)
    out["dh"] = (dh, e_dh)
    out["dz"], out["x"] = dz, x
    return out


def check_reduce(ck, tag, got, ref, co, training, grads=True):
    """got: dgamma, dbeta (None where NULL was passed), coefs [5, C]; co: the fp32 coefficients the call was given."""
    if grads:
        ck.hold(f"{tag} dbeta", got["dbeta"], *ref["dbeta"])
        ck.hold(f"{tag} dgamma", got["dgamma"], *ref["dgamma"])
    rows = got["coefs"]
    ck.exact(f"{tag} c_sc is the given scale", rows[0], co["scale"])
    ck.exact(f"{tag} c_sh is the given shift", rows[1], co["shift"])
    if training:
        ck.hold(f"{tag} c_g", rows[2], *ref["c_g"])
    else:
        ck.exact(f"{tag} c_g is the given scale", rows[2], co["scale"])
    ck.hold(f"{tag} c_a", rows[3], *ref["c_a"])
    ck.hold(f"{tag} c_b", rows[4], *ref["c_b"])
    r5 = rows.double()
    e = [ref[n][1] if ref[n][1] is not None else 4 * U * O2 * ref[n][0].abs() for n in ("c_g", "c_a", "c_b")]
    ck.hold(f"{tag} dh rebuilt from the coefficient rows", r5[2] * ref["dz"] + r5[3] * ref["x"] + r5[4], ref["dh"][0],
            e[0] * ref["dz"].abs() + e[1] * ref["x"].abs() + e[2])


# ---- the vector block ---------------------------------------------------------------------------------------------------------------
def vn_y(t, co, combine, mut=()):
    """The fp64 (yu, yv) [n, co] each of the input layout (nn.hip: vn_load_y; 1: [P | Q] blocked, 2: interleaved)."""
    t = t.double()
    u, v = t[0::2], t[1::2]
    if combine == 0:
        return u, v
    if "swap_layouts" in mut:
        combine = 3 - combine
    pu, qu, pv, qv = (u[:, :co], u[:, co:], v[:, :co], v[:, co:]) if combine == 1 else (u[:, 0::2], u[:, 1::2], v[:, 0::2], v[:, 1::2])
    return pu - qv, pv + qu


def vn_stats_ref(t, co, combine, gamma, beta, mom, rm0, rv0, mut=()):
    yu, yv = vn_y(t, co, combine, mut)
    return stats_ref((yu * yu + yv * yv).sqrt(), gamma, beta, mom, rm0, rv0, mut, vec=True)


def vn_apply_ref(t, co, combine, scale, shift, mut=()):
    """-> (out [2n, co], bound)"""
    yu, yv = vn_y(t, co, combine, mut)
    n = (yu * yu + yv * yv).sqrt()
    nc = n.clamp_min(VEC_EPS)
    z = scale.double() * n + shift.double()
    s = z.clamp_min(0) / nc
    k = O2 * ((3 * U * scale.double().abs() * n + U * z.abs()) / nc + 6 * U * s)
    il = lambda a, b: torch.stack([a, b], 1).reshape(2 * a.shape[0], co)
    return il(yu * s, yv * s), il(yu.abs() * k, yv.abs() * k)


def vn_dpq(gu, gv, combine, mut=()):
    """(dy_u, dy_v) [n, co] each -> the gradient in the layout of the input (nn.hip: VnBwdBody; the transpose of vn_combine)."""
    n, co = gu.shape
    second = gu if "dpq_sign" in mut else -gu
    if combine == 0:
        return torch.stack([gu, gv], 1).reshape(2 * n, co)
    if combine == 1:
        return torch.stack([torch.cat([gu, gv], 1), torch.cat([gv, second], 1)], 1).reshape(2 * n, 2 * co)
    il = lambda p, q: torch.stack([p, q], 2).reshape(n, 2 * co)
    return torch.stack([il(gu, gv), il(gv, second)], 1).reshape(2 * n, 2 * co)


def vn_pieces(t, co, combine, gamma, beta):
    """The fp64 quantities of the vector block that the kink margin and the backward bound share."""
    yu, yv = vn_y(t, co, combine)
    n = (yu * yu + yv * yv).sqrt()
    st = stats_ref(n, gamma, beta, MOM, None, None, vec=True)
    mean, invstd, scale, shift = (st[k][0] for k in ("mean", "invstd", "scale", "shift"))
    rho = st["invstd"][1] / invstd
    return dict(yu=yu, yv=yv, n=n, mean=mean, invstd=invstd, scale=scale, shift=shift, rho=rho, z=scale * n + shift,
                Z=scale.abs() * (n + mean.abs()) + beta.double().abs())


def vn_bwd_ref(cs, out_combine, training, mut=()):
    """-> {din, dgamma, dbeta: (ref, bound)}: the closed form of nn_math.h: vn_bwd_dy in fp64, the bounds of tests/test_gpu_sync_bn.py."""
    p = cs.pieces
    yu, yv, n, mean, invstd, scale, rho, z = (p[k] for k in ("yu", "yv", "n", "mean", "invstd", "scale", "rho", "z"))
    du, dv = cs.dout.double()[0::2], cs.dout.double()[1::2]
    nc = n.clamp_min(VEC_EPS)
    gate = (z > 0).double()
    gs, G = yu * du + yv * dv, (yu * du).abs() + (yv * dv).abs()
    dz, nhat = gate * gs / nc, (n - mean) * invstd
    m1, m2 = dz.mean(0), (dz * nhat).mean(0)
    gi = cs.gamma.double() * invstd
    r = z.clamp_min(0)
    dn = (gi * (dz - m1 - nhat * m2) if training else scale * dz) - torch.where(n > VEC_EPS, gs * r / (nc * nc), 0.0)
    w = torch.where(n > 0, dn / nc, 0.0)
    s = r / nc
    a0 = gate * G / nc
    a1 = a0 * (n + mean.abs()) * invstd
    k = 8 * U + 2 * rho
    common = k * gi.abs() * (G / nc + m1.abs() + (n + mean.abs()) * invstd * (m2.abs() + nhat.abs() * m1.abs()))
    bu, bv = common + k * (du.abs() + G / nc) * p["Z"] / nc, common + k * (dv.abs() + G / nc) * p["Z"] / nc
    return dict(din=(vn_dpq(du * s + w * yu, dv * s + w * yv, out_combine, mut), vn_dpq(bu, bv, out_combine, ("dpq_sign",))),
                dbeta=(dz.sum(0), 6 * U * a0.sum(0)), dgamma=((dz * nhat).sum(0), (8 * U + rho) * a1.sum(0)))


# ---- the embedding head -------------------------------------------------------------------------------------------------------------
def pool_ref(x, B, N, scale, shift, slope, mut=()):
    y, e, _ = act_ref(x, scale, shift, slope)
    C = x.shape[1]
    y, e = y.view(B, N, C), e.view(B, N, C)
    ymax, emax = y.max(1).values, e.max(1).values
    rows = torch.arange(N)[None, :, None].expand(B, N, C)
    at = y == ymax[:, None, :]
    first = torch.where(at, rows, N).min(1).values
    if "tie_to_highest" in mut:
        first = torch.where(at, rows, -1).max(1).values
    second = torch.where(at, torch.full_like(y, float("-inf")), y).max(1).values
    terms = cdiv(N, RT) + RT - 1
    return dict(y=y, ymax=ymax, emax=emax, first=first, decided=(ymax - second) > 2 * emax, ties=at.sum(1) > 1,
                mean=(y.sum(1) / N, O2 * (terms * U * y.abs().sum(1) + e.sum(1)) / N))


def check_pool(ck, tag, pooled, arg, ref, with_mean):
    """-> the share of (cloud, column) pairs whose row fp64 cannot decide."""
    B, N, C = ref["y"].shape
    ck.hold(f"{tag} max", pooled[:, :C], ref["ymax"], ref["emax"])
    if with_mean:
        ck.hold(f"{tag} mean", pooled[:, C:2 * C], *ref["mean"])
    a = arg.long()
    ck.true(f"{tag} arg in range", bool(((a >= 0) & (a < N)).all()))
    ya = ref["y"].gather(1, a.clamp(0, N - 1)[:, None, :])[:, 0]
    ck.hold(f"{tag} arg: its fp64 value against the fp64 maximum", ya, ref["ymax"], 2 * ref["emax"])
    dec = ref["decided"]
    ck.true(f"{tag} arg: the lowest maximal row wherever fp64 decides", bool((a[dec] == ref["first"][dec]).all()))
    und = 1.0 - float(dec.double().mean())
    print(f"[{ck.what}] {tag} arg: undecided share {und:.5f} (cap 0.001), exact ties in {int((ref['ties'] & dec).sum())} of {B * C} pairs")
    ck.true(f"{tag} arg: undecided share within 0.1 %", und <= 1e-3)
    return und


def pool_dy(dp, arg, B, N, C, with_mean, mut=()):
    """The rebuilt gradient in fp64 [B * N, C] and its error bound (two roundings)."""
    dmax = dp[:, :C].double()
    dme = dp[:, C:2 * C].double() / (1 if "dmean_not_divided" in mut else N) if with_mean else torch.zeros_like(dmax)
    dme_rows = dme[:, None, :].expand(B, N, C).clone()
    if "neighbour_cloud_mean" in mut and B > 1:      # the first row of a cloud keeps the previous cloud's cached value
        dme_rows[1:, 0] = dme[:-1]
    sel = (arg.long()[:, None, :] == torch.arange(N)[None, :, None]).double() * dmax[:, None, :]
    g = sel + dme_rows
    eg = U * dme_rows.abs() + U * g.abs() * ((sel != 0) & (dme_rows != 0)).double()
    return g.reshape(B * N, C), eg.reshape(B * N, C)


def pool_dy32(dp, arg, B, N, C, with_mean):
    """The same gradient materialised in fp32 by the same two operations (a division, an add)."""
    dmax = dp[:, :C]
    dme = dp[:, C:2 * C] / torch.tensor(float(N), dtype=torch.float32) if with_mean else torch.zeros_like(dmax)
    hit = arg.long()[:, None, :] == torch.arange(N)[None, :, None]
    return (torch.where(hit, dmax[:, None, :].expand(B, N, C), torch.zeros(())) + dme[:, None, :]).reshape(B * N, C).contiguous()


def hand_args(B, N, C):
    """An arg-max table that owes nothing to a forward pass: row 0, row N - 1 and the rows on either side of every boundary
    between row chunks of the reduction (rows_per_chunk) and of the tile kernel (tile_rows, V = 4 and 1), cycled over (b, c)."""
    R = B * N
    cuts = {0, R - 1}
    for rpc in {rows_per_chunk(R, C), tile_rows(R, C, 4), tile_rows(R, C, 1)}:
        for r in range(rpc, R, rpc):
            cuts.update((r - 1, r))
    table = torch.empty(B, C, dtype=torch.int32)
    for b in range(B):
        mine = sorted({0, N - 1} | {r - b * N for r in cuts if b * N <= r < (b + 1) * N})
        table[b] = torch.tensor([mine[(c + b) % len(mine)] for c in range(C)], dtype=torch.int32)
    return table


# ---- data -------------------------------------------------------------------------------------------------------------------------
def affine(c):
    g = torch.linspace(0.4, 1.6, c)
    g[::5] *= -1
    b = torch.linspace(-0.3, 0.3, c)
    return g, torch.where(b.abs() < 0.02, torch.full_like(b, 0.02), b)


def near_kink(x, st, beta):
    """|z| of the fp64 data against 64 u of the magnitudes of its terms -> mask of the elements that are too near."""
    z = st["scale"] * x.double() + st["shift"]
    return z.abs() < 2.0 ** -18 * ((st["scale"] * x.double()).abs() + (st["mean"] * st["scale"]).abs() + beta.double().abs())


class RowCase:
    """h [R, C] with its gradient, residual, affine parameters and running pair; clouds = (B, N): rows of equal clouds, with
    exact ties at the maximum of every third column (rows 1, 18 and 33 of a cloud repeat the column's best value)."""

    def __init__(self, R, C, seed, clouds=None, stats_only=False):
        self.R, self.C, self.clouds = R, C, clouds
        g = torch.Generator().manual_seed(seed)
        self.gamma, self.beta = affine(C)
        perm = lambda: torch.randperm(C, generator=g)
        if R == 1:
            sd = torch.full((C,), 0.1)
            x = torch.rand(1, C, generator=g) * 2 - 1
        else:
            sd = 10.0 ** torch.linspace(-3, 3, C)[perm()]
            x = sd * torch.linspace(-30, 30, C)[perm()] + sd * torch.randn(R, C, generator=g)
        x = x.float()
        if clouds is not None and clouds[1] > 1:
            B, N = clouds
            xv = x.view(B, N, C)
            best = (xv * self.gamma.sign()).argmax(1, keepdim=True)            # act is monotone: the row of the largest y
            for r in (1, 18, 33):
                if r < N:
                    xv[:, r, ::3] = xv.gather(1, best)[:, 0, ::3]
        m64, v64 = x.double().mean(0), x.double().var(0, unbiased=False)
        self.rm0 = (m64 + 0.3 * sd * torch.randn(C, generator=g)).float()
        self.rv0 = ((v64 + 0.01 * sd * sd) * torch.exp(0.5 * torch.randn(C, generator=g))).float()
        self.ev = {k: v[0] for k, v in eval_ref(self.gamma, self.beta, self.rm0, self.rv0).items()}
        if stats_only:               # the one large case runs dc_bn_stats alone: no gate, no gradient
            self.x = x
            return
        for _ in range(40):
            near = near_kink(x, self.train_stats(x), self.beta) | near_kink(x, self.ev, self.beta)
            if not near.any():
                break
            x = torch.where(near, x + (0.37 * sd).float(), x)
        else:
            raise AssertionError("could not move the data off the kink")
        self.x = x
        self.tr = self.train_stats(x)
        assert not near_kink(x, self.tr, self.beta).any() and not near_kink(x, self.ev, self.beta).any()
        amp = 10.0 ** torch.linspace(-2, 2, C)
        self.dy = (amp[perm()] * torch.randn(R, C, generator=g)).float()
        self.res = (amp[perm()] * torch.randn(R, C, generator=g)).float()
        if clouds is not None:
            self.dp = (amp[perm()].repeat(2) * torch.randn(clouds[0], 2 * C, generator=g)).float()

    def train_stats(self, x):
        return {k: v[0] for k, v in stats_ref(x, self.gamma, self.beta, MOM, None, None).items()}


@functools.lru_cache(maxsize=None)
def row_case(R, C, stats_only=False):
    return RowCase(R, C, seed=1000 + 7 * R + C, stats_only=stats_only)


@functools.lru_cache(maxsize=None)
def pool_case(B, N, C):
    return RowCase(B * N, C, seed=5000 + 131 * B + 7 * N + C, clouds=(B, N))


class VecCase:
    """t [2n, co or 2 co]: components with standard deviations log-uniform over 1e-2 .. 1e2 around a constant vector of up to 30
    standard deviations; exactly-zero vectors and vectors of norm ~1e-9."""

    def __init__(self, n, co, combine, seed):
        self.n, self.co, self.combine = n, co, combine
        g = torch.Generator().manual_seed(seed)
        perm = lambda: torch.randperm(co, generator=g)
        sd = 10.0 ** torch.linspace(-2, 2, co)[perm()]
        off = sd * torch.linspace(0, 30, co)[perm()]
        th = torch.rand(co, generator=g) * 6.2831853
        yu = off * th.cos() + sd * torch.randn(n, co, generator=g)
        yv = off * th.sin() + sd * torch.randn(n, co, generator=g)
        qu, qv = 0.3 * sd * torch.randn(n, co, generator=g), 0.3 * sd * torch.randn(n, co, generator=g)
        self.zero, self.tiny = list(range(n - 1, -1, -64)), list(range(n - 3, -1, -64))
        for i in self.zero:
            yu[i], yv[i], qu[i], qv[i] = 0.0, 0.0, 0.0, 0.0
        for i in self.tiny:
            yu[i], yv[i], qu[i], qv[i] = 6e-10, -8e-10, 0.0, 0.0
        if combine == 0:
            t = torch.stack([yu, yv], 1).reshape(2 * n, co)
        else:
            pu, pv = yu + qv, yv - qu
            if combine == 1:
                t = torch.stack([torch.cat([pu, qu], 1), torch.cat([pv, qv], 1)], 1).reshape(2 * n, 2 * co)
            else:
                il = lambda p, q: torch.stack([p, q], 2).reshape(n, 2 * co)
                t = torch.stack([il(pu, qu), il(pv, qv)], 1).reshape(2 * n, 2 * co)
        t = t.float()
        self.gamma, self.beta = affine(co)
        k = 1 if combine == 0 else 2
        for _ in range(40):           # keep z = scale |y| + shift off the kink of the ReLU (the gate of the backward)
            p = vn_pieces(t, co, combine, self.gamma, self.beta)
            near = p["z"].abs() < (2.0 ** -18 + 4 * p["rho"]) * p["Z"]
            if not near.any():
                break
            fixed = torch.tensor(self.zero + self.tiny)
            stuck = near[fixed].any(0)                # a zero vector cannot be scaled away: z = shift there, so beta moves instead
            self.beta = torch.where(stuck, self.beta + 0.07, self.beta)
            near[fixed] = False
            # scale a vector that is too near by just enough to leave the band (8 x its half width, away from the root of z):
            # a larger step would move the column's statistics by more than the band and push other vectors into it
            band = (2.0 ** -18 + 4 * p["rho"]) * p["Z"] / (p["scale"].abs() * p["n"]).clamp_min(1e-30)
            f = torch.where(near, 1.0 + (p["z"] * p["scale"]).sign() * 8 * band, torch.ones_like(band)).clamp(0.5, 2.0)
            m = f.repeat_interleave(2, 0)
            m = m if combine == 0 else (torch.cat([m, m], 1) if combine == 1 else m.repeat_interleave(2, 1))
            t = (t.double() * m).float()
        else:
            raise AssertionError("could not move the data off the kink")
        self.t, self.pieces = t, vn_pieces(t, co, combine, self.gamma, self.beta)
        assert not (self.pieces["z"].abs() < (2.0 ** -18 + 4 * self.pieces["rho"]) * self.pieces["Z"]).any()
        self.dout = ((10.0 ** torch.linspace(-2, 2, co)[perm()]) * torch.randn(2 * n, co, generator=g)).float()
        self.rm0 = (off + sd).float()
        self.rv0 = (sd * sd * torch.exp(0.5 * torch.randn(co, generator=g))).float()


@functools.lru_cache(maxsize=None)
def vec_case(n, co, combine):
    return VecCase(n, co, combine, seed=500 + 10 * co + combine + 3 * n)


class CloudCase:
    def __init__(self, B, mx, C, seed):
        g = torch.Generator().manual_seed(seed)
        amp = 10.0 ** torch.linspace(-2, 2, C)[torch.randperm(C, generator=g)]
        self.B, self.mx, self.C = B, mx, C
        self.h = (amp * (3.0 + torch.randn(B * mx, C, generator=g))).float()
        self.g = (amp * torch.randn(B, C, generator=g)).float()


@functools.lru_cache(maxsize=None)
def cloud_case(B, mx, C):
    return CloudCase(B, mx, C, seed=9000 + 17 * B + mx + C)


# ---- drivers: every call of a family through a backend (CPU fp32 tensors of the logical shapes in and out) ---------------------------
STATS_VARIANTS = (("affine running", True, True, MOM), ("plain running mom 1", False, True, 1.0), ("affine no running", True, False, MOM))


def _co32(got):
    return {k: got[k] for k in ("mean", "invstd", "scale", "shift")}


def run_rows(be, cs, ck, full=True):
    """dc_bn_stats, dc_bn_eval_coeffs, dc_bn_act / dc_bn_act2, dc_bn_act_backward_reduce on one RowCase -> {name: raw result}."""
    out = {}
    co = None
    for tag, aff, run, mom in STATS_VARIANTS:
        g, b = (cs.gamma, cs.beta) if aff else (None, None)
        rm0, rv0 = (cs.rm0, cs.rv0) if run else (None, None)
        got = be.bn_stats(cs.x, g, b, mom, rm0, rv0)
        check_coef(ck, f"dc_bn_stats {tag}", got, stats_ref(cs.x, g, b, mom, rm0, rv0))
        out.update({f"stats {tag} {k}": v for k, v in got.items() if v is not None})
        co = co or _co32(got)
        if not full:
            return out
    ev = be.eval_coeffs(cs.gamma, cs.beta, cs.rm0, cs.rv0)
    check_coef(ck, "dc_bn_eval_coeffs", ev, eval_ref(cs.gamma, cs.beta, cs.rm0, cs.rv0))
    ev0 = be.eval_coeffs(None, None, cs.rm0, cs.rv0)
    check_coef(ck, "dc_bn_eval_coeffs plain", ev0, eval_ref(None, None, cs.rm0, cs.rv0))
    out.update({f"eval {k}": v for k, v in ev.items()})
    for slope, res, second in [(SLOPE, None, False), (SLOPE, None, True), (SLOPE, cs.res, False), (SLOPE, cs.res, True),
                               (0.0, cs.res, True), (1.0, cs.res, True), (0.0, None, False), (1.0, None, False)]:
        tag = f"dc_bn_act slope {slope:.1f}{' residual' if res is not None else ''}{' two destinations' if second else ''}"
        y, y2 = be.bn_act(cs.x, co["scale"], co["shift"], slope, res, second)
        val, bound, _ = act_ref(cs.x, co["scale"], co["shift"], slope, res)
        ck.hold(tag, y, val, bound)
        if second:
            ck.exact(tag + ": second copy", y2, y)
        out[tag] = y
    for training, slope, grads in [(1, SLOPE, True), (1, 0.0, True), (1, 1.0, True), (0, SLOPE, True), (1, SLOPE, False)]:
        tag = f"dc_bn_act_backward_reduce training {training} slope {slope:.1f}{'' if grads else ' no grads'}"
        c32, st, km, ki = (co, cs.tr, 1, 1) if training else (ev, cs.ev, 0, 3)
        got = be.bwd_reduce(cs.dy, cs.x, c32, cs.gamma, slope, training, grads)
        check_reduce(ck, tag, got, bwd_ref(cs.x, cs.dy.double(), st, cs.gamma, slope, training, km, ki), c32, training, grads)
        out.update({f"{tag} {k}": v for k, v in got.items() if v is not None})
    return out


def run_vec(be, cs, ck):
    """dc_vn_stats, dc_vn_apply and dc_vn_backward (combine 3: y in, interleaved d(P, Q) out) on one VecCase."""
    out = {}
    co = None
    for tag, aff, run, mom in STATS_VARIANTS:
        g, b = (cs.gamma, cs.beta) if aff else (None, None)
        rm0, rv0 = (cs.rm0, cs.rv0) if run else (None, None)
        got = be.vn_stats(cs.t, cs.co, cs.combine, g, b, mom, rm0, rv0)
        check_coef(ck, f"dc_vn_stats {tag}", got, vn_stats_ref(cs.t, cs.co, cs.combine, g, b, mom, rm0, rv0))
        out.update({f"vn stats {tag} {k}": v for k, v in got.items() if v is not None})
        co = co or _co32(got)
    for tag, sc, sh in (("batch coefficients", co["scale"], co["shift"]), ("bias mode", torch.ones(cs.co), cs.beta - 0.2)):
        got = be.vn_apply(cs.t, cs.co, cs.combine, sc, sh)
        val, bound = vn_apply_ref(cs.t, cs.co, cs.combine, sc, sh)
        ck.hold(f"dc_vn_apply {tag}", got, val, bound)
        zero = torch.tensor(sorted(2 * i + d for i in cs.zero for d in (0, 1)))
        ck.true(f"dc_vn_apply {tag}: zero vectors give exact zeros", bool((got[zero] == 0).all()) and bool((bound[zero] == 0).all()))
        out[f"vn apply {tag}"] = got
    for oc, training in [(cs.combine, 1), (cs.combine, 0)] + ([(3, 1)] if cs.combine == 0 else []):
        tag = f"dc_vn_backward combine {oc} training {training}"
        got = be.vn_bwd(cs.dout, cs.t, cs.co, oc, co, cs.gamma, training)
        ref = vn_bwd_ref(cs, 2 if oc == 3 else oc, training)
        for name in ("din", "dgamma", "dbeta"):
            ck.hold(f"{tag} {name}", got[name], *ref[name])
        out.update({f"{tag} {k}": v for k, v in got.items()})
    return out


def run_pool(be, cs, ck):
    """dc_bn_act_pool and dc_bn_act_pool_backward on one RowCase with clouds -> ({name: raw result}, worst undecided share)."""
    (B, N), C = cs.clouds, cs.C
    out, und = {}, 0.0
    tr = _co32(be.bn_stats(cs.x, cs.gamma, cs.beta, MOM, None, None))
    ev = be.eval_coeffs(cs.gamma, cs.beta, cs.rm0, cs.rv0)
    args = {}
    for mode, c32 in (("batch", tr), ("inference", ev)):
        for slope in (SLOPE, 0.0):
            ref = pool_ref(cs.x, B, N, c32["scale"], c32["shift"], slope)
            for wm in (1, 0):
                tag = f"dc_bn_act_pool {mode} slope {slope:.1f} with_mean {wm}"
                pooled, arg = be.pool(cs.x, B, N, c32["scale"], c32["shift"], slope, wm)
                und = max(und, check_pool(ck, tag, pooled, arg, ref, wm))
                out[tag], out[tag + " arg"] = pooled, arg
            if slope == SLOPE:
                args[mode] = arg
    hand = hand_args(B, N, C)
    for training, mode, c32, st, km, ki in ((1, "batch", tr, cs.tr, 1, 1), (0, "inference", ev, cs.ev, 0, 3)):
        for wm in (1, 0):
            for aname, arg in (("own rows", args[mode]), ("hand-made rows", hand)):
                tag = f"dc_bn_act_pool_backward training {training} with_mean {wm} {aname}"
                dp = cs.dp if wm else cs.dp[:, :C].contiguous()
                got = be.pool_bwd(dp, arg, cs.x, B, N, c32, cs.gamma, SLOPE, wm, training)
                g, eg = pool_dy(dp, arg, B, N, C, wm)
                ref = bwd_ref(cs.x, g, st, cs.gamma, SLOPE, training, km, ki, eg=eg)
                for name in ("dh", "dgamma", "dbeta"):
                    ck.hold(f"{tag} {name}", got[name], *ref[name])
                two = be.bwd(pool_dy32(dp, arg, B, N, C, wm), cs.x, c32, cs.gamma, SLOPE, training)
                for name in ("dh", "dgamma", "dbeta"):
                    ck.exact(f"{tag} {name} = dc_bn_act_backward on the fp32 gradient", got[name], two[name])
                out.update({f"{tag} {k}": v for k, v in got.items()})
    return out, und


def run_cloud(be, cs, ck):
    out = {}
    ref = cs.h + cs.g.repeat_interleave(cs.mx, 0)
    for alias in (False, True):
        got = be.cloud_bias_add(cs.h, cs.g, cs.mx, alias)
        ck.exact(f"dc_cloud_bias_add{' in place' if alias else ''}", got, ref)
        out[f"bias add {alias}"] = got
    got = be.cloud_colsum(cs.h, cs.B, cs.mx)
    h64 = cs.h.double().view(cs.B, cs.mx, cs.C)
    ck.hold("dc_cloud_colsum", got, h64.sum(1), U * h64.sum(1).abs() + n53(cs.mx) * h64.abs().sum(1))
    out["colsum"] = got
    return out


# ---- the cases both tests run ---------------------------------------------------------------------------------------------------------
CHANNELS = (64, 72, 8, 7, 23, 128, 256, 1024)
SMALL_ROWS = (1, 2, 15, 16, 17)                      # below, at and above one row lane set (RT = 16)
POOLS = ((1, 1), (7, 5), (3, 17), (4, 100), (2, 256), (2, 1030))             # (clouds, N)
CLOUDS = ((1, 1), (3, 17), (3, 1000), (800, 16))                             # (clouds, mx)


def row_counts(C):
    """The smallest row counts that change the tiling: 300 = 19 chunks with a tail of 12; 1040 at C <= 64 = 65 chunks (the
    finaliser's 64 lanes take a second stride); 4410 at C = 256 = 32 rows per chunk in the reduction and the tile kernel, tail 26."""
    if C == 1024:
        return SMALL_ROWS
    return SMALL_ROWS + (300,) + ((1040,) if C <= 64 else ()) + ((4410,) if C == 256 else ())


def assert_tilings():
    assert (rows_per_chunk(300, 64), chunks_of(300, 64), 300 - 18 * 16) == (16, 19, 12)
    assert all(chunks_of(1040, c) == 65 for c in (64, 8, 7, 23))
    assert (rows_per_chunk(4410, 256), tile_rows(4410, 256, 4), chunks_of(4410, 256), 4410 - 137 * 32) == (32, 32, 138, 26)
    assert (rows_per_chunk(24000, 1024), chunks_of(24000, 1024)) == (512, 47)
    assert cloud_chunks(800, 16, 64) == (16, 1) and cloud_chunks(3, 1000, 64)[1] > 1
    assert rows_per_chunk(7 * 5, 64) == 16                                   # N = 5: a thread's rows 16 apart lie in different clouds
