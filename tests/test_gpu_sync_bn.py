"""Synchronised BatchNorm (statistics over the global batch of a data-parallel run) against fp64, with UNEVEN ranks played by
one process.

Part A: the eleven split entry points through the C ABI.  The test itself is the all-reduce: it adds the first records of
the shards.  Data: column standard deviations log-uniform over 1e-3 .. 1e3, column means up to 30 standard deviations of
either sign (the cancellation of E[x^2] - mean^2 then costs fp64 < 1e-9 relative at these row counts, so every bound below
holds for the reference alone); errors are taken per column / per element, never over a whole tensor.  Activations are
discontinuous in their derivative at z = 0: the data keep |z| further from 0 than the fp32 evaluation error of z.

Part B: the Python paths of nn/fused.py (`_sync_stats` and every `group is not None` branch) under tests/sync_sim.py, uneven
shards, against the oracle on the whole batch, at the tolerances the suite already holds the per-rank path to.

u = 2^-24 is the unit roundoff of fp32.  Bounds of part A (R = rows of all ranks):
  sums            |got - ref| <= R 2^-51 sum|addend|  (addends x, x^2 are exact in fp64; vector form: + 3 u sum|addend| for the
                  fp32 norms and + 6 u for their squares, see _check_records)
  mean .. scale   2 u |ref|;   shift, running statistics, coefficient rows: 2 u (sum of the magnitudes of their terms)
  m1, m2          2 u |ref| + 2 u sum|addend| / R;     dbeta, dgamma: 2 u sum|addend|     (addends dz, dz xhat)
  dh (BatchNorm)  8 u |gamma invstd| (|dz| + |m1| + (|h| + |mean|) invstd |m2|): the forward error bound of the fp32 expression
                  gi * (dz - m1 - xhat * m2) with fp32-rounded coefficients; (|h| + |mean|) covers the cancellation in h - mean
  dy (vector)     see test_vn_backward_split
Every check prints its worst error / bound before anything is asserted.
"""
import copy
import functools
import time

import pytest
import torch
import torch.nn.functional as F

import oracle
from deltaconv_amd._lib import lib
from tests.helpers import rel_err
from tests.sync_sim import SyncSim

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SENT = 12345.0
EPS = float(torch.tensor(1e-5, dtype=torch.float32))        # the ABI takes eps and momentum as float
MOM = float(torch.tensor(0.1, dtype=torch.float32))
ROWS = [(1, 17, 300), (1, 1)]
CHANNELS = {"c64": (64, 64, 0), "c7": (7, 7, 0), "c64_ld70_off1": (64, 70, 1)}      # name -> (C, row stride, first column)


class _Checks:
    """Every figure is printed before anything is asserted; `done()` asserts them all."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def hold(self, name, got, ref, bound):
        got, ref, bound = (t.detach().double().cpu() for t in (got, ref, bound))
        err = (got - ref).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
        worst = float(ratio.max())
        print(f"[{self.what}] {name}: worst error / bound = {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name, worst))

    def same(self, name, a, b):
        if not torch.equal(a, b):
            self.bad.append((name, "bits"))

    def done(self):
        assert not self.bad, f"{self.what}: {self.bad}"


def _ws(rows, c):
    nb = lib.raw("dc_bn_workspace_bytes")(rows, c)
    return torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV), nb


def _all_reduce_first(recs):
    """The all-reduce, played by the test: the first records of the shards summed in rank order.  -> the sum as the first
    record of a copy of rank 0's buffer (its second record stays rank 0's own, as after the in-place all-reduce of nn/fused.py)."""
    buf = recs[0].clone()
    for rec in recs[1:]:
        buf[0] += rec[0]
    return buf[0]


def _affine(c):
    """gamma / beta as tests/test_gpu_nn.py:_pair sets them (negative gamma included)."""
    g = torch.linspace(0.4, 1.6, c)
    g[::5] *= -1
    return g, torch.linspace(-0.3, 0.3, c)


def _stats64(v, gamma, beta):
    """Two-pass fp64 statistics of the columns of v -> (mean, biased var, invstd, scale, shift)."""
    v = v.double()
    mean = v.mean(0)
    var = ((v - mean) ** 2).mean(0)
    invstd = (var + EPS).rsqrt()
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    return mean, var, invstd, g * invstd, b - mean * g * invstd


def _check_records(ck, rec, rows, s0, s1, extra=0.0, total_rows=None, tag=""):
    """rec [2, 2C+1]: two identical records, the rows slot exact, the sums within R 2^-51 (+ extra) of sum|addend|;
    s0 / s1: the fp64 addends [rows, C].  extra (vector form): 3 u for the fp32 norms n, hence 6 u for their squares --
    (n (1 + 3 u))^2 = n^2 (1 + 6 u); with 3 u the sum of squares reaches 1.21 of the bound on a single point ((M, N, K) =
    (1, 40, 70), interleaved = 1: it needs 3.63 u)."""
    c = s0.shape[1]
    r = rec.cpu()
    ck.same(f"{tag}records identical", r[0], r[1])
    assert float(r[0, 2 * c]) == float(rows), (float(r[0, 2 * c]), rows)
    k = (total_rows or rows) * 2.0 ** -51 + extra
    ck.hold(f"{tag}sum_0", r[0, :c], s0.sum(0), k * s0.abs().sum(0))
    ck.hold(f"{tag}sum_1", r[0, c:2 * c], s1.sum(0), (k + extra) * s1.abs().sum(0))


def _check_coeffs(ck, tag, outs, count, gamma, beta, mom, rm0, rv0, ref):
    """dc_bn_coeffs_from_sums outputs against the fp64 statistics `ref` of the concatenated rows."""
    mean, var, invstd, scale, shift = ref
    got_mean, got_invstd, got_scale, got_shift, rm, rv = outs
    g = gamma.double() if gamma is not None else torch.ones_like(mean)
    b = beta.double() if beta is not None else torch.zeros_like(mean)
    ck.hold(f"{tag}mean", got_mean, mean, 2 * U * mean.abs())
    ck.hold(f"{tag}invstd", got_invstd, invstd, 2 * U * invstd.abs())
    ck.hold(f"{tag}scale", got_scale, scale, 2 * U * scale.abs())
    ck.hold(f"{tag}shift", got_shift, shift, 2 * U * (b.abs() + (mean * scale).abs()))
    unb = var * count / max(count - 1, 1)                  # the unbiased factor uses the TOTAL row count
    ck.hold(f"{tag}running_mean", rm, (1 - mom) * rm0.double() + mom * mean,
            2 * U * (((1 - mom) * rm0.double()).abs() + (mom * mean).abs()))
    ck.hold(f"{tag}running_var", rv, (1 - mom) * rv0.double() + mom * unb,
            2 * U * (((1 - mom) * rv0.double()).abs() + (mom * unb).abs()))


def _coeffs_variants(ck, total, count, c, gamma, beta, ref_of):
    """count = 0 (read from the device slot) and explicit; with and without gamma / beta; momentum 0.1 and 1.0."""
    rm0, rv0 = torch.linspace(-1, 1, c), torch.linspace(0.5, 2, c)
    for cnt in (0, count):
        for affine in (True, False):
            for mom in (MOM, 1.0):
                g, b = (gamma, beta) if affine else (None, None)
                coef = torch.empty(4, c, device=DEV)
                rm, rv = rm0.to(DEV), rv0.to(DEV)
                lib.call("dc_bn_coeffs_from_sums", total, cnt, c, None if g is None else g.to(DEV), None if b is None else b.to(DEV),
                         EPS, mom, rm, rv, coef[0], coef[1], coef[2], coef[3])
                _check_coeffs(ck, "", (coef[0], coef[1], coef[2], coef[3], rm, rv), count, g, b, mom, rm0, rv0, ref_of(g, b))


# ---- part A, BatchNorm ---------------------------------------------------------------------------------------------------
class _BnCase:
    def __init__(self, rows, chan):
        self.rows, (self.C, self.ld, self.off) = rows, CHANNELS[chan]
        c, r = self.C, sum(rows)
        self.R = r
        g = torch.Generator().manual_seed(1000 + 7 * r + c + self.off)
        sd = 10.0 ** torch.linspace(-3, 3, c)[torch.randperm(c, generator=g)]
        mu = sd * torch.linspace(-30, 30, c)[torch.randperm(c, generator=g)]
        x = (mu + sd * torch.randn(r, c, generator=g)).float()
        self.gamma, self.beta = _affine(c)
        for _ in range(20):          # keep z = scale x + shift away from the kink of the activation (see the module docstring)
            mean, _, _, scale, shift = _stats64(x, self.gamma, self.beta)
            z = scale * x.double() + shift
            near = z.abs() < 2.0 ** -18 * ((scale * x.double()).abs() + (mean * scale).abs() + self.beta.double().abs())
            if not near.any():
                break
            x = torch.where(near, x + (0.37 * sd).float(), x)
        else:
            raise AssertionError("could not move the data off the kink")
        self.x = x
        self.dy = ((10.0 ** torch.linspace(-2, 2, c)[torch.randperm(c, generator=g)]) * torch.randn(r, c, generator=g)).float()
        self.ref = _stats64(x, self.gamma, self.beta)
        self._fwd = None

    def put(self, t):
        """t [r, C] (CPU) -> (sentinel-filled device buffer [r, ld], its column block holding t)."""
        buf = torch.full((t.shape[0], self.ld), SENT, device=DEV)
        view = buf[:, self.off:self.off + self.C]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * self.off          # (offset 1: the scalar path chosen by alignment)
        return buf, view

    def sentinels_intact(self, buf):
        return bool((buf[:, :self.off] == SENT).all()) and bool((buf[:, self.off + self.C:] == SENT).all())

    def forward(self):
        """-> (records of the shards [2, 2C+1] each, their sum, the global coefficients [4, C] the backward entry points take)."""
        if self._fwd is None:
            recs = []
            for xs in self.x.split(self.rows):
                _, h = self.put(xs)
                rec = torch.zeros(2, 2 * self.C + 1, dtype=torch.float64, device=DEV)
                ws, nb = _ws(xs.shape[0], self.C)
                lib.call("dc_bn_sums", h, xs.shape[0], self.C, self.ld, rec, ws, nb)
                recs.append(rec)
            total = _all_reduce_first(recs)
            coef = torch.empty(4, self.C, device=DEV)
            lib.call("dc_bn_coeffs_from_sums", total, 0, self.C, self.gamma.to(DEV), self.beta.to(DEV), EPS, MOM, None, None,
                     coef[0], coef[1], coef[2], coef[3])
            self._fwd = recs, total, coef
        return self._fwd


@functools.lru_cache(maxsize=None)
def _bn_case(rows, chan):
    return _BnCase(rows, chan)


@pytest.mark.parametrize("chan", list(CHANNELS))
@pytest.mark.parametrize("rows", ROWS)
def test_bn_sums_and_coeffs(rows, chan):
    """dc_bn_sums per shard, then dc_bn_coeffs_from_sums on the summed record in all its variants."""
    case = _bn_case(rows, chan)
    ck = _Checks(f"bn forward {rows} {chan}")
    recs, total, _ = case.forward()
    for xs, rec in zip(case.x.split(rows), recs):
        _check_records(ck, rec, xs.shape[0], xs.double(), xs.double() ** 2)
    assert float(total[2 * case.C]) == case.R
    _coeffs_variants(ck, total, case.R, case.C, case.gamma, case.beta, lambda g, b: _stats64(case.x, g, b))
    ck.done()


def _dh_bound(k, gi, dz, m1, m2, h, mean, invstd):
    return k * U * gi.abs() * (dz.abs() + m1.abs() + (h.abs() + mean.abs()) * invstd * m2.abs())


DH_K = 8       # the constant of the dh bound
SLOPES = [0.2, 0.0, 1.0]


@pytest.mark.parametrize("slope", SLOPES)
@pytest.mark.parametrize("chan", list(CHANNELS))
@pytest.mark.parametrize("rows", ROWS)
def test_bn_backward_split(rows, chan, slope):
    """dc_bn_act_backward_sums per shard (scale / shift of the global batch, xhat from the summed FORWARD record) -> sum of the
    first records -> dc_sync_means -> dc_bn_act_backward_apply, and dc_bn_backward_coefs_from_sums on the same records, against
    fp64 autograd of leaky_relu(batch_norm(.)) on the concatenated rows.

    The single-pass sibling dc_bn_act_backward on the concatenated rows is measured against the same reference and bounds beside
    it (printed, not asserted).  It forms xhat = (h - mean) invstd with the fp32-rounded mean, which costs every addend of dgamma
    and m2 up to |mean| invstd u: on these data it reaches 2.7 (rows (1, 17, 300)) and 125 (rows (1, 1)) of the dgamma bound and
    1.96 of the dh bound (it would need the constant 15.7).  The split form did the same until dc_bn_act_backward_sums took its
    mean and invstd in fp64 from the forward record (dgamma summed over ranks 2.8 and 125, m2 99, dgamma of a one-row rank 4327,
    dh 1.96); now: dgamma 0.75, m2 0.35, dh 0.42."""
    case = _bn_case(rows, chan)
    c, r_all = case.C, case.R
    slope = float(torch.tensor(slope, dtype=torch.float32))        # the ABI takes the slope as float
    ck = _Checks(f"bn backward {rows} {chan} slope {slope:g}")
    _, fwd_total, coef = case.forward()
    gamma_d = case.gamma.to(DEV)

    # fp64 reference
    h = case.x.double().requires_grad_(True)
    gam, bet = case.gamma.double().requires_grad_(True), case.beta.double().requires_grad_(True)
    y = F.leaky_relu(F.batch_norm(h, None, None, gam, bet, True, 0.0, EPS), slope)
    y.backward(case.dy.double())
    mean, _, invstd, scale, shift = case.ref
    hd, dyd = case.x.double(), case.dy.double()
    z = scale * hd + shift
    dz = dyd * torch.where(z > 0, 1.0, slope)
    xhat = (hd - mean) * invstd
    m1, m2 = dz.mean(0), (dz * xhat).mean(0)
    gi = case.gamma.double() * invstd
    full = _dh_bound(DH_K, gi, dz, m1, m2, hd, mean, invstd)
    assert bool(((gi * (dz - m1 - xhat * m2) - h.grad).abs() <= 1e-3 * full).all())    # the closed form is the autograd gradient

    # the kernels, one shard after the other
    shards = []
    for xs, dys in zip(case.x.split(rows), case.dy.split(rows)):
        r = xs.shape[0]
        (_, hv), (_, dyv) = case.put(xs), case.put(dys)
        rec = torch.zeros(2, 2 * c + 1, dtype=torch.float64, device=DEV)
        ws, nb = _ws(r, c)
        lib.call("dc_bn_act_backward_sums", dyv, case.ld, hv, case.ld, r, c, coef[2], coef[3], fwd_total, EPS, slope, rec, ws, nb)
        shards.append((r, hv, dyv, rec))
    total = shards[0][3][0].clone()
    for s in shards[1:]:
        total += s[3][0]
    dh_all, dg_sum, db_sum, lo = [], torch.zeros(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64), 0
    for r, hv, dyv, rec in shards:
        sl = slice(lo, lo + r)
        lo += r
        ck.same("backward records identical", rec[0], rec[1])
        assert float(rec[0, 2 * c]) == r
        rec[0].copy_(total)                                                # the all-reduce, in place
        m = torch.full((2, c), float("nan"), device=DEV)
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        lib.call("dc_sync_means", rec, c, m[0], m[1], dg, db)
        ck.hold("m1", m[0], m1, 2 * U * m1.abs() + 2 * U * dz.abs().sum(0) / r_all)
        ck.hold("m2", m[1], m2, 2 * U * m2.abs() + 2 * U * (dz * xhat).abs().sum(0) / r_all)
        ck.hold("dbeta of a rank", db, dz[sl].sum(0), 2 * U * dz[sl].abs().sum(0))
        ck.hold("dgamma of a rank", dg, (dz[sl] * xhat[sl]).sum(0), 2 * U * (dz[sl] * xhat[sl]).abs().sum(0))
        dg_sum += dg.double().cpu()
        db_sum += db.double().cpu()
        buf, dhv = case.put(torch.zeros(r, c))
        lib.call("dc_bn_act_backward_apply", dyv, case.ld, hv, case.ld, r, c, coef[2], coef[3], coef[0], coef[1], gamma_d, slope, 1,
                 m[0], m[1], dhv, case.ld)
        assert case.sentinels_intact(buf)
        dh_all.append(dhv.cpu())
        # the fused form: five coefficient rows from the global record, dgamma / dbeta from the local one
        coefs = torch.empty(5 * c, device=DEV)
        dg2, db2 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        lib.call("dc_bn_backward_coefs_from_sums", rec[0], 0, rec[1], c, gamma_d, coef[2], coef[3], coef[0], coef[1], 1, dg2, db2, coefs)
        ck.same("fused dgamma = local", dg2, dg)
        ck.same("fused dbeta = local", db2, db)
        rows5 = coefs.view(5, c).double().cpu()
        c32 = coef.double().cpu()                                          # the fp32 coefficients the entry point was given
        s0, s1 = total[:c].cpu(), total[c:2 * c].cpu()
        gi32 = case.gamma.double() * c32[1]
        ck.same("c_sc", coefs.view(5, c)[0], coef[2])
        ck.same("c_sh", coefs.view(5, c)[1], coef[3])
        ck.hold("c_g", rows5[2], gi32, 2 * U * gi32.abs())
        ck.hold("c_a", rows5[3], -gi32 * (s1 / r_all) * c32[1], 2 * U * (gi32 * (s1 / r_all) * c32[1]).abs())
        ck.hold("c_b", rows5[4], -gi32 * (s0 / r_all) + gi32 * (s1 / r_all) * c32[1] * c32[0],
                2 * U * ((gi32 * (s0 / r_all)).abs() + (gi32 * (s1 / r_all) * c32[1] * c32[0]).abs()))
        h64, dy64 = hv.double().cpu(), dyv.double().cpu()
        dz32 = dy64 * torch.where(rows5[0] * h64 + rows5[1] > 0, 1.0, slope)
        ck.hold("dh rebuilt from the coefficient rows", rows5[2] * dz32 + rows5[3] * h64 + rows5[4], h.grad[sl],
                full[sl])
    ck.hold("dh", torch.cat(dh_all), h.grad, full)
    ck.hold("dbeta summed over ranks", db_sum, bet.grad, 2 * U * dz.abs().sum(0))
    ck.hold("dgamma summed over ranks", dg_sum, gam.grad, 2 * U * (dz * xhat).abs().sum(0))

    if slope == 0.2:             # training = 0 once: dh = scale * dz, m1 / m2 ignored (NaN here)
        r, hv, dyv, _ = shards[-1]
        nan = torch.full((2, c), float("nan"), device=DEV)
        buf, dhv = case.put(torch.zeros(r, c))
        lib.call("dc_bn_act_backward_apply", dyv, case.ld, hv, case.ld, r, c, coef[2], coef[3], coef[0], coef[1], gamma_d, slope, 0,
                 nan[0], nan[1], dhv, case.ld)
        assert case.sentinels_intact(buf)
        sl = slice(r_all - r, r_all)
        ck.hold("dh, training = 0", dhv, scale * dz[sl], 4 * U * (scale * dz[sl]).abs())   # three roundings: scale, dz, product

    # the single-pass sibling on the concatenated rows, same reference and bounds (figures only)
    sib = _Checks(f"SIBLING dc_bn_act_backward {rows} {chan} slope {slope:g}")
    (_, hv), (_, dyv), (_, dhv) = case.put(case.x), case.put(case.dy), case.put(torch.zeros(r_all, c))
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    ws, nb = _ws(r_all, c)
    lib.call("dc_bn_act_backward", dyv, case.ld, hv, case.ld, r_all, c, coef[2], coef[3], coef[0], coef[1], gamma_d, slope, 1, dhv,
             case.ld, dg, db, ws, nb)
    sib.hold("sibling dh", dhv, h.grad, full)
    sib.hold("sibling dbeta", db, bet.grad, 2 * U * dz.abs().sum(0))
    sib.hold("sibling dgamma", dg, gam.grad, 2 * U * (dz * xhat).abs().sum(0))
    ck.done()


# ---- part A, vector non-linearity ---------------------------------------------------------------------------------------------
PTS = (1, 17, 300)


def _y_of(t, combine):
    """The fp64 (y_u, y_v) [n, co] each that the kernels combine from their input layout (csrc/nn_math.h: vn_combine)."""
    u, v = t[0::2], t[1::2]
    if combine in (0, 3):
        return u, v
    co = t.shape[1] // 2
    (pu, qu, pv, qv) = (u[:, :co], u[:, co:], v[:, :co], v[:, co:]) if combine == 1 else (u[:, 0::2], u[:, 1::2], v[:, 0::2], v[:, 1::2])
    return pu - qv, pv + qu


def _expand(mask, combine):
    """[n, co] per (point, channel) -> the shape of the input layout."""
    m = mask.repeat_interleave(2, 0)
    return m if combine in (0, 3) else (torch.cat([m, m], 1) if combine == 1 else m.repeat_interleave(2, 1))


class _VnCase:
    """Components with standard deviations log-uniform over 1e-2 .. 1e2 around a constant vector of up to 30 standard deviations
    (so the norms, whose statistics are taken, have means of up to ~30 standard deviations); one zero vector."""

    def __init__(self, co, combine):
        self.co, self.combine, self.n = co, combine, sum(PTS)
        n = self.n
        g = torch.Generator().manual_seed(500 + 10 * co + combine)
        sd = 10.0 ** torch.linspace(-2, 2, co)[torch.randperm(co, generator=g)]
        off = sd * torch.linspace(0, 30, co)[torch.randperm(co, generator=g)]
        th = torch.rand(co, generator=g) * 6.2831853
        yu = off * th.cos() + sd * torch.randn(n, co, generator=g)
        yv = off * th.sin() + sd * torch.randn(n, co, generator=g)
        yu[n - 3], yv[n - 3] = 0.0, 0.0
        if combine in (0, 3):
            t = torch.stack([yu, yv], 1).reshape(2 * n, co)
        else:
            qu, qv = 0.3 * sd * torch.randn(n, co, generator=g), 0.3 * sd * torch.randn(n, co, generator=g)
            qu[n - 3], qv[n - 3] = 0.0, 0.0
            pu, pv = yu + qv, yv - qu
            if combine == 1:
                t = torch.stack([torch.cat([pu, qu], 1), torch.cat([pv, qv], 1)], 1).reshape(2 * n, 2 * co)
            else:
                il = lambda p, q: torch.stack([p, q], 2).reshape(n, 2 * co)
                t = torch.stack([il(pu, qu), il(pv, qv)], 1).reshape(2 * n, 2 * co)
        t = t.float()
        self.gamma, self.beta = _affine(co)
        for _ in range(20):           # keep z = scale |y| + shift away from the kink of the ReLU
            st = self.stats(t)
            near = st["z"].abs() < (2.0 ** -18 + 4 * st["rho"]) * st["Z"]
            if not near.any():
                break
            t = torch.where(_expand(near, combine), t * 1.3, t)
        else:
            raise AssertionError("could not move the data off the kink")
        self.t = t
        self.st = self.stats(t)
        self.dout = ((10.0 ** torch.linspace(-2, 2, co)[torch.randperm(co, generator=g)]) * torch.randn(2 * n, co, generator=g)).float()
        self._fwd = None

    def stats(self, t):
        yu, yv = _y_of(t.double(), self.combine)
        nrm = (yu * yu + yv * yv).sqrt()
        mean, var, invstd, scale, shift = _stats64(nrm, self.gamma, self.beta)
        # relative uncertainty of invstd / scale caused by the fp32 norms (relative error <= 3 u each): var = E[n^2] - mean^2
        rho = 2 * U + 6 * U * ((nrm * nrm).mean(0) + mean * mean) / (2 * (var + EPS))
        return dict(yu=yu, yv=yv, n=nrm, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, rho=rho,
                    z=scale * nrm + shift, Z=scale.abs() * (nrm + mean.abs()) + self.beta.double().abs())

    def shards(self):
        return self.t.split([2 * p for p in PTS]), self.dout.split([2 * p for p in PTS])

    def forward(self):
        if self._fwd is None:
            co, ld, lc = self.co, self.t.shape[1], 0 if self.combine == 3 else self.combine
            recs = []
            for ts in self.shards()[0]:
                n = ts.shape[0] // 2
                rec = torch.zeros(2, 2 * co + 1, dtype=torch.float64, device=DEV)
                ws, nb = _ws(n, co)
                lib.call("dc_vn_sums", ts.to(DEV), n, co, ld, lc, rec, ws, nb)
                recs.append(rec)
            total = _all_reduce_first(recs)
            coef = torch.empty(4, co, device=DEV)
            lib.call("dc_bn_coeffs_from_sums", total, 0, co, self.gamma.to(DEV), self.beta.to(DEV), EPS, MOM, None, None,
                     coef[0], coef[1], coef[2], coef[3])
            self._fwd = recs, total, coef
        return self._fwd


@functools.lru_cache(maxsize=None)
def _vn_case(co, combine):
    return _VnCase(co, combine)


@pytest.mark.parametrize("combine", [0, 1, 2])
@pytest.mark.parametrize("co", [16, 5])
def test_vn_sums_and_coeffs(co, combine):
    """dc_vn_sums per shard: the addends are fp32 norms (3 u on top of the fp64 summation term); the coefficients of the summed
    record inherit that: mean within 2 u |mean| + 3 u E|n|, invstd / scale within the relative bound rho of _VnCase.stats."""
    case = _vn_case(co, combine)
    st = case.st
    ck = _Checks(f"vn forward co {co} combine {combine}")
    recs, total, coef = case.forward()
    lo = 0
    for p, rec in zip(PTS, recs):
        nr = st["n"][lo:lo + p]
        lo += p
        _check_records(ck, rec, p, nr, nr * nr, extra=3 * U, total_rows=case.n, tag="vector ")
    assert float(total[2 * co]) == case.n
    ck.hold("vector mean", coef[0], st["mean"], 2 * U * st["mean"].abs() + 3 * U * st["n"].mean(0))
    ck.hold("vector invstd", coef[1], st["invstd"], st["rho"] * st["invstd"])
    ck.hold("vector scale", coef[2], st["scale"], st["rho"] * st["scale"].abs())
    ck.done()


@pytest.mark.parametrize("combine", [0, 1, 2, 3])
@pytest.mark.parametrize("co", [16, 5])
def test_vn_backward_split(co, combine):
    """dc_vn_backward_sums per shard -> sum of the first records -> dc_sync_means -> dc_vn_backward_apply against fp64 autograd of
    oracle.nn.VectorNonLin (BatchNorm over the norms) on all points.

    The bound, derived as for the scalar block from csrc/nn_math.h: vn_bwd_dy.  Per (point, channel): n = |y|, nc = max(n, 1e-8),
    g_s = y_u d_u + y_v d_v with G = |y_u d_u| + |y_v d_v| the magnitude of its terms, Z = |scale| (n + |mean|) + |beta| that of
    z = scale n + shift, gi = gamma invstd, nhat = (n - mean) invstd.  The kernel evaluates
        dy = d s + (dn / n) y,   s = relu(z) / nc,   dn = gi (g_s / nc - m1 - nhat m2) - g_s relu(z) / nc^2
    in fp32, and every coefficient carries the relative uncertainty rho of statistics taken over fp32 norms (_VnCase.stats).  So
        |dy_got - dy_ref| <= (8 u + 2 rho) [ |gi| (G / nc + |m1| + (n + |mean|) invstd (|m2| + |nhat| |m1|)) + (|d| + G / nc) Z / nc ]
    per component (|y_u| / n, |y_v| / n <= 1); the 8 as in the scalar bound.  The sums: dz = g_s / nc takes six roundings (two in
    g_s, three in n, the division), so dbeta of a rank is within 6 u sum (G / nc) and dgamma (a further factor nhat with its
    cancellation and its coefficients) within (8 u + rho) sum (G / nc) (n + |mean|) invstd; m1, m2: 2 u |ref| + those / R.
    combine = 3 reads y and writes the interleaved d(P, Q).  training = 0 once: dn = scale dz - ..., m1 / m2 ignored."""
    case = _vn_case(co, combine)
    st = case.st
    n_all, ld, lc = case.n, case.t.shape[1], 0 if combine == 3 else combine
    ldi = 2 * co if combine == 3 else ld
    ck = _Checks(f"vn backward co {co} combine {combine}")
    _, _, coef = case.forward()
    gamma_d = case.gamma.to(DEV)

    # fp64 reference
    vn = oracle.nn.VectorNonLin(co, batchnorm=oracle.nn.BatchNorm1d(co)).double().train()
    vn.batchnorm.bn.eps = EPS
    with torch.no_grad():
        vn.batchnorm.bn.weight.copy_(case.gamma)
        vn.batchnorm.bn.bias.copy_(case.beta)
    leaf = case.t.double().requires_grad_(True)
    yu, yv = _y_of(leaf, combine)
    vn(torch.stack([yu, yv], 1).reshape(2 * n_all, co)).backward(case.dout.double())
    ref = leaf.grad
    if combine == 3:                                   # d(P, Q) interleaved: row u = (dy_u, dy_v), row v = (dy_v, -dy_u)
        gu, gv = ref[0::2], ref[1::2]
        il = lambda p, q: torch.stack([p, q], 2).reshape(n_all, 2 * co)
        ref = torch.stack([il(gu, gv), il(gv, -gu)], 1).reshape(2 * n_all, 2 * co)
    du, dv = case.dout.double()[0::2], case.dout.double()[1::2]
    nrm, mean, invstd, scale = st["n"], st["mean"], st["invstd"], st["scale"]
    nc = nrm.clamp_min(1e-8)
    gate = (st["z"] > 0).double()
    gs, G = st["yu"] * du + st["yv"] * dv, (st["yu"] * du).abs() + (st["yv"] * dv).abs()
    dz, nhat = gate * gs / nc, (nrm - mean) * invstd
    m1, m2 = dz.mean(0), (dz * nhat).mean(0)
    gi = case.gamma.double() * invstd
    a0 = gate * G / nc                                          # magnitude of the terms of dz
    a1 = a0 * (nrm + mean.abs()) * invstd                       # ... of dz * nhat
    assert rel_err(dz.sum(0), vn.batchnorm.bn.bias.grad) < 1e-9 and rel_err((dz * nhat).sum(0), vn.batchnorm.bn.weight.grad) < 1e-9
    common = (8 * U + 2 * st["rho"]) * gi.abs() * (G / nc + m1.abs() + (nrm + mean.abs()) * invstd * (m2.abs() + nhat.abs() * m1.abs()))
    bu = common + (8 * U + 2 * st["rho"]) * (du.abs() + G / nc) * st["Z"] / nc
    bv = common + (8 * U + 2 * st["rho"]) * (dv.abs() + G / nc) * st["Z"] / nc
    bound = torch.stack([bu, bv], 1).reshape(2 * n_all, co)
    if combine in (1, 2, 3):                                    # d(P, Q): every entry is +- one component of dy
        if combine == 1:
            bound = torch.stack([torch.cat([bu, bv], 1), torch.cat([bv, bu], 1)], 1).reshape(2 * n_all, 2 * co)
        else:
            il = lambda p, q: torch.stack([p, q], 2).reshape(n_all, 2 * co)
            bound = torch.stack([il(bu, bv), il(bv, bu)], 1).reshape(2 * n_all, 2 * co)

    shards = []
    for ts, ds in zip(*case.shards()):
        n = ts.shape[0] // 2
        tin, dout = ts.to(DEV), ds.to(DEV)
        rec = torch.zeros(2, 2 * co + 1, dtype=torch.float64, device=DEV)
        ws, nb = _ws(n, co)
        lib.call("dc_vn_backward_sums", dout, co, tin, ld, combine, n, co, coef[2], coef[3], coef[0], coef[1], rec, ws, nb)
        shards.append((n, tin, dout, rec))
    total = shards[0][3][0].clone()
    for s in shards[1:]:
        total += s[3][0]
    got, lo = [], 0
    dg_sum, db_sum = torch.zeros(co, dtype=torch.float64), torch.zeros(co, dtype=torch.float64)
    for n, tin, dout, rec in shards:
        sl = slice(lo, lo + n)
        lo += n
        ck.same("vector backward records identical", rec[0], rec[1])
        assert float(rec[0, 2 * co]) == n
        rec[0].copy_(total)
        m = torch.full((2, co), float("nan"), device=DEV)
        dg, db = torch.empty(co, device=DEV), torch.empty(co, device=DEV)
        lib.call("dc_sync_means", rec, co, m[0], m[1], dg, db)
        ck.hold("vector m1", m[0], m1, 2 * U * m1.abs() + 6 * U * a0.sum(0) / n_all)
        ck.hold("vector m2", m[1], m2, 2 * U * m2.abs() + (8 * U + st["rho"]) * a1.sum(0) / n_all)
        ck.hold("vector dbeta of a rank", db, dz[sl].sum(0), 6 * U * a0[sl].sum(0))
        ck.hold("vector dgamma of a rank", dg, (dz[sl] * nhat[sl]).sum(0), (8 * U + st["rho"]) * a1[sl].sum(0))
        dg_sum += dg.double().cpu()
        db_sum += db.double().cpu()
        buf = torch.full((2 * n + 1, ldi), SENT, device=DEV)
        lib.call("dc_vn_backward_apply", dout, co, tin, ld, combine, n, co, coef[2], coef[3], coef[0], coef[1], gamma_d, 1, m[0], m[1],
                 buf, ldi)
        assert bool((buf[2 * n:] == SENT).all())
        got.append(buf[:2 * n].cpu())
    ck.hold("vector dy", torch.cat(got), ref, bound)
    ck.hold("vector dbeta summed over ranks", db_sum, vn.batchnorm.bn.bias.grad, 6 * U * a0.sum(0))
    ck.hold("vector dgamma summed over ranks", dg_sum, vn.batchnorm.bn.weight.grad, (8 * U + st["rho"]) * a1.sum(0))

    if combine in (0, 2):        # training = 0 once per layout family: the BatchNorm part is scale * dz, m1 / m2 ignored (NaN here)
        n, tin, dout, _ = shards[-1]
        nan = torch.full((2, co), float("nan"), device=DEV)
        out = torch.empty(2 * n, ldi, device=DEV)
        lib.call("dc_vn_backward_apply", dout, co, tin, ld, combine, n, co, coef[2], coef[3], coef[0], coef[1], gamma_d, 0, nan[0], nan[1],
                 out, ldi)
        sl = slice(n_all - n, n_all)
        dn = scale * dz[sl] - torch.where(nrm[sl] > 1e-8, gs[sl] * st["z"][sl].clamp_min(0) / (nc[sl] * nc[sl]), 0.0)
        w = torch.where(nrm[sl] > 0, dn / nc[sl], 0.0)
        s = st["z"][sl].clamp_min(0) / nc[sl]
        eu, ev = du[sl] * s + w * st["yu"][sl], dv[sl] * s + w * st["yv"][sl]
        if combine == 0:
            ref0 = torch.stack([eu, ev], 1).reshape(2 * n, co)
        else:
            il = lambda p, q: torch.stack([p, q], 2).reshape(n, 2 * co)
            ref0 = torch.stack([il(eu, ev), il(ev, -eu)], 1).reshape(2 * n, 2 * co)
        ck.hold("vector dy, training = 0", out, ref0, bound[2 * (n_all - n):])

    sib = _Checks(f"SIBLING dc_vn_backward co {co} combine {combine}")
    tin, dout = case.t.to(DEV), case.dout.to(DEV)
    out = torch.empty(2 * n_all, ldi, device=DEV)
    dg, db = torch.empty(co, device=DEV), torch.empty(co, device=DEV)
    ws, nb = _ws(n_all, co)
    lib.call("dc_vn_backward", dout, co, tin, ld, combine, n_all, co, coef[2], coef[3], coef[0], coef[1], gamma_d, 1, out, ldi, dg, db,
             ws, nb)
    sib.hold("sibling vector dy", out, ref, bound)
    sib.hold("sibling vector dbeta", db, vn.batchnorm.bn.bias.grad, 6 * U * a0.sum(0))
    sib.hold("sibling vector dgamma", dg, vn.batchnorm.bn.weight.grad, (8 * U + st["rho"]) * a1.sum(0))
    ck.done()


# ---- part A, the statistics products with the reduction cut open ------------------------------------------------------------------
MNK = [(1, 40, 70), (17, 40, 70), (300, 128, 64)]


def _rand(*shape, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


@pytest.mark.parametrize("m,n,k", MNK)
def test_linear_bn_sums_forward(m, n, k):
    """The h it stores is, bit for bit, the h of dc_linear_bn_stats_forward on the same operands; its record holds the fp64
    sums of that stored h."""
    ck = _Checks(f"linear bn sums {m, n, k}")
    x, w = _rand(m, k, seed=1), _rand(n, k, seed=2)
    nb = lib.raw("dc_linear_stats_workspace_bytes")(m, n, k, 0)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    h_ref, coef = torch.empty(m, n, device=DEV), torch.empty(4, n, device=DEV)
    lib.call("dc_linear_bn_stats_forward", x, k, w, k, m, n, k, h_ref, n, None, None, EPS, MOM, None, None, coef[0], coef[1], coef[2],
             coef[3], 0, ws, nb)
    buf = torch.full((m + 1, n), SENT, device=DEV)
    rec = torch.zeros(2, 2 * n + 1, dtype=torch.float64, device=DEV)
    lib.call("dc_linear_bn_sums_forward", x, k, w, k, m, n, k, buf, n, rec, 0, ws, nb)
    assert bool((buf[m:] == SENT).all())
    ck.same("stored h", buf[:m], h_ref)
    assert rel_err(buf[:m], x.double() @ w.double().t()) < 2e-6 * k ** 0.5 + 1e-6       # the bound of tests/test_gpu_gemm.py
    hd = buf[:m].double().cpu()
    _check_records(ck, rec, m, hd, hd * hd, tag="product ")
    ck.done()


@pytest.mark.parametrize("interleaved", [0, 1, 2])
@pytest.mark.parametrize("m,n,k", MNK)
def test_linear_vn_sums_forward(m, n, k, interleaved):
    """m points (2m rows), co = n: stored output bit-identical to dc_linear_vn_stats_forward; the record holds the fp64 sums of the
    norms of the stored output (interleaved = 1: of the pair combined in fp64) within the dc_vn_sums bound."""
    ck = _Checks(f"linear vn sums {m, n, k} interleaved {interleaved}")
    co = n
    wrows = 2 * co if interleaved else co
    width = co if interleaved in (0, 2) else 2 * co
    v, w = _rand(2 * m, k, seed=3), _rand(wrows, k, seed=4)
    nb = lib.raw("dc_linear_stats_workspace_bytes")(2 * m, wrows, k, 0)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    h_ref, coef = torch.empty(2 * m, width, device=DEV), torch.empty(4, co, device=DEV)
    lib.call("dc_linear_vn_stats_forward", v, k, w, k, m, co, k, h_ref, width, interleaved, None, None, EPS, MOM, None, None, coef[0],
             coef[1], coef[2], coef[3], 0, ws, nb)
    buf = torch.full((2 * m + 1, width), SENT, device=DEV)
    rec = torch.zeros(2, 2 * co + 1, dtype=torch.float64, device=DEV)
    lib.call("dc_linear_vn_sums_forward", v, k, w, k, m, co, k, buf, width, interleaved, rec, 0, ws, nb)
    assert bool((buf[2 * m:] == SENT).all())
    ck.same("stored output", buf[:2 * m], h_ref)
    yu, yv = _y_of(buf[:2 * m].double().cpu(), 2 if interleaved == 1 else 0)
    nrm = (yu * yu + yv * yv).sqrt()
    _check_records(ck, rec, m, nrm, nrm * nrm, extra=3 * U, tag="vector product ")
    ck.done()


# ---- part B: the Python paths under the simulator ------------------------------------------------------------------------------
def _pair(make_ours, make_ref):
    from tests.test_gpu_nn import _pair as pair          # parameters exactly as the per-rank tests set them
    return pair(make_ours, make_ref)


def _run_ranks(ours, shards, weights, call=lambda net, x: net(x), toggle=False):
    """Every rank runs a fresh copy of `ours` on its shard under the simulator; loss = sum(y * weight).
    -> (sim, [(y, dx, [parameter gradients], [buffers]) per rank]).  A pass whose unknown collective lay in the forward part
    skips its backward.  toggle: the sync state is switched OFF between forward and backward."""
    with SyncSim(len(shards)) as sim:
        def fn(rank, shard):
            net = copy.deepcopy(ours)
            x = shard.clone().requires_grad_(True)
            y = call(net, x)
            if sim.pending():
                return None
            try:
                sim.on = not toggle
                (y * weights[rank]).sum().backward()
            finally:
                sim.on = True
            return y.detach(), x.grad, [p.grad for p in net.parameters()], [b.clone() for b in net.buffers()]

        t0 = time.time()
        out = sim.run(fn, shards)
        torch.cuda.synchronize()
        print(f"[simulator] {sim.world} ranks, {sim.collectives} collectives, {sim.passes} passes, {time.time() - t0:.2f} s")
    return sim, out


def _compare_ranks(out, ours, ref, y_ref, dx_ref, tol_y, tol_g):
    """Outputs and input gradients concatenated over ranks, parameter gradients SUMMED over ranks, buffers on every rank
    (and bit-identical between ranks) against the oracle `ref` that saw the whole batch."""
    assert rel_err(torch.cat([o[0] for o in out]), y_ref) < tol_y
    assert rel_err(torch.cat([o[1] for o in out]), dx_ref) < tol_g
    for i, ((n1, _), (n2, p2)) in enumerate(zip(ours.named_parameters(), ref.named_parameters())):
        grads = [o[2][i] for o in out]
        if p2.grad is None:
            assert all(g is None or float(g.abs().max()) == 0 for g in grads), n1
        else:
            assert rel_err(sum(g.double() for g in grads), p2.grad) < tol_g, n1
    for i, ((n1, _), (n2, b2)) in enumerate(zip(ours.named_buffers(), ref.named_buffers())):
        for r, o in enumerate(out):
            if b2.dtype.is_floating_point:
                assert rel_err(o[3][i], b2) < tol_y, (n1, r)
            else:
                assert int(o[3][i]) == int(b2), (n1, r)
            assert torch.equal(o[3][i], out[0][3][i]), f"{n1}: rank {r} differs from rank 0"


def _module_case(ours, ref, x, rows, tol=2e-4, **kw):
    """tests/test_gpu_nn.py:_compare with the rows of x sharded over simulated ranks."""
    ours.train(); ref.train()
    xo = x.clone().requires_grad_(True)
    yo = ref(xo)
    w = torch.randn(yo.shape, generator=torch.Generator().manual_seed(9))
    yo.backward(w)
    sim, out = _run_ranks(ours, [s.to(DEV) for s in x.split(rows)], [s.to(DEV) for s in w.split(rows)], **kw)
    _compare_ranks(out, ours, ref, yo, xo.grad, tol, 5 * tol)
    return sim


@pytest.mark.parametrize("channels,rows", [((16, 32), (1, 17, 300)), ((5, 7), (1, 17, 300)), ((16, 64), (1, 1, 2))])
def test_mlp_uneven_ranks(channels, rows):
    """dc.nn.MLP: fused.linear_stats / bn_block_reduce with a group.  (16, 64) over (1, 1, 2): the categorical head of the
    segmentation net with one cloud per rank -- the documented reason for synchronised statistics."""
    import deltaconv_amd as dc
    ours, ref = _pair(lambda: dc.nn.MLP(channels), lambda: oracle.nn.MLP(channels))
    x = torch.randn(sum(rows), channels[0], generator=torch.Generator().manual_seed(4)) * 1.5 + 0.3
    sim = _module_case(ours, ref, x, rows)
    assert sim.collectives == 2


def test_single_row_in_all_is_refused():
    """One row in the whole batch: refused as torch refuses it, also with three ranks (two of them without rows), and before
    anything moves."""
    import deltaconv_amd as dc
    ours, _ = _pair(lambda: dc.nn.MLP((16, 64)), lambda: oracle.nn.MLP((16, 64)))
    ours.train()
    x = torch.randn(1, 16, device=DEV)
    nets = [copy.deepcopy(ours) for _ in range(3)]
    with SyncSim(3) as sim:        # the rank that holds the row cannot know; the ranks without rows refuse, before anything moves
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            sim.run(lambda rank, shard: nets[rank](shard), x.split((1, 0, 0)))
        assert not sim.totals
    assert int(nets[1][0][1].bn.num_batches_tracked) == 0 and int(nets[2][0][1].bn.num_batches_tracked) == 0
    with SyncSim(1):               # one rank in all
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            ours(x)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):      # (and without a group, as before)
        ours(x)
    assert int(ours[0][1].bn.num_batches_tracked) == 0


@pytest.mark.parametrize("store_y", [True, False])
@pytest.mark.parametrize("channels", [(16, 32), (6, 5)])
def test_vector_mlp_uneven_ranks(channels, store_y):
    """dc.nn.VectorMLP over point shards (1, 17, 300), zero vectors in the first rows (tests/test_gpu_nn.py:
    test_vector_mlp_blocks): dc_vn_sums and fused.vn_backward with a group."""
    import deltaconv_amd as dc
    from deltaconv_amd.nn import fused
    ours, ref = _pair(lambda: dc.nn.VectorMLP(channels), lambda: oracle.nn.VectorMLP(channels))
    v = torch.randn(2 * sum(PTS), channels[0], generator=torch.Generator().manual_seed(6))
    v[:4] = 0
    old = fused.VN_STORE_Y[0]
    fused.VN_STORE_Y[0] = store_y
    try:
        sim = _module_case(ours, ref, v, [2 * p for p in PTS])
    finally:
        fused.VN_STORE_Y[0] = old
    assert sim.collectives == 2


class _BnActRes(torch.nn.Module):
    """leaky(bn(h)) + residual through fused.bn_act (ours) / plain torch (reference); input = [h | residual]."""

    def __init__(self, c, ours):
        super().__init__()
        self.bn, self.c, self.ours = torch.nn.BatchNorm1d(c), c, ours

    def forward(self, x):
        h, res = x[:, :self.c], x[:, self.c:]
        if self.ours:
            from deltaconv_amd.nn import fused
            return fused.bn_act(h, self.bn, 0.2, res)
        return F.leaky_relu(self.bn(h), 0.2) + res


def _bn_act_pair(c):
    ours, ref = _BnActRes(c, True), _BnActRes(c, False)
    g, b = _affine(c)
    with torch.no_grad():
        for m in (ours, ref):
            m.bn.weight.copy_(g)
            m.bn.bias.copy_(b)
    return ours.to(DEV), ref


@pytest.mark.parametrize("c", [16, 7])
@pytest.mark.parametrize("toggle", [False, True])
def test_bn_act_residual_uneven_ranks(c, toggle):
    """fused.bn_act with a residual: dc_bn_sums forward, fused.bn_act_backward with a group.  toggle: dp's sync state is
    switched off between forward and backward -- the backward still reduces over the forward's group."""
    ours, ref = _bn_act_pair(c)
    x = torch.randn(sum(ROWS[0]), 2 * c, generator=torch.Generator().manual_seed(8)) * 1.5 + 0.3
    sim = _module_case(ours, ref, x, ROWS[0], toggle=toggle)
    assert sim.collectives == 2


@pytest.mark.parametrize("kind", ["mlp", "vector"])
def test_toggle_between_forward_and_backward(kind):
    """The blocks that carry their group in the flag (fused.BatchStats) and in the autograd context: sync state off before
    backward, the result is still that of the global batch."""
    import deltaconv_amd as dc
    if kind == "mlp":
        ours, ref = _pair(lambda: dc.nn.MLP((16, 32)), lambda: oracle.nn.MLP((16, 32)))
        x, rows = torch.randn(sum(ROWS[0]), 16, generator=torch.Generator().manual_seed(4)) * 1.5 + 0.3, ROWS[0]
    else:
        ours, ref = _pair(lambda: dc.nn.VectorMLP((16, 32)), lambda: oracle.nn.VectorMLP((16, 32)))
        x, rows = torch.randn(2 * sum(PTS), 16, generator=torch.Generator().manual_seed(6)), [2 * p for p in PTS]
    sim = _module_case(ours, ref, x, rows, toggle=True)
    assert sim.collectives == 2


@pytest.mark.parametrize("kind", ["mlp", "vector", "vector without BatchNorm"])
def test_no_batch_statistics_no_collective(kind):
    """Blocks that take no batch statistics (eval mode: running statistics; a vector non-linearity without BatchNorm) under an
    open group: no collective forward or backward, every rank computes what the oracle computes on its rows alone."""
    import deltaconv_amd as dc
    if kind == "mlp":
        ours, ref = _pair(lambda: dc.nn.MLP((16, 32)), lambda: oracle.nn.MLP((16, 32)))
        x, rows = torch.randn(sum(ROWS[0]), 16, generator=torch.Generator().manual_seed(4)) * 1.5 + 0.3, list(ROWS[0])
    else:
        bn = kind == "vector"
        ours, ref = _pair(lambda: dc.nn.VectorMLP((16, 32), batchnorm=bn), lambda: oracle.nn.VectorMLP((16, 32), batchnorm=bn))
        x, rows = torch.randn(2 * sum(PTS), 16, generator=torch.Generator().manual_seed(6)), [2 * p for p in PTS]
    if kind != "vector without BatchNorm":
        ours.train(); ref.train()
        with torch.no_grad():           # one training step on the whole batch each, so that the running statistics are not trivial
            ours(x.to(DEV)); ref(x)
        ours.eval(); ref.eval()
    xo = x.clone().requires_grad_(True)
    yo = ref(xo)
    w = torch.randn(yo.shape, generator=torch.Generator().manual_seed(9))
    yo.backward(w)
    sim, out = _run_ranks(ours, [t.to(DEV) for t in x.split(rows)], [t.to(DEV) for t in w.split(rows)])
    assert sim.collectives == 0 and sim.passes == 1
    _compare_ranks(out, ours, ref, yo, xo.grad, 2e-4, 1e-3)


def test_oversized_fused_block_is_refused_before_any_collective():
    """bn_block_backward of a block whose weight has more than OWN_TN_MAX_OUTPUTS entries has no synchronised form: every
    rank raises NotImplementedError before a collective, the simulator has seen no record."""
    from deltaconv_amd.nn import fused
    c, k = 2048, 1025
    assert c * k > fused.OWN_TN_MAX_OUTPUTS
    w = torch.randn(c, k, device=DEV) * 0.05
    gamma = torch.ones(c, device=DEV)
    with SyncSim(3) as sim:
        for rank, r in enumerate((1, 3, 2)):
            inp, h, dy = torch.randn(r, k, device=DEV), torch.randn(r, c, device=DEV), torch.randn(r, c, device=DEV)
            coef = torch.ones(4, c, device=DEV)
            with sim.as_rank(rank):
                with pytest.raises(NotImplementedError, match="synchronised BatchNorm backward"):
                    fused.bn_block_backward(dy, c, inp, h, coef, fused.BatchStats(sim.group), gamma, 0.2, w)
                assert sim.seen == 0
        assert not sim.recorded and not sim.totals


# ---- layers and the segmentation model ------------------------------------------------------------------------------------
def _cut(b, lo, hi):
    """Clouds [lo, hi) of a CPU batch as a batch of their own (data-parallel sharding by clouds, of any sizes)."""
    from deltaconv_amd.data import Batch
    ptr = b.ptr.tolist()
    p0, p1 = ptr[lo], ptr[hi]
    y = b.y[p0:p1] if b.y is not None and b.y.shape[0] == b.pos.shape[0] else (None if b.y is None else b.y[lo:hi])
    return Batch(b.pos[p0:p1], b.batch[p0:p1] - lo, b.norm[p0:p1], None, y, None if b.category is None else b.category[lo:hi],
                 hi - lo), (p0, p1)


LAYERS = {"centralised depth 1": dict(ci=3, co=32, depth=1, centralized=True),
          "centralised depth 2": dict(ci=3, co=32, depth=2, centralized=True),
          # 64 channels: the shape csrc/edge2.hip takes per rank; synchronised statistics switch that fusion off (fused.edge_mlp2_ok)
          "centralised depth 2, 64 channels": dict(ci=3, co=64, depth=2, centralized=True),
          "vector 32 -> 64": dict(ci=32, co=64, depth=1, centralized=False)}


@pytest.mark.parametrize("name", list(LAYERS))
def test_deltaconv_layer_uneven_ranks(name):
    """dc.nn.DeltaConv with clouds [400] | [256, 300] on two ranks (each builds its own graph and operators) against the oracle
    layer on the three clouds as one batch; tolerances of tests/test_gpu_nn.py: test_centralized_layer_vs_oracle."""
    import deltaconv_amd as dc
    from deltaconv_amd.data import synthetic_batch
    from oracle import geometry as geo
    cfg = LAYERS[name]
    ci, co = cfg["ci"], cfg["co"]
    b = synthetic_batch(3, 0, seed=50, sizes=[400, 256, 300], dup_frac=0.03)
    ours, ref = _pair(lambda: dc.nn.DeltaConv(ci, co, depth=cfg["depth"], centralized=cfg["centralized"], vector=True),
                      lambda: oracle.nn.DeltaConv(ci, co, depth=cfg["depth"], centralized=cfg["centralized"], vector=True))
    ours.train(); ref.train()
    n = b.pos.shape[0]
    ptr = geo.cloud_ptr(b.batch)
    nbr = geo.knn(b.pos, 20, ptr)
    xb, yb = geo.build_tangent_basis(b.norm)
    Go, Do = geo.build_grad_div(b.pos, b.norm, xb, yb, nbr, ptr)
    gen = torch.Generator().manual_seed(12)
    x0 = b.pos.clone() if ci == 3 else torch.randn(n, ci, generator=gen)
    v0 = (Go @ x0).detach() if ci == 3 else torch.randn(2 * n, ci, generator=gen)
    wx, wv = torch.randn(n, co, generator=gen), torch.randn(2 * n, co, generator=gen)
    x, v = x0.clone().requires_grad_(True), v0.clone().requires_grad_(True)
    xo, vo = ref(x, v, Go, Do, nbr)
    ((xo * wx).sum() + (vo * wv).sum()).backward()

    ranks = []
    for lo, hi in ((0, 1), (1, 3)):
        sb, (p0, p1) = _cut(b, lo, hi)
        bd = sb.to(DEV)
        graph = dc.geometry.Graph.knn(bd.pos, 20, bd.batch)
        assert torch.equal(graph.nbr.cpu().long() + p0, nbr[p0:p1])
        G, D = dc.geometry.build_grad_div(bd.pos, bd.norm, xb[p0:p1].to(DEV), yb[p0:p1].to(DEV), graph, bd.batch)
        ranks.append(dict(graph=graph, G=G, D=D, x=x0[p0:p1].to(DEV), v=v0[2 * p0:2 * p1].to(DEV), wx=wx[p0:p1].to(DEV),
                          wv=wv[2 * p0:2 * p1].to(DEV)))

    with SyncSim(2) as sim:
        def fn(rank, rk):
            net = copy.deepcopy(ours)
            xr, vr = rk["x"].clone().requires_grad_(True), rk["v"].clone().requires_grad_(True)
            xn, vn = net(xr, vr, rk["G"], rk["D"], rk["graph"])
            if sim.pending():
                return None
            ((xn * rk["wx"]).sum() + (vn * rk["wv"]).sum()).backward()
            return xn.detach(), vn.detach(), xr.grad, vr.grad, [p.grad for p in net.parameters()], [t.clone() for t in net.buffers()]

        t0 = time.time()
        out = sim.run(fn, ranks)
        torch.cuda.synchronize()
        print(f"[simulator] layer {name}: {sim.collectives} collectives, {sim.passes} passes, {time.time() - t0:.2f} s")
    assert sim.collectives == 6 * cfg["depth"]
    assert rel_err(torch.cat([o[0] for o in out]), xo) < 1e-3 and rel_err(torch.cat([o[1] for o in out]), vo) < 1e-3
    assert rel_err(torch.cat([o[2] for o in out]), x.grad) < 5e-3 and rel_err(torch.cat([o[3] for o in out]), v.grad) < 5e-3
    for i, ((n1, _), (_, p2)) in enumerate(zip(ours.named_parameters(), ref.named_parameters())):
        if p2.grad is not None:
            assert rel_err(sum(o[4][i].double() for o in out), p2.grad) < 5e-3, n1
        else:
            assert all(o[4][i] is None for o in out), n1
    for i, ((n1, _), (_, b2)) in enumerate(zip(ours.named_buffers(), ref.named_buffers())):
        for o in out:
            if b2.dtype.is_floating_point:
                assert rel_err(o[5][i], b2) < 1e-3, n1
            else:
                assert int(o[5][i]) == int(b2), n1
            assert torch.equal(o[5][i], out[0][5][i]), n1


def test_segmentation_model_three_ranks():
    """DeltaNetSegmentation with the categorical vector, one cloud of 128 points on each of three ranks (`lin_categorical` sees
    ONE row per rank), summed loss, against the oracle model on the three clouds: logits and every parameter gradient, held to
    the bound of tests/test_gpu_model.py: test_model_step_vs_oracle (no further from the fp64 oracle than 3x the fp32 oracle
    + 1e-3).  Backward runs only once the forward collectives are known."""
    import deltaconv_amd as dc
    from deltaconv_amd.data import Batch, synthetic_batch
    kw = dict(conv_channels=[16, 32], mlp_depth=1, embedding_size=64, categorical_vector=True, num_neighbors=10)
    b = synthetic_batch(3, 128, seed=70, num_classes=8, per_point_labels=True, categories=16)
    torch.manual_seed(1)
    no_dropout = lambda m: [d.eval() for d in m.modules() if isinstance(d, torch.nn.Dropout)] and m
    ref32 = no_dropout(oracle.models.DeltaNetSegmentation(3, 8, **kw).train())
    ref64 = no_dropout(oracle.models.DeltaNetSegmentation(3, 8, **kw).double().train())
    ref64.load_state_dict(ref32.state_dict())
    model = dc.models.DeltaNetSegmentation(3, 8, **kw)
    model.load_state_dict(ref32.state_dict())
    model = no_dropout(model.to(DEV).train())
    w = torch.randn(b.pos.shape[0], 8, generator=torch.Generator().manual_seed(3))
    l32 = ref32(b)
    (l32 * w).sum().backward()
    l64 = ref64(Batch(b.pos.double(), b.batch, b.norm.double(), None, b.y, b.category.double()))
    (l64 * w.double()).sum().backward()

    shards = []
    for r in range(3):
        sb, (p0, p1) = _cut(b, r, r + 1)
        shards.append((sb.to(DEV), w[p0:p1].to(DEV)))
    with SyncSim(3) as sim:
        def fn(rank, shard):
            net = copy.deepcopy(model)
            logits = net(shard[0])
            if sim.pending():
                return None
            (logits * shard[1]).sum().backward()
            return logits.detach(), [p.grad for p in net.parameters()], [t.clone() for t in net.buffers()]

        t0 = time.time()
        out = sim.run(fn, shards)
        torch.cuda.synchronize()
        print(f"[simulator] segmentation model: {sim.collectives} collectives, {sim.passes} passes, {time.time() - t0:.2f} s")
    logits = torch.cat([o[0] for o in out])
    e_hip, e_ref = rel_err(logits, l64), rel_err(l32, l64)
    print(f"logits: hip-vs-f64 {e_hip:.2e}  oracle32-vs-f64 {e_ref:.2e}")
    assert e_hip < 3 * e_ref + 1e-3
    gmax = max(float(p.grad.abs().max()) for p in ref64.parameters() if p.grad is not None)
    worst_hip = worst_ref = 0.0
    for i, ((n1, _), (_, p2), (_, p3)) in enumerate(zip(model.named_parameters(), ref32.named_parameters(), ref64.named_parameters())):
        if p3.grad is None:
            assert all(o[1][i] is None for o in out), n1
            continue
        scale = max(float(p3.grad.abs().max()), 1e-3 * gmax)
        got = sum(o[1][i].double().cpu() for o in out)
        worst_hip = max(worst_hip, float((got - p3.grad).abs().max()) / scale)
        worst_ref = max(worst_ref, float((p2.grad.double() - p3.grad).abs().max()) / scale)
    print(f"worst per-parameter grad error: hip-vs-f64 {worst_hip:.2e}  oracle32-vs-f64 {worst_ref:.2e}")
    assert worst_hip < 3 * worst_ref + 1e-3
    for i, ((n1, _), (_, b3)) in enumerate(zip(model.named_buffers(), ref64.named_buffers())):
        for o in out:
            if b3.dtype.is_floating_point:
                assert rel_err(o[2][i], b3) < 1e-3, n1
            else:
                assert int(o[2][i]) == int(b3), n1
            assert torch.equal(o[2][i], out[0][2][i]), n1
