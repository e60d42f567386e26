"""Plain fp64 restatement of the layer-0 edge MLP (deltaconv_amd/csrc/edge_math.h, edge.hip, the finalisers of colreduce.h):
Linear -> BatchNorm over all E = n k edges -> LeakyReLU -> max over the k-list, and its backward; with the data makers and the
bounds that tests/test_gpu_edge_abi.py (the C ABI on the device) and tests/test_edge_restate_host.py (the CPU build of
edge_math.h) hold every output element to.

Input convention.  y is fp32 [n, C]; a32 = y[nbr] - y[:, None] is evaluated in fp32 (one IEEE subtraction per element: the
kernel's `a`, bit for bit).  Everything downstream of a32 is fp64.  `autograd` restates it with torch autograd on the
materialised [n, k, C] tensor: BatchNorm over the n k rows (training: biased batch variance; eval: the running pair),
scale = gamma invstd, shift = beta - mu scale, LeakyReLU as z > 0 ? z : slope z (the kernel's convention at 0), selection by
`gather` on the slot, backward to y through both roles of every edge (+ at y_j, - at y_i), to gamma and to beta.  `closed` is
the closed form of edge_math.h in fp64 (it supplies the magnitudes of the bounds and the mutated variants of the host test);
the host test holds it to the autograd result.  eps and momentum are the widened fp32 values the ABI receives.

Slots are exact: amax / amin / argmax / argmin are the maximum, the minimum and the FIRST extremal slot of a32
(where(a == extreme, arange(k), k).min(1): torch.max promises no tie order), and the selected slot is
where(scale >= 0, argmax, argmin) on the fp32 scale.  The references take those slots, so a tie (repeated neighbours, the
gamma = 0 column) cannot put the gradient on another edge than the kernel's.

Bounds.  u = 2^-24, gamma_m = m u / (1 - m u); every bound is first order in u with the roundings counted from the code.
ORD = 1e-13 covers the order of the fp64 accumulations (E <= 6e4 terms: 6e4 2^-53 = 7e-12 of the sum of magnitudes in the
worst case, a few 1e-14 in practice; the term is there so that an exact-zero fp32 rounding does not leave a zero bound).
Sa = sum_s |a| of a point, A1 = sum |a| / E and A2 = sum a^2 / E of a column.

  s1pt     k - 1 sequential fp32 adds of exact terms: gamma_(k-1) Sa  (k u Sa to first order).
  mean     NOT one rounding: the column sum is taken over the fp32 s1pt (edge_gather: t[0] = (double)s1), so the mean
           inherits their error before its own rounding: u |mu| + dm.  For dm the add-by-add form of the s1pt error is
           used, not gamma_(k-1) Sa: add t of a point rounds the partial sum S_t, error at most u |S_t|, so
           dm = (1 + k u) u sum_points sum_(t >= 2) |S_t| / E + ORD A1 (the partial sums of terms of either sign grow like
           sqrt(t): three times tighter, and as rigorous).  (mu is a mean of differences and nearly cancels, so dm is many
           ulps of mu; it is 1e-7 of the column's spread and harmless to the normalisation, but the one-ulp form does not
           hold for this output.)
  var      (not an output) s2 / E - m^2 in fp64: dv = 2 |mu| dm + dm^2 + ORD A2.
  invstd   one rounding of 1 / sqrt(var + eps): u is + is^3 dv / 2.
  scale    one rounding of gamma is: u |sc| + |gamma| is^3 dv / 2.
  shift    one rounding of beta - m gamma is: u |sh| + |sc| dm + |mu gamma| is^3 dv / 2.
  running_mean, running_var   one rounding of (1 - momentum) old + momentum new in fp64: u |value| + momentum dm, resp.
           u |value| + momentum dv E / (E - 1); the unbiased factor E / (E - 1), the biased variance at E = 1.
           With dm, dv two to four orders below u |value| for invstd .. running_var these are one-ulp checks.
  eval     dc_bn_eval_coeffs works in fp32: is = 1 / sqrtf(rv + eps) (add, root, quotient: 2.5 u, taken as 3 u), scale =
           gamma is (4 u), shift = beta - rm gamma is (u |sh| + 5 u |rm sc|), mean = rm exactly.
  out      act(fma(scale, a*, shift)): the fma rounds once, the product with the slope once more: gamma_2 (|scale a*| +
           |shift|) against the fp64 evaluation with the DEVICE's fp32 scale and shift (which have their own check
           above); the branch of that evaluation is the device's, since the fma keeps the sign of its exact argument.
  residual out = fl(act2(fma(scale2, h2, shift2)) + max): gamma_3 ((|scale a*| + |shift|) + |scale2 h2| + |shift2|), as
           dc_knn_max_affine_residual in apply_restate.py (a contraction of slope2 z + max into one fma only removes a
           rounding).
  dzs      dout act'(z): one product, u |dz| (exact for slope 0 and 1).
  dbeta    one rounding of the fp64 sum of the rounded dz: u |dbeta| + u sum |dz| + ORD sum |dz|.
  dgamma   term fl(dz fl(fl(a* - mean) invstd)): the subtraction sees the mean's error and rounds (dm' + u |a* - mu| with dm' =
           u |mu| + dm the error of the fp32 mean), the product with invstd adds invstd's error e_is and a rounding, the
           product with the rounded dz two more:  t = |dz| (is dm' + e_is |a* - mu| + 4 u |ahat|);  u |dgamma| + sum t +
           ORD sum |dz ahat|.
  m1, m2   (workspace, not returned; held through dy) dbeta / E and dgamma / E rounded once from the fp64 sums:
           e_m1 = u |m1| + u sum |dz| / E,  e_m2 = u |m2| + sum t / E.
  dy[j,c]  = scale [ (sel - dz_j) - (m1 (d - k) + m2 (col_hat - row_hat)) ],  d = indeg(j), h = selected in-edges of (j, c):
       A   sel = h sequential adds of rounded dz, - dz_j, and the final subtraction: gamma_(h + 2) (sum_sel |dz| + |dz_j|);
       B   m1 (d - k): (e_m1 + 2 u |m1|) |d - k|  (its product, the add to the m2 product);
       C   col = fl(fl(fl(d y_j) - T) - fl(d mean)), T = d sequential adds of y_i.  The reference sums the ROUNDED a32 over
           the in-edges, the kernel works from y: one more u on every y.  The y_j term sees 4 roundings, a y_i d + 2, the
           mean term its own error and two roundings.  These act on the magnitudes the kernel ADDS, not on the result
           (offset columns: d |y_j| is 8 spreads where col is one):
               e_col = gamma_(d + 4) (d |y_j| + sum_in |y_i|) + d (dm' + 2 u |mu|)
           row = fl(s1pt - fl(k mean)):  e_row = gamma_(k + 1) Sa + k (dm' + 2 u |mu|)
           the two products with invstd and their difference D:  e_D = is (e_col + e_row) + (e_is + 2 u is) (|col| + |row|)
           m2 D: e_m2 |D| + |m2| e_D, and 3 u (|m1 (d - k)| + |m2 D|) for its product, the add and the final subtraction;
       S   the product with scale: (e_sc + u |sc|) (sum_sel |dz| + |dz_j| + |m1 (d - k)| + |m2 D|);
       bound = |sc| (A + B + C) + S.   Eval (training == 0): |sc| gamma_(h + 1) (sum_sel |dz| + |dz_j|) + the S of those two.

Undecidable activation branches.  The kernel branches on the sign of w = scale32 a* + shift32 (exact; the fma keeps it), the
fp64 chain on z64 = sc a* + sh; |w - z64| <= e_sc |a*| + e_sh, in training at most half the `out` bound.  Where |z64| is
within max(out bound, e_sc |a*| + e_sh) of 0 and slope != 1, either branch is accepted (the reference is re-run with the
device's); their count is printed and capped at 1 in 10^4 per case.  On the cases of the host test the count is 0 (asserted
there); of the device's cases only `base` at C = 128 has one such element in 79 488.

Data.  y: normal draws times column scales log-uniform over 1e-2 .. 1e2, plus 0, 1 or 8 column scales (cycling over the
columns): the cancellation in d y_j - T_j.  gamma: both signs, one exact zero and one 1e-6 when C > 2; beta in +-0.3; running
pair away from (0, 1); dout normal with one all-zero row; graphs with slot 0 = self (a = 0) and repeated neighbours (ties).

RECOUNT.  Worst error / bound of the contiguous `base` case (C = 64, slope 0.2) on an MI355X (the CPU build of edge_math.h gives
the same to two digits, the one-ulp outputs within 0.03: they see the order of the fp64 sums): s1pt 0.23, mean 0.013, invstd 0.83, scale 0.89, shift 0.09, running_mean 0.19, running_var 0.92,
out 0.50, residual out 0.59, dzs 0.95, dbeta 0.07 (training) / 0.06 (eval), dgamma 0.026 / 0.054, dy 0.48 / 0.44; eval coefficients
invstd 0.49, scale 0.40, shift 0.75.  None is below 0.01 now; two were looked at:
  mean    was 0.005 with dm = gamma_(k-1) A1.  Recounted: nothing is miscounted, the form wastes a factor of three on the partial
          sums (now the add-by-add form above: 0.013), and the rest is the averaging of 621 independent s1pt errors of either sign
          in the column sum, which no rigorous bound may assume.  shift (0.09) and running_mean (0.19) are dominated by the same term.
  dgamma, dbeta  0.03 .. 0.07: the bound adds the magnitudes of 12 420 / 621 roundings that add like a random walk (sqrt(m), not
          m); on the smaller cases they reach 0.40 and 0.83.  The mutation table of the host test shows that the bounds still bite:
          E - 1 for E in m1 / m2, a relative change of 8e-5, leaves the dy bound by a factor of 17 (base) and 41 (hub600).
Over all graphs, layouts and modes the worst figures on the device are: dzs 0.95, scale 0.97, running_mean 0.96, invstd 0.95,
running_var 0.94, shift 0.94, dbeta 0.83, residual out 0.66, dy 0.56, out 0.50, dgamma 0.40, s1pt 0.28, mean 0.05.
"""
import functools

import torch

from tests import apply_restate as R
from tests.apply_restate import G2, G3, U

ORD = 1e-13


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


EPS, MOM = f32(1e-5), f32(0.1)
SLOPES = (f32(0.2), 0.0, 1.0)
BACKWARD_MODES = ((f32(0.2), 1), (f32(0.2), 0), (0.0, 0), (1.0, 1))      # (slope, training): every slope, both modes
OFFSETS = (0.0, 1.0, 8.0)

GRAPHS = {                                           # name -> (cloud sizes, k, hub rows)
    "base": ((300, 257, 64), 20, 0),
    "k1": ((130, 64), 1, 0),
    "tiny2": ((2,), 2, 0),
    "tiny1": ((1,), 1, 0),
    "hub": ((3000,), 20, 2800),
    "hub600": ((600,), 20, 560),
    "random": ((1024, 777), 20, 0),
}


def gam(m):
    g = torch.as_tensor(m, dtype=torch.float64) * U
    return g / (1 - g)


@functools.lru_cache(maxsize=None)
def graph(name):
    sizes, k, hub = GRAPHS[name]
    return R.make_graph(sizes, k, seed=300 + k + hub + len(sizes), hub_rows=hub), sizes


class Case:
    """The data of one (graph, C) and what follows from y and nbr exactly."""

    def __init__(self, gname, c):
        self.name, self.C = gname, c
        self.nbr, self.sizes = graph(gname)
        self.n, self.k = self.nbr.shape
        n, k = self.n, self.k
        self.E = n * k
        g = torch.Generator().manual_seed(7000 + 31 * len(gname) + c + n)
        colscale = 10.0 ** (torch.rand(c, generator=g) * 4 - 2)
        self.off = torch.tensor(OFFSETS)[torch.arange(c) % 3]
        self.y = (colscale * (torch.randn(n, c, generator=g) + self.off)).float()
        self.gamma = ((0.5 + torch.rand(c, generator=g)) * (torch.randint(0, 2, (c,), generator=g) * 2.0 - 1.0)).float()
        if c > 2:
            self.gamma[c // 2] = 0.0
            self.gamma[c // 2 + 1] = 1e-6
        self.beta = (torch.rand(c, generator=g) * 0.6 - 0.3).float()
        self.rm = (0.1 * colscale * torch.randn(c, generator=g)).float()
        self.rv = (colscale ** 2 * (1.0 + torch.rand(c, generator=g))).float()
        self.dout = torch.randn(n, c, generator=g)
        if n > 2:
            self.dout[n // 2] = 0.0
        self.h2 = R.make_features(n, c, 7100 + c)
        self.sc2, self.sh2 = R.make_affine(c, 7200 + c)
        # exact consequences of y and nbr
        self.a32 = self.y[self.nbr] - self.y[:, None, :]
        assert self.a32.dtype == torch.float32
        ar = torch.arange(k).view(1, k, 1)
        self.amax, self.amin = self.a32.max(1).values, self.a32.min(1).values
        self.argmax = torch.where(self.a32 == self.amax[:, None], ar, k).min(1).values
        self.argmin = torch.where(self.a32 == self.amin[:, None], ar, k).min(1).values
        a = self.a32.double()
        self.s1, self.Sa = a.sum(1), a.abs().sum(1)
        self.Spart = a.cumsum(1)[:, 1:].abs().sum(1)                       # sum over the k - 1 adds of s1pt of |partial sum|
        self.indeg = R.in_degree(self.nbr)                                  # [n, 1]

    def slots(self, scale, last=False, swap=False):
        """The selected slot for a scale vector (fp32 or fp64: the sign decides).  last / swap: the mutations of the host test."""
        k = self.k
        if last:
            ar = torch.arange(k).view(1, k, 1)
            amx = torch.where(self.a32 == self.amax[:, None], ar, -1).max(1).values
            amn = torch.where(self.a32 == self.amin[:, None], ar, -1).max(1).values
        else:
            amx, amn = self.argmax, self.argmin
        pos = (scale >= 0) if not swap else torch.ones_like(scale, dtype=torch.bool)
        return torch.where(pos, amx, amn)


@functools.lru_cache(maxsize=None)
def case(gname, c):
    return Case(gname, c)


class Coef:
    """fp64 mean, invstd, scale, shift of one mode with the bounds of their fp32 images (e_*: absolute)."""


def coefficients(cs, training, mut=()):
    """-> Coef; training: also rm_new, rv_new and their bounds.  mut: 'unbiased_norm', 'biased_running'."""
    o = Coef()
    gamma, beta, rm, rv = (t.double() for t in (cs.gamma, cs.beta, cs.rm, cs.rv))
    E, k = cs.E, cs.k
    if training:
        a = cs.a32.double().reshape(E, cs.C)
        mu = a.sum(0) / E
        var = ((a - mu) ** 2).sum(0) / E
        A1, A2 = a.abs().sum(0) / E, (a * a).sum(0) / E
        unbiased = var * E / (E - 1) if E > 1 else var
        vn = unbiased if "unbiased_norm" in mut else var
        o.mu, o.invstd = mu, 1.0 / torch.sqrt(vn + EPS)
        o.scale = gamma * o.invstd
        o.shift = beta - mu * o.scale
        o.rm_new = (1.0 - MOM) * rm + MOM * mu
        o.rv_new = (1.0 - MOM) * rv + MOM * (var if "biased_running" in mut else unbiased)
        dm = (1 + k * U) * U * cs.Spart.sum(0) / E + ORD * A1
        dv = 2 * mu.abs() * dm + dm * dm + ORD * A2
        half = 0.5 * o.invstd ** 3 * dv
        o.e_mu = U * mu.abs() + dm
        o.e_invstd = U * o.invstd + half
        o.e_scale = U * o.scale.abs() + gamma.abs() * half
        o.e_shift = U * o.shift.abs() + o.scale.abs() * dm + (mu * gamma).abs() * half
        o.e_rm = U * o.rm_new.abs() + MOM * dm
        o.e_rv = U * o.rv_new.abs() + MOM * dv * (E / (E - 1) if E > 1 else 1.0)
    else:
        o.mu, o.invstd = rm, 1.0 / torch.sqrt(rv + EPS)
        o.scale = gamma * o.invstd
        o.shift = beta - rm * o.scale
        o.e_mu = torch.zeros_like(rm)
        o.e_invstd = 3 * U * o.invstd
        o.e_scale = 4 * U * o.scale.abs()
        o.e_shift = U * o.shift.abs() + 5 * U * (rm * o.scale).abs()
    return o


def apply_out(cs, scale32, shift32, slope):
    """The fp64 evaluation of act(scale a* + shift) with the fp32 coefficients given -> (value, bound, magnitude)."""
    a = torch.where(scale32 >= 0, cs.amax, cs.amin).double()
    sa = scale32.double() * a
    w = sa + shift32.double()
    mag = sa.abs() + shift32.double().abs()
    return torch.where(w > 0, w, slope * w), G2 * mag, mag


def residual_out(cs, scale32, shift32, slope, slope2):
    val, _, mag = apply_out(cs, scale32, shift32, slope)
    blk, B = R.affine_block(cs.h2, cs.sc2, cs.sh2, slope2)
    return blk + val, G3 * (mag + B)


def _selected(cs, slot):
    return cs.a32.double().gather(1, slot[:, None, :])[:, 0]


def undecidable(cs, co, slot, slope):
    """-> (mask of the elements whose activation branch the fp64 chain cannot decide, z64)."""
    astar = _selected(cs, slot)
    z = co.scale * astar + co.shift
    thr = torch.maximum(G2 * ((co.scale * astar).abs() + co.shift.abs()), co.e_scale * astar.abs() + co.e_shift)
    return (z.abs() <= thr) & (slope != 1.0), z


def autograd(cs, slot, slope, training, positive=None):
    """fp64 autograd on the materialised [n, k, C] tensor -> dict(out, dy, dgamma, dbeta).  positive: the branch per element
    (None: z > 0)."""
    n, k, C, E = cs.n, cs.k, cs.C, cs.E
    a = cs.a32.double().requires_grad_(True)
    gamma, beta = cs.gamma.double().requires_grad_(True), cs.beta.double().requires_grad_(True)
    if training:
        flat = a.reshape(E, C)
        mu = flat.sum(0) / E
        var = ((flat - mu) ** 2).sum(0) / E
    else:
        mu, var = cs.rm.double(), cs.rv.double()
    scale = gamma / torch.sqrt(var + EPS)
    z = a * scale + (beta - mu * scale)
    zsel = z.gather(1, slot[:, None, :])[:, 0]
    pos = (zsel.detach() > 0) if positive is None else positive
    out = zsel * torch.where(pos, 1.0, slope)
    out.backward(cs.dout.double())
    ga = a.grad
    return dict(out=out.detach(), dy=R._scatter(cs.nbr, ga) - ga.sum(1), dgamma=gamma.grad, dbeta=beta.grad)


def closed(cs, co, slot, slope, training, positive=None, mut=()):
    """The closed form of edge_math.h in fp64 with the bounds of every backward output -> dict.  mut: 'E_minus_1', 'k_for_indeg',
    'drop_m1', 'train_in_eval' (the mutations of the host test; the bounds are those of the true form)."""
    k, E = cs.k, cs.E
    astar = _selected(cs, slot)
    z = co.scale * astar + co.shift
    pos = (z > 0) if positive is None else positive
    dout = cs.dout.double()
    dz = dout * torch.where(pos, 1.0, slope)
    ahat = (astar - co.mu) * co.invstd
    dbeta, dgamma = dz.sum(0), (dz * ahat).sum(0)
    dm1 = co.e_mu                                                        # the error of the fp32 mean
    t = dz.abs() * (co.invstd * dm1 + co.e_invstd * (astar - co.mu).abs() + 4 * U * ahat.abs())
    sum_dz, sum_t = dz.abs().sum(0), t.sum(0)
    r = dict(dzs=dz, e_dzs=U * dz.abs(), dbeta=dbeta, dgamma=dgamma,
             e_dbeta=U * dbeta.abs() + (U + ORD) * sum_dz, e_dgamma=U * dgamma.abs() + sum_t + ORD * (dz * ahat).abs().sum(0))
    Em = E - 1 if "E_minus_1" in mut else E
    m1, m2 = dbeta / Em, dgamma / Em
    e_m1, e_m2 = U * m1.abs() + U * sum_dz / E, U * m2.abs() + sum_t / E
    hit = slot[:, None, :] == torch.arange(k).view(1, k, 1)
    dzb = dz[:, None, :]
    sel = R._scatter(cs.nbr, torch.where(hit, dzb, 0.0))
    selabs = R._scatter(cs.nbr, torch.where(hit, dzb.abs(), 0.0))
    h = R._scatter(cs.nbr, hit.double())
    d = cs.indeg
    g0, g0mag = sel - dz, selabs + dz.abs()
    sc, e_sc = co.scale, co.e_scale
    if training or "train_in_eval" in mut:
        y = cs.y.double()
        yabs_in = R._scatter(cs.nbr, y.abs()[:, None, :].expand(-1, k, -1))      # sum over the in-edges of |y_i|
        col = R._scatter(cs.nbr, cs.a32.double()) - d * co.mu                    # sum over the in-edges of (a32 - mu)
        if "k_for_indeg" in mut:
            col = col + (k - d) * y - (k - d) * co.mu
        row = cs.s1 - k * co.mu
        D = co.invstd * (col - row)
        p1 = torch.zeros_like(col) if "drop_m1" in mut else m1 * (d - k)
        p2 = m2 * D
        dy = sc * (g0 - (p1 + p2))
        mu_term = dm1 + 2 * U * co.mu.abs()
        e_col = gam(d + 4) * (d * y.abs() + yabs_in) + d * mu_term
        e_row = gam(k + 1) * cs.Sa + k * mu_term
        e_D = co.invstd * (e_col + e_row) + (co.e_invstd + 2 * U * co.invstd) * (col.abs() + row.abs())
        inner = (gam(h + 2) * g0mag + (e_m1 + 2 * U * m1.abs()) * (d - k).abs() + e_m2 * D.abs() + m2.abs() * e_D
                 + 3 * U * (p1.abs() + p2.abs()))
        mag = g0mag + p1.abs() + p2.abs()
    else:
        dy = sc * g0
        inner = gam(h + 1) * g0mag
        mag = g0mag
    r.update(dy=dy, e_dy=sc.abs() * inner + (e_sc + U * sc.abs()) * mag, m1=m1, m2=m2)
    return r


@functools.lru_cache(maxsize=None)
def reference(gname, c, slope, training):
    """Everything the checks of one (case, slope, mode) need, computed once: the coefficients, the exact slots, the undecidable
    mask, the autograd values and the closed form with its bounds."""
    cs = case(gname, c)
    co = coefficients(cs, training)
    slot = cs.slots(co.scale)
    und, z = undecidable(cs, co, slot, slope)
    return dict(co=co, slot=slot, und=und, z=z, auto=autograd(cs, slot, slope, training), closed=closed(cs, co, slot, slope, training))


# ---- the checks both backends share -------------------------------------------------------------------------------------------
def check_gather(ck, cs, got):
    """got: amax, amin, argmax, argmin, s1pt."""
    ck.exact("amax", got["amax"], cs.amax)
    ck.exact("amin", got["amin"], cs.amin)
    ck.exact("argmax = first maximal slot", got["argmax"], cs.argmax)
    ck.exact("argmin = first minimal slot", got["argmin"], cs.argmin)
    ck.hold("s1pt", got["s1pt"], cs.s1, gam(cs.k - 1) * cs.Sa)


def check_coefficients(ck, cs, training, got):
    """got: mean, invstd, scale, shift (+ rm_new, rv_new in training)."""
    co = coefficients(cs, training)
    tag = "batch" if training else "eval"
    ck.hold(f"{tag} mean", got["mean"], co.mu, co.e_mu)
    ck.hold(f"{tag} invstd", got["invstd"], co.invstd, co.e_invstd)
    ck.hold(f"{tag} scale", got["scale"], co.scale, co.e_scale)
    ck.hold(f"{tag} shift", got["shift"], co.shift, co.e_shift)
    if training:
        ck.hold("running_mean", got["rm_new"], co.rm_new, co.e_rm)
        ck.hold("running_var", got["rv_new"], co.rv_new, co.e_rv)
    ck.true("scale keeps the sign of gamma", bool((torch.sign(got["scale"].double()) == torch.sign(cs.gamma.double())).all()))


def check_apply(ck, cs, scale32, shift32, slope, out, arg, tag=""):
    val, bound, _ = apply_out(cs, scale32, shift32, slope)
    ck.hold(f"out slope {slope:.1f}{tag}", out, val, bound)
    if arg is not None:
        ck.exact(f"arg = where(scale >= 0, argmax, argmin){tag}", arg, cs.slots(scale32))


def check_backward(ck, cs, slope, training, scale32, shift32, got, tag=""):
    """got: dzs, dy, dgamma, dbeta (the last two may be None)."""
    ref = reference(cs.name, cs.C, slope, training)
    auto, cl = ref["auto"], ref["closed"]
    n_und = int(ref["und"].sum())
    print(f"[{ck.what}] slope {slope:.1f} training {training}{tag}: {n_und} undecidable activation branches of {cs.n * cs.C}")
    ck.true("undecidable branches at most 1 in 10^4", n_und * 10000 <= cs.n * cs.C)
    if n_und:                                        # those elements take the device's branch: the sign of scale32 a* + shift32
        w = scale32.double() * _selected(cs, ref["slot"]) + shift32.double()
        positive = torch.where(ref["und"], w > 0, ref["z"] > 0)
        auto = autograd(cs, ref["slot"], slope, training, positive)
        cl = closed(cs, ref["co"], ref["slot"], slope, training, positive)
    what = f" slope {slope:.1f} training {training}{tag}"
    ck.hold("dzs" + what, got["dzs"], cl["dzs"], cl["e_dzs"])
    ck.hold("dy" + what, got["dy"], auto["dy"], cl["e_dy"])
    if got.get("dgamma") is not None:
        ck.hold("dgamma" + what, got["dgamma"], auto["dgamma"], cl["e_dgamma"])
    if got.get("dbeta") is not None:
        ck.hold("dbeta" + what, got["dbeta"], auto["dbeta"], cl["e_dbeta"])
    return auto


def fp32_chain_dy(cs, slot, slope):
    """dy of the same chain (training) evaluated by torch in fp32 on the materialised tensor: the yardstick of the offset table."""
    a = cs.a32.clone().requires_grad_(True)
    flat = a.reshape(cs.E, cs.C)
    mu = flat.mean(0)
    var = ((flat - mu) ** 2).mean(0)
    scale = cs.gamma / torch.sqrt(var + EPS)
    z = a * scale + (cs.beta - mu * scale)
    zsel = z.gather(1, slot[:, None, :])[:, 0]
    out = torch.where(zsel > 0, zsel, slope * zsel)
    out.backward(cs.dout)
    ga = a.grad
    dy = torch.zeros(cs.n, cs.C)
    dy.index_add_(0, cs.nbr.reshape(-1), ga.reshape(cs.E, cs.C))
    return dy - ga.sum(1)


def offset_table(cs, dy_kernel, dy64, slot, slope):
    """Per offset class (0, 1, 8 spreads): worst |dy - dy64| / max |dy64| of the column, for the kernel and for the fp32
    materialised chain.  -> [(offset, kernel, fp32 chain)]; columns with gamma = 0 or 1e-6 carry no signal and are left out."""
    dy32 = fp32_chain_dy(cs, slot, slope).double()
    top = dy64.abs().max(0).values
    use = cs.gamma.abs() > 1e-3
    rows = []
    for o in OFFSETS:
        m = use & (cs.off == o) & (top > 0)
        if not bool(m.any()):
            continue
        ek = ((dy_kernel.double() - dy64).abs().max(0).values / top)[m].max()
        e32 = ((dy32 - dy64).abs().max(0).values / top)[m].max()
        rows.append((o, float(ek), float(e32)))
    return rows
