"""Plain fp64 restatement of the depth-2 centralised edge MLP (deltaconv_amd/csrc/edge2.hip; finalisers: colreduce.h, element
formulas: nn_math.h):  out[p] = max_s act2(bn2(W2 act1(bn1(y1)))),  y1 = W1 (x_j - x_i), j = nbr[p, s], both BatchNorms over all
E = n k edges; with its backward, the data makers and the bounds that tests/test_gpu_edge2_abi.py (the C ABI on the device)
and tests/test_edge2_restate_host.py (an fp32 emulation of the kernels' arithmetic in torch) hold every output element to.
The graph maker, `gam`, ORD, EPS, MOM and the slopes are those of tests/edge_restate.py; U and `_scatter` those of apply_restate.py;
`act_ref` (dc_bn_act) and O2 those of nn_restate.py.

Input conventions.  x [n, ci] and W1 [64, ci] are fp32.  Direct path (CI = ci <= 3): d32 = x[nbr] - x[:, None] is taken in fp32,
one IEEE subtraction per element (the kernels' dlt / dl, bit for bit), y1 = W1 d32 in fp64.  z path (CI = 0): z [n, 64] fp32 is
an INPUT (the fp32 product x W1^T, made once by the case), d32 = z[nbr] - z[:, None] in fp32 and y1 = d32.  Everything downstream
is fp64.  Every entry point is held on the fp32 values it is GIVEN: dc_edge2_forward on scale1 / shift1; dc_bn_act on ysel,
scale2, shift2; dc_edge2_backward on coef1, coef2, ysel, arg and s1pt -- `backward` is the closed form of the file header and of
edge2_scatter_kernel evaluated in fp64 on those values, so a backward check does not inherit the forward's errors, and the
branch of act2' at the selected element (the sign of scale2 ysel + shift2: two fp32 numbers' product plus a third, exact in
fp64 up to a rounding that keeps the sign) is decided exactly.  `autograd` restates the block with torch autograd on the
materialised [n, k, 64] tensors (own fp64 batch statistics, slots given); the host test holds `backward`, fed with the fp64
coefficients, the fp64 selected values and the exact s1pt, to it.

Selection.  y2 cannot be reproduced bit for bit, so `check_forward` asserts: (a) |ysel - y2_64[p, arg, c]| <= e_y2 there;
(b) sign y2_64[p, arg, c] >= sign y2_64[p, s, c] - (e_y2[arg] + e_y2[s]) for every slot s (at most twice the bound), sign = -1
where gamma2 < 0, else 1 (-0.0, 0.0 and NULL: the maximum); (c) exactly: where an earlier slot of the list holds a neighbour
whose source row (x row, direct; z row, CI = 0) is bitwise equal -- same id or a duplicated point --, arg is not the later
slot: such slots give bit-identical y2 and the kernel's strict > keeps the first.  The backward takes the device's slots.

Bounds.  u = 2^-24, gamma_m = m u / (1 - m u), first order in u, times O2 = 1 + 2^-20 for the second-order terms; ORD = 1e-13
of the sum of magnitudes covers the order of every fp64 accumulation.  "add-by-add": a serial fp32 sum of t terms is wrong by
at most u (1 + t u) sum_(i >= 2) |S_i| (S_i the partial sums; a sum started by an fma into 0 also rounds S_1).

  sd       (edge2_moments_kernel) k - 1 serial adds of the exact d32: add-by-add.
  BatchNorm-1 rows, running pair  (edge2_bn1_kernel) the moments sum d32 and d32 d32^T are accumulated in fp64 (products of two
           fp32 are exact there), s0 = W1 . mom, s1 = W1^T M W1 in fp64: dm = ORD A1, dv = 2 |mu| dm + dm^2 + ORD A2 with
           A1 = |W1| . sum |d| / E, A2 = mean (|W1| . |d|)^2; then the finaliser BnFin as in edge_restate.py: mean u |mu| + dm;
           invstd u is + dis, dis = the larger one-sided change of 1 / sqrt(var + eps) under var +- dv (not its first-order
           form: at k = 1 var = 0 and dv / eps is not small); scale u |sc| + |g| dis; shift u |sh| + |sc| dm + |mu g| dis;
           running_mean u |.| + mom dm; running_var u |.| + mom dv E / (E - 1) (biased at E = 1).
  y1       z path: exact.  Direct: one product and ci - 1 fmaf: gamma_ci |W1| . |d32|.
  pre1, h1 pre1 = fmaf(sc1, y1, sh1): u |pre1| + |sc1| e_y1; h1 = act1(pre1): 1-Lipschitz for slope <= 1 (a flipped branch is
           inside), the product with the slope rounds once more: e_h1 = e_pre1 + u |h1| [slope1 not 0, 1].
  y2       = W2 h1, 16 chained v_mfma_f32_16x16x4_f32: a 64-term product in an order this file does not assume:
           e_y2 = gamma_64 |W2| . |h1| + |W2| . e_h1.       ysel: e_y2 at the device's slot (a).
  sums (stats_mode 2)   s0 = sum_s y2 and s1 = fmaf(y2, y2, s1) serially per point in fp32, then fp64 over the points:
           e_S0 = sum_e e_y2 + add-by-add of the partial sums of y2 + ORD sum |y2|;
           e_S1 = sum_e (2 |y2| e_y2 + e_y2^2) + add-by-add (from S_1) of the partial sums of y2^2 + ORD sum y2^2.
  BatchNorm-2 rows, running pair   dm = e_S0 / E.  The device's variance is the exact variance of its own y2~ = y2 + delta
           plus what the two accumulations a0, a1 add: |var(y2~) - var(y2)| <= (2 sum |y2 - mu| e_y2 + sum e_y2^2) / E, and
           dv = that + a1 / E + 2 (|mu| + sum e_y2 / E) a0 / E + (a0 / E)^2 + ORD (A2 + mu^2); then as BatchNorm-1.
           dc_bn_coeffs_from_sums on the device's own records: one rounding of an fp64 value per row (2 u, nn_restate.py).
  out      dc_bn_act on the device's ysel, scale2, shift2: nn_restate.act_ref.
  dgamma2, dbeta2   (Bn2BwdF, bn_bwd_terms) dz2 = dout act2'(z2) rounds once (slope2 not 0, 1): e0; dz2 xhat2 with
           xhat2 = (ysel - mean2) invstd2 on the given rows: e1 = e0 |xhat2| + 3 u |dz2 xhat2|; fp64 sums over the n rows, one
           rounding: u |S| + sum e + ORD sum |.|.
  coefficient rows a, c, b (BwdCoefFin, not returned; they enter dy2) fp64 from fp32, one rounding: e_a = u |a|,
           e_c = u |c| + |gi| is2 e_S1 / E,  e_b = u (|gi m1| + |gi m2 is2 mean2|) + |gi| (e_S0 + is2 |mean2| e_S1) / E.
  dy2      = fmaf(a, hot, fmaf(c, y2, b)) on the RECOMPUTED y2 (e_y2 as above), hot = the rounded dz2 at the selected slot:
           e_a |hot| + |a| e0 + e_c |y2| + |c| e_y2 + e_b + 2 u (|a hot| + |c y2| + |b|).
  du1      raw = dy2 W2 (second product): gamma_64 |dy2| . |W2| + e_dy2 . |W2|; du1 = raw act1'(pre1): |act1'| e_raw + u |du1|
           [slope1 not 0, 1], and where the branch is undecidable (below) + (1 - slope1) |raw|.
  dW2      (third product) a wave's accumulator takes, slot after slot, the 64 rows of its workgroup: per slot a sum of the
           accumulator and 64 products in any order, gamma_65 (|S_(t-1)| + M_t) (S the partial sums over the slots of one
           workgroup, M_t the slot's sum of |dy2 h1|), added over the slots and the workgroups; + sum (e_dy2 |h1| + |dy2| e_h1);
           the fp64 sum over the workgroups and its rounding: u |dW2| + ORD sum M.  Dead rows of the tail workgroup carry dy2 = 0.
  dbeta1, dgamma1   cs = sum_s du1 and cy = fmaf(du1, y1, cy) serially in fp32 per point (add-by-add; e_cs = sum_s e_du1 + ..,
           e_cy = sum_s (e_du1 |y1| + |du1| e_y1) + .. from S_1), fp64 over the points; Bn1BwdFin: dbeta1 = (float) s0:
           u |s0| + sum e_cs + ORD sum |cs|; dgamma1 = (float) (invstd1 (s1 - mean1 s0)): u |dg| + invstd1 (e_s1 + |mean1| e_s0)
           + ORD invstd1 (|s1| + |mean1 s0|) -- the cancellation s1 - mean1 s0 is charged on its terms, not on the result.
           m1 = s0 / E, m2 = dg / E rounded once: e_m1 = u |m1| + e_s0 / E, e_m2 = u |m2| + e_dg / E.
  dz       (edge2_scatter_kernel) acc = sum_in du1 serially in ascending edge id: sum_in e_du1 + add-by-add; g0 = acc - cs:
           + e_cs + u |g0|.  training1: diff = (indeg src_p - T) - s1pt, CI = 0 per channel with T = sum_in z_src add-by-add:
           u (indeg |z_p| + sum_(t >= 2) |T_t| + |indeg z_p - T| + |diff|) + u sum_in |d32| (the reference sums the ROUNDED
           differences over the in-edges, as autograd on y1 does; the kernel works from the rows: one more u on each); direct: v likewise from x, tx and sd per input channel,
           diff = W1 v by one product and ci - 1 fmaf: gamma_ci |W1| . |v| + |W1| . e_v.  hin = diff - (indeg - k) mean1: + u
           |(indeg - k) mean1| + u |hin|; hat = hin invstd1: invstd1 e_hin + u |hat|; q = m1 (indeg - k) + m2 hat: e_m1 |indeg - k|
           + u |p1| + e_m2 |hat| + |m2| e_hat + u |p2| + u |q|; g = g0 - q: + u |g|; dz = scale1 g: |scale1| e_g + u |dz|.
           (A contraction of a product and an add into one fma only removes a rounding.)

Undecidable first-activation branches.  act1 is continuous: a flipped branch is inside the forward bounds.  act1' is not: the
edge elements with |pre1_64| <= e_pre1 and slope1 != 1 are marked, e_du1 is widened there by (1 - slope1) |dy2 W2|, and with it
every output the element enters (cs, cy, acc, dz of its two ends, dgamma1, dbeta1).  Their count is printed per case and
capped at 1 in 10^4 of the case's E * 64 elements.  |beta1| >= 0.05 keeps the gamma1 = 0 / 1e-6 columns and the k = 1 cases
(y1 = 0, pre1 = shift1) away from 0.

Graphs.  `base`, `k1`, `tiny2`, `tiny1`, `hub600`, `random` of edge_restate.GRAPHS; `k255` = one cloud of 70 points at k = 255
(every list repeats neighbours; its last slot holds the one point the rest of the list leaves out, so slot byte 254 can
win; a second workgroup with six live rows); `w65` = one cloud of 65 points at
k = 16 (a second workgroup with one live row).  Slot 0 is the point itself.
Data.  x: normal draws plus 0, 1, 8 per input channel (the cancellation indeg x_p - sum_in x_src of the closing pass); modes x1,
x2, x3 (direct, ci = 1 .. 3), z3, z6 (through z); gamma1, gamma2 of both signs with one exact zero, one 1e-6, gamma2 one -0.0, and
gamma2 = NULL in mode x2; running pairs away from (0, 1); dout normal with one all-zero row.  CONFIGS = (training1, training2,
slope1, slope2): all four mode pairs, every slope of edge_restate.SLOPES in either block.

RECOUNT.  Worst error / bound over all graphs, modes, configs and layouts on an MI355X (in brackets: the fp32 emulation of the host
test over its cases): sd 0.49 (0.49); BatchNorm-1 mean 0.96 (0.94), invstd 0.96 (0.95), scale 0.95 (0.95), shift 0.99 (0.99),
running_mean 0.97 (0.97), running_var 0.97 (0.97); ysel 0.10 (0.11); sums 0.035 / 0.035 (0.043 / 0.041); BatchNorm-2 mean 0.035
(0.043), invstd 0.94 (0.96), scale 0.94 (0.96), shift 0.91 (0.93), running_mean 0.035 (0.044), running_var 0.95 (0.95); rows
from the device's own sums 0.50; out 1.00 (1.00: a half-ulp case of the one-rounding bound); dz 0.073 (0.072), dW2 0.28 (0.28),
dgamma1 0.076 (0.068), dbeta1 0.078 (0.094), dgamma2 0.58 (0.57), dbeta2 0.99 (0.99); z path against direct path 0.029 (0.023).
At most one act1' branch per case is undecidable (cap: 1 in 10^4).  No output is below 0.01; the lowest were looked at:
  sums, BatchNorm-2 mean, running_mean (0.035)   the bound is sum_e e_y2 with the any-order gamma_64 of the first product on
          every edge; the device's errors are of either sign and average over the E edges, which no rigorous bound may assume.
          Nothing is miscounted: the worst ratio itself is that of tiny1 (E = 1), one 64-term product against its any-order worst case.  mean_E_minus_1
          (a relative 1 / E) leaves these bounds by 9e2 .. 8e4: they bite.
  dz, dgamma1, dbeta1 (0.07 .. 0.09)   every du1 carries the any-order bounds of two 64-term products, and dz adds them over k +
          indeg edges, the two sums over E: linear in the count where the errors add like a random walk.  indeg_k_dropped leaves the dz
          bound by 2e2 .. 1e3, n_for_E by 5e4, dgamma1_without_mean the dgamma1 bound by 8 .. 2e2.  What the dz bound does NOT
          see: E - 1 for E in the two BatchNorm-1 means (a relative 6e-5 .. 8e-5 of two of dz's four terms) moves dz by 0.18 ..
          0.74 of its bound on base, hub600 and k255 (E >= 12 000); at E = 1040 (w65) it leaves it by 2.7 .. 24.  The host test prints
          that mutation's figures without asserting them.
  the extremum check (b) (0.009) is not an output: it shows how close the device's choice is to the fp64 extremum.
"""
import functools
import types

import torch

from tests import apply_restate as R
from tests import edge_restate as ER
from tests import nn_restate as NR
from tests.apply_restate import U
from tests.edge_restate import EPS, MOM, ORD, gam
from tests.nn_restate import O2

CH, PPB = 64, 64                                     # channels of both blocks; points per workgroup (edge2.hip)
S2 = ER.SLOPES[0]
CONFIGS = ((1, 1, S2, S2), (1, 0, 0.0, 1.0), (0, 1, 1.0, 0.0), (0, 0, S2, S2))     # (training1, training2, slope1, slope2)
MODES = {"x1": (1, False), "x2": (2, False), "x3": (3, False), "z3": (3, True), "z6": (6, True)}      # name -> (ci, through z)
GRAPHS = {"k255": ((70,), 255, 0), "w65": ((65,), 16, 0)}
ALL_GRAPHS = ("base", "k1", "tiny2", "tiny1", "hub600", "random", "k255", "w65")
UND_CAP = 10000                                      # undecidable branches: at most 1 in 10^4 (the project's figure)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in GRAPHS:
        sizes, k, hub = GRAPHS[name]
        nbr = R.make_graph(sizes, k, seed=900 + k, hub_rows=hub)
        if name == "k255":           # the last slot holds the one point the rest of the list leaves out: byte 254 can win
            n = nbr.shape[0]
            last = (torch.arange(n) + 1) % n
            nbr = torch.where(nbr == last[:, None], torch.arange(n)[:, None], nbr)
            nbr[:, k - 1] = last
        return nbr, sizes
    return ER.graph(name)


def _gamma(g, zero_at):
    v = ((0.5 + torch.rand(CH, generator=g)) * (torch.randint(0, 2, (CH,), generator=g) * 2.0 - 1.0)).float()
    v[zero_at], v[zero_at + 1] = 0.0, 1e-6
    return v


def _beta(g):
    return ((0.05 + 0.25 * torch.rand(CH, generator=g)) * (torch.randint(0, 2, (CH,), generator=g) * 2.0 - 1.0)).float()


def partial_abs(t, first):
    """t [n, k, C] (fp64): sum over the serial adds of |partial sum|, from the second partial (first = 1) or the first (0)."""
    return t.cumsum(1)[:, first:].abs().sum(1)


def seg_partial_abs(nbr, t):
    """t [E, C]: the term of edge e, summed at its target in ascending edge id -> sum_(i >= 2) |partial sum| per target [n, C]."""
    n = nbr.shape[0]
    tgt = nbr.reshape(-1)
    order = torch.argsort(tgt, stable=True)
    seg, ts = tgt[order], t[order]
    run = ts.cumsum(0)
    start = torch.ones_like(seg, dtype=torch.bool)
    start[1:] = seg[1:] != seg[:-1]
    idx = torch.arange(seg.numel())
    first = torch.cummax(torch.where(start, idx, 0), 0).values                  # index of the segment's first edge
    base = run[first] - ts[first]                                               # the running sum before the segment
    part = torch.where(start[:, None], 0.0, (run - base).abs())
    out = torch.zeros(n, t.shape[1], dtype=torch.float64)
    out.index_add_(0, seg, part)
    return out


class Case:
    """The data of one (graph, mode) and what follows from it exactly."""

    def __init__(self, gname, mode):
        self.name, self.mode = gname, mode
        self.nbr, self.sizes = graph(gname)
        self.n, self.k = self.nbr.shape
        n, k = self.n, self.k
        self.E = n * k
        self.ci, self.via_z = MODES[mode]
        ci = self.ci
        g = torch.Generator().manual_seed(8100 + 17 * ALL_GRAPHS.index(gname) + ci)          # x3 and z3 share their data
        self.off = torch.tensor(ER.OFFSETS)[torch.arange(ci) % 3]
        self.x = (torch.randn(n, ci, generator=g) + self.off).float()
        self.W1 = (torch.randn(CH, ci, generator=g) * 0.7).float()
        self.W2 = (torch.randn(CH, CH, generator=g) * 0.25).float()
        self.gamma1, self.beta1 = _gamma(g, 32), _beta(g)
        self.gamma2, self.beta2 = _gamma(g, 10), _beta(g)
        self.gamma2[12] = -0.0
        if mode == "x2":
            self.gamma2 = None                                                   # the NULL form: gamma2 = 1
        self.rm1, self.rv1 = (0.1 * torch.randn(CH, generator=g)).float(), (0.5 + torch.rand(CH, generator=g)).float()
        self.rm2, self.rv2 = (0.1 * torch.randn(CH, generator=g)).float(), (0.5 + torch.rand(CH, generator=g)).float()
        self.dout = torch.randn(n, CH, generator=g)
        if n > 2:
            self.dout[n // 2] = 0.0
        self.z = (self.x @ self.W1.t()).contiguous() if self.via_z else None     # an input of the z path
        self.src = self.z if self.via_z else self.x
        self.d32 = self.src[self.nbr] - self.src[:, None, :]
        assert self.d32.dtype == torch.float32
        d = self.d32.double()
        if self.via_z:
            self.y1, self.e_y1 = d, torch.zeros_like(d)
        else:
            self.y1 = d @ self.W1.double().t()
            self.e_y1 = gam(ci) * (d.abs() @ self.W1.double().abs().t())
        self.sd, self.sd_bound = d.sum(1), U * (1 + k * U) * partial_abs(d, 1)    # exact s1pt / sd and the bound of its fp32 image
        self.indeg = R.in_degree(self.nbr)
        # ties: slots of one list whose source rows are bitwise equal; `later` marks every slot that has an earlier twin
        _, cls = torch.unique(self.src.contiguous().view(torch.int32), dim=0, return_inverse=True)
        c = cls[self.nbr]
        eq = c[:, :, None] == c[:, None, :]
        first = torch.where(eq, torch.arange(k).view(1, 1, k), k).min(2).values
        self.later = first < torch.arange(k).view(1, k)
        # every edge slot and every reduction index carries weight
        assert bool((self.W1 != 0).all()) and bool((self.W2 != 0).all()) and bool((self.x != 0).all())
        assert bool((self.dout != 0).any(1).sum() >= n - 1) and bool((self.dout != 0).any(0).all())
        if n > 2:
            assert all(bool((self.d32[:, s] != 0).any()) for s in range(1, k)), "a slot without a non-zero difference"
        if gname in ("base", "hub600", "random", "k255", "w65"):
            assert bool(self.later.any()), "the graph was meant to hold ties"
        if gname == "k255":
            assert not bool(self.later[:, 254].any()) and bool(self.later[:, 1:254].any(1).all())
        self.chunks = (n + PPB - 1) // PPB

    def g2(self):
        return self.gamma2.double() if self.gamma2 is not None else torch.ones(CH, dtype=torch.float64)

    def sign(self, mut=()):
        if self.gamma2 is None or "gamma2_sign_ignored" in mut:
            return torch.ones(CH, dtype=torch.float64)
        return torch.where(self.gamma2 < 0, -1.0, 1.0).double()


@functools.lru_cache(maxsize=None)
def case(gname, mode):
    return Case(gname, mode)


# ---- BatchNorm finaliser (BnFin) ------------------------------------------------------------------------------------------------
def coef_ref(mu, var, gamma, beta, rm, rv, E, dm, dv, mut=()):
    """-> {name: (fp64 value, bound)} of mean, invstd, scale, shift, rm_new, rv_new for column statistics known to dm, dv."""
    g = gamma.double() if gamma is not None else torch.ones_like(mu)
    b = beta.double() if beta is not None else torch.zeros_like(mu)
    unb = var * E / (E - 1) if E > 1 else var
    vn = unb if "unbiased_norm" in mut else var
    if "mean_E_minus_1" in mut and E > 1:
        mu = mu * E / (E - 1)
    is_ = 1.0 / torch.sqrt(vn + EPS)
    dis = torch.maximum(is_ - 1.0 / torch.sqrt(vn + dv + EPS), 1.0 / torch.sqrt((vn - dv).clamp_min(0.0) + EPS) - is_)
    scale = g * is_
    shift = b - mu * scale
    rm_new = (1.0 - MOM) * rm.double() + MOM * mu
    rv_new = (1.0 - MOM) * rv.double() + MOM * (var if "biased_running" in mut else unb)
    return dict(mean=(mu, O2 * (U * mu.abs() + dm)), invstd=(is_, O2 * (U * is_ + dis)), scale=(scale, O2 * (U * scale.abs() + g.abs() * dis)),
                shift=(shift, O2 * (U * shift.abs() + scale.abs() * dm + (mu * g).abs() * dis + dm * g.abs() * dis)),
                rm_new=(rm_new, O2 * (U * rm_new.abs() + MOM * dm)),
                rv_new=(rv_new, O2 * (U * rv_new.abs() + MOM * dv * (E / (E - 1) if E > 1 else 1.0))))


def bn1_ref(cs, mut=()):
    """dc_edge2_bn1_stats (direct path) -> {name: (value, bound)}: sd and the BatchNorm-1 rows with the running pair."""
    E = cs.E
    flat = cs.y1.reshape(E, CH)
    mu = flat.sum(0) / E
    var = ((flat - mu) ** 2).sum(0) / E
    mag = cs.d32.double().abs().reshape(E, -1)
    if not cs.via_z:
        mag = mag @ cs.W1.double().abs().t()
    dm = ORD * mag.sum(0) / E
    dv = 2 * mu.abs() * dm + dm * dm + ORD * (mag * mag).sum(0) / E
    out = coef_ref(mu, var, cs.gamma1, cs.beta1, cs.rm1, cs.rv1, E, dm, dv, mut)
    out["sd"] = (-cs.sd if "sd_reversed" in mut else cs.sd, cs.sd_bound)
    return out


def eval_ref(gamma, beta, rm, rv):
    return NR.eval_ref(gamma, beta, rm, rv)


# ---- forward ---------------------------------------------------------------------------------------------------------------
class Fwd:
    """pre1, h1, y2 of every edge in fp64 for given scale1 / shift1, with their bounds and the undecidable mask."""


def forward_ref(cs, sc1, sh1, slope1, mut=()):
    f = Fwd()
    sc, sh = sc1.double(), sh1.double()
    W2 = cs.W2.double()
    f.pre = sc * cs.y1 + sh
    f.e_pre = U * f.pre.abs() + sc.abs() * cs.e_y1
    s1 = 0.0 if "act1_relu" in mut else slope1
    f.h = torch.where(f.pre > 0, f.pre, s1 * f.pre)
    f.e_h = f.e_pre + (U * f.h.abs() if slope1 not in (0.0, 1.0) else 0.0)
    f.y2 = f.h @ W2.t()
    f.e_y2 = O2 * (gam(CH) * (f.h.abs() @ W2.abs().t()) + f.e_h @ W2.abs().t())
    f.und = (f.pre.abs() <= f.e_pre) & (slope1 != 1.0)
    f.slope1 = slope1
    return f


def slots(cs, f, mut=()):
    """The first extremal slot of sign y2_64 (last: the mutation) -> int64 [n, 64]."""
    k = cs.k
    m = cs.sign(mut) * f.y2
    top = m.max(1).values
    ar = torch.arange(k).view(1, k, 1)
    tie = m >= (top - 1e-12 * top.abs())[:, None]     # twins: a blocked fp64 product may differ in the last bits between equal rows
    if "last_slot_on_ties" in mut:
        return torch.where(tie, ar, -1).max(1).values
    return torch.where(tie, ar, k).min(1).values


def gather_slot(t, slot):
    return t.gather(1, slot.long()[:, None, :])[:, 0]


def bn2_ref(cs, f, mut=()):
    """-> {name: (value, bound)}: sum0, sum1 (the stats_mode 2 records) and the BatchNorm-2 rows with the running pair."""
    E, k = cs.E, cs.k
    y, e = f.y2, f.e_y2
    S0, S1 = y.sum((0, 1)), (y * y).sum((0, 1))
    mu = S0 / E
    var = ((y - mu) ** 2).sum((0, 1)) / E
    a0 = (U * (1 + k * U) * partial_abs(y, 1)).sum(0)
    a1 = (U * (1 + k * U) * partial_abs(y * y, 0)).sum(0)
    se = e.sum((0, 1))
    e_S0 = O2 * (se + a0 + ORD * y.abs().sum((0, 1)))
    e_S1 = O2 * ((2 * y.abs() * e + e * e).sum((0, 1)) + a1 + ORD * S1)
    dm = e_S0 / E
    dv = O2 * (((2 * (y - mu).abs() * e + e * e).sum((0, 1)) + a1) / E + 2 * (mu.abs() + se / E) * a0 / E + (a0 / E) ** 2
               + ORD * (S1 / E + mu * mu))
    out = coef_ref(mu, var, cs.gamma2, cs.beta2, cs.rm2, cs.rv2, E, dm, dv, mut)
    out["sum0"], out["sum1"] = (S0, e_S0), (S1, e_S1)
    return out


def sums_coef_ref(sums, gamma, beta):
    """dc_bn_coeffs_from_sums on a record of fp64 sums [2 C + 1] -> {name: (value, bound)}: one rounding of an fp64 value."""
    E = float(sums[2 * CH])
    mu = sums[:CH] / E
    var = (sums[CH:2 * CH] / E - mu * mu).clamp_min(0.0)
    g = gamma.double() if gamma is not None else torch.ones_like(mu)
    b = beta.double() if beta is not None else torch.zeros_like(mu)
    is_ = 1.0 / torch.sqrt(var + EPS)
    return dict(mean=(mu, 2 * U * mu.abs()), invstd=(is_, 2 * U * is_), scale=(g * is_, 2 * U * (g * is_).abs()),
                shift=(b - mu * g * is_, 2 * U * (b.abs() + (mu * g * is_).abs())))


# ---- backward ------------------------------------------------------------------------------------------------------------------
def backward_ref(cs, f, coef1, coef2, slope2, t1, t2, ysel, arg, s1pt, mut=()):
    """The closed form of edge2.hip's backward in fp64 on the values the entry point is given (any float dtype: the host test
    passes fp64 ones) -> {name: (value, bound)} for dz, dW2, dgamma1, dbeta1, dgamma2, dbeta2; f = forward_ref on coef1's rows."""
    n, k, E = cs.n, cs.k, cs.E
    slope1 = f.slope1
    mean1, is1, sc1, _ = (t.double() for t in coef1)
    mean2, is2, sc2, sh2 = (t.double() for t in coef2)
    ysel, s1pt = ysel.double(), (s1pt.double() if s1pt is not None else None)
    W1, W2, dout = cs.W1.double(), cs.W2.double(), cs.dout.double()
    aW2 = W2.abs()
    # 1. d z2 and the BatchNorm-2 sums
    z2 = sc2 * ysel + sh2
    sl2 = slope1 if "act2_slope1" in mut else slope2
    da = torch.where(z2 > 0, 1.0, sl2).double()
    dz2 = dout * da
    e0 = U * dz2.abs() * ((da != 1.0) & (da != 0.0))
    xh = (ysel if "dgamma2_without_mean" in mut else ysel - mean2) * is2
    S0, S1 = dz2.sum(0), (dz2 * xh).sum(0)
    e_S0 = e0.sum(0) + ORD * dz2.abs().sum(0)
    e_S1 = (e0 * xh.abs() + 3 * U * (dz2 * xh).abs()).sum(0) + ORD * (dz2 * xh).abs().sum(0)
    out = dict(dbeta2=(S0, O2 * (U * S0.abs() + e_S0)), dgamma2=(S1, O2 * (U * S1.abs() + e_S1)))
    zero = torch.zeros(CH, dtype=torch.float64)
    if t2:
        gi = cs.g2() * is2
        m1, m2 = S0 / E, S1 / E
        a, c, b = gi, -gi * m2 * is2, -gi * m1 + gi * m2 * is2 * mean2
        e_a, e_c = U * a.abs(), U * c.abs() + gi.abs() * is2 * e_S1 / E
        e_b = U * ((gi * m1).abs() + (gi * m2 * is2 * mean2).abs()) + gi.abs() * (e_S0 + is2 * mean2.abs() * e_S1) / E
    else:
        a, c, b, e_a, e_c, e_b = sc2, zero, zero, zero, zero, zero
    # 2. the recompute pass
    hit = arg.long()[:, None, :] == torch.arange(k).view(1, k, 1)
    hot = torch.where(hit, dz2[:, None, :], 0.0)
    e_hot = torch.where(hit, e0[:, None, :], 0.0)
    y2 = f.y2
    dy2 = a * hot + c * y2 + b
    e_dy2 = e_a * hot.abs() + a.abs() * e_hot + e_c * y2.abs() + c.abs() * f.e_y2 + e_b + 2 * U * ((a * hot).abs() + (c * y2).abs() + b.abs())
    raw = dy2 @ W2
    e_raw = gam(CH) * (dy2.abs() @ aW2) + e_dy2 @ aW2
    sl1 = slope2 if "act1_prime_slope2" in mut else slope1
    d1 = torch.where(f.pre > 0, 1.0, sl1).double()
    du = raw * d1
    e_du = d1.abs() * e_raw + U * du.abs() * ((d1 != 1.0) & (d1 != 0.0)) + f.und * (1.0 - slope1) * raw.abs()
    # dW2: the workgroups' accumulators slot after slot, then fp64 over the workgroups
    h = f.h
    dW, e_dW, Mtot = torch.zeros(CH, CH, dtype=torch.float64), torch.zeros(CH, CH, dtype=torch.float64), torch.zeros(CH, CH, dtype=torch.float64)
    for blk in range(cs.chunks):
        rows = slice(blk * PPB, min((blk + 1) * PPB, n))
        T = torch.einsum("psn,psc->snc", dy2[rows], h[rows])
        M = torch.einsum("psn,psc->snc", dy2[rows].abs(), h[rows].abs())
        S = T.cumsum(0)
        dW += S[-1]
        Mtot += M.sum(0)
        e_dW += gam(CH + 1) * ((S - T).abs() + M).sum(0)
    if "tail_rows_counted" in mut:
        dW = dW + (cs.chunks * PPB - n) * torch.einsum("sn,sc->nc", dy2[n - 1], h[n - 1])
    e_dW = e_dW + torch.einsum("psn,psc->nc", e_dy2, h.abs()) + torch.einsum("psn,psc->nc", dy2.abs(), f.e_h) + U * dW.abs() + ORD * Mtot
    out["dW2"] = (dW, O2 * e_dW)
    # the per-point sums and the BatchNorm-1 sums
    y1 = cs.y1
    csum = du.sum(1)
    e_cs = e_du.sum(1) + U * (1 + k * U) * partial_abs(du, 1)
    cy = (du * y1).sum(1)
    e_cy = (e_du * y1.abs() + du.abs() * cs.e_y1).sum(1) + U * (1 + k * U) * partial_abs(du * y1, 0)
    s0, s1 = csum.sum(0), cy.sum(0)
    e_s0, e_s1 = e_cs.sum(0) + ORD * csum.abs().sum(0), e_cy.sum(0) + ORD * cy.abs().sum(0)
    dg = is1 * (s1 if "dgamma1_without_mean" in mut else s1 - mean1 * s0)
    e_dg = is1 * (e_s1 + mean1.abs() * e_s0) + ORD * is1 * (s1.abs() + (mean1 * s0).abs())
    out["dbeta1"], out["dgamma1"] = (s0, O2 * (U * s0.abs() + e_s0)), (dg, O2 * (U * dg.abs() + e_dg))
    # 3. the closing pass
    acc = R._scatter(cs.nbr, du)
    e_acc = R._scatter(cs.nbr, e_du) + U * (1 + cs.indeg * U) * seg_partial_abs(cs.nbr, du.reshape(E, CH))
    g0 = acc if "own_row_dropped" in mut else acc - csum
    e_g = e_acc + e_cs + U * g0.abs()
    g = g0
    if t1:
        Em = E - 1 if "E_minus_1" in mut else n if "n_for_E" in mut else E
        m1, m2 = s0 / Em, dg / Em
        e_m1, e_m2 = U * m1.abs() + e_s0 / E, U * m2.abs() + e_dg / E
        d = cs.indeg
        src = cs.src.double()
        T = R._scatter(cs.nbr, src[:, None, :].expand(-1, k, -1))
        PT = seg_partial_abs(cs.nbr, src[:, None, :].expand(-1, k, -1).reshape(E, -1))
        w = R._scatter(cs.nbr, cs.d32.double())                  # sum_in (src_p - src_i) over the ROUNDED differences, as autograd sees them
        v = w - s1pt
        e_v = U * (R._scatter(cs.nbr, cs.d32.double().abs()) + (d * src).abs() + (1 + d * U) * PT + (d * src - T).abs() + v.abs())
        if cs.via_z:
            diff, e_diff = v, e_v
        else:
            diff = v @ W1.t()
            e_diff = gam(cs.ci) * (v.abs() @ W1.abs().t()) + e_v @ W1.abs().t()
        dk = d - k
        hin = diff - dk * mean1
        e_hin = e_diff + U * (dk * mean1).abs() + U * hin.abs()
        hat = hin * is1
        e_hat = is1 * e_hin + U * hat.abs()
        p1 = torch.zeros_like(hat) if "indeg_k_dropped" in mut else m1 * dk
        p2 = m2 * hat
        q = p1 + p2
        e_q = e_m1 * dk.abs() + U * p1.abs() + e_m2 * hat.abs() + m2.abs() * e_hat + U * p2.abs() + U * q.abs()
        g = g0 - q
        e_g = e_g + e_q + U * g.abs()
    dz = sc1 * g
    out["dz"] = (dz, O2 * (sc1.abs() * e_g + U * dz.abs()))
    # the magnitudes each output is summed from (the scale of the host test's closed form = autograd comparison)
    gmag = R._scatter(cs.nbr, du.abs()) + du.abs().sum(1) + ((p1.abs() + p2.abs()) if t1 else 0.0)
    out["_mag"] = dict(dz=sc1.abs() * gmag, dW2=Mtot, dbeta1=du.abs().sum((0, 1)), dbeta2=dz2.abs().sum(0), dgamma2=(dz2.abs() * is2 * (ysel.abs() + mean2.abs())).sum(0),
                       dgamma1=is1 * ((du * y1).abs().sum((0, 1)) + mean1.abs() * du.abs().sum((0, 1))))
    return out


def autograd(cs, slot, t1, t2, slope1, slope2):
    """fp64 autograd on the materialised [n, k, 64] tensors with its own batch statistics -> dict(out, dz, dW2, dgamma1, ...)."""
    E = cs.E
    y1 = cs.y1.clone().requires_grad_(True)
    g1, b1 = cs.gamma1.double().requires_grad_(True), cs.beta1.double().requires_grad_(True)
    g2, b2 = cs.g2().requires_grad_(True), cs.beta2.double().requires_grad_(True)
    W2 = cs.W2.double().requires_grad_(True)

    def bn(t, g, b, training, rm, rv):
        if training:
            flat = t.reshape(E, CH)
            mu = flat.sum(0) / E
            var = ((flat - mu) ** 2).sum(0) / E
        else:
            mu, var = rm.double(), rv.double()
        scale = g / torch.sqrt(var + EPS)
        return t * scale + (b - mu * scale)

    p1 = bn(y1, g1, b1, t1, cs.rm1, cs.rv1)
    h1 = torch.where(p1 > 0, p1, slope1 * p1)
    y2 = h1 @ W2.t()
    p2 = gather_slot(bn(y2, g2, b2, t2, cs.rm2, cs.rv2), slot)
    out = torch.where(p2 > 0, p2, slope2 * p2)
    out.backward(cs.dout.double())
    ga = y1.grad
    return dict(out=out.detach(), dz=R._scatter(cs.nbr, ga) - ga.sum(1), dW2=W2.grad, dgamma1=g1.grad, dbeta1=b1.grad,
                dgamma2=g2.grad, dbeta2=b2.grad)


class Exact:
    """The fp64 chain of one (case, config) from the case's own data: coefficients, forward, slots, backward (host test)."""


@functools.lru_cache(maxsize=2)
def exact(gname, mode, cfg):
    return exact_chain(gname, mode, cfg)


def exact_chain(gname, mode, cfg, mut=()):
    cs = case(gname, mode)
    t1, t2, slope1, slope2 = cfg
    o = Exact()
    o.cfg = cfg
    o.bn1 = bn1_ref(cs, mut)
    if t1:
        o.coef1 = [o.bn1[name][0] for name in ("mean", "invstd", "scale", "shift")]
    else:
        e = eval_ref(cs.gamma1, cs.beta1, cs.rm1, cs.rv1)
        o.coef1 = [e[name][0] for name in ("mean", "invstd", "scale", "shift")]
    o.f = forward_ref(cs, o.coef1[2], o.coef1[3], slope1, mut)
    o.slot = slots(cs, o.f, mut)
    o.ysel = gather_slot(o.f.y2, o.slot)
    o.bn2 = bn2_ref(cs, o.f, mut)
    if t2:
        o.coef2 = [o.bn2[name][0] for name in ("mean", "invstd", "scale", "shift")]
    else:
        e = eval_ref(cs.gamma2, cs.beta2, cs.rm2, cs.rv2)
        o.coef2 = [e[name][0] for name in ("mean", "invstd", "scale", "shift")]
    z2 = o.coef2[2] * o.ysel + o.coef2[3]
    sl = slope1 if "act2_slope1" in mut else slope2
    o.out = torch.where(z2 > 0, z2, sl * z2)
    o.bwd = backward_ref(cs, o.f, o.coef1, o.coef2, slope2, t1, t2, o.ysel, o.slot, o.bn1["sd"][0], mut)
    return o


# ---- the checks both backends share -------------------------------------------------------------------------------------------
def check_named(ck, tag, got, ref, names):
    for name in names:
        if got.get(name) is not None:
            ck.hold(f"{tag} {name}", got[name], *ref[name])


def check_bn1(ck, cs, got):
    """got: sd, mean, invstd, scale, shift, rm_new, rv_new of dc_edge2_bn1_stats."""
    check_named(ck, "bn1", got, bn1_ref(cs), ("sd", "mean", "invstd", "scale", "shift", "rm_new", "rv_new"))


_FWD = {}


def forward_of(cs, sc1, sh1, slope1):
    """forward_ref, kept per (case, the bits of the coefficient rows, slope)."""
    key = (cs.name, cs.mode, sc1.float().numpy().tobytes(), sh1.float().numpy().tobytes(), slope1)
    if key not in _FWD:
        if len(_FWD) > 6:
            _FWD.clear()
        _FWD[key] = forward_ref(cs, sc1, sh1, slope1)
    return _FWD[key]


def check_forward(ck, cs, sc1, sh1, slope1, ysel, arg):
    """(a), (b), (c) of the module docstring on the device's ysel / arg -> the Fwd."""
    f = forward_of(cs, sc1, sh1, slope1)
    k = cs.k
    ck.true("slot in range", bool((arg.long() < k).all()))
    a = arg.long().clamp_max(k - 1)
    ya, ea = gather_slot(f.y2, a), gather_slot(f.e_y2, a)
    ck.hold("ysel against y2_64 at the device's slot", ysel, ya, ea)
    m = cs.sign() * f.y2
    ma = gather_slot(m, a)
    ck.hold("the slot is an extremum of sign(gamma2) y2_64", (m - ma[:, None]).clamp_min(0.0), torch.zeros_like(m), f.e_y2 + ea[:, None])
    bad = int(cs.later.gather(1, a).sum())
    print(f"[{ck.what}] first-slot tie rule: {bad} selected slots have an earlier bitwise-equal twin ({int(cs.later.sum())} later twins)")
    ck.true("ties keep the first slot", bad == 0)
    if cs.name == "k255":
        ck.true("slot byte 254 is selected somewhere", bool((arg == 254).any()))
    return f


def check_bn2(ck, cs, f, got):
    """got: any of mean, invstd, scale, shift, rm_new, rv_new (stats_mode 1) and sum0, sum1 (stats_mode 2)."""
    check_named(ck, "bn2", got, bn2_ref(cs, f), ("sum0", "sum1", "mean", "invstd", "scale", "shift", "rm_new", "rv_new"))


def check_out(ck, ysel, sc2, sh2, slope2, out):
    val, bound, _ = NR.act_ref(ysel, sc2, sh2, slope2)
    ck.hold(f"out slope2 {slope2:.1f}", out, val, bound)


def undecidable_count(ck, cs, f):
    n_und = int(f.und.sum())
    print(f"[{ck.what}] {n_und} undecidable act1' branches of {cs.E * CH}")
    ck.true("undecidable branches at most 1 in 10^4", n_und * UND_CAP <= cs.E * CH)
    return n_und


BWD_NAMES = ("dz", "dW2", "dgamma1", "dbeta1", "dgamma2", "dbeta2")


def check_backward(ck, cs, f, coef1, coef2, slope2, t1, t2, ysel, arg, s1pt, got, tag=""):
    """got: dz, dW2 and the four parameter gradients (None where NULL was passed) of dc_edge2_backward -> the reference."""
    ref = backward_ref(cs, f, coef1, coef2, slope2, t1, t2, ysel, arg, s1pt)
    undecidable_count(ck, cs, f)
    check_named(ck, f"backward{tag}", got, ref, BWD_NAMES)
    return ref


def check_paths(ck, cs_x, cs_z, sc1, sh1, slope1, ysel_x, ysel_z):
    """The direct path and the z path of one ci = 3 case (the same x, W1, W2 and the same scale1 / shift1 bits: inference
    coefficients) agree within the sum of their bounds, not in bits.  Both are held to the direct path's fp64 chain: the z path
    with what its input z = fl(x W1^T) (a ci-term fp32 product in any order: a = gamma_ci |x| . |W1|) and the subtraction
    z_j - z_i add to y1:  a_j + a_i + u |z_j - z_i| + u |W1| . |x_j - x_i| (the direct chain rounds x_j - x_i, the exact one does
    not).  Each ysel is within its bound of the extremum over the slots, and |max_s a_s - max_s b_s| <= max_s |a_s - b_s|."""
    assert torch.equal(cs_x.x, cs_z.x) and torch.equal(cs_x.W1, cs_z.W1) and torch.equal(cs_x.W2, cs_z.W2) and cs_x.ci == cs_z.ci
    a = gam(cs_x.ci) * (cs_x.x.double().abs() @ cs_x.W1.double().abs().t())
    e_y1 = (a[cs_x.nbr] + a[:, None, :] + U * cs_z.d32.double().abs() + U * (cs_x.d32.double().abs() @ cs_x.W1.double().abs().t()))
    fx = forward_of(cs_x, sc1, sh1, slope1)
    fz = forward_ref(types.SimpleNamespace(y1=cs_x.y1, e_y1=e_y1, W2=cs_x.W2), sc1, sh1, slope1)
    ck.hold("ysel of the z path against ysel of the direct path", ysel_z, ysel_x, (fx.e_y2 + fz.e_y2).max(1).values)
