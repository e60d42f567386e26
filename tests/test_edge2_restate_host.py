"""The fp64 restatement, the data and the bounds of tests/edge2_restate.py on the CPU: against itself (the closed form of
edge2.hip's backward equals fp64 autograd on the materialised tensors), against an fp32 emulation of the kernels' arithmetic in
torch (fp32 elementwise steps in the kernels' order, fp32 matmuls for the three products, serial fp32 sums where the kernels sum
serially, fp64 where they use fp64), which passes through the same check drivers as the device's results and stays within every
bound, and against mutations of the restatement, each of which leaves a bound on every case it changes.  Runs without a GPU;
tests/test_gpu_edge2_abi.py applies the same checks to the device."""
import pytest
import torch

from tests import edge2_restate as E2
from tests.apply_cases import Checks
from tests.edge2_restate import CH, PPB
from tests.edge_restate import EPS, MOM, ORD

HOST_CASES = [(g, m) for g in E2.ALL_GRAPHS for m in E2.MODES]


# ---- the fp32 emulation -----------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fmaf on fp32 tensors: the product of two fp32 is exact in fp64; the fp64 sum rounds to 53 bits before the 24."""
    return (a.double() * b.double() + c.double()).float()


def act(t, slope):
    return torch.where(t > 0, t, torch.tensor(slope, dtype=torch.float32) * t)


def bnfin(s0, s1, rows, gamma, beta, rm, rv):
    """BnFin of colreduce.h on fp64 column sums -> fp32 rows."""
    m = s0 / rows
    var = (s1 / rows - m * m).clamp_min(0.0)
    is_ = 1.0 / torch.sqrt(var + EPS)
    g = gamma.double() if gamma is not None else torch.ones_like(m)
    b = beta.double() if beta is not None else torch.zeros_like(m)
    unb = var * rows / (rows - 1) if rows > 1 else var
    return dict(mean=m.float(), invstd=is_.float(), scale=(g * is_).float(), shift=(b - m * g * is_).float(),
                rm_new=((1.0 - MOM) * rm.double() + MOM * m).float(), rv_new=((1.0 - MOM) * rv.double() + MOM * unb).float())


def eval_coeffs(gamma, beta, rm, rv):
    """bn_eval_coeffs_kernel: fp32."""
    is_ = 1.0 / torch.sqrt(rv + torch.tensor(EPS, dtype=torch.float32))
    g = gamma if gamma is not None else torch.ones_like(rm)
    b = beta if beta is not None else torch.zeros_like(rm)
    return dict(mean=rm.clone(), invstd=is_, scale=g * is_, shift=b - rm * g * is_)


def w1_dot(W1, v):
    """W1 [64, ci] times v [..., ci] as the kernels do: one product, then fmaf per further input channel."""
    a = W1[:, 0] * v[..., 0:1]
    for d in range(1, W1.shape[1]):
        a = fma(W1[:, d], v[..., d:d + 1], a)
    return a


def serial_sum(t):
    s = t[:, 0].clone()
    for i in range(1, t.shape[1]):
        s = s + t[:, i]
    return s


def serial_fma_sum(a, b):
    s = torch.zeros_like(a[:, 0])
    for i in range(a.shape[1]):
        s = fma(a[:, i], b[:, i], s)
    return s


def in_edge_sum(nbr, t):
    """t [E, C] fp32 summed at the edge's target, serially in ascending edge id."""
    n = nbr.shape[0]
    tgt = nbr.reshape(-1)
    order = torch.argsort(tgt, stable=True)
    seg = tgt[order]
    start = torch.ones_like(seg, dtype=torch.bool)
    start[1:] = seg[1:] != seg[:-1]
    idx = torch.arange(seg.numel())
    pos = idx - torch.cummax(torch.where(start, idx, 0), 0).values
    out = torch.zeros(n, t.shape[1], dtype=torch.float32)
    for step in range(int(pos.max()) + 1):
        sel = order[pos == step]
        out[tgt[sel]] = out[tgt[sel]] + t[sel]
    return out


def emulate(cs, cfg):
    """Every entry point of edge2.hip for one (case, config) in the kernels' arithmetic -> dict of fp32 results."""
    t1, t2, slope1, slope2 = cfg
    n, k, E = cs.n, cs.k, cs.E
    o = {}
    d = cs.d32
    # BatchNorm-1: dc_edge2_bn1_stats (direct) / dc_edge_gather_stats (through z; held by its own suite: here fp64 sums of d32)
    s1pt = serial_sum(d)
    dd = d.double().reshape(E, -1)
    if cs.via_z:
        s0, s1 = dd.sum(0), (dd * dd).sum(0)
    else:
        W = cs.W1.double()
        mom1, mom2 = dd.sum(0), dd.t() @ dd
        s0, s1 = W @ mom1, ((W @ mom2) * W).sum(1)
    o["bn1"] = dict(bnfin(s0, s1, E, cs.gamma1, cs.beta1, cs.rm1, cs.rv1), sd=s1pt)
    c1 = o["bn1"] if t1 else eval_coeffs(cs.gamma1, cs.beta1, cs.rm1, cs.rv1)
    o["coef1"] = torch.stack([c1[name] for name in ("mean", "invstd", "scale", "shift")])
    mean1, is1, sc1, sh1 = o["coef1"]
    # forward
    y1 = d if cs.via_z else w1_dot(cs.W1, d)
    h = act(fma(sc1, y1, sh1), slope1)
    y2 = (h.reshape(E, CH) @ cs.W2.t()).reshape(n, k, CH)
    sg = cs.sign().float()
    m = sg * y2
    top = m.max(1).values
    o["arg"] = torch.where(m == top[:, None], torch.arange(k).view(1, k, 1), k).min(1).values.to(torch.uint8)
    o["ysel"] = sg * top
    S0, S1 = serial_sum(y2).double().sum(0), serial_fma_sum(y2, y2).double().sum(0)
    o["bn2"] = dict(bnfin(S0, S1, E, cs.gamma2, cs.beta2, cs.rm2, cs.rv2), sum0=S0, sum1=S1)
    c2 = o["bn2"] if t2 else eval_coeffs(cs.gamma2, cs.beta2, cs.rm2, cs.rv2)
    o["coef2"] = torch.stack([c2[name] for name in ("mean", "invstd", "scale", "shift")])
    mean2, is2, sc2, sh2 = o["coef2"]
    o["out"] = act(fma(sc2, o["ysel"], sh2), slope2)
    # backward 1: d z2, its two sums, the coefficient rows
    z2 = fma(sc2, o["ysel"], sh2)
    dz2 = cs.dout * torch.where(z2 > 0, 1.0, slope2).float()
    bx = dz2 * ((o["ysel"] - mean2) * is2)
    B0, B1 = dz2.double().sum(0), bx.double().sum(0)
    if t2:
        gi = cs.g2() * is2.double()
        m1, m2 = B0 / E, B1 / E
        ca, cc, cb = gi.float(), (-gi * m2 * is2.double()).float(), (-gi * m1 + gi * m2 * is2.double() * mean2.double()).float()
    else:
        ca, cc, cb = sc2, torch.zeros(CH), torch.zeros(CH)
    # 2: the recompute pass
    hot = torch.where(o["arg"].long()[:, None, :] == torch.arange(k).view(1, k, 1), dz2[:, None, :], torch.zeros(()))
    dy2 = fma(ca, hot, fma(cc, y2, cb))
    du = (dy2.reshape(E, CH) @ cs.W2).reshape(n, k, CH) * torch.where(h > 0, 1.0, slope1).float()
    csum, cy = serial_sum(du), serial_fma_sum(du, y1)
    dW = torch.zeros(CH, CH, dtype=torch.float64)
    for blk in range(cs.chunks):
        rows = slice(blk * PPB, min((blk + 1) * PPB, n))
        acc = torch.zeros(CH, CH)
        for s in range(k):
            acc = acc + dy2[rows, s].t() @ h[rows, s]
        dW += acc.double()
    s0, s1 = csum.double().sum(0), cy.double().sum(0)
    dg = is1.double() * (s1 - mean1.double() * s0)
    m1 = (s0 / E).float() if t1 else torch.zeros(CH)
    m2 = (dg / E).float() if t1 else torch.zeros(CH)
    # 3: the closing pass
    acc = in_edge_sum(cs.nbr, du.reshape(E, CH))
    g = acc - csum
    if t1:
        indeg = cs.indeg.float()
        T = in_edge_sum(cs.nbr, cs.src[:, None, :].expand(-1, k, -1).reshape(E, -1))
        v = (indeg * cs.src - T) - s1pt
        diff = v if cs.via_z else w1_dot(cs.W1, v)
        hat = (diff - (indeg - float(k)) * mean1) * is1
        g = g - (m1 * (indeg - float(k)) + m2 * hat)
    o["bwd"] = dict(dz=sc1 * g, dW2=dW.float(), dgamma1=dg.float(), dbeta1=s0.float(), dgamma2=B1.float(), dbeta2=B0.float())
    return o


WORST = {}


class Noting(Checks):
    """Checks that also keeps the worst ratio per output name over all cases (the RECOUNT figures of the emulation)."""

    def hold(self, name, got, ref, bound):
        before = len(self.bad)
        super().hold(name, got, ref, bound)
        got, ref, bound = (torch.as_tensor(t).detach().double() for t in (got, ref, bound))
        ratio = torch.where(bound > 0, (got - ref).abs() / bound.clamp_min(1e-300), torch.zeros_like(bound))
        key = name.split(" slope2")[0]
        WORST[key] = max(WORST.get(key, 0.0), float(ratio.max())) if len(self.bad) == before else float("inf")


@pytest.mark.parametrize("gname,mode", HOST_CASES)
def test_fp32_emulation_holds_the_bounds(gname, mode):
    cs = E2.case(gname, mode)
    ck = Noting(f"emulation {gname} {mode}")
    for cfg in E2.CONFIGS:
        t1, t2, slope1, slope2 = cfg
        ck.what = f"emulation {gname} {mode} training {t1}{t2} slopes {slope1:.1f} {slope2:.1f}"
        o = emulate(cs, cfg)
        if not cs.via_z and t1:
            E2.check_bn1(ck, cs, o["bn1"])
        f = E2.check_forward(ck, cs, o["coef1"][2], o["coef1"][3], slope1, o["ysel"], o["arg"])
        E2.check_bn2(ck, cs, f, o["bn2"])
        E2.check_out(ck, o["ysel"], o["coef2"][2], o["coef2"][3], slope2, o["out"])
        E2.check_backward(ck, cs, f, o["coef1"], o["coef2"], slope2, t1, t2, o["ysel"], o["arg"], o["bn1"]["sd"] if t1 else None, o["bwd"])
    ck.done()
    print("worst error / bound so far:", {k_: round(v, 3) for k_, v in sorted(WORST.items())})


@pytest.mark.parametrize("gname,mode", HOST_CASES)
def test_closed_form_equals_autograd(gname, mode):
    """The closed form of the file header and of edge2_scatter_kernel in fp64, fed with the fp64 coefficients, the fp64 selected
    values and the exact s1pt, against fp64 autograd on the materialised tensors: both are fp64 evaluations of one real function in
    different orders, 100 ORD = 1e-11 of the column's scale apart at the most (ORD = 1e-13 is the order term of one fp64
    accumulation relative to its magnitudes and the chain stacks a few dozen of them).  The column's scale is the largest sum of
    magnitudes an element of the column is added from (`_mag` of backward_ref): with batch statistics in the second block
    sum_e dy2 = 0, so dbeta1 at slope1 = 1 and the dW2 column of the gamma1 = 0 channel are exact zeros reached by cancellation."""
    cs = E2.case(gname, mode)
    ck = Checks(f"closed = autograd {gname} {mode}")
    for cfg in E2.CONFIGS:
        ex = E2.exact(gname, mode, cfg)
        auto = E2.autograd(cs, ex.slot, *cfg)
        ck.what = f"closed = autograd {gname} {mode} {cfg}"
        E2.undecidable_count(ck, cs, ex.f)
        for name in ("out",) + E2.BWD_NAMES:
            val = ex.out if name == "out" else ex.bwd[name][0]
            a = auto[name]
            mag = a.abs() if name == "out" else ex.bwd["_mag"][name]
            scale = mag.max(0).values if a.dim() == 2 else mag.max()
            ck.hold(name, val, a, 100 * ORD * scale * torch.ones_like(a))
    ck.done()


@pytest.mark.parametrize("gname", E2.ALL_GRAPHS)
def test_direct_and_z_path_agree(gname):
    cx, cz = E2.case(gname, "x3"), E2.case(gname, "z3")
    cfg = E2.CONFIGS[3]
    ox, oz = emulate(cx, cfg), emulate(cz, cfg)
    assert torch.equal(ox["coef1"], oz["coef1"])
    ck = Checks(f"emulation {gname} x3 / z3")
    E2.check_paths(ck, cx, cz, ox["coef1"][2], ox["coef1"][3], cfg[2], ox["ysel"], oz["ysel"])
    ck.done()


# ---- mutations ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("last_slot_on_ties", "gamma2_sign_ignored", "n_for_E", "act1_prime_slope2", "own_row_dropped", "indeg_k_dropped",
             "unbiased_norm", "biased_running", "tail_rows_counted", "sd_reversed", "mean_E_minus_1", "act1_relu", "act2_slope1",
             "dgamma2_without_mean", "dgamma1_without_mean")
REPORTED = ("E_minus_1",)                            # printed, not asserted: inside the dz bound for E >= 12 000 (RECOUNT of edge2_restate.py)
MUT_CASES = (("base", "x3"), ("hub600", "z3"), ("k255", "x3"), ("w65", "x2"), ("k1", "x1"), ("tiny1", "x3"), ("tiny2", "z6"))
MUT_CONFIGS = (E2.CONFIGS[0], E2.CONFIGS[1])


def _ratio(mutated, true, bound):
    err = (mutated.double() - true.double()).abs()
    return float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0)).max())


def _outputs(cs, ex):
    """name -> value of every returned output of the exact chain (bn1 rows only where dc_edge2_bn1_stats computes them)."""
    o = {f"bn1 {k_}": v[0] for k_, v in ex.bn1.items()}
    o.update({f"bn2 {k_}": v[0] for k_, v in ex.bn2.items()})
    o.update({k_: ex.bwd[k_][0] for k_ in E2.BWD_NAMES})
    o["ysel"], o["out"] = ex.ysel, ex.out
    return o


def _distance(cs, true, mutated):
    """-> {output: worst |mutated - true| / bound}; the slot checks (b), (c) are applied to the mutated slots as to a device's."""
    bounds = {f"bn1 {k_}": v[1] for k_, v in true.bn1.items()}
    bounds.update({f"bn2 {k_}": v[1] for k_, v in true.bn2.items()})
    bounds.update({k_: true.bwd[k_][1] for k_ in E2.BWD_NAMES})
    bounds["ysel"] = E2.gather_slot(true.f.e_y2, true.slot)
    bounds["out"] = E2.NR.act_ref(true.ysel, true.coef2[2], true.coef2[3], true.cfg[3])[1] + true.coef2[2].abs() * bounds["ysel"]
    a, b = _outputs(cs, true), _outputs(cs, mutated)
    d = {name: _ratio(b[name], a[name], bounds[name]) for name in a}
    m = cs.sign() * true.f.y2
    ma, ea = E2.gather_slot(m, mutated.slot), E2.gather_slot(true.f.e_y2, mutated.slot)
    d["arg (b)"] = _ratio((m - ma[:, None]).clamp_min(0.0), torch.zeros_like(m), true.f.e_y2 + ea[:, None])
    d["arg (c)"] = float("inf") if bool(cs.later.gather(1, mutated.slot).any()) else 0.0
    return d


def test_mutations_leave_the_bounds():
    """Each mutation of the restatement pushes at least one output past its bound on every case it changes (a case it leaves
    alone -- equal values everywhere -- shows 0), and every returned output is pushed past its bound by at least one."""
    hit, missed = set(), []
    for gname, mode in MUT_CASES:
        cs = E2.case(gname, mode)
        for cfg in MUT_CONFIGS:
            true = E2.exact(gname, mode, cfg)
            for mut in MUTATIONS + REPORTED:
                d = _distance(cs, true, E2.exact_chain(gname, mode, cfg, (mut,)))
                worst = max(d, key=d.get)
                changed = any(v > 0 for v in d.values())
                print(f"{mut:24s} {gname:7s} {mode} training {cfg[0]}{cfg[1]} slopes {cfg[2]:.1f} {cfg[3]:.1f}: "
                      f"{'unchanged' if not changed else f'{d[worst]:.3g} x bound in {worst}'}")
                if mut in REPORTED:
                    continue
                hit.update(name for name, v in d.items() if v > 1.0)
                if changed and not d[worst] > 1.0:
                    missed.append((mut, gname, mode, cfg, worst, d[worst]))
    assert not missed, f"mutations inside every bound on a case they change: {missed}"
    true = E2.exact(*MUT_CASES[0], MUT_CONFIGS[0])
    names = set(_outputs(E2.case(*MUT_CASES[0]), true))
    assert names <= hit, f"outputs no mutation pushes past its bound: {sorted(names - hit)}"
