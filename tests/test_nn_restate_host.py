"""The fp64 restatement, the data and the bounds of tests/nn_restate.py on the CPU: against the CPU build of
deltaconv_amd/csrc/nn_math.h run in the kernels' own chunk and lane order (tests/hostcheck: hc_nn_*), with the share of
arg-max pairs that fp64 alone cannot decide held under its cap, and against mutations of the restatement, each of which must
leave its bound by a factor of 10 somewhere: the bounds bite.  Runs without a GPU; tests/test_gpu_nn_abi.py applies the same
drivers to the device."""
import ctypes

import pytest
import torch

from tests import nn_restate as NR
from tests.apply_cases import Checks
from tests.test_hostcheck_ell import hc, P          # noqa: F401  (hc: the module fixture that builds and binds libhostcheck.so)

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
NAN = float("nan")


class Host:
    """The backend of the drivers of tests/nn_restate.py over libhostcheck.so (contiguous operands)."""

    def __init__(self, lib):
        self.lib = lib
        lib.hc_nn_bn_stats.argtypes = [vp, cl, ci, vp, vp, cf, cf] + [vp] * 6
        lib.hc_nn_vn_stats.argtypes = [vp, cl, ci, ci, vp, vp, cf, cf] + [vp] * 6
        lib.hc_nn_eval_coeffs.argtypes = [vp] * 4 + [cf, ci] + [vp] * 4
        lib.hc_nn_bn_act.argtypes = [vp, cl, ci, vp, vp, cf, vp, vp, vp]
        lib.hc_nn_bwd_reduce.argtypes = [vp, vp, cl, ci] + [vp] * 5 + [cf, ci] + [vp] * 3
        lib.hc_nn_bwd.argtypes = [ci, vp, vp, vp, ci, ci, vp, cl, ci] + [vp] * 5 + [cf, ci] + [vp] * 3
        lib.hc_nn_vn_apply.argtypes = [vp, cl, ci, ci, vp, vp, vp]
        lib.hc_nn_vn_bwd.argtypes = [vp, vp, ci, cl, ci] + [vp] * 5 + [ci] + [vp] * 3
        lib.hc_nn_pool.argtypes = [vp, ci, ci, ci, vp, vp, cf, ci, vp, vp]
        lib.hc_nn_cloud_bias_add.argtypes = [vp, vp, cl, ci, cl, vp]
        lib.hc_nn_cloud_colsum.argtypes = [vp, ci, cl, ci, vp]

    @staticmethod
    def _stats_out(c, rm0, rv0):
        o = {k: torch.full((c,), NAN) for k in ("mean", "invstd", "scale", "shift")}
        o["rm"], o["rv"] = (rm0.clone(), rv0.clone()) if rm0 is not None else (None, None)
        return o

    def bn_stats(self, x, gamma, beta, mom, rm0, rv0):
        o = self._stats_out(x.shape[1], rm0, rv0)
        self.lib.hc_nn_bn_stats(P(x), x.shape[0], x.shape[1], P(gamma), P(beta), NR.EPS, mom, P(o["rm"]), P(o["rv"]), P(o["mean"]),
                                P(o["invstd"]), P(o["scale"]), P(o["shift"]))
        return o

    def vn_stats(self, t, co, combine, gamma, beta, mom, rm0, rv0):
        o = self._stats_out(co, rm0, rv0)
        self.lib.hc_nn_vn_stats(P(t), t.shape[0] // 2, co, combine, P(gamma), P(beta), NR.EPS, mom, P(o["rm"]), P(o["rv"]), P(o["mean"]),
                                P(o["invstd"]), P(o["scale"]), P(o["shift"]))
        return o

    def eval_coeffs(self, gamma, beta, rm, rv):
        o = {k: torch.full_like(rm, NAN) for k in ("mean", "invstd", "scale", "shift")}
        self.lib.hc_nn_eval_coeffs(P(gamma), P(beta), P(rm), P(rv), NR.EPS, rm.numel(), P(o["mean"]), P(o["invstd"]), P(o["scale"]), P(o["shift"]))
        return o

    def bn_act(self, x, scale, shift, slope, res, second):
        y = torch.full_like(x, NAN)
        y2 = torch.full_like(x, NAN) if second else None
        self.lib.hc_nn_bn_act(P(x), x.shape[0], x.shape[1], P(scale), P(shift), slope, P(res), P(y), P(y2))
        return y, y2

    def bwd_reduce(self, dy, x, co, gamma, slope, training, grads):
        c = x.shape[1]
        o = dict(dgamma=torch.full((c,), NAN) if grads else None, dbeta=torch.full((c,), NAN) if grads else None, coefs=torch.full((5, c), NAN))
        self.lib.hc_nn_bwd_reduce(P(dy), P(x), x.shape[0], c, P(co["scale"]), P(co["shift"]), P(co["mean"]), P(co["invstd"]), P(gamma), slope,
                                  training, P(o["dgamma"]), P(o["dbeta"]), P(o["coefs"]))
        return o

    def _bwd(self, pool, dy, dp, arg, n, wm, x, co, gamma, slope, training):
        c = x.shape[1]
        o = dict(dh=torch.full_like(x, NAN), dgamma=torch.full((c,), NAN), dbeta=torch.full((c,), NAN))
        self.lib.hc_nn_bwd(pool, P(dy), P(dp), P(arg), n, wm, P(x), x.shape[0], c, P(co["scale"]), P(co["shift"]), P(co["mean"]),
                           P(co["invstd"]), P(gamma), slope, training, P(o["dh"]), P(o["dgamma"]), P(o["dbeta"]))
        return o

    def bwd(self, dy, x, co, gamma, slope, training):
        return self._bwd(0, dy, None, None, 1, 0, x, co, gamma, slope, training)

    def pool_bwd(self, dp, arg, x, B, N, co, gamma, slope, wm, training):
        return self._bwd(1, None, dp, arg, N, wm, x, co, gamma, slope, training)

    def vn_apply(self, t, co, combine, scale, shift):
        out = torch.full((t.shape[0], co), NAN)
        self.lib.hc_nn_vn_apply(P(t), t.shape[0] // 2, co, combine, P(scale), P(shift), P(out))
        return out

    def vn_bwd(self, dout, t, co, combine, c32, gamma, training):
        o = dict(din=torch.full((t.shape[0], 2 * co if combine else co), NAN), dgamma=torch.full((co,), NAN), dbeta=torch.full((co,), NAN))
        self.lib.hc_nn_vn_bwd(P(dout), P(t), combine, t.shape[0] // 2, co, P(c32["scale"]), P(c32["shift"]), P(c32["mean"]), P(c32["invstd"]),
                              P(gamma), training, P(o["din"]), P(o["dgamma"]), P(o["dbeta"]))
        return o

    def pool(self, x, B, N, scale, shift, slope, wm):
        c = x.shape[1]
        pooled, arg = torch.full((B, (1 + wm) * c), NAN), torch.full((B, c), -1, dtype=torch.int32)
        self.lib.hc_nn_pool(P(x), B, N, c, P(scale), P(shift), slope, wm, P(pooled), P(arg))
        return pooled, arg

    def cloud_bias_add(self, h, g, mx, alias):
        y = h.clone() if alias else torch.full_like(h, NAN)
        self.lib.hc_nn_cloud_bias_add(P(y if alias else h), P(g), h.shape[0], h.shape[1], mx, P(y))
        return y

    def cloud_colsum(self, x, B, mx):
        out = torch.full((B, x.shape[1]), NAN)
        self.lib.hc_nn_cloud_colsum(P(x), B, mx, x.shape[1], P(out))
        return out


def test_tilings():
    NR.assert_tilings()


@pytest.mark.parametrize("c", NR.CHANNELS)
def test_rows_cpu_build_holds_the_bounds(hc, c):
    be = Host(hc)
    for r in NR.row_counts(c):
        ck = Checks(f"host rows {r} C {c}")
        NR.run_rows(be, NR.row_case(r, c), ck)
        ck.done()


@pytest.mark.parametrize("combine", [0, 1, 2])
@pytest.mark.parametrize("co", NR.CHANNELS)
def test_vectors_cpu_build_holds_the_bounds(hc, co, combine):
    be = Host(hc)
    for n in NR.row_counts(co):
        ck = Checks(f"host vectors {n} co {co} combine {combine}")
        NR.run_vec(be, NR.vec_case(n, co, combine), ck)
        ck.done()


@pytest.mark.parametrize("c", NR.CHANNELS)
def test_pool_cpu_build_holds_the_bounds(hc, c):
    """Also: the fp64 reference alone leaves at most 0.1 % of the (cloud, column) pairs of a case undecided, and the data hold
    exact ties at the maximum wherever a cloud has two rows."""
    be = Host(hc)
    for B, N in NR.POOLS:
        cs = NR.pool_case(B, N, c)
        ck = Checks(f"host pool {B} x {N} C {c}")
        _, und = NR.run_pool(be, cs, ck)
        for co in (cs.tr, cs.ev):
            ref = NR.pool_ref(cs.x, B, N, co["scale"].float(), co["shift"].float(), NR.SLOPE)
            assert 1.0 - float(ref["decided"].double().mean()) <= 1e-3
            assert N == 1 or int((ref["ties"] & ref["decided"]).sum()) > 0
        assert und <= 1e-3
        ck.done()


@pytest.mark.parametrize("c", [64, 7, 256])
def test_cloud_sums_cpu_build(hc, c):
    be = Host(hc)
    for B, mx in NR.CLOUDS:
        ck = Checks(f"host cloud {B} x {mx} C {c}")
        NR.run_cloud(be, NR.cloud_case(B, mx, c), ck)
        ck.done()


# ---- mutations ----------------------------------------------------------------------------------------------------------------------
def _distance(mutated, true, bound):
    err = (mutated.double() - true.double()).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(ratio.max())


def _mutation_distances():
    """-> {mutation: (worst |mutated - true| / bound, the output it shows in, the case)}."""
    out = {}

    def note(mut, name, where, d):
        if d > out.get(mut, (0.0, "", ""))[0]:
            out[mut] = (d, name, where)

    for r, c in ((2, 7), (300, 64)):
        cs = NR.row_case(r, c)
        where = f"rows {r} C {c}"
        true = NR.stats_ref(cs.x, cs.gamma, cs.beta, NR.MOM, cs.rm0, cs.rv0)
        mutd = NR.stats_ref(cs.x, cs.gamma, cs.beta, NR.MOM, cs.rm0, cs.rv0, mut=("biased_running_var",))
        note("biased_running_var", "running_var", where, _distance(mutd["rv"][0], *true["rv"]))
        sc, sh = cs.tr["scale"].float(), cs.tr["shift"].float()
        val, bound, _ = NR.act_ref(cs.x, sc, sh, NR.SLOPE, cs.res)
        note("residual_before_act", "y", where, _distance(NR.act_ref(cs.x, sc, sh, NR.SLOPE, cs.res, mut=("residual_before_act",))[0], val, bound))
        true = NR.bwd_ref(cs.x, cs.dy.double(), cs.tr, cs.gamma, NR.SLOPE, 1, 1, 1)
        for mut in ("drop_m2", "eval_in_training"):
            mutd = NR.bwd_ref(cs.x, cs.dy.double(), cs.tr, cs.gamma, NR.SLOPE, 1, 1, 1, mut=(mut,))
            for name in ("c_a", "c_b", "dh"):
                note(mut, name, where, _distance(mutd[name][0], *true[name]))
        # the check of c_sh is exact: any column that differs from its neighbour shows it
        note("coef_row_off_by_one", "c_sh", where, float("inf") if not torch.equal(sh.roll(-1), sh) else 0.0)
    for B, N, c in ((7, 5, 8), (3, 17, 64), (4, 100, 64)):
        cs = NR.pool_case(B, N, c)
        where = f"pool {B} x {N} C {c}"
        sc, sh = cs.tr["scale"].float(), cs.tr["shift"].float()
        true, mutd = NR.pool_ref(cs.x, B, N, sc, sh, NR.SLOPE), NR.pool_ref(cs.x, B, N, sc, sh, NR.SLOPE, mut=("tie_to_highest",))
        dec = true["decided"]
        note("tie_to_highest", "arg", where, float("inf") if not torch.equal(mutd["first"][dec], true["first"][dec]) else 0.0)
        arg = true["first"].to(torch.int32)
        g, eg = NR.pool_dy(cs.dp, arg, B, N, c, 1)
        ref = NR.bwd_ref(cs.x, g, cs.tr, cs.gamma, NR.SLOPE, 1, 1, 1, eg=eg)
        for mut in ("neighbour_cloud_mean", "dmean_not_divided"):
            gm, _ = NR.pool_dy(cs.dp, arg, B, N, c, 1, mut=(mut,))
            mutd = NR.bwd_ref(cs.x, gm, cs.tr, cs.gamma, NR.SLOPE, 1, 1, 1, eg=eg)
            for name in ("dh", "dgamma", "dbeta"):
                note(mut, name, where, _distance(mutd[name][0], *ref[name]))
    for n, co, combine in ((17, 8, 1), (300, 64, 2)):
        cs = NR.vec_case(n, co, combine)
        where = f"vectors {n} co {co} combine {combine}"
        true = NR.vn_stats_ref(cs.t, co, combine, cs.gamma, cs.beta, NR.MOM, cs.rm0, cs.rv0)
        mutd = NR.vn_stats_ref(cs.t, co, combine, cs.gamma, cs.beta, NR.MOM, cs.rm0, cs.rv0, mut=("swap_layouts",))
        note("swap_layouts", "mean", where, _distance(mutd["mean"][0], *true["mean"]))
        sc, sh = true["scale"][0].float(), true["shift"][0].float()
        val, bound = NR.vn_apply_ref(cs.t, co, combine, sc, sh)
        note("swap_layouts", "out", where, _distance(NR.vn_apply_ref(cs.t, co, combine, sc, sh, mut=("swap_layouts",))[0], val, bound))
        val, bound = NR.vn_bwd_ref(cs, combine, 1)["din"]
        note("dpq_sign", "din", where, _distance(NR.vn_bwd_ref(cs, combine, 1, mut=("dpq_sign",))["din"][0], val, bound))
    return out


MUTATIONS = ("biased_running_var", "drop_m2", "eval_in_training", "neighbour_cloud_mean", "dmean_not_divided", "tie_to_highest",
             "dpq_sign", "swap_layouts", "residual_before_act", "coef_row_off_by_one")


def test_mutations_leave_the_bounds():
    """Biased running variance, the m2 term dropped, the inference formula in training mode, the mean gradient of the
    neighbouring cloud on a cloud's first row, dmean not divided by N, ties to the highest row, the sign of -dy_u in the second
    half of d(P, Q) flipped, interleaved and blocked (P, Q) swapped, the residual added before the activation, the second coefficient row off by one column."""
    table = _mutation_distances()
    for mut in MUTATIONS:
        d, name, where = table.get(mut, (0.0, "-", "-"))
        print(f"{mut:24s} {d:12.3g}  ({name}, {where})")
    missed = [mut for mut in MUTATIONS if table.get(mut, (0.0,))[0] < 10.0]
    assert not missed, f"mutations within 10 x their bound everywhere: {missed}"
