"""The fp64 restatement, the data and the bounds of tests/edge_restate.py on the CPU: against the CPU build of
deltaconv_amd/csrc/edge_math.h (tests/hostcheck: hc_edge_all, every intermediate returned, V = 4 and V = 1), against itself
(the closed form equals the autograd result; no activation branch of this data is undecidable), and against mutations of the
restatement, each of which must leave its bound by a factor of 10 somewhere on the `base` or `hub600` data: the bounds bite.
Runs without a GPU; tests/test_gpu_edge_abi.py applies the same checks to the device."""
import ctypes

import pytest
import torch

from tests import edge_restate as ER
from tests.apply_cases import Checks
from tests.test_hostcheck_ell import hc, P          # noqa: F401  (hc: the module fixture that builds and binds libhostcheck.so)


def _run_host(lib, cs, v, slope, training):
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.hc_edge_all.argtypes = [ci] + [vp] * 4 + [ci] * 3 + [vp] * 2 + [cf] * 3 + [ci] + [vp] * 16
    n, k, C = cs.n, cs.k, cs.C
    nbr32 = cs.nbr.to(torch.int32).contiguous()
    tptr, tedge = torch.zeros(n + 1, dtype=torch.int32), torch.zeros(n * k, dtype=torch.int32)
    lib.hc_csc_build(P(nbr32), n, k, P(tptr), P(tedge))
    f = lambda *s: torch.full(s, float("nan"))
    b = lambda *s: torch.full(s, 255, dtype=torch.uint8)
    o = dict(amax=f(n, C), amin=f(n, C), argmax=b(n, C), argmin=b(n, C), s1pt=f(n, C), coef=f(4, C), out=f(n, C), arg=b(n, C),
             dzs=f(n, C), dy=f(n, C), dgamma=f(C), dbeta=f(C), m12=f(2, C), rm_new=cs.rm.clone(), rv_new=cs.rv.clone())
    lib.hc_edge_all(v, P(cs.y), P(nbr32), P(tptr), P(tedge), n, k, C, P(cs.gamma), P(cs.beta), ER.EPS, ER.MOM, slope, training,
                    P(o["rm_new"]), P(o["rv_new"]), P(o["amax"]), P(o["amin"]), P(o["argmax"]), P(o["argmin"]), P(o["s1pt"]),
                    P(o["coef"]), P(o["out"]), P(o["arg"]), P(cs.dout), P(o["dzs"]), P(o["dy"]), P(o["dgamma"]), P(o["dbeta"]),
                    P(o["m12"]))
    o["mean"], o["invstd"], o["scale"], o["shift"] = o["coef"]
    return o


def _check(ck, cs, o, slope, training):
    ER.check_gather(ck, cs, o)
    ER.check_coefficients(ck, cs, training, o)
    if not training:
        ck.exact("eval leaves the running pair alone", torch.stack([o["rm_new"], o["rv_new"]]), torch.stack([cs.rm, cs.rv]))
    ER.check_apply(ck, cs, o["scale"], o["shift"], slope, o["out"], o["arg"])
    ER.check_backward(ck, cs, slope, training, o["scale"], o["shift"], o)
    ref = ER.reference(cs.name, cs.C, slope, training)
    ck.true("no undecidable activation branch in this data", int(ref["und"].sum()) == 0)
    cl = ref["closed"]
    ck.hold("m1", o["m12"][0], cl["m1"], ER.U * cl["m1"].abs() + cl["e_dbeta"] / cs.E)
    ck.hold("m2", o["m12"][1], cl["m2"], ER.U * cl["m2"].abs() + cl["e_dgamma"] / cs.E)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("slope", ER.SLOPES)
@pytest.mark.parametrize("gname,c", [("base", 64), ("base", 72), ("base", 8), ("base", 7), ("base", 23), ("k1", 64), ("k1", 7),
                                     ("tiny2", 8), ("tiny2", 7), ("tiny1", 8), ("tiny1", 7), ("hub600", 64), ("hub600", 23)])
def test_cpu_build_holds_the_bounds(hc, gname, c, slope, training):
    cs = ER.case(gname, c)
    ck = Checks(f"host {gname} C {c}")
    res = {}
    for v in (4, 1):
        if c % v == 0:
            ck.what = f"host {gname} C {c} V {v}"
            res[v] = _run_host(hc, cs, v, slope, training)
            _check(ck, cs, res[v], slope, training)
    if 4 in res:
        ck.what = f"host {gname} C {c}"
        for name, t in res[4].items():
            ck.exact(f"V 4 = V 1: {name}", t, res[1][name])
    ck.done()


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("slope", ER.SLOPES)
@pytest.mark.parametrize("gname,c", [("base", 64), ("base", 7), ("k1", 7), ("tiny2", 7), ("tiny1", 7), ("hub600", 64)])
def test_closed_form_equals_autograd(gname, c, slope, training):
    """The closed form of edge_math.h, restated in fp64, against autograd on the materialised tensor: 1e-9 of the bound's own
    magnitudes apart at the most (both are fp64 evaluations of the same real function in different orders), and no
    undecidable activation branch in this data."""
    ref = ER.reference(gname, c, slope, training)
    auto, cl = ref["auto"], ref["closed"]
    ck = Checks(f"closed = autograd {gname} C {c} slope {slope:.1f} training {training}")
    ck.true("no undecidable activation branch", int(ref["und"].sum()) == 0)
    for name in ("dy", "dgamma", "dbeta"):
        ck.hold(name, cl[name], auto[name], 1e-3 * cl["e_" + name])          # e_* is ~1e-7 of the magnitudes: 1e-10 of them
    ck.done()


def _distance(name, mutated, true, bound):
    """worst |mutated - true| / bound over the elements (inf where a zero bound is left)."""
    err = (mutated.double() - true.double()).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
    return float(ratio.max())


def _mutation_distances(gname, c, slope):
    """-> {mutation: (worst distance / bound, the output it shows in)} on one case."""
    cs = ER.case(gname, c)
    out = {}

    def note(mut, name, d):
        if d > out.get(mut, (0.0, ""))[0]:
            out[mut] = (d, name)

    tr = ER.reference(gname, c, slope, 1)
    ev = ER.reference(gname, c, slope, 0)
    co, cl = tr["co"], tr["closed"]
    # statistics
    for mut, names in (("unbiased_norm", (("invstd", "invstd"), ("scale", "scale"), ("shift", "shift"))), ("biased_running", (("rv_new", "rv"),))):
        m = ER.coefficients(cs, 1, mut=(mut,))
        for attr, e in names:
            note(mut, attr, _distance(attr, getattr(m, attr), getattr(co, attr), getattr(co, "e_" + e)))
    # slots: exact checks, any difference is a failure
    first = cs.slots(co.scale)
    for mut, slot in (("last_extremal_slot", cs.slots(co.scale, last=True)), ("amax_for_negative_scale", cs.slots(co.scale, swap=True))):
        note(mut, "arg", float("inf") if not torch.equal(slot, first) else 0.0)
        sc32, sh32 = co.scale.float(), co.shift.float()
        val, bound, _ = ER.apply_out(cs, sc32, sh32, slope)
        a = cs.a32.double().gather(1, slot[:, None, :])[:, 0]
        w = sc32.double() * a + sh32.double()
        note(mut, "out", _distance("out", torch.where(w > 0, w, slope * w), val, bound))
    # backward, training
    for mut in ("E_minus_1", "k_for_indeg", "drop_m1"):
        m = ER.closed(cs, co, tr["slot"], slope, 1, mut=(mut,))
        for name in ("dy", "dgamma", "dbeta"):
            note(mut, name, _distance(name, m[name], cl[name], cl["e_" + name]))
    m = ER.closed(cs, ev["co"], ev["slot"], slope, 0, mut=("train_in_eval",))
    note("train_in_eval", "dy", _distance("dy", m["dy"], ev["closed"]["dy"], ev["closed"]["e_dy"]))
    return out


MUTATIONS = ("unbiased_norm", "biased_running", "E_minus_1", "last_extremal_slot", "amax_for_negative_scale", "k_for_indeg", "drop_m1",
             "train_in_eval")


def test_mutations_leave_the_bounds():
    """unbiased variance in the normalisation, biased variance in running_var, E - 1 for E in m1 / m2, the last extremal slot,
    amax for a negative scale, k for indeg in the column term, the m1 (indeg - k) term dropped, the training terms in eval."""
    slope = ER.SLOPES[0]
    table = {g: _mutation_distances(g, 64, slope) for g in ("base", "hub600")}
    print(f"{'mutation':28s} {'base':>24s} {'hub600':>24s}")
    for mut in MUTATIONS:
        print(f"{mut:28s} " + " ".join(f"{table[g][mut][0]:14.3g} ({table[g][mut][1]:>7s})" for g in table))
    missed = [mut for mut in MUTATIONS if max(table[g][mut][0] for g in table) < 10.0]
    assert not missed, f"mutations within 10 x their bound everywhere: {missed}"
