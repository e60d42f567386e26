"""The cases and checks that tests/test_gpu_apply_abi.py (the C ABI on the device) and tests/test_apply_restate_host.py (the CPU
build of ell_math.h) share: data of a (graph, channel count) pair, and one driver that runs every body through a `backend`,
holds each output element to the bound of tests/apply_restate.py and returns the raw results for bit comparisons.

A backend takes and returns CPU fp32 tensors of the logical shapes (layouts, sentinels and vector widths are its business):
    fwd(op, x) -> out                              op in "grad" | "div" | "div_curl_norm" | "hodge"
    T(op, dy, prev, v=None) -> out                 the transposes; prev = None: accumulate 0, else the destination's content
    grad_T_sum(dy, a, b) -> out                    b may be None
    knn_sum(h, scale) -> out;   knn_sum_T(dout, scale, prev) -> out
    knn_max(h) -> (out, arg);   knn_max_affine(h, scale, shift, slope) -> (out, arg)
    knn_max_affine_residual(h, scale, shift, slope, h2, scale2, shift2, slope2) -> (out, out2, arg)
    knn_max_T(arg, dout, prev, variant) -> out     variant 0 / 1: the two loop forms of the max-aggregation backward
    max_T_variants                                 the variants the backend has
"""
import functools

import torch

from tests import apply_restate as R

SLOPE = float(torch.tensor(0.2, dtype=torch.float32))        # the entry points take slopes and scales as float


class Checks:
    """Every figure is printed before anything is asserted; `done()` asserts them all."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def hold(self, name, got, ref, bound):
        got, ref, bound = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, bound))
        err = (got - ref).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0))
        worst = float(ratio.max())
        print(f"[{self.what}] {name}: worst error / bound = {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name, worst))

    def exact(self, name, got, ref):
        ok = torch.equal(got.double().cpu(), ref.double().cpu())
        print(f"[{self.what}] {name}: {'identical' if ok else 'DIFFERENT'}")
        if not ok:
            self.bad.append((name, "not exact"))

    def true(self, name, cond):
        if not cond:
            print(f"[{self.what}] {name}: FAILED")
            self.bad.append((name, "false"))

    def done(self):
        assert not self.bad, f"{self.what}: {self.bad}"


class Case:
    """The data of one (graph, C): operators, features, gradients, previous contents for accumulate = 1."""

    def __init__(self, nbr, c, seed):
        self.nbr, self.C = nbr, c
        self.n, self.k = nbr.shape
        n, k = self.n, self.k
        self.G, self.D = R.make_coef(n, k, seed + 1), R.make_coef(n, k, seed + 2)
        self.x = R.make_features(n, c, seed + 3)
        self.v = R.make_vectors(n, c, seed + 4)
        self.dc = R.make_features(n, 2 * c, seed + 5)
        self.dy1, self.dy2, self.dy3 = R.make_features(n, c, seed + 6), R.make_features(2 * n, c, seed + 7), R.make_features(n, 3 * c, seed + 8)
        self.a, self.b = R.make_features(n, c, seed + 9), R.make_features(n, c, seed + 10)
        self.prev1, self.prev2, self.prevdc = R.make_features(n, c, seed + 11), R.make_features(2 * n, c, seed + 12), R.make_features(n, 2 * c, seed + 13)
        self.h, self.h2 = R.make_features(n, c, seed + 14), R.make_features(n, c, seed + 15)
        (self.sc, self.sh), (self.sc2, self.sh2) = R.make_affine(c, seed + 16), R.make_affine(c, seed + 17)
        self.mean_scale = float(torch.tensor(1.0 / k, dtype=torch.float32))


GRAPHS = {                                           # name -> (cloud sizes, k, hub rows)
    "base": ((300, 257, 64), 20, 0),
    "k1": ((130, 64), 1, 0),
    "k7": ((130, 64), 7, 0),
    "k64": ((130, 64), 64, 0),
    "hub": ((2400,), 20, 2200),
    "k85": ((300,), 85, 0),
    "k128": ((300,), 128, 0),
    "k255": ((300,), 255, 0),
}


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (nbr, cloud sizes) of a named graph: the same for the device and the host tests."""
    sizes, k, hub = GRAPHS[name]
    return R.make_graph(sizes, k, seed=100 + k + hub, hub_rows=hub), sizes


@functools.lru_cache(maxsize=None)
def case(name, c):
    return Case(graph(name)[0], c, seed=1000 * len(name) + c)


ALL = ("grad", "div", "div_curl_norm", "hodge", "grad_T", "div_T", "div_curl_norm_T", "hodge_T", "grad_T_sum", "knn_sum", "knn_sum_T",
       "knn_max", "knn_max_affine", "knn_max_affine_residual", "knn_max_T")


def run(backend, case, ck, which=ALL):
    """-> {name: raw result} of every body in `which`."""
    nbr, c = case.nbr, case.C
    out = {}

    def lin(name, got, ref, extra=2):
        val, S, m = ref
        ck.hold(name, got, val, R.gamma_bound(m, S, extra))
        out[name] = got

    if "grad" in which:
        lin("grad", backend.fwd("grad", case.x), R.grad(nbr, case.G, case.x))
    if "div" in which:
        lin("div", backend.fwd("div", case.v), R.div(nbr, case.D, case.v))
    if "div_curl_norm" in which:
        got = backend.fwd("div_curl_norm", case.v)
        (val, S, m), nb = R.div_curl_norm(nbr, case.D, case.v)
        ck.hold("div|curl", got[:, :2 * c], val[:, :2 * c], R.gamma_bound(m, S[:, :2 * c]))
        ck.hold("norm", got[:, 2 * c:], val[:, 2 * c:], nb)
        ck.true("norm of a zero vector is 0", bool((got[:, 2 * c:][val[:, 2 * c:] == 0] == 0).all()) and bool((val[:, 2 * c:] == 0).any()))
        out["div_curl_norm"] = got
    if "hodge" in which:
        lin("hodge", backend.fwd("hodge", case.dc), R.hodge(nbr, case.G, case.dc))
    for acc in (0, 1):
        tag = f" accumulate {acc}"
        if "grad_T" in which:
            p = case.prev1 if acc else None
            lin("grad_T" + tag, backend.T("grad", case.dy2, p), R.grad_T(nbr, case.G, case.dy2, p))
        if "div_T" in which:
            p = case.prev2 if acc else None
            lin("div_T" + tag, backend.T("div", case.dy1, p), R.div_T(nbr, case.D, case.dy1, p))
        if "div_curl_norm_T" in which:
            p = case.prev2 if acc else None
            lin("div_curl_norm_T" + tag, backend.T("div_curl_norm", case.dy3, p, v=case.v), R.div_curl_norm_T(nbr, case.D, case.dy3, case.v, p),
                extra=6)
        if "hodge_T" in which:
            p = case.prevdc if acc else None
            lin("hodge_T" + tag, backend.T("hodge", case.dy2, p), R.hodge_T(nbr, case.G, case.dy2, p))
        if "knn_sum_T" in which:
            p = case.prev1 if acc else None
            for sname, scale in (("sum", 1.0), ("mean", case.mean_scale)):
                lin(f"knn_{sname}_T" + tag, backend.knn_sum_T(case.dy1, scale, p), R.knn_sum_T(nbr, case.dy1, scale, p))
    if "grad_T_sum" in which:
        for b in (case.b, None):
            lin("grad_T_sum" + (" a + b" if b is not None else " a"), backend.grad_T_sum(case.dy2, case.a, b),
                R.grad_T_sum(nbr, case.G, case.dy2, case.a, b))
    if "knn_sum" in which:
        for sname, scale in (("sum", 1.0), ("mean", case.mean_scale)):
            lin(f"knn_{sname}", backend.knn_sum(case.h, scale), R.knn_sum(nbr, case.h, scale))
    arg_plain = None
    if "knn_max" in which:
        got, arg_plain = backend.knn_max(case.h)
        val, slot = R.knn_max(nbr, case.h)
        ck.exact("knn_max value", got, val)
        ck.exact("knn_max first maximal slot", arg_plain, slot)
        out["knn_max"], out["knn_max arg"] = got, arg_plain

    def affine(name, got, arg, y, e, block=None):
        ymax, _ = R.first_max(y)
        emax = e.max(1).values
        if block is None:
            ck.hold(name + " value", got, ymax, emax)
        else:
            r, B = block
            ck.hold(name + " value", got, r + ymax, R.G3 * (emax / R.G2 + B))
        a = arg.long()[:, None, :]
        ck.true(name + " slot in range", bool((arg.long() < nbr.shape[1]).all()))
        ya, ea = y.gather(1, a.clamp_max(nbr.shape[1] - 1))[:, 0], e.gather(1, a.clamp_max(nbr.shape[1] - 1))[:, 0]
        et = e.gather(1, y.argmax(1, keepdim=True))[:, 0]
        ck.hold(name + " slot: its fp64 value against the fp64 maximum", ya, ymax, ea + et)
        out[name], out[name + " arg"] = got, arg

    if "knn_max_affine" in which:
        got, arg = backend.knn_max_affine(case.h, case.sc, case.sh, SLOPE)
        y, e = R.affine_candidates(nbr, case.h, case.sc, case.sh, SLOPE)
        affine("knn_max_affine", got, arg, y, e)
        if c > 2:       # the column with scale 0 is constant: slot 0 wins
            ck.true("constant column takes slot 0", bool((arg[:, c // 2] == 0).all()))
    if "knn_max_affine_residual" in which:
        got, got2, arg = backend.knn_max_affine_residual(case.h, case.sc, case.sh, SLOPE, case.h2, case.sc2, case.sh2, SLOPE)
        y, e = R.affine_candidates(nbr, case.h, case.sc, case.sh, SLOPE)
        affine("knn_max_affine_residual", got, arg, y, e, block=R.affine_block(case.h2, case.sc2, case.sh2, SLOPE))
        ck.exact("residual form: second copy", got2, got)
    if "knn_max_T" in which:
        if arg_plain is None:                        # the forward entry is not part of this run: the slots of the restatement (exact)
            arg_plain = R.knn_max(nbr, case.h)[1].to(torch.uint8)
        for acc in (0, 1):
            p = case.prev1 if acc else None
            ref = R.knn_max_T(nbr, arg_plain, case.dy1, p)
            for variant in backend.max_T_variants:
                lin(f"knn_max_T accumulate {acc} variant {variant}", backend.knn_max_T(arg_plain, case.dy1, p, variant), ref)
    return out


def same_bits(ck, what, res, base):
    """Every result of `res` bit-identical to its namesake in `base`."""
    for name, t in res.items():
        ck.exact(f"{what}: {name}", t, base[name])
