"""The layer-0 edge MLP kernels (csrc/edge.hip, edge_math.h, the finalisers of colreduce.h) through the C ABI, per element
against the fp64 restatement of tests/edge_restate.py, in every layout that changes the vector width or the tiling of the
column reduction: dc_edge_gather_stats (compute_stats 1 and 0), dc_edge_max_apply, dc_edge_max_apply_residual,
dc_edge_max_backward (training 1 and 0, with and without dgamma / dbeta) and dc_edge_max_backward_tiled.

Bounds, data and the handling of undecidable activation branches: the docstring of tests/edge_restate.py (u = 2^-24, every
rounding counted from the code).  tests/test_edge_restate_host.py holds the CPU build of edge_math.h to the same bounds on the
same data and shows that mutations of the restatement leave them.

Graphs (tests/edge_restate.py: GRAPHS; slot 0 = self, the rest random points of the same cloud, repeats allowed): `base` =
clouds 300 / 257 / 64 at k = 20 (several row chunks with a short tail), `k1` (amax = amin = s1pt = var = 0), `tiny2` and `tiny1`
(E = 1: running_var falls back to the biased variance), `hub` = 3000 points of which 2800 list the same 19 targets (in-degree
above ECAPT = 2560, most points in-degree 0), `random` = 1024 / 777 (the unique sources of a tile exceed CAPT = 248).  The CSC
comes from dc_csc_build, the inference coefficients from dc_bn_eval_coeffs, the workspaces from dc_bn_workspace_bytes.

Layouts: y, dout, dy, out, h2, out2 are column blocks of SENT-filled buffers with one spare row; a layout is (C, row stride,
first column).  amax, amin, s1pt, dzs and the slot bytes are contiguous [n, C] and 16-byte aligned, as the header documents
and the product passes them (with a sentinel row behind).  Every call restates the entry point's own `v4` condition from the
pointers and strides it passes and asserts the width against the table.  For one C every layout returns the bits of the
contiguous one; two repeats of every call return equal bits; the sentinels stay intact.  Every check prints its worst
error / bound before anything is asserted."""
import functools

import pytest
import torch

from deltaconv_amd._lib import lib
from tests import edge_restate as ER
from tests.apply_cases import Checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0

LAYOUTS = {                                          # name -> (C, row stride, first column)
    "c64": (64, 64, 0), "c72": (72, 72, 0), "c8": (8, 8, 0), "c7": (7, 7, 0), "c23": (23, 23, 0), "c64_ld68": (64, 68, 0),
    "c64_ld65": (64, 65, 0), "c64_ld70_off1": (64, 70, 1), "c128": (128, 128, 0),
}
WIDTH = {"c64": 4, "c72": 4, "c8": 4, "c7": 1, "c23": 1, "c64_ld68": 4, "c64_ld65": 1, "c64_ld70_off1": 1, "c128": 4}
CONTIGUOUS = {64: "c64", 72: "c72", 8: "c8", 7: "c7", 23: "c23", 128: "c128"}
SLOPE = ER.SLOPES[0]


def _v4(c, lds, ptrs):
    """The `v4` condition of the entry points restated: C, every leading dimension and every base allow 16-byte accesses."""
    return c % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs)


class _Buf:
    """An operand: a [rows, C] column block of a SENT-filled [rows + 1, ld] buffer."""

    def __init__(self, layout, rows, content=None):
        c, ld, off = LAYOUTS[layout]
        self.ld, self.off, self.w = ld, off, c
        self.buf = torch.full((rows + 1, ld), SENT, device=DEV)
        self.view = self.buf[:rows, off:off + c]
        if content is None:
            self.view.fill_(float("nan"))
        else:
            assert tuple(content.shape) == (rows, c)
            self.view.copy_(content)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (4 * off) % 16 and self.view.stride(0) == ld

    @property
    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        b = self.buf
        ok = bool((b[:, :self.off] == SENT).all()) and bool((b[:, self.off + self.w:] == SENT).all()) and bool((b[-1] == SENT).all())
        assert ok, "sentinels around the output were overwritten"
        return self.view.cpu()


class _Flat:
    """A contiguous, 16-byte aligned [n, C] intermediate with a sentinel row behind it."""

    def __init__(self, n, c, dtype=torch.float32):
        self.sent = 255 if dtype == torch.uint8 else SENT
        self.buf = torch.full((n + 1, c), self.sent, dtype=dtype, device=DEV)
        self.view = self.buf[:n]
        self.view.fill_(254 if dtype == torch.uint8 else float("nan"))
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

    def result(self):
        assert bool((self.buf[-1] == self.sent).all()), "the row behind a contiguous intermediate was overwritten"
        return self.view.cpu()


def _ws(n, c):
    nbytes = int(lib.raw("dc_bn_workspace_bytes")(n, c))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=DEV), nbytes


@functools.lru_cache(maxsize=None)
def _device_graph(gname, graph=ER.graph):
    nbr, sizes = graph(gname)
    n, k = nbr.shape
    nbr32 = nbr.to(torch.int32).to(DEV)
    ptr = torch.tensor([sum(sizes[:q]) for q in range(len(sizes) + 1)], dtype=torch.int32, device=DEV)
    tptr = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    tedge = torch.full((n * k,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(n * (k + 1), dtype=torch.int32, device=DEV)
    lib.call("dc_csc_build", nbr32, ptr, len(sizes), n, k, tptr, tedge, ws, ws.numel() * 4)
    return nbr32, ptr, tptr, tedge


def _twice(ck, what, fn):
    """Run a call twice on fresh buffers: equal bits.  -> the first run's (cpu results, device handles)."""
    (r1, h1), (r2, _) = fn(), fn()
    bits = lambda t: t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)      # NaN-proof comparison
    ck.true(f"{what}: two runs give equal bits", all(torch.equal(bits(r1[name]), bits(r2[name])) for name in r1))
    return r1, h1


class Run:
    """Every entry point of one (graph, layout), checked against the restatement; `res` keeps the raw results by name for the
    bit comparisons between layouts, `dev` the device tensors the tiled backward starts from."""

    def __init__(self, gname, lname):
        self.g, self.l = gname, lname
        self.C = LAYOUTS[lname][0]
        self.cs = ER.case(gname, self.C)
        self.n, self.k = self.cs.n, self.cs.k
        self.nbr32, self.ptr, self.tptr, self.tedge = _device_graph(gname)
        self.ck = Checks(f"{gname} {lname}")
        self.v4 = WIDTH[lname] == 4
        self.gamma, self.beta = self.cs.gamma.to(DEV), self.cs.beta.to(DEV)
        self.res, self.dev = {}, {}

    def _width(self, what, lds, ptrs):
        got = _v4(self.C, lds, ptrs)
        assert got == self.v4, f"{what} in layout {self.l} runs V = {4 if got else 1}, the table says {WIDTH[self.l]}"

    # ---- forward ----
    def gather(self, stats):
        cs, n, k, C = self.cs, self.n, self.k, self.C

        def once():
            y = _Buf(self.l, n, cs.y)
            fl = {name: _Flat(n, C) for name in ("amax", "amin", "s1pt")}
            by = {name: _Flat(n, C, torch.uint8) for name in ("argmax", "argmin")}
            coef = torch.full((4, C), float("nan"), device=DEV)
            rm, rv = cs.rm.to(DEV), cs.rv.to(DEV)
            ws, nb = _ws(n, C)
            self._width("dc_edge_gather_stats", [y.ld], [y.ptr])
            if not stats:
                lib.call("dc_bn_eval_coeffs", self.gamma, self.beta, rm, rv, ER.EPS, C, coef[0], coef[1], coef[2], coef[3])
            lib.call("dc_edge_gather_stats", y.view, y.ld, self.nbr32, n, k, C, stats, self.gamma, self.beta, ER.EPS, ER.MOM,
                     rm if stats else None, rv if stats else None, fl["amax"].view, fl["amin"].view, by["argmax"].view, by["argmin"].view,
                     fl["s1pt"].view, coef[0], coef[1], coef[2], coef[3], ws, nb)
            r = {name: t.result() for name, t in {**fl, **by}.items()}
            c = coef.cpu()
            r.update(mean=c[0], invstd=c[1], scale=c[2], shift=c[3], rm_new=rm.cpu(), rv_new=rv.cpu())
            assert torch.equal(y.result(), cs.y)                              # the input and its sentinels are untouched
            return r, dict(y=y, coef=coef, **{name: t.view for name, t in {**fl, **by}.items()})

        self.ck.what = f"{self.g} {self.l} compute_stats {stats}"
        r, h = _twice(self.ck, "dc_edge_gather_stats", once)
        ER.check_gather(self.ck, cs, r)
        ER.check_coefficients(self.ck, cs, stats, r)
        if not stats:
            self.ck.exact("compute_stats 0 leaves the running pair alone", torch.stack([r["rm_new"], r["rv_new"]]), torch.stack([cs.rm, cs.rv]))
        for name, t in r.items():
            self.res[f"stats {stats} {name}"] = t
        self.dev[stats] = h
        return r, h

    def apply(self, stats, r, h):
        cs, n, C = self.cs, self.n, self.C
        for slope in ER.SLOPES:
            def once():
                out, arg = _Buf(self.l, n), _Flat(n, C, torch.uint8)
                self._width("dc_edge_max_apply", [out.ld], [out.ptr, h["amax"].data_ptr(), h["amin"].data_ptr()])
                lib.call("dc_edge_max_apply", h["amax"], h["amin"], h["argmax"], h["argmin"], n, C, h["coef"][2], h["coef"][3], slope,
                         out.view, out.ld, arg.view)
                return dict(out=out.result(), arg=arg.result()), dict(arg=arg.view)

            o, ha = _twice(self.ck, f"dc_edge_max_apply slope {slope:.1f}", once)
            ER.check_apply(self.ck, cs, r["scale"], r["shift"], slope, o["out"], o["arg"])
            self.res[f"stats {stats} out slope {slope:.1f}"] = o["out"]
            self.res[f"stats {stats} arg slope {slope:.1f}"] = o["arg"]
            if slope == SLOPE:
                h["arg"] = ha["arg"]
                h["xmax"] = o["out"]

    def residual(self, stats, r, h):
        """dc_edge_max_apply_residual with and without out2: against fp64, and the bits of dc_edge_max_apply + dc_bn_act2(residual)."""
        cs, n, C = self.cs, self.n, self.C
        sc2, sh2 = cs.sc2.to(DEV), cs.sh2.to(DEV)
        val, bound = ER.residual_out(cs, r["scale"], r["shift"], SLOPE, SLOPE)
        for second in (True, False):
            def once():
                h2, out, arg = _Buf(self.l, n, cs.h2), _Buf(self.l, n), _Flat(n, C, torch.uint8)
                out2 = _Buf(self.l, n) if second else None
                self._width("dc_edge_max_apply_residual", [out.ld, h2.ld] + ([out2.ld] if second else []),
                            [out.ptr, h2.ptr, h["amax"].data_ptr(), h["amin"].data_ptr()] + ([out2.ptr] if second else []))
                lib.call("dc_edge_max_apply_residual", h["amax"], h["amin"], h["argmax"], h["argmin"], n, C, h["coef"][2], h["coef"][3], SLOPE,
                         h2.view, h2.ld, sc2, sh2, SLOPE, out.view, out.ld, out2.view if second else None, out2.ld if second else 0, arg.view)
                res = dict(out=out.result(), arg=arg.result())
                if second:
                    res["out2"] = out2.result()
                return res, None

            tag = " with out2" if second else " without out2"
            o, _ = _twice(self.ck, "dc_edge_max_apply_residual" + tag, once)
            self.ck.hold("residual out" + tag, o["out"], val, bound)
            self.ck.exact("residual arg" + tag, o["arg"], cs.slots(r["scale"]))
            if second:
                self.ck.exact("residual form: second copy", o["out2"], o["out"])
            # the two-call form: dc_edge_max_apply into a buffer of this layout, then dc_bn_act2 with it as the residual
            xmax, h2, y1 = _Buf(self.l, n), _Buf(self.l, n, cs.h2), _Buf(self.l, n)
            y2 = _Buf(self.l, n) if second else None
            lib.call("dc_edge_max_apply", h["amax"], h["amin"], h["argmax"], h["argmin"], n, C, h["coef"][2], h["coef"][3], SLOPE, xmax.view,
                     xmax.ld, None)
            lib.call("dc_bn_act2", h2.view, n, C, h2.ld, sc2, sh2, SLOPE, xmax.view, xmax.ld, y1.view, y1.ld, y2.view if second else None,
                     y2.ld if second else 0)
            self.ck.exact("residual form = dc_edge_max_apply + dc_bn_act2(residual)" + tag, o["out"], y1.result())
            self.res[f"stats {stats} residual{tag}"] = o["out"]

    # ---- backward ----
    def _backward_once(self, h, slope, training, with_grads=True, plan=None):
        cs, n, k, C = self.cs, self.n, self.k, self.C
        dout, dy, dzs = _Buf(self.l, n, cs.dout), _Buf(self.l, n), _Flat(n, C)
        dg = torch.full((C,), float("nan"), device=DEV) if with_grads else None
        db = torch.full((C,), float("nan"), device=DEV) if with_grads else None
        ws, nb = _ws(n, C)
        y, coef = h["y"], h["coef"]
        if plan is None:
            self._width("dc_edge_max_backward", [dout.ld, y.ld, dy.ld], [dout.ptr, y.ptr, dy.ptr])
            lib.call("dc_edge_max_backward", dout.view, dout.ld, y.view, y.ld, self.tptr, self.tedge, n, k, C, h["amax"], h["amin"],
                     h["argmax"], h["argmin"], h["s1pt"], coef[2], coef[3], coef[0], coef[1], slope, training, dzs.view, dy.view, dy.ld,
                     dg, db, ws, nb)
        else:
            assert y.ld == C and y.off == 0
            lib.call("dc_edge_max_backward_tiled", dout.view, dout.ld, y.view, plan.blob, *plan.args, C, h["amax"], h["amin"], h["arg"],
                     h["s1pt"], coef[2], coef[3], coef[0], coef[1], slope, training, dzs.view, dy.view, dy.ld, dg, db, ws, nb)
        r = dict(dzs=dzs.result(), dy=dy.result())
        if with_grads:
            r.update(dgamma=dg.cpu(), dbeta=db.cpu())
        assert torch.equal(dout.result(), cs.dout)
        return r, None

    def backward(self, fwd):
        """fwd: {compute_stats: (results, handles)}.  Every (slope, training) of ER.BACKWARD_MODES; training = the mode of the forward."""
        for slope, training in ER.BACKWARD_MODES:
            r, h = fwd[training]
            what = f"slope {slope:.1f} training {training}"
            self.ck.what = f"{self.g} {self.l}"
            o, _ = _twice(self.ck, "dc_edge_max_backward " + what, lambda: self._backward_once(h, slope, training))
            auto = ER.check_backward(self.ck, self.cs, slope, training, r["scale"], r["shift"], o)
            for name, t in o.items():
                self.res[f"backward {what} {name}"] = t
            if slope == SLOPE and training:          # the product passes NULL for the gradient of a parameter that wants none
                o0, _ = self._backward_once(h, slope, training, with_grads=False)
                self.ck.exact("dy without dgamma / dbeta", o0["dy"], o["dy"])
                self.ck.exact("dzs without dgamma / dbeta", o0["dzs"], o["dzs"])
                self.dy_train, self.dy64 = o["dy"], auto["dy"]


@functools.lru_cache(maxsize=None)
def _run(gname, lname):
    """Every gather-path entry point once in this layout -> the Run (checks not yet asserted)."""
    run = Run(gname, lname)
    fwd = {}
    for stats in (1, 0):
        r, h = run.gather(stats)
        run.apply(stats, r, h)
        run.residual(stats, r, h)
        fwd[stats] = (r, h)
    run.backward(fwd)
    torch.cuda.synchronize()
    return run


def _print_offsets(run):
    """The offset table of DESIGN.md: per offset class the worst dy error relative to the column's max |dy64|."""
    ref = ER.reference(run.g, run.C, SLOPE, 1)
    print(f"[{run.g} {run.l}] offset (spreads) | kernel | fp32 materialised chain   (worst |dy - dy64| / max |dy64| per column)")
    for off, ek, e32 in ER.offset_table(run.cs, run.dy_train, run.dy64, ref["slot"], SLOPE):
        print(f"[{run.g} {run.l}] {off:16.0f} | {ek:.2e} | {e32:.2e}")


@pytest.mark.parametrize("lname", ["c64", "c72", "c8", "c7", "c23", "c64_ld68", "c64_ld65", "c64_ld70_off1"])
@pytest.mark.parametrize("gname", ["base", "k1", "tiny2", "tiny1", "hub", "random"])
def test_layouts(gname, lname):
    run = _run(gname, lname)
    c = LAYOUTS[lname][0]
    if lname != CONTIGUOUS[c]:                       # independence from stride and alignment: the bits of the contiguous layout
        base = _run(gname, CONTIGUOUS[c])
        run.ck.what = f"{gname} {lname}"
        assert base.res.keys() == run.res.keys()
        for name, t in run.res.items():
            run.ck.exact(f"= {CONTIGUOUS[c]}: {name}", t, base.res[name])
    elif lname == "c64" and gname in ("base", "hub"):
        _print_offsets(run)
    run.ck.done()


def _plan(gname):
    """The transposed tile plan of a graph (random positions: no spatial coherence), built as tests/test_gpu_tileT.py does."""
    from deltaconv_amd.geometry import Graph
    nbr32, ptr, _, _ = _device_graph(gname)
    _, sizes = ER.graph(gname)
    g = torch.Generator().manual_seed(5)
    gr = Graph(nbr32, ptr, len(sizes), max(sizes), pos=torch.randn(nbr32.shape[0], 3, generator=g).to(DEV))
    gr.tile_plan(force_P=64)
    return gr.tile_plan_T()


@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("gname", ["base", "hub", "random"])
def test_tiled_backward(gname, c):
    """dc_edge_max_backward_tiled on graphs whose tiles overflow the LDS capacity (hub: edge records beyond ECAPT = 2560 and
    targets without in-edges; random: unique sources beyond CAPT = 248): the fp64 bounds, and the bits of the gather form."""
    run = _run(gname, CONTIGUOUS[c])
    pt = _plan(gname)
    assert pt is not None
    hdr = pt.section("hdr").cpu()
    if gname == "random":
        assert int(hdr[:, 0].max()) > 248
    if gname == "hub":
        assert int(hdr[:, 2].max()) > 2560 and int((pt.section("tg")[:, :, 2] == 0).sum()) > 0
    ck = Checks(f"{gname} C {c} tiled")
    fwd = {stats: ({name[len(f"stats {stats} "):]: t for name, t in run.res.items() if name.startswith(f"stats {stats} ")}, run.dev[stats])
           for stats in (1, 0)}
    for slope, training in ER.BACKWARD_MODES[:2]:
        r, h = fwd[training]
        what = f"slope {slope:.1f} training {training}"
        o, _ = _twice(ck, "dc_edge_max_backward_tiled " + what, lambda: run._backward_once(h, slope, training, plan=pt))
        ER.check_backward(ck, run.cs, slope, training, r["scale"], r["shift"], o, tag=" tiled")
        for name, t in o.items():
            ck.exact(f"tiled = gather: {name} {what}", t, run.res[f"backward {what} {name}"])
    run.ck.done()
    ck.done()
