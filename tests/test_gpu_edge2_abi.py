"""The depth-2 edge MLP kernels (csrc/edge2.hip) through the C ABI, per element against the fp64 restatement of
tests/edge2_restate.py: dc_edge2_bn1_stats, dc_edge2_forward (stats_mode 0, 1, 2), dc_bn_act on ysel and dc_edge2_backward
(training1 x training2, with and without dgamma* / dbeta*), on every graph and input width of that module, with strided and
contiguous x, lddo = 64 and 68, and the XCD block remap on and off.

Bounds, data, the selection checks (a), (b), (c) and the handling of undecidable act1' branches: the docstring of
tests/edge2_restate.py.  tests/test_edge2_restate_host.py holds an fp32 emulation of the kernels to the same bounds on the same data
and shows that mutations of the restatement leave them.

Buffers (the idioms of tests/test_gpu_edge_abi.py): x, dout and out are column blocks of SENT-filled buffers with a spare row;
z, ysel, arg, dz and dW2 are contiguous with a sentinel row behind; outputs are pre-filled with NaN, the slot bytes with 254 / 255;
workspaces have the size dc_edge2_workspace_bytes states and a sentinel tail behind it.  The CSC comes from dc_csc_build, the
inference coefficients from dc_bn_eval_coeffs, the statistics of the z path from dc_edge_gather_stats (held by its own suite).
One chain = every call of one (case, config) once, on fresh buffers; two chains give equal bits, and so do the chains with strided
x, lddo = 68 and DC_OPT_XCD_REMAP = 0.  Every check prints its worst error / bound before anything is asserted."""
import functools

import pytest
import torch

from deltaconv_amd._lib import lib
from tests import edge2_restate as E2
from tests import test_gpu_edge_abi as EA
from tests.apply_cases import Checks
from tests.edge2_restate import CH
from tests.edge_restate import EPS, MOM
from tests.test_gpu_edge_abi import DEV, SENT, _Buf, _Flat, _twice

pytestmark = pytest.mark.gpu
GUARD = 7.25
ROWS = ("mean", "invstd", "scale", "shift")
for _ci in (1, 2, 3):                                # the layouts of x: contiguous and with one spare column
    EA.LAYOUTS[f"x{_ci}"] = (_ci, _ci, 0)
    EA.LAYOUTS[f"x{_ci}_ld"] = (_ci, _ci + 1, 0)


def _ws(n, k, backward):
    nb = int(lib.raw("dc_edge2_workspace_bytes")(n, k, backward))
    assert nb % 8 == 0
    return torch.full((nb // 8 + 64,), GUARD, dtype=torch.float64, device=DEV), nb


def _tail_ok(ws, nb):
    return bool((ws[nb // 8:] == GUARD).all())


def _filled(content, behind=1):
    """A contiguous, 16-byte aligned input with a sentinel row behind it -> the view of the content."""
    buf = torch.full((content.shape[0] + behind,) + tuple(content.shape[1:]), SENT, device=DEV)
    buf[:content.shape[0]].copy_(content)
    return buf[:content.shape[0]]


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


class Run:
    """The device side of one (graph, mode): the operands that do not change between chains."""

    def __init__(self, gname, mode):
        self.cs = cs = E2.case(gname, mode)
        self.n, self.k = cs.n, cs.k
        self.nbr32, self.ptr, self.tptr, self.tedge = EA._device_graph(gname, E2.graph)
        dev = lambda t: None if t is None else t.to(DEV)
        self.W1, self.W2 = dev(cs.W1), dev(cs.W2)
        self.g1, self.b1, self.g2, self.b2 = dev(cs.gamma1), dev(cs.beta1), dev(cs.gamma2), dev(cs.beta2)
        assert self.W2.data_ptr() % 16 == 0

    def chain(self, cfg, strided=False, lddo=64, grads=True):
        """Every entry point once for one config -> {name: cpu tensor}.  Asserts sentinels, tails and untouched inputs."""
        cs, n, k, ci = self.cs, self.n, self.k, self.cs.ci
        t1, t2, slope1, slope2 = cfg
        r = {}
        # operands
        if cs.via_z:
            z, x, xv, ldx, W1 = _Buf("c64", n, cs.z), None, None, 0, None
            zv = z.view
        else:
            x = _Buf(f"x{ci}_ld" if strided else f"x{ci}", n, cs.x)
            z, zv, xv, ldx, W1 = None, None, x.view, x.ld, self.W1
        rm1, rv1, rm2, rv2 = (t.to(DEV) for t in (cs.rm1, cs.rv1, cs.rm2, cs.rv2))
        coef1, s1pt = _nan(4, CH), None
        ws, nb = _ws(n, k, 0)
        # BatchNorm-1
        if t1 and not cs.via_z:
            sd = _Flat(n, ci)
            lib.call("dc_edge2_bn1_stats", xv, ldx, ci, W1, self.nbr32, n, k, self.g1, self.b1, EPS, MOM, rm1, rv1, sd.view, coef1[0],
                     coef1[1], coef1[2], coef1[3], ws, nb)
            assert _tail_ok(ws, nb), "dc_edge2_bn1_stats wrote behind its workspace"
            r["sd"], s1pt = sd.result(), sd.view
            r["rm1_new"], r["rv1_new"] = rm1.cpu(), rv1.cpu()
        elif t1:
            fl = {name: _Flat(n, CH) for name in ("amax", "amin", "s1pt")}
            by = {name: _Flat(n, CH, torch.uint8) for name in ("argmax", "argmin")}
            nbw = int(lib.raw("dc_bn_workspace_bytes")(n, CH))
            wsg = torch.empty((nbw + 7) // 8, dtype=torch.float64, device=DEV)
            lib.call("dc_edge_gather_stats", zv, CH, self.nbr32, n, k, CH, 1, self.g1, self.b1, EPS, MOM, rm1, rv1, fl["amax"].view,
                     fl["amin"].view, by["argmax"].view, by["argmin"].view, fl["s1pt"].view, coef1[0], coef1[1], coef1[2], coef1[3], wsg, nbw)
            r["sd"], s1pt = fl["s1pt"].result(), fl["s1pt"].view
        else:
            lib.call("dc_bn_eval_coeffs", self.g1, self.b1, rm1, rv1, EPS, CH, coef1[0], coef1[1], coef1[2], coef1[3])
        r["coef1"] = coef1.cpu()
        # forward, the three statistics modes
        fwd = {}
        for mode in (1, 0, 2):
            ysel, arg = _Flat(n, CH), _Flat(n, CH, torch.uint8)
            coef2 = _nan(4, CH)
            sums = torch.full((2 * (2 * CH + 1) + 64,), GUARD, dtype=torch.float64, device=DEV)
            rows = [coef2[0], coef2[1], coef2[2], coef2[3]] if mode == 1 else [None] * 4
            ws, nb = _ws(n, k, 0)
            lib.call("dc_edge2_forward", zv, xv, ldx, ci, W1, self.nbr32, n, k, self.W2, coef1[2], coef1[3], slope1, mode, self.g2, self.b2,
                     EPS, MOM, rm2 if mode == 1 else None, rv2 if mode == 1 else None, ysel.view, arg.view, *rows,
                     sums if mode == 2 else None, ws, nb)
            assert _tail_ok(ws, nb), "dc_edge2_forward wrote behind its workspace"
            fwd[mode] = (ysel, arg)
            r[f"ysel mode {mode}"], r[f"arg mode {mode}"] = ysel.result(), arg.result()
            if mode == 1:
                r["coef2 batch"], r["rm2_new"], r["rv2_new"] = coef2.cpu(), rm2.cpu(), rv2.cpu()
            else:
                assert bool(torch.isnan(coef2).all())
            if mode == 2:
                assert bool((sums[2 * (2 * CH + 1):] == GUARD).all()), "dc_edge2_forward wrote behind double [2][2 * 64 + 1]"
                r["sums"] = sums[:2 * (2 * CH + 1)].view(2, 2 * CH + 1).cpu()
                coefB = _nan(4, CH)
                lib.call("dc_bn_coeffs_from_sums", sums, 0, CH, self.g2, self.b2, EPS, MOM, None, None, coefB[0], coefB[1], coefB[2], coefB[3])
                r["coef2 from sums"] = coefB.cpu()
            else:
                assert bool((sums == GUARD).all())
        ysel, arg = fwd[1]
        if t2:
            coef2 = r["coef2 batch"].to(DEV)
        else:
            coef2 = _nan(4, CH)
            lib.call("dc_bn_eval_coeffs", self.g2, self.b2, cs.rm2.to(DEV), cs.rv2.to(DEV), EPS, CH, coef2[0], coef2[1], coef2[2], coef2[3])
        r["coef2"] = coef2.cpu()
        out = _Buf("c64_ld68", n)
        lib.call("dc_bn_act", ysel.view, n, CH, CH, coef2[2], coef2[3], slope2, None, 0, out.view, out.ld)
        r["out"] = out.result()
        # backward
        dout = _Buf("c64" if lddo == 64 else "c64_ld68", n, cs.dout)
        dz, dW2 = _Flat(n, CH), _Flat(CH, CH)
        pg = [_nan(CH) if grads else None for _ in range(4)]
        ws, nb = _ws(n, k, 1)
        lib.call("dc_edge2_backward", dout.view, dout.ld, zv, xv, ldx, ci, W1, self.nbr32, self.tptr, self.tedge, n, k, self.W2, coef1, coef2,
                 self.g2, slope1, slope2, t1, t2, ysel.view, arg.view, s1pt, dz.view, CH, dW2.view, *pg, ws, nb)
        assert _tail_ok(ws, nb), "dc_edge2_backward wrote behind its workspace"
        r["dz"], r["dW2"] = dz.result(), dW2.result()
        for name, t in zip(("dgamma1", "dbeta1", "dgamma2", "dbeta2"), pg):
            if t is not None:
                r[name] = t.cpu()
        # inputs and the sentinels around them are untouched
        assert torch.equal(dout.result(), cs.dout) and torch.equal(ysel.result(), r["ysel mode 1"]) and torch.equal(arg.result(), r["arg mode 1"])
        assert torch.equal(z.result(), cs.z) if cs.via_z else torch.equal(x.result(), cs.x)
        assert torch.equal(coef1.cpu(), r["coef1"]) and torch.equal(coef2.cpu(), r["coef2"])
        return r


@functools.lru_cache(maxsize=None)
def _run(gname, mode):
    return Run(gname, mode)


def _rows(t):
    return dict(zip(ROWS, t))


def _same(ck, what, a, b, names=None):
    bits = lambda t: t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)
    for name in (names or a.keys()):
        ok = torch.equal(bits(a[name]), bits(b[name]))
        if not ok:
            print(f"[{ck.what}] {what}: {name} DIFFERENT")
        ck.true(f"{what}: {name}", ok)


def _check_chain(ck, cs, cfg, r):
    """One chain's results against the restatement."""
    t1, t2, slope1, slope2 = cfg
    k, E = cs.k, cs.E
    c1, c2 = r["coef1"], r["coef2"]
    if t1 and not cs.via_z:
        E2.check_bn1(ck, cs, dict(_rows(c1), sd=r["sd"], rm_new=r["rm1_new"], rv_new=r["rv1_new"]))
    for mode in (0, 2):
        ck.exact(f"ysel of stats_mode {mode} = stats_mode 1", r[f"ysel mode {mode}"], r["ysel mode 1"])
        ck.exact(f"arg of stats_mode {mode} = stats_mode 1", r[f"arg mode {mode}"], r["arg mode 1"])
    ysel, arg = r["ysel mode 1"], r["arg mode 1"]
    f = E2.check_forward(ck, cs, c1[2], c1[3], slope1, ysel, arg)
    sums = r["sums"]
    E2.check_bn2(ck, cs, f, dict(_rows(r["coef2 batch"]), rm_new=r["rm2_new"], rv_new=r["rv2_new"], sum0=sums[0, :CH], sum1=sums[0, CH:2 * CH]))
    ck.exact("the two stats_mode 2 records", sums[1], sums[0])
    ck.true("the records' row count", float(sums[0, 2 * CH]) == E)
    ref = E2.sums_coef_ref(sums[0], cs.gamma2, cs.beta2)
    for tag, rows in (("dc_bn_coeffs_from_sums", r["coef2 from sums"]), ("stats_mode 1", r["coef2 batch"])):
        E2.check_named(ck, f"{tag} against the device's own sums:", _rows(rows), ref, ROWS)
    E2.check_out(ck, ysel, c2[2], c2[3], slope2, r["out"])
    E2.check_backward(ck, cs, f, c1, c2, slope2, t1, t2, ysel, arg, r.get("sd") if t1 else None, r)


@pytest.mark.parametrize("mode", list(E2.MODES))
@pytest.mark.parametrize("gname", E2.ALL_GRAPHS)
def test_chain(gname, mode):
    run = _run(gname, mode)
    cs = run.cs
    ck = Checks(f"{gname} {mode}")
    opt = lib.raw("dc_set_option")
    for cfg in E2.CONFIGS:
        ck.what = f"{gname} {mode} training {cfg[0]}{cfg[1]} slopes {cfg[2]:.1f} {cfg[3]:.1f}"
        r, _ = _twice(ck, "every call of the chain", lambda: (run.chain(cfg), None))
        _check_chain(ck, cs, cfg, r)
        _same(ck, "lddo 68 = lddo 64", run.chain(cfg, lddo=68), r)
        if not cs.via_z:
            _same(ck, "strided x = contiguous x", run.chain(cfg, strided=True), r)
        opt(0, 0)
        try:
            _same(ck, "DC_OPT_XCD_REMAP 0 = 1", run.chain(cfg), r)
        finally:
            opt(0, 1)
        r0 = run.chain(cfg, grads=False)
        _same(ck, "dgamma* / dbeta* NULL", r0, r, names=r0.keys())
    torch.cuda.synchronize()
    ck.done()


@pytest.mark.parametrize("gname", E2.ALL_GRAPHS)
def test_direct_and_z_path_agree(gname):
    """The same ci = 3 case through x and through z, inference coefficients (the same scale1 / shift1 bits for both)."""
    cfg = E2.CONFIGS[3]
    rx, rz = _run(gname, "x3").chain(cfg), _run(gname, "z3").chain(cfg)
    assert torch.equal(rx["coef1"], rz["coef1"])
    ck = Checks(f"{gname} x3 / z3")
    E2.check_paths(ck, E2.case(gname, "x3"), E2.case(gname, "z3"), rx["coef1"][2], rx["coef1"][3], cfg[2], rx["ysel mode 1"], rz["ysel mode 1"])
    ck.done()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _rc(name, *args):
    """The entry point's return code (lib.call raises on a refusal)."""
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return int(lib.raw(name)(*conv, torch.cuda.current_stream().cuda_stream))


def test_refusals():
    """Each returns an error code and writes nothing."""
    run = _run("w65", "x3")
    cs, n, k = run.cs, run.n, run.k
    x = _filled(cs.x)
    z = _filled((cs.x @ cs.W1.t()).contiguous())
    coef1, coef2 = torch.ones(4, CH, device=DEV), torch.ones(4, CH, device=DEV)
    ysel, arg, dz, dW2 = _Flat(n + 1, CH), _Flat(n + 1, CH, torch.uint8), _Flat(n + 1, CH + 4), _Flat(CH, CH)
    rows2 = _nan(4, CH)
    ysel_in, arg_in = torch.zeros(n + 1, CH, device=DEV), torch.zeros(n + 1, CH, dtype=torch.uint8, device=DEV)
    dout, sd = _filled(cs.dout), torch.zeros(n, 3, device=DEV)
    W2off = torch.zeros(CH * CH + 4, device=DEV)
    wf, nbf = _ws(n, k, 0)
    wb, nbb = _ws(n, k, 1)

    def fwd(zz=None, xx=x, ci=3, kk=k, W2=run.W2, ys=ysel.view, ar=arg.view, rows=None, mode=1, nb=nbf):
        rows = [rows2[0], rows2[1], rows2[2], rows2[3]] if rows is None else rows
        return _rc("dc_edge2_forward", zz, xx, 3 if xx is not None else 0, ci, run.W1, run.nbr32, n, kk, W2, coef1[2], coef1[3], 0.2, mode,
                   run.g2, run.b2, EPS, MOM, None, None, ys, ar, *rows, None, wf, nb)

    def bwd(zz=None, kk=k, W2=run.W2, ys=ysel_in, ar=arg_in, s1=sd, lddz=CH, t1=1, nb=nbb, dzv=dz.view):
        return _rc("dc_edge2_backward", dout, CH, zz, x, 3, 3, run.W1, run.nbr32, run.tptr, run.tedge, n, kk, W2, coef1, coef2, run.g2, 0.2, 0.2,
                   t1, 1, ys, ar, s1, dzv, lddz, dW2.view, None, None, None, None, wb, nb)

    assert fwd() == 0 and bwd() == 0                 # the helpers' own arguments are accepted ...
    torch.cuda.synchronize()
    for t in (ysel, arg, dz, dW2):                   # ... then every output is reset and must stay so
        t.view.fill_(254 if t.view.dtype == torch.uint8 else float("nan"))
    rows2.fill_(float("nan"))
    refused = {
        "forward k = 256": fwd(kk=256), "backward k = 256": bwd(kk=256),
        "forward z NULL with ci = 4": fwd(ci=4),
        "backward lddz = 68": bwd(lddz=CH + 4),
        "forward misaligned W2": fwd(W2=W2off[1:]), "backward misaligned W2": bwd(W2=W2off[1:]),
        "forward misaligned ysel": fwd(ys=ysel.buf.view(-1)[1:]), "backward misaligned ysel": bwd(ys=ysel_in.view(-1)[1:]),
        "forward misaligned arg": fwd(ar=arg.buf.view(-1)[1:]), "backward misaligned arg": bwd(ar=arg_in.view(-1)[1:]),
        "forward workspace one byte short": fwd(nb=nbf - 1), "backward workspace one byte short": bwd(nb=nbb - 1),
        "backward training1 without s1pt": bwd(s1=None),
        "forward stats_mode 1 without the coefficient rows": fwd(rows=[None] * 4),
    }
    torch.cuda.synchronize()
    print(refused)
    assert all(rc != 0 for rc in refused.values()), refused
    for t in (ysel, arg, dz, dW2):
        v = t.buf
        assert bool((v[:-1] == 254).all()) if v.dtype == torch.uint8 else bool(torch.isnan(v[:-1]).all()), "a refused call wrote to an output"
    assert bool(torch.isnan(rows2).all()) and _tail_ok(wf, nbf) and _tail_ok(wb, nbb)


# ---- the autograd path returns the bits of the ABI calls it is made of --------------------------------------------------------------
@pytest.mark.parametrize("gname", ["hub600", "k255"])
def test_fused_edge_mlp2_returns_the_bits_of_the_abi_chain(gname):
    import deltaconv_amd as dc
    from deltaconv_amd.geometry import Graph
    from deltaconv_amd.nn import fused
    run = _run(gname, "x3")
    cs, n = run.cs, run.n
    cfg = E2.CONFIGS[0]
    r = run.chain(cfg)
    gr = Graph(run.nbr32, run.ptr, len(cs.sizes), max(cs.sizes), pos=cs.x.to(DEV))
    mlp = dc.nn.MLP([3, CH, CH]).to(DEV)
    with torch.no_grad():
        for blk, W, g, b, rm, rv in ((mlp[0], cs.W1, cs.gamma1, cs.beta1, cs.rm1, cs.rv1), (mlp[1], cs.W2, cs.gamma2, cs.beta2, cs.rm2, cs.rv2)):
            blk[0].weight.copy_(W); blk[1].bn.weight.copy_(g); blk[1].bn.bias.copy_(b)
            blk[1].bn.running_mean.copy_(rm); blk[1].bn.running_var.copy_(rv)
    mlp.train(True)
    xd = cs.x.to(DEV).requires_grad_(True)
    out, slots = fused.edge_mlp2(xd, gr, mlp[0][0], mlp[0][1].bn, cfg[2], mlp[1][0], mlp[1][1].bn, cfg[3])
    out.backward(cs.dout.to(DEV))
    ck = Checks(f"fused.edge_mlp2 {gname}")
    got = dict(out=out.detach().cpu(), arg=slots.cpu(), dW2=mlp[1][0].weight.grad.cpu(), dgamma1=mlp[0][1].bn.weight.grad.cpu(),
               dbeta1=mlp[0][1].bn.bias.grad.cpu(), dgamma2=mlp[1][1].bn.weight.grad.cpu(), dbeta2=mlp[1][1].bn.bias.grad.cpu(),
               rm1_new=mlp[0][1].bn.running_mean.cpu(), rv1_new=mlp[0][1].bn.running_var.cpu(), rm2_new=mlp[1][1].bn.running_mean.cpu(),
               rv2_new=mlp[1][1].bn.running_var.cpu())
    ref = dict(r, arg=r["arg mode 1"])
    _same(ck, "autograd path = ABI chain", got, ref)
    ck.done()
