"""The single-rank entry points of csrc/nn.hip (nn_math.h, the finalisers of colreduce.h) through the C ABI, per element against
the fp64 restatement of tests/nn_restate.py, in every layout that changes the vector width or the tiling: dc_bn_stats,
dc_vn_stats, dc_bn_eval_coeffs, dc_bn_act, dc_bn_act2, dc_bn_act_backward_reduce (alone, deferred and paired inside
dc_finalisers_begin .. dc_finalisers_end), dc_vn_apply, dc_vn_backward (for the layout of d(P, Q)), dc_bn_act_pool, dc_bn_act_pool_backward (against fp64 and, bit for bit,
against dc_bn_act_backward on the gradient materialised in fp32), dc_cloud_bias_add, dc_cloud_colsum.

Bounds, data, the kink margin and the undecided arg-max pairs: the docstring of tests/nn_restate.py (u = 2^-24, every rounding
counted from the code).  tests/test_nn_restate_host.py holds the CPU build of the same headers to the same bounds on the same
data and shows that mutations of the restatement leave them.

Layouts: operands and results are column blocks of SENT-filled buffers with one spare row; a layout is (C, row stride, first
column); for the vector block the table describes co and the input stride is doubled for combine 1 and 2.  Coefficient vectors,
arg-max tables and workspaces are contiguous (arg-max with a sentinel row behind); workspaces are filled with NaN before every
call.  Every call restates the entry point's own `v4` condition from the pointers and strides it passes and asserts the width
against the table.  For one C every layout returns the bits of the contiguous one; every call runs twice on fresh buffers and
returns equal bits; the sentinels stay intact.  Every check prints its worst error / bound before anything is asserted."""
import functools

import pytest
import torch

from deltaconv_amd._lib import lib
from tests import nn_restate as NR
from tests.apply_cases import Checks

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0
NAN = float("nan")

LAYOUTS = {                                          # name -> (C, row stride, first column)
    "c64": (64, 64, 0), "c72": (72, 72, 0), "c8": (8, 8, 0), "c7": (7, 7, 0), "c23": (23, 23, 0), "c64_ld68": (64, 68, 0),
    "c64_ld65": (64, 65, 0), "c64_ld70_off1": (64, 70, 1), "c128": (128, 128, 0), "c256": (256, 256, 0), "c1024": (1024, 1024, 0),
}
WIDTH = {"c64": 4, "c72": 4, "c8": 4, "c7": 1, "c23": 1, "c64_ld68": 4, "c64_ld65": 1, "c64_ld70_off1": 1, "c128": 4, "c256": 4, "c1024": 4}
CONTIGUOUS = {64: "c64", 72: "c72", 8: "c8", 7: "c7", 23: "c23", 128: "c128", 256: "c256", 1024: "c1024"}


def _v4(c, lds, ptrs):
    """The `v4` condition of the entry points restated: C, every leading dimension and every base allow 16-byte accesses."""
    return c % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs)


class _Buf:
    """An operand: a [rows, w] column block, `off` columns in, of a SENT-filled [rows + 1, ld] buffer."""

    def __init__(self, rows, w, ld, off, content=None):
        self.ld, self.off, self.w = ld, off, w
        self.buf = torch.full((rows + 1, ld), SENT, device=DEV)
        self.view = self.buf[:rows, off:off + w]
        if content is None:
            self.view.fill_(NAN)
        else:
            assert tuple(content.shape) == (rows, w), (tuple(content.shape), rows, w)
            self.content = content
            self.view.copy_(content)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (4 * off) % 16 and (rows <= 1 or self.view.stride(0) == ld)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        b = self.buf
        ok = bool((b[:, :self.off] == SENT).all()) and bool((b[:, self.off + self.w:] == SENT).all()) and bool((b[-1] == SENT).all())
        assert ok, "sentinels around an operand were overwritten"
        return self.view.cpu()

    def untouched(self):
        r = self.result()
        assert torch.equal(r.view(torch.int32), self.content.view(torch.int32)), "an input was modified"


class _Args:
    """A contiguous int32 [B, C] table with a sentinel row behind it."""

    def __init__(self, B, C, content=None):
        self.buf = torch.full((B + 1, C), -7, dtype=torch.int32, device=DEV)
        self.view = self.buf[:B]
        if content is not None:
            self.view.copy_(content)

    def result(self):
        assert bool((self.buf[-1] == -7).all()), "the row behind the arg-max table was overwritten"
        return self.view.cpu()


def _ws(rows, c):
    nbytes = int(lib.raw("dc_bn_workspace_bytes")(rows, c))
    return torch.full(((nbytes + 7) // 8,), NAN, dtype=torch.float64, device=DEV), nbytes


def _vec(c, content=None):
    """A per-column vector with a sentinel behind it -> (buffer, view)."""
    buf = torch.full((c + 1,), SENT, device=DEV)
    if content is None:
        buf[:c] = NAN
    else:
        buf[:c] = content.to(DEV)
    return buf


def _vres(buf):
    assert float(buf[-1]) == SENT, "the element behind a per-column output was overwritten"
    return buf[:-1].cpu()


def _d(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t if t.dtype != torch.float32 else t.contiguous().view(torch.int32)         # NaN-proof comparison


class Dev:
    """The backend of the drivers of tests/nn_restate.py over the C ABI in one layout."""

    def __init__(self, lname, ck):
        self.l, self.ck = lname, ck
        self.C, self.ld, self.off = LAYOUTS[lname]
        self.v4 = WIDTH[lname] == 4

    def _width(self, what, lds, ptrs, c=None):
        got = _v4(self.C if c is None else c, lds, ptrs)
        assert got == self.v4, f"{what} in layout {self.l} runs V = {4 if got else 1}, the table says {WIDTH[self.l]}"

    def _twice(self, what, fn):
        r1, r2 = fn(), fn()
        same = all((a is None and b is None) or torch.equal(_bits(a), _bits(b)) for a, b in zip(r1, r2))
        self.ck.true(f"{what}: two runs give equal bits", same)
        return r1

    def _put(self, t, w=None, ld=None):
        return _Buf(t.shape[0], self.C if w is None else w, self.ld if ld is None else ld, self.off, t)

    def _new(self, rows, w=None, ld=None):
        return _Buf(rows, self.C if w is None else w, self.ld if ld is None else ld, self.off)

    # ---- statistics ----
    def _stats(self, name, call, c, rm0, rv0):
        def once():
            o = [_vec(c) for _ in range(4)]
            rm, rv = (_vec(c, rm0), _vec(c, rv0)) if rm0 is not None else (None, None)
            call(o, rm, rv)
            return [_vres(t) for t in o] + [None if rm is None else _vres(rm), None if rv is None else _vres(rv)]

        r = self._twice(name, once)
        return dict(zip(("mean", "invstd", "scale", "shift", "rm", "rv"), r))

    def bn_stats(self, x, gamma, beta, mom, rm0, rv0):
        R, C = x.shape

        def call(o, rm, rv):
            h = self._put(x)
            ws, nb = _ws(R, C)
            self._width("dc_bn_stats", [h.ld], [h.ptr])
            lib.call("dc_bn_stats", h.view, R, C, h.ld, _d(gamma), _d(beta), NR.EPS, mom, None if rm is None else rm[:C],
                     None if rv is None else rv[:C], o[0][:C], o[1][:C], o[2][:C], o[3][:C], ws, nb)
            h.untouched()

        return self._stats("dc_bn_stats", call, C, rm0, rv0)

    def vn_stats(self, t, co, combine, gamma, beta, mom, rm0, rv0):
        n, k = t.shape[0] // 2, 2 if combine else 1

        def call(o, rm, rv):
            a = self._put(t, k * co, k * self.ld)
            ws, nb = _ws(n, co)
            self._width("dc_vn_stats", [a.ld], [a.ptr])
            lib.call("dc_vn_stats", a.view, n, co, a.ld, combine, _d(gamma), _d(beta), NR.EPS, mom, None if rm is None else rm[:co],
                     None if rv is None else rv[:co], o[0][:co], o[1][:co], o[2][:co], o[3][:co], ws, nb)
            a.untouched()

        return self._stats("dc_vn_stats", call, co, rm0, rv0)

    def eval_coeffs(self, gamma, beta, rm, rv):
        c = rm.numel()

        def once():
            o = [_vec(c) for _ in range(4)]
            lib.call("dc_bn_eval_coeffs", _d(gamma), _d(beta), rm.to(DEV), rv.to(DEV), NR.EPS, c, o[0][:c], o[1][:c], o[2][:c], o[3][:c])
            return [_vres(t) for t in o]

        return dict(zip(("mean", "invstd", "scale", "shift"), self._twice("dc_bn_eval_coeffs", once)))

    # ---- the scalar block ----
    def bn_act(self, x, scale, shift, slope, res, second):
        R, C = x.shape

        def once():
            h, y = self._put(x), self._new(R)
            r = self._put(res) if res is not None else None
            y2 = self._new(R) if second else None
            self._width("dc_bn_act", [h.ld, y.ld] + ([r.ld] if r else []) + ([y2.ld] if y2 else []),
                        [h.ptr, y.ptr] + ([r.ptr] if r else []) + ([y2.ptr] if y2 else []))
            if second:
                lib.call("dc_bn_act2", h.view, R, C, h.ld, scale.to(DEV), shift.to(DEV), slope, r.view if r else None, r.ld if r else 0,
                         y.view, y.ld, y2.view, y2.ld)
            else:
                lib.call("dc_bn_act", h.view, R, C, h.ld, scale.to(DEV), shift.to(DEV), slope, r.view if r else None, r.ld if r else 0,
                         y.view, y.ld)
            h.untouched()
            return [y.result(), y2.result() if second else None]

        return self._twice("dc_bn_act", once)

    def _co(self, co):
        return [co[k].to(DEV) for k in ("scale", "shift", "mean", "invstd")]

    def bwd_reduce(self, dy, x, co, gamma, slope, training, grads):
        R, C = x.shape

        def once():
            g, h = self._put(dy), self._put(x)
            dg, db, coefs = (_vec(C) if grads else None), (_vec(C) if grads else None), _vec(5 * C)
            ws, nb = _ws(R, C)
            self._width("dc_bn_act_backward_reduce", [g.ld, h.ld], [g.ptr, h.ptr])
            lib.call("dc_bn_act_backward_reduce", g.view, g.ld, h.view, h.ld, R, C, *self._co(co), _d(gamma), slope, training,
                     dg[:C] if grads else None, db[:C] if grads else None, coefs[:5 * C], ws, nb)
            return [_vres(dg) if grads else None, _vres(db) if grads else None, _vres(coefs).view(5, C)]

        return dict(zip(("dgamma", "dbeta", "coefs"), self._twice("dc_bn_act_backward_reduce", once)))

    def bwd(self, dy, x, co, gamma, slope, training):
        R, C = x.shape
        g, h, dh = self._put(dy), self._put(x), self._new(R)
        dg, db = _vec(C), _vec(C)
        ws, nb = _ws(R, C)
        self._width("dc_bn_act_backward", [g.ld, h.ld, dh.ld], [g.ptr, h.ptr, dh.ptr])
        lib.call("dc_bn_act_backward", g.view, g.ld, h.view, h.ld, R, C, *self._co(co), _d(gamma), slope, training, dh.view, dh.ld,
                 dg[:C], db[:C], ws, nb)
        return dict(dh=dh.result(), dgamma=_vres(dg), dbeta=_vres(db))

    # ---- the vector block ----
    def vn_apply(self, t, co, combine, scale, shift):
        n, k = t.shape[0] // 2, 2 if combine else 1

        def once():
            a, out = self._put(t, k * co, k * self.ld), self._new(2 * n)
            self._width("dc_vn_apply", [a.ld, out.ld], [a.ptr, out.ptr])
            lib.call("dc_vn_apply", a.view, n, co, a.ld, combine, scale.to(DEV), shift.to(DEV), out.view, out.ld)
            a.untouched()
            return [out.result()]

        return self._twice("dc_vn_apply", once)[0]

    def vn_bwd(self, dout, t, co, combine, c32, gamma, training):
        n, k, ko = t.shape[0] // 2, 2 if combine in (1, 2) else 1, 2 if combine else 1

        def once():
            a, d, din = self._put(t, k * co, k * self.ld), self._put(dout), self._new(2 * n, ko * co, ko * self.ld)
            dg, db = _vec(co), _vec(co)
            ws, nb = _ws(n, co)
            self._width("dc_vn_backward", [a.ld, d.ld, din.ld], [a.ptr, d.ptr, din.ptr])
            lib.call("dc_vn_backward", d.view, d.ld, a.view, a.ld, combine, n, co, *self._co(c32), gamma.to(DEV), training, din.view,
                     din.ld, dg[:co], db[:co], ws, nb)
            a.untouched()
            return [din.result(), _vres(dg), _vres(db)]

        return dict(zip(("din", "dgamma", "dbeta"), self._twice("dc_vn_backward", once)))

    # ---- the embedding head ----
    def pool(self, x, B, N, scale, shift, slope, wm):
        C = x.shape[1]
        w = (1 + wm) * C

        def once():
            h, pooled, arg = self._put(x), _Buf(B, w, w + 5, 2), _Args(B, C)
            self._width("dc_bn_act_pool", [h.ld], [h.ptr])
            lib.call("dc_bn_act_pool", h.view, h.ld, B, N, C, scale.to(DEV), shift.to(DEV), slope, wm, pooled.view, pooled.ld, arg.view)
            h.untouched()
            return [pooled.result(), arg.result()]

        return self._twice("dc_bn_act_pool", once)

    def pool_bwd(self, dp, arg, x, B, N, co, gamma, slope, wm, training):
        C = x.shape[1]
        w = (1 + wm) * C

        def once():
            h, dh, d, a = self._put(x), self._new(B * N), _Buf(B, w, w + 5, 2, dp), _Args(B, C, arg)
            dg, db = _vec(C), _vec(C)
            ws, nb = _ws(B * N, C)
            self._width("dc_bn_act_pool_backward", [h.ld, dh.ld], [h.ptr, dh.ptr])
            lib.call("dc_bn_act_pool_backward", d.view, d.ld, a.view, h.view, h.ld, B, N, C, *self._co(co), _d(gamma), slope, wm, training,
                     dh.view, dh.ld, dg[:C], db[:C], ws, nb)
            h.untouched()
            return [dh.result(), _vres(dg), _vres(db)]

        return dict(zip(("dh", "dgamma", "dbeta"), self._twice("dc_bn_act_pool_backward", once)))

    # ---- the per-cloud half of the segmentation head ----
    def cloud_bias_add(self, h, g, mx, alias):
        n, C = h.shape

        def once():
            a, b = self._put(h), self._put(g)
            y = a if alias else self._new(n)
            self._width("dc_cloud_bias_add", [a.ld, b.ld, y.ld], [a.ptr, b.ptr, y.ptr])
            lib.call("dc_cloud_bias_add", a.view, a.ld, b.view, b.ld, n, C, mx, y.view, y.ld)
            b.untouched()
            return [y.result()]

        return self._twice("dc_cloud_bias_add", once)[0]

    def cloud_colsum(self, x, B, mx):
        C = x.shape[1]

        def once():
            a, out = self._put(x), self._new(B)
            nb = int(lib.raw("dc_cloud_colsum_workspace_bytes")(B, mx, C))
            ws = torch.full((nb // 8 + 1,), NAN, dtype=torch.float64, device=DEV)
            self._width("dc_cloud_colsum", [a.ld], [a.ptr])
            lib.call("dc_cloud_colsum", a.view, a.ld, B, mx, C, out.view, out.ld, ws, nb)
            a.untouched()
            return [out.result()]

        return self._twice("dc_cloud_colsum", once)[0]


def _same_as_contiguous(ck, lname, res, base):
    assert base.keys() == res.keys()
    for name, t in res.items():
        ck.exact(f"= {CONTIGUOUS[LAYOUTS[lname][0]]}: {name}", t, base[name])


@functools.lru_cache(maxsize=None)
def _rows(lname, R):
    ck = Checks(f"rows {R} {lname}")
    res = NR.run_rows(Dev(lname, ck), NR.row_case(R, LAYOUTS[lname][0]), ck)
    torch.cuda.synchronize()
    return ck, res


def test_tilings():
    NR.assert_tilings()


@pytest.mark.parametrize("lname,R", [(l, R) for l in LAYOUTS for R in NR.row_counts(LAYOUTS[l][0])])
def test_rows(lname, R):
    """dc_bn_stats, dc_bn_eval_coeffs, dc_bn_act / dc_bn_act2, dc_bn_act_backward_reduce (1040 rows: 65 chunks need C <= 64;
    4410: C = 256 alone; C = 1024: the small counts)."""
    c = LAYOUTS[lname][0]
    ck, res = _rows(lname, R)
    if lname != CONTIGUOUS[c]:
        _same_as_contiguous(ck, lname, res, _rows(CONTIGUOUS[c], R)[1])
    ck.done()


def test_bn_stats_at_the_row_cap():
    """24 000 x 1024: the one shape whose chunks reach the cap of 512 rows (47 chunks)."""
    assert NR.rows_per_chunk(24000, 1024) == 512
    ck = Checks("rows 24000 c1024")
    NR.run_rows(Dev("c1024", ck), NR.row_case(24000, 1024, stats_only=True), ck, full=False)
    ck.done()


@functools.lru_cache(maxsize=None)
def _vectors(lname, combine):
    co = LAYOUTS[lname][0]
    ck = Checks(f"vectors {lname} combine {combine}")
    res = {}
    for n in NR.row_counts(co):
        ck.what = f"vectors {n} {lname} combine {combine}"
        res.update({f"{n} {k}": v for k, v in NR.run_vec(Dev(lname, ck), NR.vec_case(n, co, combine), ck).items()})
    torch.cuda.synchronize()
    return ck, res


@pytest.mark.parametrize("combine", [0, 1, 2])
@pytest.mark.parametrize("lname", list(LAYOUTS))
def test_vectors(lname, combine):
    """dc_vn_stats, dc_vn_apply and dc_vn_backward; the table describes co, the input stride is doubled for combine 1 and 2."""
    co = LAYOUTS[lname][0]
    ck, res = _vectors(lname, combine)
    if lname != CONTIGUOUS[co]:
        _same_as_contiguous(ck, lname, res, _vectors(CONTIGUOUS[co], combine)[1])
    ck.done()


@functools.lru_cache(maxsize=None)
def _pool(lname, B, N):
    ck = Checks(f"pool {B} x {N} {lname}")
    res, und = NR.run_pool(Dev(lname, ck), NR.pool_case(B, N, LAYOUTS[lname][0]), ck)
    torch.cuda.synchronize()
    return ck, res, und


@pytest.mark.parametrize("B,N", NR.POOLS)
@pytest.mark.parametrize("lname", list(LAYOUTS))
def test_pool(lname, B, N):
    """dc_bn_act_pool and dc_bn_act_pool_backward; N = 5: a thread changes cloud at every step (PoolDy's cache)."""
    c = LAYOUTS[lname][0]
    ck, res, und = _pool(lname, B, N)
    if lname != CONTIGUOUS[c]:
        _same_as_contiguous(ck, lname, res, _pool(CONTIGUOUS[c], B, N)[1])
    assert und <= 1e-3
    ck.done()


@functools.lru_cache(maxsize=None)
def _cloud(lname, B, mx):
    ck = Checks(f"cloud {B} x {mx} {lname}")
    res = NR.run_cloud(Dev(lname, ck), NR.cloud_case(B, mx, LAYOUTS[lname][0]), ck)
    torch.cuda.synchronize()
    return ck, res


@pytest.mark.parametrize("B,mx", NR.CLOUDS)
@pytest.mark.parametrize("lname", [l for l in LAYOUTS if l != "c1024"])
def test_cloud_sums(lname, B, mx):
    """dc_cloud_bias_add (also in place) and dc_cloud_colsum; (800, 16): more clouds than target workgroups, one chunk each."""
    c = LAYOUTS[lname][0]
    ck, res = _cloud(lname, B, mx)
    if lname != CONTIGUOUS[c]:
        _same_as_contiguous(ck, lname, res, _cloud(CONTIGUOUS[c], B, mx)[1])
    ck.done()


# ---- deferred and paired reductions -------------------------------------------------------------------------------------------------
class _Reduce:
    """One dc_bn_act_backward_reduce call with its operands, outputs and a NaN-filled workspace."""

    def __init__(self, R, lname):
        self.R, self.l = R, lname
        self.C, self.ld, self.off = LAYOUTS[lname]
        self.cs = NR.row_case(R, self.C)
        self.co = {k: self.cs.tr[k].float() for k in ("scale", "shift", "mean", "invstd")}         # one rounding each: km = ki = 1

    def launch(self):
        C, cs = self.C, self.cs
        self.g, self.h = _Buf(self.R, C, self.ld, self.off, cs.dy), _Buf(self.R, C, self.ld, self.off, cs.x)
        self.dg, self.db, self.coefs = _vec(C), _vec(C), _vec(5 * C)
        self.ws, nb = _ws(self.R, C)
        self.keep = [self.co[k].to(DEV) for k in ("scale", "shift", "mean", "invstd")] + [cs.gamma.to(DEV)]
        assert _v4(C, [self.g.ld, self.h.ld], [self.g.ptr, self.h.ptr]) == (WIDTH[self.l] == 4)
        lib.call("dc_bn_act_backward_reduce", self.g.view, self.g.ld, self.h.view, self.h.ld, self.R, C, *self.keep[:4], self.keep[4],
                 NR.SLOPE, 1, self.dg[:C], self.db[:C], self.coefs[:5 * C], self.ws, nb)

    def results(self):
        self.g.untouched()
        self.h.untouched()
        return dict(dgamma=_vres(self.dg), dbeta=_vres(self.db), coefs=_vres(self.coefs).view(5, self.C))


DEFERRED = {
    "unequal pair": [(4410, "c256"), (130, "c8")],
    "unequal pair reversed": [(130, "c8"), (4410, "c256")],
    "a pair and a single": [(4410, "c256"), (130, "c8"), (300, "c64")],
    "scalar width beside 16-byte": [(300, "c64_ld65"), (300, "c64")],
}


@pytest.mark.parametrize("name", list(DEFERRED))
def test_deferred_and_paired_reductions(name):
    """Announced dc_bn_act_backward_reduce calls inside one dc_finalisers_begin .. dc_finalisers_end: 16-byte layouts queue both
    stages (two first stages share one launch whose grid is the larger member's; the smaller member's surplus blocks return),
    a scalar-width layout only its finaliser.  Every output: the bits of the same call outside a batch, and the fp64 bounds."""
    calls = [_Reduce(R, l) for R, l in DEFERRED[name]]
    alone = []
    for c in calls:
        c.launch()
        torch.cuda.synchronize()
        alone.append(c.results())
    assert lib.raw("dc_finalisers_begin")() == 0
    try:
        for c in calls:
            assert lib.raw("dc_finaliser_defer_next")() == 0
            c.launch()
    except BaseException:
        lib.call("dc_finalisers_end", 1)
        raise
    lib.call("dc_finalisers_end", 0)
    torch.cuda.synchronize()
    ck = Checks(f"deferred: {name}")
    for i, (c, a) in enumerate(zip(calls, alone)):
        got = c.results()
        tag = f"call {i} ({c.R} x {c.l})"
        for k in got:
            ck.exact(f"{tag} {k} = the bits outside a batch", _bits(got[k]), _bits(a[k]))
        ref = NR.bwd_ref(c.cs.x, c.cs.dy.double(), c.cs.tr, c.cs.gamma, NR.SLOPE, 1, 1, 1)
        NR.check_reduce(ck, tag, got, ref, c.co, 1)
    ck.done()
