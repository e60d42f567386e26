"""The forward and input-gradient dense products of csrc/gemm.hip through the C ABI, every element against the fp64 restatement
and the bounds of tests/gemm_restate.py (their derivation: that module's docstring), in every operand-load mode, tile, multiply
path, epilogue and with the BatchNorm-backward prologue: dc_linear_forward, dc_linear_backward_input and
dc_linear_bn_backward_input (accumulate 0 and 1), dc_linear_bn_stats_forward, dc_linear_vn_stats_forward (interleaved 0, 1, 2),
dc_linear_bn_sums_forward and dc_linear_vn_sums_forward (their product output and sentinels; their sums stay with
tests/test_gpu_sync_bn.py).  tests/test_gemm_restate_host.py holds fp32 emulations to the same bounds on the same data and shows
that mutations leave them.

Layouts: every operand and output is a column block of a larger buffer with one spare row (gemm_restate.OPERAND: contiguous;
4 columns in with a leading dimension that keeps 16-byte accesses; 1 column in; an odd leading dimension), inputs NaN outside
the block (a value that leaks in shows as NaN), outputs SENT outside and NaN inside (accumulate: `base`), per-column outputs
with a sentinel behind, the coefficient rows of the prologue one float off where the layout says so, workspaces NaN-filled with a
sentinel behind.  Every call restates run_gemm's mode and launch_fast's path from the pointers and strides it passes and asserts
them against the case table; runs twice on fresh buffers and must return equal bits; leaves sentinels and inputs intact; returns
no NaN.

Across calls, on the exact chain (gemm_restate's docstring: the reduction order depends neither on the tile nor on the guards):
(a) every layout returns the bits of the contiguous one; (b) a ragged problem returns the bits of the corner of the same problem
zero-padded to whole tiles and run with option 3 = 1 (compared through int32 views; -0.f cannot arise: an accumulator starts at
+0.f and a cancelling sum rounds to +0.f); (c) the four tiles return equal bits; (d) accumulate 1 = base + accumulate 0 bit for
bit (in the drivers, every path); (e) the coefficient outputs and the running pair within the bounds of tests/nn_restate.py,
computed from the y the kernel stored.  tile = 0 runs once per shape of the table (contiguous operands) and returns the bits of
the forced tile that the restated pick_tile names.

The instantiation set the case table reaches, (BM, BN, AL, BL, MODE, EPI, PRO, X3, BP, DMA), is written out in EXPECTED
(per family and tile: (BL, MODE, X3, BP, DMA); AL = 0; EPI and PRO are the family's): modes 0 to 4 of the exact chain for every
family and tile, the in-loop split on 128-column tiles, the plane-fed loops (registers and DMA ring; prologue: registers only).
test_instantiations_reached reads the kernel names of one walk over the table and fails on a missing or an extra tuple.

Refusals: null pointer, N or K < 1, a leading dimension below the row, a leading dimension of 2^21, a workspace one byte short
(every statistics entry point checks it), M == 0.  The `store_y` / `accumulate` conflict that run_gemm refuses cannot be passed
through the C ABI (dc_linear_vn_*_forward set accumulate = 0 and the epilogue themselves); what the ABI can get wrong for the
combined store is its leading dimension, which is refused here.

What the earlier dense-product tests reach, from reading their parametrisations (tests/test_gpu_gemm.py): the forward product meets
modes 1 and 2 on every forced tile, mode 4 only with tile = 0 (test_strided_operands_and_outputs; its odd-stride weight view has an
odd K as well, so that call is mode 2 and mode 3 is not reached at all); the input gradient meets modes 1, 3 and 4, never 2; the
prologue form only through fused.bn_block_backward against the unfused pair; the statistics epilogues modes 0, 1 and 2.

Measured on an MI355X, worst error / bound over the whole table (recorded, not thresholds), product outputs per path:
    family   exact   split   planes (registers)   planes (DMA)        statistics outputs (mean .. running pair)
    fwd      0.243   0.414   0.414                0.414
    bwd      0.364   0.414   0.414                0.414               (accumulate 1 included)
    pro      0.406   0.355   0.467                --                  (accumulate 1 included)
    bn       0.243   0.414   0.414                0.414               0.493
    vn0      0.300   0.414   0.414                0.414               0.249
    vn1      0.243   0.414   0.414                0.414               0.265
    vn2      0.222   0.283   0.283                0.283               0.216
Every bit comparison (a) - (d), tile = 0, the two runs of every call and the sums forms' outputs: identical.  Wall time of this file:
about 9 s, of which the walk under the profiler takes 5.5 s and no other test more than 0.4 s."""
import contextlib
import re

import pytest
import torch

from deltaconv_amd._lib import lib
from tests import gemm_restate as GR
from tests import nn_restate as NR
from tests.apply_cases import Checks
from tests.test_gpu_gemm_dma import Planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = GR.SENT
NAN = float("nan")
FAMS = list(GR.FAMILIES)

# family -> tile -> (BL, MODE, X3, BP, DMA) of every instantiation the table reaches
_GUARDED = lambda bl: [(bl, m, 0, 0, 0) for m in (0, 1, 2, 3, 4)]
EXPECTED = {
    "fwd": {1: _GUARDED(0) + [(0, 0, 2, 0, 0), (0, 0, 2, 1, 0), (0, 0, 2, 1, 1)], 2: _GUARDED(0) + [(0, 0, 2, 1, 0), (0, 0, 2, 1, 1)],
            3: _GUARDED(0) + [(0, 0, 2, 1, 0), (0, 0, 2, 1, 1)], 4: _GUARDED(0) + [(0, 0, 2, 0, 0), (0, 0, 2, 1, 0), (0, 0, 2, 1, 1)]},
    "bwd": {1: _GUARDED(1) + [(1, 0, 2, 0, 0), (0, 0, 2, 1, 0), (0, 0, 2, 1, 1)], 2: _GUARDED(1) + [(0, 0, 2, 1, 0), (0, 0, 2, 1, 1)],
            3: _GUARDED(1) + [(0, 0, 2, 1, 0), (0, 0, 2, 1, 1)], 4: _GUARDED(1) + [(1, 0, 2, 0, 0), (0, 0, 2, 1, 0), (0, 0, 2, 1, 1)]},
    "pro": {1: _GUARDED(1) + [(1, 0, 1, 0, 0), (0, 0, 2, 1, 0)], 2: _GUARDED(1) + [(0, 0, 2, 1, 0)],
            3: _GUARDED(1) + [(0, 0, 2, 1, 0)], 4: _GUARDED(1) + [(1, 0, 1, 0, 0), (0, 0, 2, 1, 0)]},
}
for _f in ("bn", "vn0", "vn1", "vn2"):
    EXPECTED[_f] = EXPECTED["fwd"]


def expected_set(family, tile):
    _, epi, pro = GR.FAMILIES[family]
    bm, bn = GR.TILES[tile]
    return {GR.Inst(bm, bn, 0, bl, mode, epi, pro, x3, bp, dma) for bl, mode, x3, bp, dma in EXPECTED[family][tile]}


@contextlib.contextmanager
def options(case):
    """The library switches of a case (3: exact chain, 13: plane-fed loop through registers), put back to 0 whatever happens.  (The
    library has no getter; like `staging` in tests/test_gpu_gemm_dma.py this suite runs from the default switches, and the path
    every call asserts would fail first if 3 or 13 were preset.)"""
    opt = lib.raw("dc_set_option")
    kv = {"exact": {3: 1}, "planes_regs": {13: 1}}.get(case.opt, {})
    try:
        for k, v in kv.items():
            assert opt(k, v) == 0
        yield
    finally:
        for k in kv:
            opt(k, 0)


def _bits(t):
    return t if t.dtype != torch.float32 else t.contiguous().view(torch.int32)         # NaN-proof comparison


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(_bits(a), _bits(b)))


def _outside_ok(t, outside):
    return bool(torch.isnan(t).all()) if outside != outside else bool((t == outside).all())


class _Buf:
    """A [rows, w] column block, `off` columns in, of a [rows + 1, ld] buffer filled with `outside`; content None: NaN inside."""

    def __init__(self, geo, content=None, outside=SENT):
        rows, w, ld, off = geo
        self.ld, self.off, self.w, self.outside = ld, off, w, outside
        self.buf = torch.full((rows + 1, ld), outside, device=DEV)
        self.view = self.buf[:rows, off:off + w]
        self.content = content
        if content is None:
            self.view.fill_(NAN)
        else:
            assert tuple(content.shape) == (rows, w), (tuple(content.shape), rows, w)
            self.view.copy_(content)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (4 * off) % 16 and (rows <= 1 or self.view.stride(0) == ld)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def result(self):
        b = self.buf
        ok = _outside_ok(b[:, :self.off], self.outside) and _outside_ok(b[:, self.off + self.w:], self.outside) and _outside_ok(b[-1], self.outside)
        assert ok, "the surroundings of a buffer were overwritten"
        return self.view.cpu()

    def untouched(self):
        assert torch.equal(_bits(self.result()), _bits(self.content)), "an input was modified"


class _Vec:
    """n values of `dtype` with a sentinel either side, `shift` elements off the 16-byte boundary of the allocation + 16 bytes."""

    def __init__(self, n, content=None, dtype=torch.float32, shift=0):
        per16 = 16 // torch.empty((), dtype=dtype).element_size()
        self.lo, self.n = per16 + shift, n
        self.buf = torch.full((self.lo + n + 1,), SENT, dtype=dtype, device=DEV)
        self.view = self.buf[self.lo:self.lo + n]
        if content is None:
            self.view.fill_(NAN)
        else:
            self.view.copy_(content.reshape(-1))
        assert self.buf.data_ptr() % 16 == 0

    def result(self):
        assert bool((self.buf[:self.lo] == SENT).all()) and float(self.buf[-1]) == SENT, "the elements around a vector were overwritten"
        return self.view.cpu()


def _d(t):
    return None if t is None else t.to(DEV)


class Dev:
    """The backend of the drivers of tests/gemm_restate.py over the C ABI, in the layout, tile and options of a case."""

    def __init__(self, ck, twice=True):
        self.ck, self.twice, self.path, self.seen = ck, twice, None, []

    def begin(self, case, cs=None, tile=None):
        self.case, self.geo = case, GR.geometry(case)
        self.tile = case.tile if tile is None else tile
        self.bl, self.epi, self.pro = GR.FAMILIES[case.family]
        self.planes = case.opt.startswith("planes")

    # ---- what every call shares ----
    def _dispatch(self, a, b, out, h=None, coefs=None):
        ptr = dict(a=a.ptr, b=b.ptr, out=out.ptr)
        if h is not None:
            ptr.update(h=h.ptr, coefs=coefs.view.data_ptr())
        inst, path = GR.case_dispatch(self.case, ptr, self.tile)
        assert (inst.MODE, path) == (self.case.mode, self.case.path), f"{self.case}: the call runs {inst} ({path})"
        self.path = path
        self.seen.append(inst)

    def _operands(self, a_like, b, base, out_outside=SENT):
        A = [_Buf(self.geo["a"], t, NAN) for t in a_like]
        B = _Buf(self.geo["b"], b, NAN)
        O = _Buf(self.geo["out"], base, out_outside)
        pl = None
        if self.planes:
            assert B.view.is_contiguous()
            pl = Planes(B.view)
        return A, B, O, pl

    def _hint(self, pl):
        if pl is not None:
            pl.hint(self.bl == GR.B_KN)

    def _twice(self, what, fn):
        r1 = fn()
        if self.twice:
            r2 = fn()
            self.ck.true(f"{what}: two runs give equal bits", all(_same(a, b) for a, b in zip(r1, r2)))
        return r1

    def _ws(self, M, C, R):
        nb = int(lib.raw("dc_linear_stats_workspace_bytes")(M, C, R, self.tile))
        bm = GR.pick_tile(M, C, R, self.tile)[0]
        assert nb == GR.cdiv(M, bm) * 2 * C * 8
        return _Vec((nb + 7) // 8, dtype=torch.float64), nb

    # ---- the products ----
    def forward(self, x, w):
        (M, R), C = x.shape, w.shape[0]

        def once():
            (X,), W, Y, pl = self._operands([x], w, None)
            self._dispatch(X, W, Y)
            with options(self.case):
                self._hint(pl)
                lib.call("dc_linear_forward", X.view, X.ld, W.view, W.ld, M, C, R, Y.view, Y.ld, self.tile)
            X.untouched(), W.untouched()
            return [Y.result()]

        return self._twice("dc_linear_forward", once)[0]

    def backward_input(self, dy, w, base):
        (M, R), C = dy.shape, w.shape[1]

        def once():
            (G,), W, D, pl = self._operands([dy], w, base)
            self._dispatch(G, W, D)
            with options(self.case):
                self._hint(pl)
                lib.call("dc_linear_backward_input", G.view, G.ld, W.view, W.ld, M, R, C, D.view, D.ld, int(base is not None), self.tile)
            G.untouched(), W.untouched()
            return [D.result()]

        return self._twice("dc_linear_backward_input", once)[0]

    def bn_backward_input(self, dy, h, coefs, slope, w, base):
        (M, R), C = dy.shape, w.shape[1]

        def once():
            (G, H), W, D, pl = self._operands([dy, h], w, base)
            cf = _Vec(5 * R, coefs, shift=1 if self.case.layout == "cck" else 0)
            self._dispatch(G, W, D, H, cf)
            with options(self.case):
                self._hint(pl)
                lib.call("dc_linear_bn_backward_input", G.view, G.ld, H.view, H.ld, cf.view, slope, W.view, W.ld, M, R, C, D.view, D.ld,
                         int(base is not None), self.tile)
            G.untouched(), H.untouched(), W.untouched()
            assert torch.equal(_bits(cf.result()), _bits(coefs.reshape(-1))), "the coefficient rows were modified"
            return [D.result()]

        return self._twice("dc_linear_bn_backward_input", once)[0]

    # ---- the statistics epilogues ----
    def _coef_call(self, c, rm0, rv0, invoke):
        o = [_Vec(c) for _ in range(4)]
        rm, rv = (_Vec(c, rm0), _Vec(c, rv0)) if rm0 is not None else (None, None)
        invoke([t.view for t in o], None if rm is None else rm.view, None if rv is None else rv.view)
        return [t.result() for t in o] + [None if rm is None else rm.result(), None if rv is None else rv.result()]

    def bn_stats(self, x, w, gamma, beta, mom, rm0, rv0):
        (M, R), C = x.shape, w.shape[0]

        def once():
            (X,), W, Y, pl = self._operands([x], w, None)
            ws, nb = self._ws(M, C, R)
            self._dispatch(X, W, Y)

            def invoke(o, rm, rv):
                with options(self.case):
                    self._hint(pl)
                    lib.call("dc_linear_bn_stats_forward", X.view, X.ld, W.view, W.ld, M, C, R, Y.view, Y.ld, _d(gamma), _d(beta), NR.EPS, mom,
                             rm, rv, o[0], o[1], o[2], o[3], self.tile, ws.view, nb)

            r = self._coef_call(C, rm0, rv0, invoke)
            X.untouched(), W.untouched(), ws.result()
            return [Y.result()] + r

        r = self._twice("dc_linear_bn_stats_forward", once)
        return r[0], dict(zip(("mean", "invstd", "scale", "shift", "rm", "rv"), r[1:]))

    def vn_stats(self, v, w, co, interleaved, gamma, beta, mom, rm0, rv0):
        (M, R), C = v.shape, w.shape[0]
        assert C == (2 * co if interleaved else co) and M % 2 == 0

        def once():
            (V,), W, Y, pl = self._operands([v], w, None)
            ws, nb = self._ws(M, C, R)
            self._dispatch(V, W, Y)

            def invoke(o, rm, rv):
                with options(self.case):
                    self._hint(pl)
                    lib.call("dc_linear_vn_stats_forward", V.view, V.ld, W.view, W.ld, M // 2, co, R, Y.view, Y.ld, interleaved, _d(gamma),
                             _d(beta), NR.EPS, mom, rm, rv, o[0], o[1], o[2], o[3], self.tile, ws.view, nb)

            r = self._coef_call(co, rm0, rv0, invoke)
            V.untouched(), W.untouched(), ws.result()
            return [Y.result()] + r

        r = self._twice("dc_linear_vn_stats_forward", once)
        return r[0], dict(zip(("mean", "invstd", "scale", "shift", "rm", "rv"), r[1:]))

    def bn_sums(self, x, w):
        (M, R), C = x.shape, w.shape[0]
        (X,), W, Y, pl = self._operands([x], w, None)
        ws, nb = self._ws(M, C, R)
        sums = _Vec(2 * (2 * C + 1), dtype=torch.float64)                     # two identical records [sum | sum of squares | rows]
        self._dispatch(X, W, Y)
        with options(self.case):
            self._hint(pl)
            lib.call("dc_linear_bn_sums_forward", X.view, X.ld, W.view, W.ld, M, C, R, Y.view, Y.ld, sums.view, self.tile, ws.view, nb)
        X.untouched(), W.untouched(), ws.result()
        rec = sums.result().view(2, 2 * C + 1)
        self.ck.true("dc_linear_bn_sums_forward: two finite records that end with the row count",
                     bool(torch.isfinite(rec).all()) and torch.equal(rec[0], rec[1]) and float(rec[0, -1]) == M)
        return Y.result()

    def vn_sums(self, v, w, co, interleaved):
        (M, R), C = v.shape, w.shape[0]
        (V,), W, Y, pl = self._operands([v], w, None)
        ws, nb = self._ws(M, C, R)
        sums = _Vec(2 * (2 * co + 1), dtype=torch.float64)
        self._dispatch(V, W, Y)
        with options(self.case):
            self._hint(pl)
            lib.call("dc_linear_vn_sums_forward", V.view, V.ld, W.view, W.ld, M // 2, co, R, Y.view, Y.ld, interleaved, sums.view, self.tile,
                     ws.view, nb)
        V.untouched(), W.untouched(), ws.result()
        rec = sums.result().view(2, 2 * co + 1)
        self.ck.true("dc_linear_vn_sums_forward: two finite records that end with the point count",
                     bool(torch.isfinite(rec).all()) and torch.equal(rec[0], rec[1]) and float(rec[0, -1]) == M // 2)
        return Y.result()


def _raw(be, case, cs=None, tile=None):
    """The outputs of a case without the reference: for bit comparisons."""
    cs = GR.data(case) if cs is None else cs
    be.begin(case, cs, tile)
    return GR.raw_outputs(be, case, cs)


def _equal(ck, what, res, base, keys=None, corner=None):
    for k in (keys or base):
        a, b = res[k], base[k]
        if corner is not None:
            a = a[:b.shape[0], :b.shape[1]]
        ck.true(f"{what}: {k} has the same bits", _same(a, b))


@pytest.mark.parametrize("tile", [1, 2, 3, 4])
@pytest.mark.parametrize("family", FAMS)
def test_every_element_every_layout(family, tile):
    """The case table of one (family, tile): bounds, sentinels, determinism, modes and paths; then (a) and (b)."""
    ck = Checks(f"{family} tile {tile}")
    be = Dev(ck)
    res = {}
    for case in GR.plan(family, tile):
        cs = GR.data(case)
        be.begin(case, cs)
        print(f"--- {case}")
        res[case] = GR.run_case(be, case, ck, cs)
    assert set(be.seen) == expected_set(family, tile), set(be.seen) ^ expected_set(family, tile)
    # (a) on the exact chain every layout returns the bits of the contiguous one
    firsts = {}
    for case, r in res.items():
        if case.path == "exact":
            base = firsts.setdefault(case.kind, (case, r))
            if base[0] is not case:
                _equal(ck, f"(a) {case.kind} {case.layout}/{case.opt} against {base[0].layout}/{base[0].opt}", r, base[1])
    assert all(c.layout == "ccc" for c, _ in firsts.values()) and len(firsts) == 8
    # (b) a ragged problem = the corner of the zero-padded one on the exact chain
    quiet = Dev(ck, twice=False)
    for kind in ("rag4a", "rag4b", "odd"):
        case, r = firsts[kind]
        big = GR.padded(case.shape, tile)
        pc = case._replace(kind="padded", shape=big, layout="ccc", opt="exact", mode=0, path="exact")
        rp = _raw(quiet, pc, GR.data(case).zero_padded(*big))
        _equal(ck, f"(b) {kind} against the corner of {big}", rp, {k: r[k] for k in GR.PRODUCT_KEYS if k in r}, corner=True)
    ck.done()


@pytest.mark.parametrize("family", FAMS)
def test_tiles_and_the_automatic_tile_return_equal_bits(family):
    """(c) The exact chain reduces in an order that does not depend on the tile: a ragged and a whole problem (option 3 = 1) give
    the same product bits on all four tiles.  tile = 0, on every shape of the table, returns every output bit of the forced tile
    that the restated pick_tile names (at these sizes always a 64-row tile)."""
    ck = Checks(f"{family} tiles")
    be = Dev(ck, twice=False)
    for kind, shape, opt, mode in (("rag4", (132, 140, 36), "default", 1), ("whole", (256, 128, 96), "exact", 0)):
        res = {t: _raw(be, GR.Case(family, t, kind, shape, "ccc", opt, mode, "exact")) for t in GR.TILES}
        for t in (2, 3, 4):
            _equal(ck, f"(c) {shape} tile {t} against tile 1", res[t], res[1], keys=[k for k in GR.PRODUCT_KEYS if k in res[1]])
    # tile = 0, once per shape of the table (contiguous, default options): the forced tile is the one the restated pick_tile names,
    # the mode and path both runs must take come from the restated dispatch, and the kernels are ones the table already reaches
    shapes = sorted({c.shape for t in GR.TILES for c in GR.plan(family, t)})
    assert len(shapes) == 23, len(shapes)
    known = set().union(*(expected_set(family, t) for t in GR.TILES))
    for shape in shapes:
        t = GR.forced_tile(*shape)
        case = GR.Case(family, t, "auto", shape, "ccc", "default", None, None)
        inst, path = GR.case_dispatch(case)
        assert inst in known and (inst.BM, inst.BN) == GR.pick_tile(*shape, 0), (shape, inst)
        case = case._replace(mode=inst.MODE, path=path)
        _equal(ck, f"tile 0 on {shape} against tile {t}", _raw(be, case, tile=0), _raw(be, case))
    assert set(be.seen) <= known
    ck.done()


def test_instantiations_reached():
    """One walk over the whole table under the profiler: the template arguments in the kernel names are exactly EXPECTED, and
    EXPECTED holds modes 0 to 4 for every (tile, family)."""
    from torch.profiler import ProfilerActivity, profile
    want = set()
    for family in FAMS:
        for tile in GR.TILES:
            want |= expected_set(family, tile)
            assert expected_set(family, tile) == GR.expected_instantiations(family, tile)
            assert {i.MODE for i in expected_set(family, tile)} == {0, 1, 2, 3, 4}, (family, tile)
    be = Dev(Checks("walk"), twice=False)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:          # kernel names only: the walk makes ~50 000 host-side events
        for family in FAMS:
            for tile in GR.TILES:
                for case in GR.plan(family, tile):
                    _raw(be, case)
        torch.cuda.synchronize()
    seen = set()
    for e in prof.events():
        m = re.search(r"gemm_kernel<([^>]*)>", e.name)
        if m:
            args = [int(v) for v in re.findall(r"-?\d+", m.group(1))]
            assert len(args) == 10, e.name
            seen.add(GR.Inst(*args))
    assert seen, "no dense-product kernel in the trace"
    assert seen == want, f"missing {sorted(want - seen)}, not expected {sorted(seen - want)}"
    assert seen == set(be.seen)


# ---- refusals: nothing is launched, every output keeps its fill, the error text is the entry point's --------------------------
def _refused(name, args, rc_want, text, outputs):
    rc = lib.raw(name)(*args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == rc_want, (name, rc, lib.last_error())
    if text is not None:
        assert lib.last_error() == text, lib.last_error()
    for o in outputs:
        r = o.result()
        assert bool(torch.isnan(r).all()), f"{name}: a refused call wrote to an output"


def _small():
    M, C, R = 8, 8, 8
    g = lambda rows, w: (rows, w, w, 0)
    x, w = _Buf(g(M, R), GR.binades((M, R), 1), NAN), _Buf(g(C, R), GR.binades((C, R), 2), NAN)
    return M, C, R, x, w, _Buf(g(M, C))


def test_refusals_of_the_plain_products():
    M, C, R, x, w, y = _small()
    p = lambda b: b.ptr
    fwd = lambda **k: (k.get("x", p(x)), k.get("ldx", R), k.get("w", p(w)), k.get("ldw", R), k.get("M", M), k.get("N", C), k.get("K", R),
                       k.get("y", p(y)), k.get("ldy", C), 0)
    for kw, text in [(dict(x=None), "null pointer"), (dict(w=None), "null pointer"), (dict(y=None), "null pointer"), (dict(N=0), "bad size"),
                     (dict(K=0), "bad size"), (dict(M=-1), "bad size"), (dict(ldx=R - 1), "bad size"), (dict(ldw=R - 1), "bad size"),
                     (dict(ldy=C - 1), "bad size"), (dict(ldx=1 << 21), "leading dimension above 2^21 elements"),
                     (dict(ldw=1 << 21), "leading dimension above 2^21 elements")]:
        _refused("dc_linear_forward", fwd(**kw), -1, "dc_linear_forward: " + text, [y])
    _refused("dc_linear_forward", fwd(M=0), 0, None, [y])                    # M == 0: DC_OK, nothing written
    bwd = lambda **k: (k.get("x", p(x)), k.get("ldx", R), k.get("w", p(w)), k.get("ldw", R), k.get("M", M), k.get("N", R), k.get("K", C),
                       k.get("y", p(y)), k.get("ldy", C), k.get("acc", 0), 0)
    for kw, text in [(dict(x=None), "null pointer"), (dict(y=None), "null pointer"), (dict(N=0), "bad size"), (dict(K=0), "bad size"),
                     (dict(ldx=R - 1), "bad size"), (dict(ldw=C - 1), "bad size"), (dict(ldy=C - 1), "bad size"),
                     (dict(ldx=1 << 21, acc=1), "leading dimension above 2^21 elements"), (dict(ldw=1 << 21), "leading dimension above 2^21 elements")]:
        _refused("dc_linear_backward_input", bwd(**kw), -1, "dc_linear_backward_input: " + text, [y])
    _refused("dc_linear_backward_input", bwd(M=0, acc=1), 0, None, [y])
    h, cf = _Buf((M, R, R, 0), GR.binades((M, R), 3), NAN), _Vec(5 * R, GR.binades((5, R), 4))
    pro = lambda **k: (k.get("x", p(x)), k.get("ldx", R), k.get("h", p(h)), k.get("ldh", R), k.get("cf", cf.view.data_ptr()), 0.2, k.get("w", p(w)),
                       k.get("ldw", R), k.get("M", M), k.get("N", R), k.get("K", C), k.get("y", p(y)), k.get("ldy", C), 0, 0)
    for kw, text in [(dict(h=None), "null pointer"), (dict(cf=None), "null pointer"), (dict(N=0), "bad size"), (dict(ldh=R - 1), "bad size"),
                     (dict(ldh=1 << 21), "leading dimension above 2^21 elements"), (dict(ldx=1 << 21), "leading dimension above 2^21 elements")]:
        _refused("dc_linear_bn_backward_input", pro(**kw), -1, "dc_linear_bn_backward_input: " + text, [y])
    _refused("dc_linear_bn_backward_input", pro(M=0), 0, None, [y])
    x.untouched(), w.untouched(), h.untouched()


def test_refusals_of_the_statistics_forms():
    """Every statistics entry point checks its workspace (gemm.hip: `workspace_bytes < dc_linear_stats_workspace_bytes`): one byte
    short is refused with DC_ERR_WORKSPACE before anything is launched.  M == 0 is a bad size here (statistics of no rows)."""
    M, C, R, x, w, y = _small()
    co = C // 2
    nb = int(lib.raw("dc_linear_stats_workspace_bytes")(M, C, R, 0))
    ws = _Vec((nb + 7) // 8, dtype=torch.float64)
    o = [_Vec(C) for _ in range(4)]
    sums = _Vec(2 * (2 * C + 1), dtype=torch.float64)
    outs = [y, ws, sums] + o
    p, vp = (lambda b: b.ptr), (lambda v: v.view.data_ptr())
    bn = lambda **k: (k.get("x", p(x)), k.get("ldx", R), p(w), k.get("ldw", R), k.get("M", M), k.get("N", C), k.get("K", R), k.get("y", p(y)),
                      k.get("ldy", C), None, None, NR.EPS, NR.MOM, None, None, k.get("mean", vp(o[0])), vp(o[1]), vp(o[2]), vp(o[3]), 0,
                      k.get("ws", vp(ws)), k.get("nb", nb))
    name = "dc_linear_bn_stats_forward"
    for kw, rc, text in [(dict(x=None), -1, "null pointer"), (dict(mean=None), -1, "null pointer"), (dict(M=0), -1, "bad size"),
                         (dict(K=0), -1, "bad size"), (dict(ldy=C - 1), -1, "bad size"), (dict(nb=nb - 1), -3, "workspace too small"),
                         (dict(ws=None), -3, "workspace too small"), (dict(ldx=1 << 21), -1, "leading dimension above 2^21 elements")]:
        _refused(name, bn(**kw), rc, f"{name}: {text}", outs)
    vn = lambda il, **k: (p(x), k.get("ldx", R), p(w), R, k.get("n", M // 2), co if il else C, R, p(y), k.get("ldy", co if il == 2 else C), il,
                          None, None, NR.EPS, NR.MOM, None, None, vp(o[0]), vp(o[1]), vp(o[2]), vp(o[3]), 0, vp(ws), k.get("nb", nb))
    name = "dc_linear_vn_stats_forward"
    for il, kw, rc, text in [(1, dict(ldy=C - 1), -1, "bad size"), (2, dict(ldy=co - 1), -1, "bad size"), (0, dict(ldy=C - 1), -1, "bad size"),
                             (1, dict(n=0), -1, "bad size"), (2, dict(nb=nb - 1), -3, "workspace too small"),
                             (1, dict(ldx=1 << 21), -1, "leading dimension above 2^21 elements")]:
        _refused(name, vn(il, **kw), rc, f"{name}: {text}", outs)
    name = "dc_linear_bn_sums_forward"
    bs = lambda **k: (p(x), R, p(w), R, k.get("M", M), C, R, p(y), k.get("ldy", C), k.get("sums", vp(sums)), 0, vp(ws), k.get("nb", nb))
    for kw, rc, text in [(dict(sums=None), -1, "null pointer"), (dict(M=0), -1, "bad size"), (dict(ldy=C - 1), -1, "bad size"),
                         (dict(nb=nb - 1), -3, "workspace too small")]:
        _refused(name, bs(**kw), rc, f"{name}: {text}", outs)
    name = "dc_linear_vn_sums_forward"
    vs = lambda il, **k: (p(x), R, p(w), R, M // 2, co if il else C, R, p(y), k.get("ldy", co if il == 2 else C), il, k.get("sums", vp(sums)), 0,
                          vp(ws), k.get("nb", nb))
    for il, kw, rc, text in [(1, dict(sums=None), -1, "null pointer"), (2, dict(ldy=co - 1), -1, "bad size"), (1, dict(nb=nb - 1), -3, "workspace too small")]:
        _refused(name, vs(il, **kw), rc, f"{name}: {text}", outs)
    x.untouched(), w.untouched()
