"""The gather-path sparse applies and neighbourhood aggregations (csrc/apply.hip, aggregate.hip, ell_stage.h, ell_math.h)
through the C ABI, per element against the fp64 restatement of tests/apply_restate.py, in every layout that makes
`dcstage::pick_v` choose another vector width.

Bounds: derived in the docstring of tests/apply_restate.py (u = 2^-24, m = fma terms of the element's chain, S = sum of the
magnitudes of the added terms): linear bodies gamma_(m + 2) S = (m + 2) u S to first order, norm 3 u |n|, div|curl|norm^T
gamma_(m + 6) S, max_affine gamma_2 max_s (|scale h_s| + |shift|), its residual form gamma_3 (that / gamma_2 + |scale2 h2| + |shift2|), the slot
of an affine maximum within e_w + e_t of the fp64 maximum (w the returned slot, t the fp64 winner: the sum of the two slots'
bounds is what the arithmetic implies, one alone is not), plain dc_knn_max exact in value and first maximal slot.
tests/test_apply_restate_host.py holds the CPU build of the same bodies to the same bounds on the same data.

Data (tests/apply_restate.py: make_*): per-row coefficient magnitudes log-uniform over 1e-3 .. 1e3 with random signs, feature
columns with scales over 1e-2 .. 1e2, exactly-zero tangent vectors (the |v| = 0 subgradient branch), graphs built here (slot
0 = self, the rest random points of the same cloud; the hub cloud has 19 columns of more than T_CHUNK = 2048 in-edges).  The
CSC arrays come from dc_csc_build and the permuted coefficients from dc_csc_permute_coef, as in the product; the references
use neither.

Layouts: every operand is a column block of a SENT-filled buffer with one spare row; a layout is (C, row stride of a C-wide
operand, first column); an operand of 2C or 3C columns gets the stride + C or + 2C (same residue mod 4 at C = 64).  The
width `pick_v` must choose is restated here (`_width`) from the pointers and strides actually passed and asserted per call
against the table: a layout that silently tests another path fails.  For one C every layout must return the bits of the
contiguous one.  Every check prints its worst error / bound before anything is asserted.

The aggregations exist at 16 bytes and as scalars only: a layout whose applies run V = 2 runs them at V = 1, and that width
(4 or 1) is asserted per call as well.

Long k-lists.  The staged forward skeleton asks for (points per block + 1) * k * 12 + 16 bytes of dynamic LDS
(ell_stage.h: fwd_lds_bytes, restated here as `_stage_bytes`) and takes no opt-in for more than 64 KiB, so of k in
{85, 128, 255} x C in {1, 4, 16, 64} on one cloud of 300 points only C = 64 can launch the forward entries (17 staged points:
52 036 bytes at k = 255; C = 1, 4 and 16 stage 65 points: 66 316 bytes at k = 85): test_long_k_lists_forward runs dc_apply_grad,
dc_apply_div_curl_norm, dc_knn_max and dc_knn_sum (and the other forward entries) there and asserts from the arithmetic that
the pairs it leaves out are exactly those whose request exceeds 64 KiB -- the open defect of the documented k <= 255 that
DESIGN.md and include/deltaconv_hip.h record.  The transposed skeletons stage fixed-size chunks, so test_k255_transposed runs
every transposed entry and both max-backward loops at k = 255 (slot byte 254) for all four channel counts, and at C = 64 in the
8-byte and scalar layouts too; where dc_knn_max cannot launch, the slot bytes come from the restatement (they are exact).
"""
import functools

import pytest
import torch

from deltaconv_amd._lib import lib
from tests.apply_cases import ALL, Checks, case as _case, graph as _graph, run, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0

LAYOUTS = {                                          # name -> (C, row stride, first column)
    "c64": (64, 64, 0), "c8": (8, 8, 0), "c6": (6, 6, 0), "c64_ld70_off6": (64, 70, 6), "c64_ld66": (64, 66, 0),
    "c64_ld70_off1": (64, 70, 1), "c64_ld65": (64, 65, 0), "c7": (7, 7, 0),
    "c1": (1, 1, 0), "c4": (4, 4, 0), "c16": (16, 16, 0),           # the long k-lists
}
CASES = {                                            # name -> (layout of the inputs, layout of the outputs, width pick_v must choose)
    "c64": ("c64", "c64", 4), "c8": ("c8", "c8", 4), "c6": ("c6", "c6", 2), "c64_ld70_off6": ("c64_ld70_off6", "c64_ld70_off6", 2),
    "c64_ld66": ("c64_ld66", "c64_ld66", 2), "c64_ld70_off1": ("c64_ld70_off1", "c64_ld70_off1", 1), "c64_ld65": ("c64_ld65", "c64_ld65", 1),
    "c7": ("c7", "c7", 1), "in_c64_out_off6": ("c64", "c64_ld70_off6", 2), "in_off6_out_c64": ("c64_ld70_off6", "c64", 2),
    "c1": ("c1", "c1", 1), "c4": ("c4", "c4", 4), "c16": ("c16", "c16", 4),
}
CONTIGUOUS = {64: "c64", 8: "c8", 6: "c6", 7: "c7", 1: "c1", 4: "c4", 16: "c16"}


def _width(c, lds, ptrs):
    """dcstage::pick_v (ell_stage.h) restated: 16-byte accesses when C, every leading dimension and every base allow them,
    8-byte accesses for even counts / strides / 8-byte aligned bases, else one float."""
    v = 4 if c % 4 == 0 else (2 if c % 2 == 0 else 1)
    for ld in lds:
        if ld % 2:
            return 1
        if ld % 4:
            v = min(v, 2)
    for p in ptrs:
        if p % 8:
            return 1
        if p % 16:
            v = min(v, 2)
    return v


def _stage_bytes(c, v, k):
    """dcstage::fwd_lds_bytes (ell_stage.h) restated: the dynamic LDS the staged forward skeleton requests."""
    groups = c // v
    tpb = 256 if groups >= 4 else 64 * groups
    return ((tpb + groups - 1) // groups + 1) * k * 12 + 16


@functools.lru_cache(maxsize=None)
def _device_graph(gname):
    """nbr and the CSC of dc_csc_build on the device."""
    nbr, sizes = _graph(gname)
    n, k = nbr.shape
    nbr32 = nbr.to(torch.int32).to(DEV)
    ptr = torch.tensor([sum(sizes[:q]) for q in range(len(sizes) + 1)], dtype=torch.int32, device=DEV)
    tptr = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
    tedge = torch.full((n * k,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(n * (k + 1), dtype=torch.int32, device=DEV)
    lib.call("dc_csc_build", nbr32, ptr, len(sizes), n, k, tptr, tedge, ws, ws.numel() * 4)
    return nbr32, tptr, tedge


class _Buf:
    """An operand: a [rows, W] column block of a SENT-filled [rows + 1, ld] buffer."""

    def __init__(self, layout, rows, width, content=None):
        c, ld, off = LAYOUTS[layout]
        self.ld, self.off, self.w = ld + (width - c), off, width
        self.buf = torch.full((rows + 1, self.ld), SENT, device=DEV)
        self.view = self.buf[:rows, off:off + width]
        if content is None:
            self.view.fill_(float("nan"))
        else:
            assert tuple(content.shape) == (rows, width)
            self.view.copy_(content)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == (4 * off) % 16 and self.view.stride(0) == self.ld

    def intact(self):
        b = self.buf
        return bool((b[:, :self.off] == SENT).all()) and bool((b[:, self.off + self.w:] == SENT).all()) and bool((b[-1] == SENT).all())

    def result(self):
        assert self.intact(), "sentinels around the output were overwritten"
        return self.view.cpu()


class DeviceBackend:
    max_T_variants = (0, 1)          # DC_OPT_GATHER_BATCH (option 1): 0 = batched edge loop, 1 = the generic transposed skeleton

    def __init__(self, gname, cname):
        self.lin, self.lout, self.expect = CASES[cname]
        self.cs = _case(gname, LAYOUTS[self.lin][0])
        self.n, self.k, self.C = self.cs.n, self.cs.k, self.cs.C
        self.nbr32, self.tptr, self.tedge = _device_graph(gname)
        self._coefs = {}

    def _coef(self, op, transposed):
        key = ("G" if op in ("grad", "hodge") else "D", transposed)
        if key not in self._coefs:
            coef = (self.cs.G if key[0] == "G" else self.cs.D).to(DEV).contiguous()
            if transposed:
                ct = torch.empty_like(coef)
                lib.call("dc_csc_permute_coef", coef, self.tedge, self.n * self.k, ct)
                coef = ct
            self._coefs[key] = coef
        return self._coefs[key]

    def _picked(self, *bufs):
        """The width pick_v must choose for these operands is the one the case is in the table for."""
        got = _width(self.C, [b.ld for b in bufs], [b.view.data_ptr() for b in bufs])
        assert got == self.expect, f"this layout runs V = {got}, the table says {self.expect}"

    def _picked_agg(self, *bufs):
        """The aggregations: 16-byte accesses where the applies of this case take them, scalars otherwise."""
        got = _width(self.C, [b.ld for b in bufs], [b.view.data_ptr() for b in bufs])
        assert (4 if got == 4 else 1) == (4 if self.expect == 4 else 1), f"this layout runs the aggregations at V = {got}"

    def _in(self, t):
        return _Buf(self.lin, t.shape[0], t.shape[1], t)

    def _out(self, rows, width, prev=None):
        return _Buf(self.lout, rows, width, prev)

    def fwd(self, op, x):
        rows, mult = {"grad": (2, 1), "div": (1, 1), "div_curl_norm": (1, 3), "hodge": (2, 1)}[op]
        i, o = self._in(x), self._out(rows * self.n, mult * self.C)
        self._picked(i, o)
        lib.call("dc_apply_" + op, self._coef(op, False), self.nbr32, self.n, self.k, i.view, self.C, i.ld, o.view, o.ld)
        return o.result()

    def T(self, op, dy, prev, v=None):
        rows, mult = {"grad": (1, 1), "div": (2, 1), "div_curl_norm": (2, 1), "hodge": (1, 2)}[op]
        i, o = self._in(dy), self._out(rows * self.n, mult * self.C, prev)
        acc = int(prev is not None)
        if op == "div_curl_norm":
            vb = self._in(v)
            self._picked(i, vb, o)
            lib.call("dc_apply_div_curl_norm_T", self._coef(op, True), self.tptr, self.tedge, self.n, self.k, i.view, self.C, i.ld, vb.view,
                     vb.ld, o.view, o.ld, acc)
        else:
            self._picked(i, o)
            lib.call(f"dc_apply_{op}_T", self._coef(op, True), self.tptr, self.tedge, self.n, self.k, i.view, self.C, i.ld, o.view, o.ld, acc)
        return o.result()

    def grad_T_sum(self, dy, a, b):
        i, ab, o = self._in(dy), self._in(a), self._out(self.n, self.C)
        bb = self._in(b) if b is not None else None
        self._picked(*[t for t in (i, ab, bb, o) if t is not None])
        lib.call("dc_apply_grad_T_sum", self._coef("grad", True), self.tptr, self.tedge, self.n, self.k, i.view, self.C, i.ld, ab.view, ab.ld,
                 bb.view if bb else None, bb.ld if bb else 0, o.view, o.ld)
        return o.result()

    def knn_sum(self, h, scale):
        i, o = self._in(h), self._out(self.n, self.C)
        self._picked_agg(i, o)
        lib.call("dc_knn_sum", self.nbr32, self.n, self.k, i.view, self.C, i.ld, scale, o.view, o.ld)
        return o.result()

    def knn_sum_T(self, dout, scale, prev):
        i, o = self._in(dout), self._out(self.n, self.C, prev)
        self._picked_agg(i, o)
        lib.call("dc_knn_sum_backward", self.tptr, self.tedge, self.n, self.k, i.view, self.C, i.ld, scale, o.view, o.ld, int(prev is not None))
        return o.result()

    def _arg(self):
        return torch.full((self.n + 1, self.C), 255, dtype=torch.uint8, device=DEV)

    def _arg_result(self, arg):
        assert bool((arg[-1] == 255).all()), "the row behind the slot bytes was overwritten"
        return arg[:-1].cpu()

    def knn_max(self, h):
        i, o, arg = self._in(h), self._out(self.n, self.C), self._arg()
        self._picked_agg(i, o)
        lib.call("dc_knn_max", self.nbr32, self.n, self.k, i.view, self.C, i.ld, o.view, o.ld, arg)
        return o.result(), self._arg_result(arg)

    def knn_max_affine(self, h, scale, shift, slope):
        i, o, arg = self._in(h), self._out(self.n, self.C), self._arg()
        self._picked_agg(i, o)
        lib.call("dc_knn_max_affine", self.nbr32, self.n, self.k, i.view, self.C, i.ld, scale.to(DEV), shift.to(DEV), slope, o.view, o.ld, arg)
        return o.result(), self._arg_result(arg)

    def knn_max_affine_residual(self, h, scale, shift, slope, h2, scale2, shift2, slope2):
        i, i2, o, o2, arg = self._in(h), self._in(h2), self._out(self.n, self.C), self._out(self.n, self.C), self._arg()
        self._picked_agg(i, i2, o, o2)
        lib.call("dc_knn_max_affine_residual", self.nbr32, self.n, self.k, i.view, self.C, i.ld, scale.to(DEV), shift.to(DEV), slope, i2.view,
                 i2.ld, scale2.to(DEV), shift2.to(DEV), slope2, o.view, o.ld, o2.view, o2.ld, arg)
        return o.result(), o2.result(), self._arg_result(arg)

    def knn_max_T(self, arg, dout, prev, variant):
        i, o = self._in(dout), self._out(self.n, self.C, prev)
        self._picked_agg(i, o)
        opt = lib.raw("dc_set_option")
        opt(1, variant)
        try:
            lib.call("dc_knn_max_backward", self.tptr, self.tedge, self.n, self.k, arg.to(DEV).contiguous(), i.view, self.C, i.ld, o.view, o.ld,
                     int(prev is not None))
        finally:
            opt(1, 0)
        return o.result()


@functools.lru_cache(maxsize=None)
def _results(gname, cname, which=ALL):
    """Every body of `which` run once in this layout: -> (results, the checks, not yet asserted)."""
    be = DeviceBackend(gname, cname)
    ck = Checks(f"{gname} {cname}")
    return run(be, be.cs, ck, which), ck


def _run_case(gname, cname, which=ALL):
    res, ck = _results(gname, cname, which)
    c = LAYOUTS[CASES[cname][0]][0]
    if cname != CONTIGUOUS[c]:                       # independence from alignment: the bits of the contiguous layout of this C
        base, _ = _results(gname, CONTIGUOUS[c], which)
        same_bits(ck, f"= {CONTIGUOUS[c]}", res, base)
    ck.done()


@pytest.mark.parametrize("cname", ["c64", "c8", "c6", "c64_ld70_off6", "c64_ld66", "c64_ld70_off1", "c64_ld65", "c7", "in_c64_out_off6",
                                   "in_off6_out_c64"])
def test_layouts(cname):
    """The base graph (ragged clouds 300 / 257 / 64, k = 20) in every layout of the table."""
    _run_case("base", cname)


@pytest.mark.parametrize("cname", ["c64", "c64_ld70_off6", "c7"])
@pytest.mark.parametrize("gname", ["k1", "k7", "k64"])
def test_other_k(gname, cname):
    """k = 1 (the self loop alone), 7 (odd, below the unroll) and 64 on clouds of 130 and 64 points, at the three widths."""
    _run_case(gname, cname)


@pytest.mark.parametrize("cname", ["c64", "c6"])
def test_hub_columns_longer_than_a_chunk(cname):
    """One cloud of 2400 points whose 19 hub targets have more than 2200 in-edges each: the transposed skeletons stage such
    a column in more than one chunk of T_CHUNK = 2048 entries (C = 64: 16 points per block; C = 6: the 8-byte path)."""
    nbr, _ = _graph("hub")
    assert int(torch.bincount(nbr.reshape(-1)).max()) > 2048
    _run_case("hub", cname)


LONG_K, LONG_C = (85, 128, 255), (1, 4, 16, 64)
FWD = ("grad", "div", "div_curl_norm", "hodge", "knn_sum", "knn_max", "knn_max_affine", "knn_max_affine_residual")
TRANSPOSED = ("grad_T", "div_T", "div_curl_norm_T", "hodge_T", "grad_T_sum", "knn_sum_T", "knn_max_T")


def _fits(c, k):
    """Can the forward skeleton launch this contiguous shape?  (V as pick_v chooses it for C alone.)"""
    return _stage_bytes(c, 4 if c % 4 == 0 else (2 if c % 2 == 0 else 1), k) <= 64 * 1024


@pytest.mark.parametrize("k", LONG_K)
def test_long_k_lists_forward(k):
    """The forward entries at k in {85, 128, 255}, C = 64, on one cloud of 300 points, and the arithmetic that says which of
    the pairs k x C in {1, 4, 16, 64} cannot launch: exactly the three small channel counts, at every one of these k."""
    assert [c for c in LONG_C if _fits(c, k)] == [64]
    assert _stage_bytes(64, 4, 255) == 52036 and _stage_bytes(4, 4, 85) == 66316 and _stage_bytes(1, 1, 255) == 198916
    _run_case(f"k{k}", "c64", FWD)


@pytest.mark.parametrize("cname", ["c1", "c4", "c16", "c64", "c64_ld70_off6", "c64_ld65"])
def test_k255_transposed(cname):
    """Every transposed entry, accumulate 0 and 1, and both max-backward loops at k = 255: slot byte 254."""
    _run_case("k255", cname, TRANSPOSED)
