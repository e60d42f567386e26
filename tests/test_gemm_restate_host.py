"""CPU: the bounds, the data and the restated dispatch of tests/gemm_restate.py mean something.

Emulations, passed as `backend` to the drivers of tests/gemm_restate.py on every case of its table:
  * the exact chain in fp32 (one rounding per multiply-add, formed through fp64: the product of two fp32 values is exact there) in
    the kernel's documented k order -- K tiles of 32, fragment set j, step t, the pair k = 8 j + t, 8 j + 4 + t;
  * the split products: three bf16 planes by torch casts (tests/test_split_arithmetic.py: split3), the six kept partial products
    smallest first, one fp32 rounding per 16 products and accumulator (whole tiles only, as in the library);
  * the prologue in fp32: z = fmaf, dz = dy * slope, t = fmaf, dh = fmaf;
  * the statistics from the emulated output in fp64, rounded once.
Each stays within every bound.  Each mutation listed in MUTATIONS leaves a bound on EVERY case, over all four tiles, in which
it changes the bits of the emulated output (i.e. changes an addend that is not an exact zero), and that set of cases is
non-empty for every mutation and every family it applies to.  The restated pick_tile / load_mode / path are held to a hand-written table and to the modes and
paths the case table names; tests/test_gpu_gemm_abi.py relies on them."""
import functools

import numpy as np
import pytest
import torch

from tests import gemm_restate as GR
from tests import nn_restate as NR
from tests.apply_cases import Checks
from tests.test_split_arithmetic import split3

F32, F64 = np.float32, np.float64
NAN = float("nan")
PRODUCT_MUTATIONS = ("drop_last_k", "drop_tail_first_k", "next_weight_row", "skip_last_row", "read_past_k")
MUTATIONS = {m: tuple(GR.FAMILIES) for m in PRODUCT_MUTATIONS}
MUTATIONS.update(base_twice=("bwd", "pro"), gate_inverted=("pro",), ca_for_cb=("pro",))


class Emu:
    """The backend of the drivers: an fp32 emulation of one multiply path, optionally with one mutation."""

    def __init__(self, path, mut=None):
        self.path, self.mut = path, mut

    def begin(self, case, cs):
        self.tile, self.cs = GR.TILES[case.tile], cs

    def _mm(self, a, b, base=None):
        A, B = a.double().numpy(), b.double().numpy()
        (M, R), C = A.shape, B.shape[1]
        bm, bn = self.tile
        mut = self.mut
        if mut == "next_weight_row":                  # the last column tile reads the weights of the column behind
            idx = np.arange(C)
            j0 = bn * ((C - 1) // bn)
            idx[j0:] = np.minimum(idx[j0:] + 1, C - 1)
            B = B[:, idx]
        skip = set()
        if mut == "drop_last_k":
            skip.add(R - 1)
        if mut == "drop_tail_first_k" and R % 32:
            skip.add(32 * (R // 32))
        acc = np.zeros((M, C), F32)
        if self.path == "exact":
            for t0 in range(0, R, 32):
                for j in range(4):
                    for t in range(4):
                        for k in (t0 + 8 * j + t, t0 + 8 * j + 4 + t):
                            if k < R and k not in skip:
                                acc = (acc.astype(F64) + np.outer(A[:, k], B[k])).astype(F32)
        else:
            assert R % 16 == 0
            A32, B32 = torch.from_numpy(A).float(), torch.from_numpy(B).float()
            for k in skip:
                A32[:, k] = 0.0
            ah, am, al = (p.double().numpy() for p in split3(A32)[:3])
            bh, bm_, bl = (p.double().numpy() for p in split3(B32)[:3])
            for s in range(0, R, 16):
                for p, q in ((al, bh), (ah, bl), (am, bm_), (am, bh), (ah, bm_), (ah, bh)):
                    acc = (acc.astype(F64) + p[:, s:s + 16] @ q[s:s + 16]).astype(F32)
        if mut == "read_past_k":                      # one more k: an element of ordinary operand size from each operand's neighbour
            acc = (acc.astype(F64) + np.outer(np.roll(A[:, R - 1], 1), np.roll(B[R - 1], 1))).astype(F32)
        out = torch.from_numpy(acc)
        if base is not None:
            out = base + out
            if mut == "base_twice":
                out = out + base
        if mut == "skip_last_row" and M % bm:
            out[M - 1] = base[M - 1] if base is not None else NAN
        return out

    def forward(self, x, w):
        return self._mm(x, w.t())

    def backward_input(self, dy, w, base):
        return self._mm(dy, w, base)

    def bn_backward_input(self, dy, h, coefs, slope, w, base):
        f = lambda t: t.double().numpy()
        rnd = lambda v: v.astype(F32).astype(F64)
        cf = f(coefs)
        if self.mut == "ca_for_cb":
            cf = cf.copy()
            cf[4] = cf[3]
        z = rnd(cf[0] * f(h) + cf[1])
        gate = z > 0
        if self.mut == "gate_inverted":
            gate = gate.copy()
            gate[self.cs.site] = ~gate[self.cs.site]
        dz = np.where(gate, f(dy), rnd(f(dy) * F64(F32(slope))))
        dh = rnd(cf[2] * dz + rnd(cf[3] * f(h) + cf[4]))
        return self._mm(torch.from_numpy(dh).float(), w, base)

    @staticmethod
    def _stats(v, gamma, beta, mom, rm0, rv0):
        R = v.shape[0]
        mean, sq = v.sum(0) / R, (v * v).sum(0) / R
        var = (sq - mean * mean).clamp_min(0)
        invstd = (var + NR.EPS).rsqrt()
        scale = invstd * (gamma.double() if gamma is not None else 1.0)
        out = dict(mean=mean, invstd=invstd, scale=scale, shift=(beta.double() if beta is not None else 0.0) - mean * scale, rm=None, rv=None)
        if rm0 is not None:
            out["rm"] = (1 - mom) * rm0.double() + mom * mean
            out["rv"] = (1 - mom) * rv0.double() + mom * var * (R / (R - 1) if R > 1 else 1.0)
        return {k: None if t is None else t.float() for k, t in out.items()}

    def bn_stats(self, x, w, gamma, beta, mom, rm0, rv0):
        y = self._mm(x, w.t())
        return y, self._stats(y.double(), gamma, beta, mom, rm0, rv0)

    def vn_stats(self, v, w, co, interleaved, gamma, beta, mom, rm0, rv0):
        out = self._mm(v, w.t())
        u, d = out[0::2], out[1::2]
        yu, yv = (u[:, 0::2] - d[:, 1::2], d[:, 0::2] + u[:, 1::2]) if interleaved else (u, d)
        n = torch.sqrt(yu * yu + yv * yv)             # fp32: at most the three roundings the bound of dc_vn_stats counts
        if interleaved == 2:
            out = torch.stack([yu, yv], 1).reshape(out.shape[0], co)
        return out, self._stats(n.double(), gamma, beta, mom, rm0, rv0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(be, case, tag):
    cs = GR.data(case)
    ck = Checks(tag)
    be.begin(case, cs)
    return GR.run_case(be, case, ck, cs), ck


@functools.lru_cache(maxsize=None)
def _clean(case):
    res, ck = _run(Emu(case.path if case.path in ("exact", "split") else "split"), case, f"{case}")
    return res, ck


def _cases(family, tiles=(1, 2, 3, 4)):
    return [c for t in tiles for c in GR.plan(family, t)]


@pytest.mark.parametrize("tile", [1, 2, 3, 4])
@pytest.mark.parametrize("family", list(GR.FAMILIES))
def test_emulations_stay_within_every_bound(family, tile):
    """The emulation of the path a case names (planes: the split products) holds every bound of every case; the exact chain is
    also run on the whole-tile cases that name a split path (option 3 = 1 runs it there)."""
    for case in GR.plan(family, tile):
        _, ck = _clean(case)
        ck.done()
        if case.path != "exact" and case.opt == "default":
            _, ck = _run(Emu("exact"), case._replace(path="exact"), f"{case} exact")
            ck.done()


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutations_leave_the_bounds(mut):
    """Every case whose emulated output the mutation changes must fail a check; there is such a case in every family."""
    for family in MUTATIONS[mut]:
        applies = caught = 0
        for case in _cases(family):
            if case.layout != "ccc" or case.opt not in ("default", "exact"):
                continue                                # the emulation does not depend on the layout: one run per shape and path
            clean, _ = _clean(case)
            got, ck = _run(Emu(case.path, mut), case, f"{mut} {case}")
            changed = any(not torch.equal(_bits(got[k]), _bits(clean[k])) for k in clean if clean[k].dtype == torch.float32)
            if changed:
                applies += 1
                caught += bool(ck.bad)
                assert ck.bad, f"{mut} went unnoticed on {case}"
        print(f"{mut} / {family}: caught on {caught} of {applies} cases it changes")
        assert applies > 0, f"{mut} changes nothing in family {family}"


def test_reference_alone_satisfies_the_data_conditions():
    """What the mutation test needs from the data, checked on the reference for every distinct (family, shape) of all four tiles:
    EVERY reduction index carries a non-zero addend (no column of a, no row of b is all zero -- so the last k, the first k of the
    tail tile and any other are visible), the operands hold exact zeros and both signs, ragged-K and ragged-row cases exist in
    every family, no z is an exact zero, and the element whose gate is inverted changes dh unless the slope is 1 (slopes 0.2, 0
    and 1 all occur)."""
    slopes = set()
    for family in GR.FAMILIES:
        cases = {(c.tile, c.shape): c for c in _cases(family)}
        assert len(cases) == 32, len(cases)                      # eight kinds of shape on four tiles
        assert any(c.shape[2] % 32 for c in cases.values()) and any(c.shape[0] % GR.TILES[c.tile][0] for c in cases.values())
        for case in cases.values():
            cs = GR.data(case)
            M, C, R = case.shape
            a, b = (cs.dh, cs.w.double()) if family == "pro" else (cs.a.double(), cs.b.double())
            assert a.shape == (M, R) and b.shape == (R, C)
            assert bool((a != 0).any(0).all()), (case, "a column of a is all zero")
            assert bool((b != 0).any(1).all()), (case, "a row of b is all zero")
            if M * R >= 1000:
                assert bool((b == 0).any()) and bool((b > 0).any()) and bool((b < 0).any())
                assert family == "pro" or (bool((a == 0).any()) and bool((a > 0).any()) and bool((a < 0).any()))
            if family == "pro":
                slopes.add(cs.slope)
                i, k = cs.site
                assert cs.slope == 1.0 or (float(cs.dy[i, k]) != 0 and float(cs.coefs[2, k]) != 0)
                assert bool((GR.dh_ref(cs.dy, cs.h, cs.coefs, cs.slope)[2] != 0).all())
    assert slopes == set(NR.SLOPES)


def test_dispatch_of_the_case_table():
    """The restated run_gemm / launch_fast conditions give, for buffers on 16-byte boundaries, the mode and path every case
    names; every (family, tile) reaches modes 0 to 4, modes 1 to 4 at a shape whose extents alone allow mode 1."""
    for family in GR.FAMILIES:
        for tile in GR.TILES:
            modes, at_rag4 = set(), set()
            for case in GR.plan(family, tile):
                inst, path = GR.case_dispatch(case)
                assert (inst.MODE, path) == (case.mode, case.path), (case, inst, path)
                assert (inst.BM, inst.BN) == GR.TILES[tile]
                modes.add(inst.MODE)
                if case.kind.startswith("rag4"):
                    at_rag4.add(inst.MODE)
            assert modes == {0, 1, 2, 3, 4} and at_rag4 == {1, 2, 3, 4}, (family, tile, modes, at_rag4)
            assert {i.MODE for i in GR.expected_instantiations(family, tile)} == {0, 1, 2, 3, 4}


def test_dispatch_by_hand():
    """pick_tile, load_mode and dispatch against values worked out by hand from gemm.hip."""
    pt = GR.pick_tile
    assert [pt(1, 8, 5, t) for t in (1, 2, 3, 4)] == [(128, 128), (128, 64), (64, 64), (64, 128)]
    assert pt(256, 128, 32, 0) == (64, 64)            # 64 x 128 would leave 4 workgroups: 64-column tiles
    assert pt(256, 128, 32, 0, wide=1) == (64, 128)   # switch 11 keeps the wide tile
    assert pt(1, 8, 5, 0) == (64, 64) and pt(63, 20, 33, 0) == (64, 64)
    assert pt(132, 140, 36, 0) == (64, 128)           # 140 is no multiple of 64: the narrow-tile rule does not apply
    assert pt(32768, 256, 512, 0) == (128, 128) and pt(4096, 192, 100, 0) == (64, 64) and pt(65536, 64, 64, 0) == (128, 64)
    assert pt(100, 64, 64, 0) == (64, 64) and pt(49152, 128, 64, 0) == (128, 128)
    lm = GR.load_mode
    assert [lm(True, True, True), lm(False, True, True), lm(True, False, False), lm(True, True, False), lm(False, False, True)] == [0, 1, 2, 3, 4]
    d = GR.dispatch
    I = GR.Inst
    A = 1 << 20                                       # an aligned address
    # forward, whole 128 x 128 tiles: the in-loop split; option 3: the exact chain; a hint: the DMA ring, switch 13: registers
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A, 128) == (I(128, 128, 0, 0, 0, 0, 0, 2, 0, 0), "split")
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A, 128, exact=1) == (I(128, 128, 0, 0, 0, 0, 0, 0, 0, 0), "exact")
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A, 128, planes=True) == (I(128, 128, 0, 0, 0, 0, 0, 2, 1, 1), "planes_dma")
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A, 128, planes=True, a_regs=1) == (I(128, 128, 0, 0, 0, 0, 0, 2, 1, 0), "planes_regs")
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A, 128, planes=True, exact=1)[1] == "exact"
    # 64-column tiles: the exact chain without planes, the split with them
    assert d("bn", 128, 64, 32, 3, A, 32, A, 32, A, 64) == (I(64, 64, 0, 0, 0, 1, 0, 0, 0, 0), "exact")
    assert d("bn", 128, 64, 32, 3, A, 32, A, 32, A, 64, planes=True) == (I(64, 64, 0, 0, 0, 1, 0, 2, 1, 1), "planes_dma")
    # an output one float off: whole tiles are lost, 16-byte loads stay
    assert d("fwd", 256, 128, 96, 1, A, 96, A, 96, A + 4, 136) == (I(128, 128, 0, 0, 1, 0, 0, 0, 0, 0), "exact")
    # the input gradient: b4 looks at the output columns, not at the reduction length
    assert d("bwd", 63, 20, 33, 3, A, 33, A, 20, A, 20)[0].MODE == 4 and d("fwd", 63, 20, 33, 3, A, 33, A, 33, A, 20)[0].MODE == 2
    assert d("bwd", 132, 140, 36, 1, A, 36, A + 4, 148, A, 140)[0] == I(128, 128, 0, 1, 3, 0, 0, 0, 0, 0)
    assert d("bwd", 132, 140, 36, 1, A, 39, A, 140, A, 140)[0].MODE == 4 and d("bwd", 132, 140, 36, 1, A + 4, 44, A, 143, A, 140)[0].MODE == 2
    # the prologue: h and the coefficient rows enter; planes never take the DMA ring; the split loop is the simple one
    p = dict(ph=A, ldh=96, pcoef=A, ncoef=96)
    assert d("pro", 256, 128, 96, 1, A, 96, A, 128, A, 128, **p) == (I(128, 128, 0, 1, 0, 0, 1, 1, 0, 0), "split")
    assert d("pro", 256, 128, 96, 1, A, 96, A, 128, A, 128, **dict(p, pcoef=A + 4)) == (I(128, 128, 0, 1, 1, 0, 1, 0, 0, 0), "exact")
    assert d("pro", 256, 128, 96, 1, A, 96, A, 128, A, 128, **dict(p, ph=A + 4))[0].MODE == 4
    assert d("pro", 256, 128, 96, 1, A, 96, A, 128, A, 128, **dict(p, ldh=97))[0].MODE == 4
    assert d("pro", 256, 128, 96, 1, A, 96, A, 128, A, 128, planes=True, **p) == (I(128, 128, 0, 0, 0, 0, 1, 2, 1, 0), "planes_regs")
    # the combined store: the leading dimension and base of y [M, co] decide `whole`
    assert d("vn2", 256, 128, 32, 1, A, 32, A, 32, A, 64)[1] == "split" and d("vn2", 256, 128, 32, 1, A, 32, A, 32, A, 65)[0].MODE == 1
    assert GR.padded((132, 140, 36), 1) == (256, 256, 64) and GR.padded((60, 56, 68), 3) == (64, 64, 96)
    assert GR.forced_tile(256, 128, 32) == 3 and GR.forced_tile(132, 140, 36) == 4
