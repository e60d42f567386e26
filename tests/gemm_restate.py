"""An fp64 restatement, in plain torch, of the forward and input-gradient dense products of deltaconv_amd/csrc/gemm.hip
(gemm_kernel: every operand-load mode, tile, epilogue and the BatchNorm-backward prologue) with a per-element bound for every
output, the dispatch of run_gemm / launch_fast restated from the pointers and strides a call passes, the data and the case table,
and one driver per family that runs a call through a `backend` and holds each output with `Checks`.  No import of the package:
tests/test_gemm_restate_host.py passes fp32 emulations of the two multiply paths (and mutations of them), tests/test_gpu_gemm_abi.py
the C ABI on the device.  The statistics epilogues are held by the restatement and bounds of tests/nn_restate.py (dc_bn_stats,
dc_vn_stats), computed from the y the kernel stored.  The weight-gradient forms (A_KM, dc_gemm_tn*) are not covered; a family is a
driver `run_<family>` plus its rows in `plan()`, so they can be added in the same form.

The product, in its own terms: out[M, C] (+)= a[M, R] b[R, C], R the reduction length.
    dc_linear_forward            Y = X W^T:      a = X [M, K],  b = W^T (W [N, K] stored: B_NK),  C = N, R = K
    dc_linear_backward_input     dX (+)= dY W:   a = dY [M, N], b = W [N, K] as stored (B_KN),    C = K, R = N
    dc_linear_bn_backward_input  dX (+)= dh W,   dh = c_g dz + c_a h + c_b,  dz = dy (c_sc h + c_sh > 0 ? 1 : slope), the five
                                 coefficient rows taken as given in fp32 (gemm_split.h: bn_bwd_one)
    dc_linear_bn_stats_forward, dc_linear_vn_stats_forward (interleaved 0 / 1 / 2), dc_linear_{bn,vn}_sums_forward: the forward
                                 product with a statistics epilogue.

Bounds.  u = 2^-24; the fp32 inputs enter the fp64 reference exactly; S_ij = sum_k |a_ik| |b_kj| in fp64; g(n) = n u / (1 - n u)
(n roundings in a row, any order); O2 = 1 + 2^-20 as in tests/nn_restate.py.  No constant is fitted to an output.
  exact chain (v_mfma_f32_32x32x2_f32 = an fmaf chain from 0.f; every guarded mode, 64-column tiles, option 3 = 1): R fused
      multiply-adds, one rounding each, zeros from the guards add nothing:  |got - ref| <= g(R) S.
  accumulate: out = fl(base + t): one more rounding, u (|base + ref| + e_t), on top of the bound e_t of t.
  prologue: z = fmaf(c_sc, h, c_sh) is one correctly rounded operation on the given values, so its sign is the fp64 sign unless
      the exact z is 0 (the data keep z off exact zero, asserted; no element is excluded).  dh is formed by dz = dy * slope (one
      rounding, only where the gate is closed and slope != 1), t = fmaf(c_a, h, c_b), dh = fmaf(c_g, dz, t) (one each):
          e_dh = O2 u (|c_g dz| [closed, slope != 1] + |c_a h + c_b| + |dh|),
      carried through the product as E = sum_k e_dh_ik |w_kj|; the chain runs on the fp32 dh, |dh32| <= |dh| + e_dh:
          |got - ref| <= E + g(R) (S + E)          (S from |dh|; the split paths: their factor in place of g(R)).
  split products (whole tiles on 128-column tiles, pre-split weight planes on every tile): an operand is hi + mid + lo in bf16;
      the six kept partial products reproduce a b within 2^-22 |a b| = 4 u |a b| (tests/test_split_arithmetic.py); a product of
      two bf16 values is exact in fp32 and each v_mfma_f32_32x32x16_bf16 rounds ONCE per 16 products and accumulator, so an
      accumulator sees n = 6 R / 16 roundings, each of a partial sum of magnitude at most
      sum (|hi| + |mid| + |lo|)_a (|hi| + |mid| + |lo|)_b <= (1 + 2^-7)^2 S <= (1 + 2^-6) S:
          |got - ref| <= O2 (g(3 R / 8) (1 + 2^-6) + 4 u) S           -- (c R + 4) u S with c = 0.38.
      Limit: a deterministic bound of this kind cannot see the loss of a single third-order plane (lo.hi or hi.lo weigh 2^-16 of
      a product, 256 u, below g(3 R / 8) from R = 700 on and never far above it); that loss stays guarded by the rule
      `split error <= 1.5 x exact chain's + 1e-7` at the large shapes of tests/test_gpu_gemm.py, which is neither weakened nor
      repeated here.
  combined store (interleaved = 2): y_u = P_u - Q_v, y_v = P_v + Q_u of the fp32 (P, Q): the bounds of the two products plus
      one rounding u (|y| + e_P + e_Q), as dc_vn_apply's combination is held in tests/nn_restate.py.
  statistics: tests/nn_restate.py stats_ref / vn_stats_ref on the stored output (interleaved 1: combine 2 of the stored PQ;
      interleaved 0 and 2: combine 0 of the stored y -- the kernel takes its norms from the same floats it stores).

Reduction order of the exact chain (gemm.hip:15-27, read_piece / mfma_one): K tiles of 32 in order; inside a tile fragment set
j = 0..3, step t = 0..3, the pair k = 8 j + t then 8 j + 4 + t.  Nothing in it depends on BM or BN, the guarded loads fetch the
same floats (zeros beyond the extents, which add fma(0, 0, acc) = acc as acc is never -0.f: it starts at +0.f and a sum that
cancels gives +0.f), so on the exact chain every layout, every tile and the zero-padded problem return the same bits.

Dispatch (run_gemm, gemm.hip:1171-1203; launch_fast, gemm.hip:1077-1104), `dispatch()` below:
    whole = M % bm == 0, C % bn == 0, R % 32 == 0, ldc % 4 == 0, out 16-byte aligned (prologue: coefs aligned, ncoef % 4 == 0)
    a4 = R % 4 == 0, lda % 4 == 0, a aligned (prologue: ldh % 4 == 0, h aligned);  b4 = (B_NK: R, B_KN: C) % 4 == 0, ldb % 4 == 0, b aligned
    mode = 0 if whole and a4 and b4, else 1 (a4, b4), 3 (a4), 4 (b4), 2
    planes (a hint for this weight, C % 32 == 0, R % 16 == 0, mode 0 whatever b4, options 3 and 9 off): the forward form over the
    planes, X3 = 2, BP = 1, through the DMA ring unless prologue or option 13; else mode 0 and bn == 128 (option 3 = 0): the
    in-loop split (X3 = 2, prologue 1); else the exact chain in `mode`.

Data: operands normal x 2^(-6 .. 6) per element, both signs, about one element in 17 an exact zero at random places, no column of
a and no row of b all zero (every reduction index carries weight; asserted); prologue: dy / h / coefficients
from the RowCase of tests/nn_restate.py (gamma of both signs, column scales 1e-3 .. 1e3; at least 16 rows, of which a tiny
shape takes the first), slopes 0.2 / 0 / 1, and the weight
row k scaled by 1 / rms(dh[:, k]) so that every k carries weight in the sums (a dropped k is visible whichever it is)."""
import collections
import functools

import torch

from tests import nn_restate as NR
from tests.apply_cases import Checks  # noqa: F401  (the drivers take one)

U, O2 = NR.U, NR.O2
B_NK, B_KN = 0, 1
EPI_NONE, EPI_COLSTATS, EPI_VNSTATS, EPI_VNSTATS0 = 0, 1, 2, 3
TILES = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (64, 128)}
SENT = 12345.0

# family -> (B layout, EPI, PRO, accumulate forms, interleaved)
FAMILIES = collections.OrderedDict([
    ("fwd", (B_NK, EPI_NONE, 0)), ("bwd", (B_KN, EPI_NONE, 0)), ("pro", (B_KN, EPI_NONE, 1)), ("bn", (B_NK, EPI_COLSTATS, 0)),
    ("vn0", (B_NK, EPI_VNSTATS0, 0)), ("vn1", (B_NK, EPI_VNSTATS, 0)), ("vn2", (B_NK, EPI_VNSTATS, 0))])


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def g(n):
    return n * U / (1.0 - n * U)


def path_factor(R, path):
    """e <= path_factor S."""
    if path == "exact":
        return g(R)
    return O2 * (g(6 * R / 16) * (1 + 2.0 ** -6) + 4 * U)


def acc_bound(total, e):
    return e + U * (total.abs() + e)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def pick_tile(M, N, K, tile, wide=0):
    """gemm.hip: pick_tile -> (bm, bn)."""
    if tile in TILES:
        return TILES[tile]
    bn = 128 if N > 64 else 64
    if N % 128 != 0 and N % 64 == 0:
        bn = 64
    tn = cdiv(N, bn)
    bm = 128 if cdiv(M, 128) * tn >= 384 else 64
    if M % bm != 0 and M % 64 == 0:
        bm = 64
    if bm == 64 and bn == 128 and N % 64 == 0 and cdiv(M, 64) * tn < 256 and wide == 0:
        bn = 64
    return bm, bn


def forced_tile(M, N, K, wide=0):
    """The `tile` argument that forces what tile = 0 picks."""
    return {v: k for k, v in TILES.items()}[pick_tile(M, N, K, 0, wide)]


def load_mode(whole, a4, b4):
    if whole and a4 and b4:
        return 0
    return 1 if a4 and b4 else (3 if a4 else (4 if b4 else 2))


Inst = collections.namedtuple("Inst", "BM BN AL BL MODE EPI PRO X3 BP DMA")


def dispatch(family, M, C, R, tile, pa, lda, pb, ldb, pc, ldc, ph=0, ldh=0, pcoef=0, ncoef=0, planes=False, exact=0, a_regs=0,
             no_planes=0, wide=0):
    """The instantiation run_gemm launches for a product out[M, C] = a[M, R] b (addresses in bytes, strides in elements) and
    the name of its multiply path."""
    bl, epi, pro = FAMILIES[family]
    bm, bn = pick_tile(M, C, R, tile, wide)
    al16 = lambda p: p % 16 == 0
    whole = M % bm == 0 and C % bn == 0 and R % 32 == 0 and ldc % 4 == 0 and al16(pc)
    a4 = R % 4 == 0 and lda % 4 == 0 and al16(pa)
    b4 = (R if bl == B_NK else C) % 4 == 0 and ldb % 4 == 0 and al16(pb)
    if pro:
        a4 = a4 and ldh % 4 == 0 and al16(ph)
        whole = whole and al16(pcoef) and ncoef % 4 == 0
    if planes and C % 32 == 0 and R % 16 == 0 and load_mode(whole, a4, True) == 0 and exact == 0 and no_planes == 0:
        dma = 1 if (not pro and a_regs == 0) else 0
        return Inst(bm, bn, 0, B_NK, 0, epi, pro, 2, 1, dma), "planes_dma" if dma else "planes_regs"
    mode = load_mode(whole, a4, b4)
    if mode == 0 and (exact == 2 or (exact == 0 and bn == 128)):
        return Inst(bm, bn, 0, bl, 0, epi, pro, 1 if pro else 2, 0, 0), "split"
    return Inst(bm, bn, 0, bl, mode, epi, pro, 0, 0, 0), "exact"


# ---- layouts and the case table ---------------------------------------------------------------------------------------------------
# an operand [rows, w] is a column block of a [rows + 1, ld] buffer whose base is 16-byte aligned: name -> (ld(w), first column)
OPERAND = {
    "c": (lambda w: w, 0),                           # contiguous
    "p": (lambda w: w + 8, 4),                       # 4 columns in, ld a multiple of 4 where w is: 16-byte accesses remain possible
    "o": (lambda w: w + 8, 1),                       # 1 column in: an unaligned base
    "d": (lambda w: (w | 1) + 2, 0),                 # an odd leading dimension
}
# a layout = the operand layouts of (a, b, out); h follows a; 'k': the coefficient rows start one float off a 16-byte boundary
LAYOUTS = {"ccc": "ccc", "ppp": "ppp", "pcp": "pcp", "cco": "cco", "su": "odc", "vs": "pop", "sv": "dpo", "cck": "ccc"}
# the mode a layout gives where the extents alone allow mode 0 ("whole") or mode 1 ("rag4")
MODE_OF = {"whole": {"ccc": 0, "ppp": 0, "pcp": 0, "cco": 1, "cck": 1, "su": 2, "vs": 3, "sv": 4},
           "rag4": {"ccc": 1, "ppp": 1, "su": 2, "vs": 3, "sv": 4}}
Case = collections.namedtuple("Case", "family tile kind shape layout opt mode path")


def shapes(tile, family):
    """kind -> (M, C, R): the smallest shapes at which each path of a forced tile can go wrong.  Vector families: even rows,
    interleaved columns even."""
    bm, bn = TILES[tile]
    vec = family.startswith("vn")
    il = family in ("vn1", "vn2")
    return collections.OrderedDict([
        ("whole32", (2 * bm, bn, 32)), ("whole96", (2 * bm, bn, 96)),                 # two row tiles: two chunks of partials
        ("rag4a", (bm + 4, bn + 12, 36)), ("rag4b", (bm - 4, bn - 8, 68)),            # ragged, every extent a multiple of 4
        ("odd", (bm + (2 if vec else 1), bn + (6 if il else 3), 35)),                  # odd R: dword loads whatever the layout
        ("tiny1", (2 if vec else 1, 8, 5)), ("tiny2", (2, 16, 32)), ("tiny3", (62 if vec else 63, 20, 33))])


def _whole_path(family, tile, opt):
    pro = FAMILIES[family][2]
    if opt.startswith("planes"):
        return "planes_regs" if (pro or opt == "planes_regs") else "planes_dma"
    return "split" if (opt == "default" and TILES[tile][1] == 128) else "exact"


def plan(family, tile):
    """The cases of one (family, forced tile), each naming the mode and path it must reach."""
    bl, _, pro = FAMILIES[family]
    out = []
    for kind, shp in shapes(tile, family).items():
        if kind.startswith("whole"):
            rows = [("ccc", "default"), ("ccc", "exact"), ("ccc", "planes_dma"), ("cco", "default")] if kind == "whole32" else \
                   [("ccc", "default"), ("ppp", "default"), ("ccc", "exact"), ("pcp", "planes_dma")]
            rows += [("ccc" if kind == "whole32" else "pcp", "planes_regs")] if not pro else []
            rows += [("cck", "default")] if pro and kind == "whole96" else []
            for lay, opt in rows:
                mode = MODE_OF["whole"][lay]
                out.append(Case(family, tile, kind, shp, lay, opt, mode, _whole_path(family, tile, opt) if mode == 0 else "exact"))
        elif kind.startswith("rag4"):
            for lay in ("ccc", "ppp", "su", "vs", "sv") if kind == "rag4a" else ("ccc", "su", "vs", "sv"):
                out.append(Case(family, tile, kind, shp, lay, "default", MODE_OF["rag4"][lay], "exact"))
        elif kind == "odd":
            for lay in ("ccc", "su"):
                out.append(Case(family, tile, kind, shp, lay, "default", 2, "exact"))
        else:
            # tiny, contiguous: R = 5 and 33 leave dword loads for a and a K-contiguous b; a reduction-major b [R, C] keeps its
            # 16-byte loads along C (8 and 20 are multiples of 4): mode 4.  (2, 16, 32): ragged rows only: mode 1.
            mode = 1 if kind == "tiny2" else (4 if bl == B_KN else 2)
            out.append(Case(family, tile, kind, shp, "ccc", "default", mode, "exact"))
    return out


def expected_instantiations(family, tile):
    bl, epi, pro = FAMILIES[family]
    bm, bn = TILES[tile]
    out = set()
    for c in plan(family, tile):
        if c.path.startswith("planes"):
            out.add(Inst(bm, bn, 0, B_NK, 0, epi, pro, 2, 1, 1 if c.path == "planes_dma" else 0))
        elif c.path == "split":
            out.add(Inst(bm, bn, 0, bl, 0, epi, pro, 1 if pro else 2, 0, 0))
        else:
            out.add(Inst(bm, bn, 0, bl, c.mode, epi, pro, 0, 0, 0))
    return out


def geometry(case):
    """operand -> (rows, width, leading dimension, first column) of the buffers of a case; h has the geometry of a."""
    M, C, R = case.shape
    la, lb, lc = LAYOUTS[case.layout]
    dims = {"a": (M, R, la), "b": ((C, R, lb) if FAMILIES[case.family][0] == B_NK else (R, C, lb)),
            "out": (M, C // 2 if case.family == "vn2" else C, lc)}
    return {k: (rows, w, OPERAND[l][0](w), OPERAND[l][1]) for k, (rows, w, l) in dims.items()}


OPTIONS = {"default": dict(), "exact": dict(exact=1), "planes_dma": dict(planes=True), "planes_regs": dict(planes=True, a_regs=1)}


def case_dispatch(case, ptr=None, tile=None):
    """dispatch() of a case; ptr: operand -> address of its first element (default: buffers on 16-byte boundaries)."""
    geo = geometry(case)
    ptr = ptr or {k: 4096 + 4 * off for k, (_, _, _, off) in geo.items()}
    M, C, R = case.shape
    kw = dict(OPTIONS[case.opt])
    if FAMILIES[case.family][2]:
        kw.update(ph=ptr.get("h", ptr["a"]), ldh=geo["a"][2], pcoef=ptr.get("coefs", 4096 + (4 if case.layout == "cck" else 0)), ncoef=R)
    return dispatch(case.family, M, C, R, case.tile if tile is None else tile, ptr["a"], geo["a"][2], ptr["b"], geo["b"][2],
                    ptr["out"], geo["out"][2], **kw)


def padded(shape, tile):
    bm, bn = TILES[tile]
    M, C, R = shape
    return cdiv(M, bm) * bm, cdiv(C, bn) * bn, cdiv(R, 32) * 32


# ---- data ---------------------------------------------------------------------------------------------------------------------
def binades(shape, seed, live=None):
    """Normal values x 2^(-6 .. 6), about one element in 17 an exact zero at random places (a fixed stride would line up with a
    row length: 68 = 4 x 17).  live = 0 / 1: no column / no row is left all zero, so that every reduction index carries weight."""
    gen = torch.Generator().manual_seed(seed)
    x0 = (torch.randn(*shape, generator=gen) * torch.exp2(torch.randint(-6, 7, shape, generator=gen).float())).float()
    x = torch.where(torch.rand(*shape, generator=gen) < 1.0 / 17, torch.zeros(()), x0)
    if live is not None:
        dead = (x != 0).sum(live, keepdim=True) == 0
        x = torch.where(dead, x0, x)
        assert bool(((x != 0).sum(live) > 0).all())
    return x


def pad_to(t, rows, cols):
    out = torch.zeros(rows, cols, dtype=t.dtype)
    out[:t.shape[0], :t.shape[1]] = t
    return out


class Prod:
    """out[M, C] (+)= a[M, R] b[R, C] with the fp64 product and S; b is what dc_linear_backward_input takes as W [N = R, K = C],
    its transpose what dc_linear_forward takes as W [N = C, K = R]."""

    def __init__(self, M, C, R):
        self.M, self.C, self.R = M, C, R
        seed = 7919 * M + 31 * C + R
        self.a, self.b, self.base = binades((M, R), seed, live=0), binades((R, C), seed + 1, live=1), binades((M, C), seed + 2)
        self.bt = self.b.t().contiguous()
        self.ref = self.a.double() @ self.b.double()
        self.S = self.a.double().abs() @ self.b.double().abs()
        co = C // 2 if C % 2 == 0 else C
        self.affine = {c: NR.affine(c) for c in {C, co}}
        gen = torch.Generator().manual_seed(seed + 3)
        self.rm0 = torch.randn(C, generator=gen)
        self.rv0 = torch.rand(C, generator=gen) + 0.5

    def zero_padded(self, Mp, Cp, Rp):
        p = Prod.__new__(Prod)
        p.M, p.C, p.R = Mp, Cp, Rp
        p.a, p.b, p.base = pad_to(self.a, Mp, Rp), pad_to(self.b, Rp, Cp), pad_to(self.base, Mp, Cp)
        p.bt = p.b.t().contiguous()
        p.affine = {c: NR.affine(c) for c in {Cp, Cp // 2}}
        p.rm0, p.rv0 = torch.zeros(Cp), torch.ones(Cp)
        return p


@functools.lru_cache(maxsize=None)
def prod(M, C, R):
    return Prod(M, C, R)


def dh_ref(dy, h, coefs, slope):
    """-> (dh, e_dh, z) in fp64 from the fp32 operands and the five fp32 coefficient rows."""
    dy, h, cf = dy.double(), h.double(), coefs.double()
    z = cf[0] * h + cf[1]
    closed = z <= 0
    dz = torch.where(closed, slope * dy, dy)
    t = cf[3] * h + cf[4]
    dh = cf[2] * dz + t
    e = O2 * U * ((cf[2] * dz).abs() * (closed & (slope != 1.0)).double() + t.abs() + dh.abs())
    return dh, e, z


class Pro:
    """dX[M, C] (+)= dh[M, R] w[R, C]: dy, h, gamma and the batch statistics of a RowCase; the coefficient rows are the fp64 values
    of tests/nn_restate.py bwd_ref rounded to fp32 and then taken as given."""

    def __init__(self, M, C, R, slope):
        self.M, self.C, self.R, self.slope = M, C, R, slope
        # (BatchNorm backward over one or two rows is identically zero -- dh would be the cancellation noise of its coefficients:
        #  the tiny shapes take the first rows of a 16-row case together with that case's coefficients)
        rc = NR.row_case(max(M, 16), R)
        self.dy, self.h = rc.dy[:M].contiguous(), rc.x[:M].contiguous()
        ref = NR.bwd_ref(rc.x, rc.dy.double(), rc.tr, rc.gamma, slope, 1, 1, 1)
        self.coefs = torch.stack([rc.tr["scale"], rc.tr["shift"], ref["c_g"][0], ref["c_a"][0], ref["c_b"][0]]).float().contiguous()
        self.dh, self.e_dh, z = dh_ref(self.dy, self.h, self.coefs, slope)
        assert bool((z != 0).all()), "an exact z of 0: the gate is undecided"
        assert bool((self.dh != 0).any(0).all()), "a column of dh is all zero"
        rms = self.dh.pow(2).mean(0).sqrt().clamp_min(1e-30)
        seed = 104729 + 7919 * M + 31 * C + R
        self.w = (binades((R, C), seed, live=1).double() / rms[:, None]).float()
        self.base = (binades((M, C), seed + 1) * 4.0).float()
        self.ref = self.dh @ self.w.double()
        self.S = self.dh.abs() @ self.w.double().abs()
        self.E = self.e_dh @ self.w.double().abs()
        # the element whose gate a mutation inverts: the largest change of dh relative to its column
        self.site = divmod(int(((self.coefs[2].double() * self.dy.double()).abs() / rms).argmax()), R)

    def zero_padded(self, Mp, Cp, Rp):
        p = Pro.__new__(Pro)
        p.M, p.C, p.R, p.slope = Mp, Cp, Rp, self.slope
        p.dy, p.h, p.coefs = pad_to(self.dy, Mp, Rp), pad_to(self.h, Mp, Rp), pad_to(self.coefs, 5, Rp)
        p.w, p.base = pad_to(self.w, Rp, Cp), pad_to(self.base, Mp, Cp)
        return p


def slope_of(shape):
    return NR.SLOPES[sum(shape) % 3]


@functools.lru_cache(maxsize=None)
def pro(M, C, R):
    return Pro(M, C, R, slope_of((M, C, R)))


def data(case):
    return pro(*case.shape) if case.family == "pro" else prod(*case.shape)


# ---- drivers: one per family.  A backend takes and returns CPU fp32 tensors of the logical shapes; after a call `be.path` names
# the multiply path the call took ("exact" | "split" | "planes_regs" | "planes_dma").
def _hold_product(ck, tag, be, got, ref, S, R, E=None):
    f = path_factor(R, be.path)
    e = f * S if E is None else E + f * (S + E)
    ck.hold(f"{tag} [{be.path}]", got, ref, e)
    ck.true(f"{tag}: no NaN in the output", not bool(torch.isnan(got).any()))
    return e


def run_fwd(be, cs, ck):
    y = be.forward(cs.a, cs.bt)
    _hold_product(ck, "dc_linear_forward", be, y, cs.ref, cs.S, cs.R)
    return {"y": y}


def run_bwd(be, cs, ck):
    plain = be.backward_input(cs.a, cs.b, None)
    e = _hold_product(ck, "dc_linear_backward_input accumulate 0", be, plain, cs.ref, cs.S, cs.R)
    acc = be.backward_input(cs.a, cs.b, cs.base)
    total = cs.ref + cs.base.double()
    ck.hold(f"dc_linear_backward_input accumulate 1 [{be.path}]", acc, total, acc_bound(total, e))
    ck.exact("accumulate 1 = base + accumulate 0", acc, cs.base + plain)
    return {"dx": plain, "dx acc": acc}


def run_pro(be, cs, ck):
    plain = be.bn_backward_input(cs.dy, cs.h, cs.coefs, cs.slope, cs.w, None)
    tag = f"dc_linear_bn_backward_input slope {cs.slope:.1f}"
    e = _hold_product(ck, tag + " accumulate 0", be, plain, cs.ref, cs.S, cs.R, cs.E)
    acc = be.bn_backward_input(cs.dy, cs.h, cs.coefs, cs.slope, cs.w, cs.base)
    total = cs.ref + cs.base.double()
    ck.hold(f"{tag} accumulate 1 [{be.path}]", acc, total, acc_bound(total, e))
    ck.exact("accumulate 1 = base + accumulate 0", acc, cs.base + plain)
    return {"dx": plain, "dx acc": acc}


def _running(cs, c, plain):
    if plain:
        return None, None, None, None, 1.0
    gamma, beta = cs.affine[c]
    return gamma, beta, cs.rm0[:c].contiguous(), cs.rv0[:c].contiguous(), NR.MOM


def run_bn(be, cs, ck, plain=False):
    gamma, beta, rm0, rv0, mom = _running(cs, cs.C, plain)
    y, co = be.bn_stats(cs.a, cs.bt, gamma, beta, mom, rm0, rv0)
    _hold_product(ck, "dc_linear_bn_stats_forward y", be, y, cs.ref, cs.S, cs.R)
    NR.check_coef(ck, "dc_linear_bn_stats_forward", co, NR.stats_ref(y, gamma, beta, mom, rm0, rv0))
    out = {"y": y, **{k: v for k, v in co.items() if v is not None}}
    if hasattr(be, "bn_sums"):
        y2 = be.bn_sums(cs.a, cs.bt)
        ck.exact("dc_linear_bn_sums_forward y = the statistics form's", y2, y)
    return out


def run_vn(be, cs, ck, interleaved, plain=False):
    co = cs.C // 2 if interleaved else cs.C
    gamma, beta, rm0, rv0, mom = _running(cs, co, plain)
    name = f"dc_linear_vn_stats_forward interleaved {interleaved}"
    got, coef = be.vn_stats(cs.a, cs.bt, co, interleaved, gamma, beta, mom, rm0, rv0)
    f = path_factor(cs.R, be.path)
    e = f * cs.S
    if interleaved == 2:
        yu, yv = NR.vn_y(cs.ref, co, 2)
        bu, bv = e[0::2, 0::2] + e[1::2, 1::2], e[1::2, 0::2] + e[0::2, 1::2]
        il = lambda p, q: torch.stack([p, q], 1).reshape(2 * p.shape[0], co)
        ref, bound = il(yu, yv), il(bu, bv)
        ck.hold(f"{name} y [{be.path}]", got, ref, bound + U * (ref.abs() + bound))
    else:
        ck.hold(f"{name} product [{be.path}]", got, cs.ref, e)
    ck.true(f"{name}: no NaN in the output", not bool(torch.isnan(got).any()))
    NR.check_coef(ck, name, coef, NR.vn_stats_ref(got, co, 2 if interleaved == 1 else 0, gamma, beta, mom, rm0, rv0))
    out = {"out": got, **{k: v for k, v in coef.items() if v is not None}}
    if hasattr(be, "vn_sums"):
        ck.exact(f"dc_linear_vn_sums_forward interleaved {interleaved}: output = the statistics form's", be.vn_sums(cs.a, cs.bt, co, interleaved), got)
    return out


PRODUCT_KEYS = ("y", "dx", "dx acc", "out")         # the product outputs among the results of a driver


def raw_outputs(be, case, cs):
    """The calls of a case without reference and checks (statistics in the plain form) -> {name: raw result}: bit comparisons."""
    fam = case.family
    if fam == "fwd":
        return {"y": be.forward(cs.a, cs.bt)}
    if fam == "bwd":
        return {"dx": be.backward_input(cs.a, cs.b, None), "dx acc": be.backward_input(cs.a, cs.b, cs.base)}
    if fam == "pro":
        return {"dx": be.bn_backward_input(cs.dy, cs.h, cs.coefs, cs.slope, cs.w, None),
                "dx acc": be.bn_backward_input(cs.dy, cs.h, cs.coefs, cs.slope, cs.w, cs.base)}
    if fam == "bn":
        y, co = be.bn_stats(cs.a, cs.bt, None, None, 1.0, None, None)
        return {"y": y, **{k: v for k, v in co.items() if v is not None}}
    il = int(fam[2])
    out, co = be.vn_stats(cs.a, cs.bt, cs.C // 2 if il else cs.C, il, None, None, 1.0, None, None)
    return {"out": out, **{k: v for k, v in co.items() if v is not None}}


def run_case(be, case, ck, cs=None):
    """One case of the table through the backend -> {name: raw result}."""
    cs = data(case) if cs is None else cs
    plain = case.kind.startswith("tiny")             # the tiny shapes take the form without affine parameters and running pair
    fam = case.family
    if fam == "fwd":
        return run_fwd(be, cs, ck)
    if fam == "bwd":
        return run_bwd(be, cs, ck)
    if fam == "pro":
        return run_pro(be, cs, ck)
    if fam == "bn":
        return run_bn(be, cs, ck, plain)
    return run_vn(be, cs, ck, int(fam[2]), plain)
