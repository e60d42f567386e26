"""The CPU build of deltaconv_amd/csrc/ell_math.h (tests/hostcheck) at the vector widths V = 1, 2 and 4 against the fp64
restatement of tests/apply_restate.py, on the data and with the checks of tests/apply_cases.py that
tests/test_gpu_apply_abi.py applies to the device: every output element within its derived bound, and the three widths
bit-identical (the bodies are written per channel with explicit fma: V must not change a chain).  Runs without a GPU: the
proof that the bounds hold for the reference arithmetic itself.  The CSC arrays come from the host twin of dc_csc_build."""
import pytest
import torch

from tests.apply_cases import Checks, case, run, same_bits
from tests.test_hostcheck_ell import hc, P          # noqa: F401  (hc: the module fixture that builds and binds libhostcheck.so)

OPS = {"grad": 0, "div": 1, "div_curl_norm": 2, "hodge": 3}
IN_MULT = {"grad": 1, "div": 1, "div_curl_norm": 1, "hodge": 2}           # row widths in units of C
OUT_MULT = {"grad": 1, "div": 1, "div_curl_norm": 3, "hodge": 1}
OUT_ROWS = {"grad": 2, "div": 1, "div_curl_norm": 1, "hodge": 2}          # rows in units of n


class HostBackend:
    """Contiguous tensors, one vector width for every body (the aggregations exist at 4 and 1: 2 runs their scalar form)."""
    max_T_variants = (0,)

    def __init__(self, lib, cs, v):
        self.lib, self.cs, self.V, self.VA = lib, cs, v, (4 if v == 4 else 1)
        self.n, self.k, self.C = cs.n, cs.k, cs.C
        self.nbr32 = cs.nbr.to(torch.int32).contiguous()
        self.tptr = torch.zeros(self.n + 1, dtype=torch.int32)
        self.tedge = torch.zeros(self.n * self.k, dtype=torch.int32)
        lib.hc_csc_build(P(self.nbr32), self.n, self.k, P(self.tptr), P(self.tedge))

    def _coef(self, op):
        return (self.cs.G if op in ("grad", "hodge") else self.cs.D).contiguous()

    def fwd(self, op, x):
        c = self.C
        out = torch.full((OUT_ROWS[op] * self.n, OUT_MULT[op] * c), float("nan"))
        self.lib.hc_ell_fwd(OPS[op], self.V, P(self._coef(op)), P(self.nbr32), self.n, self.k, P(x.contiguous()), c, IN_MULT[op] * c, P(out),
                            OUT_MULT[op] * c)
        return out

    def T(self, op, dy, prev, v=None):
        c = self.C
        rows, mult = {"grad": (1, 1), "div": (2, 1), "div_curl_norm": (2, 1), "hodge": (1, 2)}[op]
        out = prev.clone() if prev is not None else torch.full((rows * self.n, mult * c), float("nan"))
        self.lib.hc_ell_T(OPS[op], self.V, P(self._coef(op)), P(self.tptr), P(self.tedge), self.n, self.k, P(dy.contiguous()), c, dy.shape[1],
                          P(out), mult * c, int(prev is not None), P(v), c if v is not None else 0)
        return out

    def grad_T_sum(self, dy, a, b):
        c = self.C
        out = torch.full((self.n, c), float("nan"))
        self.lib.hc_grad_T_sum(self.V, P(self.cs.G.contiguous()), P(self.tptr), P(self.tedge), self.n, self.k, P(dy), c, c, P(a), c, P(b),
                               c if b is not None else 0, P(out), c)
        return out

    def knn_sum(self, h, scale):
        out = torch.full((self.n, self.C), float("nan"))
        self.lib.hc_knn_sum(self.VA, P(self.nbr32), self.n, self.k, P(h), self.C, self.C, scale, P(out), self.C)
        return out

    def knn_sum_T(self, dout, scale, prev):
        out = prev.clone() if prev is not None else torch.full((self.n, self.C), float("nan"))
        self.lib.hc_knn_sum_bwd(self.VA, P(self.tptr), P(self.tedge), self.n, self.k, P(dout), self.C, self.C, scale, P(out), self.C,
                                int(prev is not None))
        return out

    def knn_max(self, h):
        out, arg = torch.full((self.n, self.C), float("nan")), torch.full((self.n, self.C), 255, dtype=torch.uint8)
        self.lib.hc_knn_max(self.VA, P(self.nbr32), self.n, self.k, P(h), self.C, self.C, P(out), self.C, P(arg))
        return out, arg

    def knn_max_affine(self, h, scale, shift, slope):
        out, arg = torch.full((self.n, self.C), float("nan")), torch.full((self.n, self.C), 255, dtype=torch.uint8)
        self.lib.hc_knn_max_affine(self.VA, P(self.nbr32), self.n, self.k, P(h), self.C, self.C, P(scale), P(shift), slope, P(out), self.C, P(arg))
        return out, arg

    def knn_max_affine_residual(self, h, scale, shift, slope, h2, scale2, shift2, slope2):
        out, out2 = torch.full((self.n, self.C), float("nan")), torch.full((self.n, self.C), float("nan"))
        arg = torch.full((self.n, self.C), 255, dtype=torch.uint8)
        self.lib.hc_knn_max_affine_residual(self.VA, P(self.nbr32), self.n, self.k, P(h), self.C, self.C, P(scale), P(shift), slope, P(h2), self.C,
                                            P(scale2), P(shift2), slope2, P(out), self.C, P(out2), self.C, P(arg))
        return out, out2, arg

    def knn_max_T(self, arg, dout, prev, variant):
        out = prev.clone() if prev is not None else torch.full((self.n, self.C), float("nan"))
        self.lib.hc_knn_max_bwd(self.VA, P(self.tptr), P(self.tedge), self.n, self.k, P(arg), P(dout), self.C, self.C, P(out), self.C,
                                int(prev is not None))
        return out


@pytest.mark.parametrize("name,c", [("base", 64), ("base", 8), ("base", 6), ("base", 7), ("k1", 64), ("k1", 6), ("k7", 64), ("k7", 6),
                                    ("k64", 64), ("k64", 6), ("hub", 64), ("hub", 6)])
def test_widths_hold_the_bounds_and_agree(hc, name, c):
    cs = case(name, c)
    if name == "hub":
        assert int(torch.bincount(cs.nbr.reshape(-1)).max()) > 2048          # columns longer than one staged chunk of the device
    ck = Checks(f"host {name} C {c}")
    res = {}
    for v in (1, 2, 4):
        if c % v == 0:
            ck.what = f"host {name} C {c} V {v}"
            res[v] = run(HostBackend(hc, cs, v), cs, ck)
    ck.what = f"host {name} C {c}"
    for v in res:
        if v != 1:
            same_bits(ck, f"V {v} = V 1", res[v], res[1])
    ck.done()
