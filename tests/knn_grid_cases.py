"""The case list of the exact grid search (csrc/knn_grid_math.h, csrc/knn_grid.hip), shared by the host tests
(tests/test_knn_grid_host.py) and the GPU tests (tests/test_gpu_knn_grid.py): the smallest shapes at which each mechanism of the
search can fail.  Every case is built once (fixed seeds) and must not be modified by a test.

    SELF[name]()  -> (pos fp32 [N,3] torch CPU, sizes: the cloud sizes, k)
    CROSS[name]() -> (query [Nq,3], qsizes, ref [Nr,3], rsizes, k)
    TARGETS       the grid shapes every case runs at: the default, one cell (1e9), the cell cap (0.25)
"""
import functools

import numpy as np
import torch

from deltaconv_amd.data import synthetic_batch

TARGETS = (None, 1e9, 0.25)


def _surface(sizes, seed, **kw):
    if isinstance(sizes, tuple):
        b = synthetic_batch(sizes[0], sizes[1], seed=seed, **kw)
        sizes = [sizes[1]] * sizes[0]
    else:
        b = synthetic_batch(len(sizes), 0, seed=seed, sizes=sizes, **kw)
    return b.pos.float().contiguous(), list(sizes)


def _ties(n, k, dups):
    """The construction of test_knn_massive_ties (tests/test_gpu_geometry.py): `dups` coincident points per cloud."""
    g = torch.Generator().manual_seed(5)
    pos = torch.randn(2 * n, 3, generator=g)
    for c in range(2):
        idx = torch.randperm(n, generator=g)[:dups] + c * n
        pos[idx] = pos[idx[0]].clone()
    return pos, [n, n], k


def _lattice(k):
    a = torch.arange(10, dtype=torch.float32) * 0.125                           # points exactly on cell faces, hundreds of ties
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3).contiguous(), [1000], k


def _shifted():
    pos, sizes = _surface((1, 1000), 7)
    return pos + 4096.0, sizes, 20                                              # ulp 2^-11 .. 2^-12: coarse quantisation of (p - lo)


def _flat_z():
    pos, sizes = _surface((1, 600), 8)
    pos = pos.clone()
    pos[:, 2] = 0.25
    return pos, sizes, 20


def _line_x():
    g = torch.Generator().manual_seed(9)
    pos = torch.zeros(500, 3)
    pos[:, 0] = torch.rand(500, generator=g)
    pos[:, 1], pos[:, 2] = -1.5, 3.0
    return pos, [500], 16


def _coincident():
    return torch.full((100, 3), 0.375), [100], 16


def _clumps():
    g = torch.Generator().manual_seed(10)
    a = torch.randn(300, 3, generator=g) * 0.1
    b = torch.randn(300, 3, generator=g) * 0.1 + torch.tensor([1000.0, 0.0, 0.0])
    far = torch.tensor([[500.0, 800.0, -700.0]])                                # every neighbour of this one is far away
    return torch.cat([a, far, b], 0).contiguous(), [601], 10


def _case(fn):
    return functools.lru_cache(maxsize=None)(fn)


SELF = {
    "ragged_64_1000_257_k20": _case(lambda: _surface([64, 1000, 257], 32) + (20,)),
    "one_5000_k16": _case(lambda: _surface((1, 5000), 31) + (16,)),
    "whole_2x100_k64": _case(lambda: _surface((2, 100), 31) + (64,)),
    "whole_2x40_k40": _case(lambda: _surface((2, 40), 31) + (40,)),
    "ties_1024_k20_200": _case(lambda: _ties(1024, 20, 200)),
    "ties_700_k30_700": _case(lambda: _ties(700, 30, 700)),
    "ties_4096_k10_300": _case(lambda: _ties(4096, 10, 300)),
    "ties_130_k40_100": _case(lambda: _ties(130, 40, 100)),
    "lattice_k1": _case(lambda: _lattice(1)),
    "lattice_k20": _case(lambda: _lattice(20)),
    "lattice_k64": _case(lambda: _lattice(64)),
    "shifted_4096": _case(_shifted),
    "flat_z": _case(_flat_z),
    "line_x": _case(_line_x),
    "coincident_100": _case(_coincident),
    "clumps_and_outlier": _case(_clumps),
}


def _outside(k):
    g = torch.Generator().manual_seed(11)
    ref = torch.rand(700 + 257, 3, generator=g)
    qry = (torch.rand(300 + 65, 3, generator=g) - 0.5) * 3.0 + 0.5              # 3x the reference box: most queries outside it
    qry[:5] = ref[:5]                                                           # ... and some on reference points
    return qry, [300, 65], ref, [700, 257], k


def _few_and_empty():
    g = torch.Generator().manual_seed(12)
    ref = torch.rand(2 + 0 + 50, 3, generator=g)                                # a cloud of 2 < k points, an empty one, a full one
    qry = torch.rand(20 + 10 + 30, 3, generator=g)
    return qry, [20, 10, 30], ref, [2, 0, 50], 3


def _non_finite():
    g = torch.Generator().manual_seed(13)
    ref = torch.rand(400, 3, generator=g)
    qry = torch.rand(100, 3, generator=g)
    ref[3, 0], ref[77, 1], ref[200, 2], ref[399, 0] = float("nan"), float("inf"), -float("inf"), float("nan")
    qry[0, 1], qry[50, 2], qry[99, 0] = float("nan"), float("inf"), -float("inf")
    return qry, [100], ref, [400], 16


CROSS = {
    "outside_k1": _case(lambda: _outside(1)),
    "outside_k3": _case(lambda: _outside(3)),
    "outside_k16": _case(lambda: _outside(16)),
    "few_and_empty_k3": _case(_few_and_empty),
    "non_finite_k16": _case(_non_finite),
}


def self_as_cross(name):
    """A self case as a cross case: every third point of each cloud queries its whole cloud, k cut to the cross form's 16."""
    pos, sizes, k = SELF[name]()
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate([np.arange(ptr[b], ptr[b + 1], 3) for b in range(len(sizes))])
    return pos[rows].contiguous(), [len(range(0, s, 3)) for s in sizes], pos, sizes, min(k, 16)


def ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
