"""The cases of Euclidean farthest-point sampling (``geometry.fps``, csrc/fps_euclid.hip), seeded; shared by the host and the GPU
tests.  A case: ``clouds`` (float32 [n,3] arrays of one launch), exactly one of ``ratio`` / ``n_samples``, ``start`` (local ids,
or None for row 0).  ``expected(case)`` -> the picks of every cloud by the numpy restatement, computed once per case.

The kernel's instances change at 64, 1 024, 2 048, 4 096 and 8 192 points (points per thread x workgroup size); the sizes
straddle each of them."""
import functools

import numpy as np

from tests import fps_euclid_restate as R

CAP = 16384                                   # FPS_EUCLID_MAX_POINTS (asserted against the library in both test files)


def normal(seed, n, scale=1.0, shift=0.0):
    return (np.random.default_rng(seed).standard_normal((n, 3)) * scale + shift).astype(np.float32)


def _coincident():
    pos = normal(300, 1000)
    rows = np.random.default_rng(301).choice(1000, 295, replace=False)
    pos[rows] = pos[rows[0]]
    return pos


def _lattice():
    g = np.arange(8, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).copy()


def _nonfinite():
    pos = normal(310, 200)
    pos[17, 1] = np.nan
    pos[90, 0] = np.inf
    return pos


def case(name, clouds, ratio=None, n_samples=None, start=None):
    return dict(name=name, clouds=[np.ascontiguousarray(c, dtype=np.float32) for c in clouds], ratio=ratio, n_samples=n_samples,
                start=start)


RAGGED_SIZES = (1, 65, 1025, 300, 2049)
CASES = [case(f"n{n}", [normal(100 + i, n)], ratio=4) for i, n in enumerate((1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097))] + [
    case("n8193_64_picks", [normal(120, 8193)], n_samples=64),
    case("cap_64_picks", [normal(121, CAP)], n_samples=64),
    case("full_order_257", [normal(130, 257)], ratio=1),
    case("one_pick", [normal(131, 300)], n_samples=1),
    case("ragged", [normal(140 + i, n) for i, n in enumerate(RAGGED_SIZES)], ratio=3),
    case("coincident_295_of_1000", [_coincident()], ratio=1),
    case("lattice_8x8x8", [_lattice()], ratio=1),
    case("shifted_4096", [normal(150, 500, 1.0, 4096.0)], ratio=4),
    case("nan_and_inf_rows", [_nonfinite()], ratio=1),
    case("start_at_the_nan_row", [_nonfinite()], ratio=2, start=[17]),
    case("start_at_the_inf_row", [_nonfinite()], ratio=2, start=[90]),
    case("nonzero_starts", [normal(160, 100), normal(161, 257), normal(162, 70)], ratio=4, start=[50, 256, 69]),
    case("ratio_1", [normal(170, 130)], ratio=1),
    case("ratio_3", [normal(170, 130)], ratio=3),
    case("ratio_4", [normal(170, 130)], ratio=4),
    case("n_samples_37", [normal(171, 100), normal(172, 64)], n_samples=37),
]
BY_NAME = {c["name"]: c for c in CASES}
NAMES = list(BY_NAME)
TIE_FREE = ("n65", "n1025", "full_order_257", "ratio_3")     # continuous draws around the origin: no two maxima coincide


def picks_of(c, b):
    """How many picks cloud b of the case asks for."""
    n = c["clouds"][b].shape[0]
    return -(-n // c["ratio"]) if c["ratio"] is not None else c["n_samples"]


def start_of(c, b):
    return 0 if c["start"] is None else int(c["start"][b])


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = BY_NAME[name]
    return tuple(R.sample(pos, picks_of(c, b), start_of(c, b)) for b, pos in enumerate(c["clouds"]))


def expected(c):
    """-> per cloud the int64 local picks of the restatement (shared: do not write to them)."""
    return _expected(c["name"])


def ptr_of(c):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in c["clouds"]])]).astype(np.int64)
