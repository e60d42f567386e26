"""numpy restatement of the rules of exact farthest-point sampling on a cell grid (deltaconv_amd/csrc/fps_grid_math.h): the state and
selection of tests/fps_euclid_restate.py, the grid and ``bound2`` of tests/knn_grid_restate.py, and the box rule -- a pick updates
only the points whose cell lies within Chebyshev distance R of its own.  Written from the header's rules, vectorised over the
points of one cloud; shared by tests/test_fps_grid_host.py and tests/test_gpu_fps_grid.py."""
import numpy as np

from tests import fps_euclid_restate as E
from tests import knn_grid_restate as K

F = np.float32
CAP = 262144                                  # FPS_GRID_MAX_POINTS (asserted against the header, the host build and Python)
DEFAULT_TARGET = 0.5                          # FPS_GRID_TARGET, dcfpsg::DEFAULT_TARGET (asserted)


def box_radius(D, min_h, rcover):
    """The smallest r in 0 .. rcover with bound2(r) >= D, or rcover."""
    if rcover == 0:
        return 0
    ok = np.nonzero(K.bound2(np.arange(rcover), min_h) >= F(D))[0]
    return int(ok[0]) if ok.size else rcover


def sample(pos, m, start=0, target=DEFAULT_TARGET, trace=None, history=None):
    """pos float32 [n,3], m <= n picks from local row `start` -> (int64 [m] local ids in pick order, int64 [2] stats).
    ``trace``: a list that receives (pick id, R, D, grid, mask of the finite points inside the box) per updating pick;
    ``history``: a list that receives the stats after every pick but the last (entry r - 2 is the stats of the r-pick sample)."""
    pos = np.ascontiguousarray(pos, dtype=F).reshape(-1, 3)
    n = pos.shape[0]
    finite = np.isfinite(pos).all(1)
    G = K.grid_of(pos, target)
    cell = np.zeros((n, 3), np.int64)
    cell[finite] = K.cells(G, pos[finite])
    md = np.where(finite, F(np.inf), F(-0.5)).astype(F)
    picks, stats = np.empty(m, dtype=np.int64), np.zeros(2, np.int64)
    cur, D, r = int(start), F(np.inf), 0
    while r < m:
        picks[r] = cur
        r += 1
        if r == m:
            break
        if finite[cur]:
            rcover = int(np.maximum(cell[cur], G["g"] - 1 - cell[cur]).max())
            R = box_radius(D, G["min_h"], rcover)
            inside = finite & (np.abs(cell - cell[cur]).max(1) <= R)
            lo, hi = np.maximum(cell[cur] - R, 0), np.minimum(cell[cur] + R, G["g"] - 1)
            stats += (int(inside.sum()), int(np.prod(hi - lo + 1)))
            if trace is not None:
                trace.append((cur, R, D, G, inside))
            md[cur] = -1.0
            d2 = E.dist2(pos, pos[cur])
            lower = inside & (md >= 0) & (d2 < md)
            md[lower] = d2[lower]
        else:
            md[cur] = -1.0                     # (never selected again: the tail below passes over the start)
        if history is not None:
            history.append(stats.copy())
        live = finite & (md >= 0)
        if not live.any():                     # every finite point is taken: the non-finite rows in ascending id, without the start
            rest = [i for i in np.nonzero(~finite)[0] if i != int(start)]
            picks[r:] = rest[:m - r]
            break
        top = md[live].max()
        cur = int(np.nonzero(live & (md == top))[0][0])       # the FIRST index of the maximum
        D = top
    return picks, stats
