"""numpy restatement of the rules of Euclidean farthest-point sampling (deltaconv_amd/csrc/fps_euclid_math.h), vectorised over the
points of one cloud; shared by tests/test_fps_euclid_host.py and tests/test_gpu_fps_euclid.py."""
import numpy as np


def dist2(pos, c):
    """The contract's fp32 distance of every row of pos [n,3] to c [3]: (dx*dx + dy*dy) + dz*dz, every operation rounded."""
    with np.errstate(all="ignore"):
        d = pos - c
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def sample(pos, m, start=0):
    """pos float32 [n,3], m <= n picks from local row `start` -> int64 [m] local ids in pick order."""
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    md = np.where(np.isfinite(pos).all(1), np.float32(np.inf), np.float32(-0.5)).astype(np.float32)
    picks, cur = np.empty(m, dtype=np.int64), int(start)
    for r in range(m):
        picks[r] = cur
        md[cur] = -1.0
        d2 = dist2(pos, pos[cur])
        lower = (md >= 0) & (d2 < md)                  # a NaN d2 compares false; marked and non-finite points are not touched
        md[lower] = d2[lower]
        cur = int(np.argmax(md))                       # the FIRST index of the maximum
    return picks
