"""numpy restatement of the device surface sampler (deltaconv_amd/csrc/mesh_math.h), shared by tests/test_mesh_host.py (CPU)
and tests/test_gpu_mesh.py: fp64 face areas, integer weights and their uint64 running sum, the Philox draws, the face pick
through the high half of a 64 x 64-bit product, the fp32 fold / point / normal -- bit for bit, with no scan tree to restate
(integer sums and a maximum have no order).  Expected values against the host class: ``T.SamplePoints`` run in fp64 with
``torch.multinomial`` and ``torch.rand`` patched to hand out the restated picks and fractions."""
import contextlib

import numpy as np
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd.datasets import Data
from tests.batch_restate import philox4x32_10

MESH_KEY = 0x6D657368
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def areas(vert, face):
    """vert float32 [V,3], face int [F,3] -> fp64 [F]: |e1 x e2| from the widened vertices; 0 for an id outside [0, V) or a
    non-finite value."""
    vert, face = np.asarray(vert, dtype=np.float32), np.asarray(face, dtype=np.int64).reshape(-1, 3)
    ok = np.all((face >= 0) & (face < vert.shape[0]), axis=1)
    p = vert.astype(np.float64)[np.where(ok[:, None], face, 0)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(all="ignore"):
        a = np.sqrt((cx * cx + cy * cy) + cz * cz)
    a[~ok | ~np.isfinite(a)] = 0.0
    return a


def weights(a):
    """fp64 areas -> uint64 weights in [0, 2^32] relative to the largest (truncating cast); all 0 without a positive area."""
    amax = a.max()
    if not amax > 0:
        return np.zeros(a.shape, dtype=np.uint64)
    return ((a / amax) * 4294967296.0).astype(np.uint64)


def cdf_of(vert, face):
    """-> (w uint64 [F], cdf uint64 [F]); total = cdf[-1]."""
    w = weights(areas(vert, face))
    return w, np.cumsum(w, dtype=np.uint64)


def mulhi64(a, b):
    """High 64 bits of the 128-bit product of uint64 arrays, from 32-bit halves (no partial sum overflows 64 bits)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    ah, al, bh, bl = a >> _S32, a & _M32, b >> _S32, b & _M32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def draws(seed, rnd, mesh, num):
    """The four Philox words of samples 0 .. num-1 of dataset index `mesh` in round `rnd`."""
    rnd = int(rnd)
    assert 0 <= rnd < 2 ** 63 and 0 <= int(seed) < 2 ** 32 and 0 <= int(mesh) < 2 ** 32
    return philox4x32_10(np.arange(num, dtype=np.uint64), mesh, rnd & 0xFFFFFFFF, rnd >> 32, seed, MESH_KEY)


def pick(cdf, r):
    """cdf uint64 [F] -> int64 [num]: the first face with cdf[f] > (u * total) >> 64; total = 0: (u * F) >> 64."""
    cdf = np.asarray(cdf, dtype=np.uint64)
    u = (r[0].astype(np.uint64) << _S32) | r[1].astype(np.uint64)
    total = cdf[-1]
    if total == 0:
        return mulhi64(u, np.uint64(cdf.shape[0])).astype(np.int64)
    return np.searchsorted(cdf, mulhi64(u, total), side="right").astype(np.int64)


def fold(r):
    """-> (f1, f2) float32 [num] after the fold of sample_points.py:36-38."""
    f1 = (r[2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    f2 = (r[3] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    over = (f1 + f2).astype(np.float32) > np.float32(1)
    return np.where(over, np.float32(1) - f1, f1).astype(np.float32), np.where(over, np.float32(1) - f2, f2).astype(np.float32)


def sample(vert, face, num, seed=0, rnd=0, mesh=0, y_vert=None, cdf=None):
    """The restated sample of one mesh -> dict(face_id int64 [num], f1, f2, pos float32 [num,3], norm float32 [num,3],
    y int64 [num] | None, w, cdf, total).  ``cdf``: use this one (the device's own) instead of the restated one."""
    vert, face = np.asarray(vert, dtype=np.float32), np.asarray(face, dtype=np.int64).reshape(-1, 3)
    w, own = cdf_of(vert, face)
    cdf = own if cdf is None else np.asarray(cdf).view(np.uint64) if np.asarray(cdf).dtype == np.int64 else np.asarray(cdf, dtype=np.uint64)
    r = draws(seed, rnd, mesh, num)
    fid = pick(cdf, r)
    f1, f2 = fold(r)
    ids = face[fid]
    ok = np.all((ids >= 0) & (ids < vert.shape[0]), axis=1)
    p = vert[np.where(ok[:, None], ids, 0)]
    p0 = p[:, 0]
    e1, e2 = (p[:, 1] - p0).astype(np.float32), (p[:, 2] - p0).astype(np.float32)
    with np.errstate(all="ignore"):
        t1, t2 = (f1[:, None] * e1).astype(np.float32), (f2[:, None] * e2).astype(np.float32)
        pos = ((p0 + t1).astype(np.float32) + t2).astype(np.float32)
        cx = ((e1[:, 1] * e2[:, 2]).astype(np.float32) - (e1[:, 2] * e2[:, 1]).astype(np.float32)).astype(np.float32)
        cy = ((e1[:, 2] * e2[:, 0]).astype(np.float32) - (e1[:, 0] * e2[:, 2]).astype(np.float32)).astype(np.float32)
        cz = ((e1[:, 0] * e2[:, 1]).astype(np.float32) - (e1[:, 1] * e2[:, 0]).astype(np.float32)).astype(np.float32)
        sq = (((cx * cx).astype(np.float32) + (cy * cy).astype(np.float32)).astype(np.float32) + (cz * cz).astype(np.float32)).astype(np.float32)
        ln = np.maximum(np.sqrt(sq).astype(np.float32), np.float32(1e-12))
        norm = (np.stack([cx, cy, cz], axis=1) / ln[:, None]).astype(np.float32)
    pos[~ok], norm[~ok] = 0, 0
    y = None
    if y_vert is not None:
        y = np.where(ok, np.asarray(y_vert, dtype=np.int64)[np.where(ok, ids[:, 0], 0)], -1)
    return dict(face_id=fid, f1=f1, f2=f2, pos=pos, norm=norm, y=y, w=w, cdf=cdf, total=int(cdf[-1]))


@contextlib.contextmanager
def _patched_draws(picks, fracs):
    """``torch.multinomial`` hands out `picks`, ``torch.rand`` hands out `fracs`, once each (the precedent:
    tests/batch_restate.py::_patched_draws)."""
    left = {"multinomial": [picks], "rand": [fracs]}
    old_m, old_r = torch.multinomial, torch.rand

    def multinomial(p, n, replacement=False, **k):
        v = left["multinomial"].pop(0)
        assert replacement and n == v.shape[0] and bool((p[v] > 0).all()), "a zero-probability face was restated"
        return v

    def rand(*size, **k):
        v = left["rand"].pop(0)
        assert tuple(size) == tuple(v.shape), (size, v.shape)
        return v.clone()

    torch.multinomial, torch.rand = multinomial, rand
    try:
        yield
    finally:
        torch.multinomial, torch.rand = old_m, old_r
    assert not left["multinomial"] and not left["rand"], "SamplePoints consumed fewer draws than restated"


def expected(vert, face, num, seed=0, rnd=0, mesh=0, y_vert=None):
    """fp64 ``(pos, norm, y | None)`` of ``T.SamplePoints(num, include_normals=True)`` on the restated picks and UNFOLDED
    fractions (the class folds them itself)."""
    r = draws(seed, rnd, mesh, num)
    _, cdf = cdf_of(vert, face)
    fid = torch.from_numpy(pick(cdf, r))
    raw = np.stack([(r[2] >> np.uint32(8)).astype(np.float64), (r[3] >> np.uint32(8)).astype(np.float64)], axis=1) * 2.0 ** -24
    data = Data(pos=torch.from_numpy(np.asarray(vert, dtype=np.float64)),
                face=torch.from_numpy(np.asarray(face, dtype=np.int64).reshape(-1, 3).T.copy()))
    if y_vert is not None:
        data.y = torch.from_numpy(np.asarray(y_vert, dtype=np.int64))
    with _patched_draws(fid, torch.from_numpy(raw)):
        data = T.SamplePoints(num, include_normals=True, include_labels=y_vert is not None)(data)
    return data.pos, data.norm, (data.y if y_vert is not None else None)


def bound(want):
    """The project's bound for a few fp32 roundings (tests/batch_restate.py::bound): 64 * 2^-24 * max(1, max |expected|)."""
    return 64 * 2.0 ** -24 * max(1.0, float(want.abs().max()))


def with_tiny_face(pos, face, factor=2.0 ** -40):
    """pos [V,3] float32, face [3,F] as the readers give them -> the mesh with one more face, at the origin, whose area is
    `factor` of the largest face's (a right triangle with legs sqrt(largest * factor))."""
    pos, face = torch.as_tensor(pos), torch.as_tensor(face)
    big = float(areas(pos.numpy(), face.t().numpy()).max())
    s = float(np.float32(np.sqrt(big * factor)))
    v = pos.shape[0]
    pos = torch.cat([pos, torch.tensor([[0, 0, 0], [s, 0, 0], [0, s, 0]], dtype=torch.float32)])
    return pos, torch.cat([face, torch.tensor([[v], [v + 1], [v + 2]])], dim=1)
