"""numpy restatement of the draws of the batch assembly kernel (deltaconv_amd/csrc/batch_math.h) and the expected
values of its augmentation ops, shared by tests/test_loader_host.py (CPU) and tests/test_gpu_loader.py.

Draws: Philox-4x32-10 in uint64 arithmetic, the counter layout and the fp32 uniform formula of batch_math.h -- bit for
bit.  Expected values: the repository's own CPU transform classes (pinned to the reference's outputs by
tests/test_transforms.py) applied to fp64 copies of an item, their random draws replaced by the restated ones
(``random.uniform`` / ``Tensor.uniform_`` patched for the duration of one call); RandomJitter by its formula."""
import contextlib
import random

import numpy as np
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd.datasets import Data
from deltaconv_amd.loader import RandomJitter

BATCH_KEY = 0x6261746B
PER_CLOUD = 0xFFFFFFFF
_M32 = np.uint64(0xFFFFFFFF)

# the training-time recipes of the reference's five scripts (experiments/train_modelnet.py:37-40, train_shapenet.py:36-39,
# train_scanobjectnn.py:47-52, train_shapeseg.py:37-41, train_shrec.py:37-42); PyG's RandomTranslate = RandomJitter
RECIPES = {
    "modelnet": lambda: [T.RandomScale((4 / 5, 5 / 4)), T.RandomTranslateGlobal(0.1)],
    "shapenet": lambda: [T.RandomScale((2 / 3, 3 / 2)), T.RandomTranslateGlobal(0.2)],
    "scanobjectnn": lambda: [T.RandomRotate(360, 1), RandomJitter(0.01), T.RandomScale((4 / 5, 5 / 4)),
                             T.RandomTranslateGlobal(0.1)],
    "shapeseg": lambda: [T.RandomScale((0.8, 1.2)), T.RandomRotate(360, axis=2), T.RandomTranslateGlobal(0.1)],
    "shrec": lambda: [T.RandomRotate(360, 0), T.RandomRotate(360, 1), T.RandomRotate(360, 2), T.RandomTranslateGlobal(0.1)],
}
SINGLE_OPS = {
    "scale": lambda: [T.RandomScale((0.5, 2.0))],
    "rotate0": lambda: [T.RandomRotate(360, 0)],
    "rotate1": lambda: [T.RandomRotate((-30, 170), 1)],
    "rotate2": lambda: [T.RandomRotate(180, 2)],
    "translate": lambda: [T.RandomTranslateGlobal((0.1, 0.2, 0.3))],
    "normals": lambda: [T.RandomNormals(0.1)],
    "jitter": lambda: [RandomJitter((0.01, 0.02, 0.03))],
}


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words (broadcastable unsigned arrays) and key words -> four uint32 arrays."""
    x, y, z, w = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x, np.uint64(0xCD9E8D57) * z       # 32 x 32 -> 64 bits: no overflow
        x, y, z, w = (p1 >> np.uint64(32)) ^ y ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ w ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return tuple(v.astype(np.uint32) for v in (x, y, z, w))


def draw(seed, step, cloud, op_pos, point):
    """The Philox output of one (seed, step, dataset cloud index, op position, point | PER_CLOUD); arrays broadcast."""
    step = int(step)
    assert 0 <= step < 2 ** 61 and 0 <= op_pos < 8
    return philox4x32_10(point, cloud, step & 0xFFFFFFFF, ((step >> 32) << 3) | op_pos, seed, BATCH_KEY)


def uniform(r, lo, hi):
    """fp32, every operation rounded on its own: lo + ((r >> 8) * 2^-24) * (hi - lo)."""
    lo, hi = np.float32(lo), np.float32(hi)
    u = (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (lo + (u * np.float32(hi - lo)).astype(np.float32)).astype(np.float32)


def _three(t):
    return [abs(float(a)) for a in ([t] * 3 if isinstance(t, (int, float)) else t)]


def cloud_draw(t, seed, step, cloud, op_pos):
    """Per-cloud parameters of transform `t` at op position op_pos; `cloud` a scalar or an array of dataset indices:
    scale -> [..., 3] factors, rotate -> [...] degrees, translate -> [..., 3] offsets (float32)."""
    r = draw(seed, step, cloud, op_pos, PER_CLOUD)
    if isinstance(t, T.RandomScale):
        return np.stack([uniform(r[a], t.scales[0], t.scales[1]) for a in range(3)], axis=-1)
    if isinstance(t, T.RandomRotate):
        return uniform(r[0], t.degrees[0], t.degrees[1])
    if isinstance(t, T.RandomTranslateGlobal):
        lim = _three(t.translate)
        return np.stack([uniform(r[a], -lim[a], lim[a]) for a in range(3)], axis=-1)
    raise TypeError(t)


def point_draw(t, seed, step, cloud, op_pos, n):
    """[n, 3] float32 offsets of a per-point op (RandomNormals / RandomJitter)."""
    lim = _three(t.translate)
    r = draw(seed, step, cloud, op_pos, np.arange(n, dtype=np.uint64))
    return np.stack([uniform(r[a], -lim[a], lim[a]) for a in range(3)], axis=-1)


@contextlib.contextmanager
def _patched_draws(tensors=(), degrees=()):
    """`Tensor.uniform_` hands out `tensors` in order (shape-checked), `random.uniform` hands out `degrees`."""
    tensors, degrees = list(tensors), list(degrees)
    old_t, old_r = torch.Tensor.uniform_, random.uniform

    def uniform_(self, *a, **k):
        v = tensors.pop(0)
        assert tuple(v.shape) == tuple(self.shape), (v.shape, self.shape)
        return self.copy_(v)

    torch.Tensor.uniform_, random.uniform = uniform_, lambda *a: degrees.pop(0)
    try:
        yield
    finally:
        torch.Tensor.uniform_, random.uniform = old_t, old_r
    assert not tensors and not degrees, "a transform consumed fewer draws than restated"


def expected(item, transforms, seed, step, cloud):
    """fp64 (pos, norm | None) of `item` (dataset index `cloud`) after `transforms` with the restated draws."""
    data = Data(pos=item.pos.double().clone())
    nrm = getattr(item, "norm", None)
    if nrm is not None:
        data.norm = nrm.double().clone()
    n = data.pos.shape[0]
    f64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    for o, t in enumerate(transforms):
        if isinstance(t, T.RandomScale):
            with _patched_draws([f64(cloud_draw(t, seed, step, cloud, o))]):
                data = t(data)
        elif isinstance(t, T.RandomRotate):
            with _patched_draws(degrees=[float(cloud_draw(t, seed, step, cloud, o))]):
                data = t(data)
        elif isinstance(t, T.RandomTranslateGlobal):
            off = cloud_draw(t, seed, step, cloud, o)
            with _patched_draws([f64(off[a:a + 1]) for a in range(3)]):
                data = t(data)
        elif isinstance(t, T.RandomNormals):
            jit = point_draw(t, seed, step, cloud, o, n)
            with _patched_draws([f64(jit[:, a]) for a in range(3)]):
                data = t(data)
        elif isinstance(t, RandomJitter):
            data.pos = data.pos + f64(point_draw(t, seed, step, cloud, o, n))
        else:
            raise TypeError(t)
    return data.pos, getattr(data, "norm", None)


def bound(want):
    """The issue's bound: 64 * 2^-24 * max(1, max |expected|) -- a recipe is at most five ops of a handful of fp32
    roundings on values of magnitude <= 2, sincosf within a few ulp, the fp32 angle <= 4e-7 |pos|."""
    return 64 * 2.0 ** -24 * max(1.0, float(want.abs().max()))


def make_items(n_clouds, sizes, normals=True, distinct=8, seed=0, **extra):
    """`n_clouds` Data items of the given point counts (an int or a list) from ``synthetic_cloud``; only `distinct` different
    surfaces per size are generated (the draws depend on the dataset index, not on the content)."""
    from deltaconv_amd.data import synthetic_cloud
    sizes = [sizes] * n_clouds if isinstance(sizes, int) else list(sizes)
    cache, items = {}, []
    for i, n in enumerate(sizes):
        key = (n, i % distinct)
        if key not in cache:
            p, nr = synthetic_cloud(max(n, 16), 7000 + 100 * seed + i % distinct, normals=normals)     # (one point alone
            cache[key] = (p[:n], nr[:n] if normals else None)                                       # cannot be normalised)
        p, nr = cache[key]
        d = Data(pos=p.clone(), y=torch.tensor([i % 40]))
        if normals:
            d.norm = nr.clone()
        items.append(d)
    return items
