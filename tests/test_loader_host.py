"""Host side of the device-resident loader (deltaconv_amd/loader.py), without a GPU: the index logic of DeviceLoader, the
translation of transforms into the kernel's op list, the numpy restatement of the kernel's draws (tests/batch_restate.py)
against Philox known answers, and a g++ build of csrc/batch_math.h (tests/hostcheck_batch) against that restatement (drawn
parameters: bitwise) and against the repository's CPU transform classes run in fp64 on the restated draws (points and
normals: within 64 * 2^-24 * max(1, max |expected|))."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd.datasets import Compose, Data
from deltaconv_amd.loader import (DeviceLoader, RandomJitter, translate_transforms, OP_SCALE, OP_ROTATE, OP_TRANSLATE,
                                  OP_NORMAL_JITTER, OP_POINT_JITTER)
from tests import batch_restate as R
from tests.helpers import ROOT


class _HostStore:
    """What DeviceLoader's index logic reads of a store: the cloud count and the sizes (no device involved)."""

    def __init__(self, sizes, norm=True):
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.norm = object() if norm else None
        self.device = "cpu"

    def __len__(self):
        return int(self.sizes.shape[0])


# ---- index logic ----------------------------------------------------------------------------------------------------------
def test_permutation_is_a_function_of_seed_and_epoch():
    st = _HostStore([16] * 100)
    a = DeviceLoader(st, 8, shuffle=True, seed=3)
    b = DeviceLoader(st, 8, shuffle=True, seed=3, drop_last=True)
    assert a.batch_indices(5) == DeviceLoader(st, 8, shuffle=True, seed=3).batch_indices(5)
    assert a.batch_indices(5)[:12] == b.batch_indices(5)                      # the same order, whatever else differs
    flat = lambda bi: [i for batch in bi for i in batch]
    assert sorted(flat(a.batch_indices(0))) == list(range(100))
    assert flat(a.batch_indices(0)) != flat(a.batch_indices(1))
    assert flat(a.batch_indices(0)) != flat(DeviceLoader(st, 8, shuffle=True, seed=4).batch_indices(0))
    a.set_epoch(7)
    assert a.batch_indices() == a.batch_indices(7)


def test_last_batch_and_no_shuffle():
    st = _HostStore([16] * 100)
    keep, drop = DeviceLoader(st, 8), DeviceLoader(st, 8, drop_last=True)
    assert len(keep) == 13 and len(drop) == 12
    bi = keep.batch_indices(0)
    assert [len(b) for b in bi] == [8] * 12 + [4]
    assert [i for b in bi for i in b] == list(range(100))                     # shuffle=False: arange, in every epoch
    assert keep.batch_indices(3) == bi
    assert drop.batch_indices(0) == bi[:12]
    assert len(DeviceLoader(st, 100)) == 1 and len(DeviceLoader(st, 101, drop_last=True)) == 0
    assert len(DeviceLoader(st, 10)) == 10 == len(DeviceLoader(st, 10, drop_last=True))


@pytest.mark.parametrize("world", [2, 8])
def test_rank_shares_are_disjoint_equal_and_cover_the_epoch(world):
    st = _HostStore([16] * 96)
    for epoch in (0, 4):
        whole = [i for b in DeviceLoader(st, 96, shuffle=True, seed=9).batch_indices(epoch) for i in b]
        shares = []
        for rank in range(world):
            ld = DeviceLoader(st, 5, shuffle=True, seed=9, rank=rank, world=world)
            shares.append([i for b in ld.batch_indices(epoch) for i in b])
            assert len(ld) == -(-(96 // world) // 5)
        assert all(len(s) == 96 // world for s in shares)
        union = [i for s in shares for i in s]
        assert len(set(union)) == len(union) == 96 and set(union) == set(whole)
        # the permutation is the same on every rank: rank r holds every world-th entry of it
        assert all(shares[r] == whole[r::world] for r in range(world))
    # a cloud count that does not divide: equally long shares, the tail of the epoch's order sits out
    st = _HostStore([16] * 99)
    shares = [DeviceLoader(st, 99, shuffle=True, seed=1, rank=r, world=world).batch_indices(2)[0] for r in range(world)]
    assert all(len(s) == 99 // world for s in shares) and len({i for s in shares for i in s}) == world * (99 // world)


# ---- transforms -> op list ---------------------------------------------------------------------------------------------------
def test_the_five_recipes_translate_in_order():
    f = np.float32
    ops = {k: translate_transforms(Compose(v())) for k, v in R.RECIPES.items()}
    assert ops["modelnet"] == [(OP_SCALE, (4 / 5, 5 / 4, 0.0)), (OP_TRANSLATE, (0.1, 0.1, 0.1))]
    assert ops["shapenet"] == [(OP_SCALE, (2 / 3, 3 / 2, 0.0)), (OP_TRANSLATE, (0.2, 0.2, 0.2))]
    assert ops["scanobjectnn"] == [(OP_ROTATE, (-360.0, 360.0, 1.0)), (OP_POINT_JITTER, (0.01, 0.01, 0.01)),
                                   (OP_SCALE, (4 / 5, 5 / 4, 0.0)), (OP_TRANSLATE, (0.1, 0.1, 0.1))]
    assert ops["shapeseg"] == [(OP_SCALE, (0.8, 1.2, 0.0)), (OP_ROTATE, (-360.0, 360.0, 2.0)), (OP_TRANSLATE, (0.1, 0.1, 0.1))]
    assert ops["shrec"] == [(OP_ROTATE, (-360.0, 360.0, 0.0)), (OP_ROTATE, (-360.0, 360.0, 1.0)),
                            (OP_ROTATE, (-360.0, 360.0, 2.0)), (OP_TRANSLATE, (0.1, 0.1, 0.1))]
    # a list and a single transform are taken like a Compose; None is the pure gather of the evaluation loaders
    assert translate_transforms(R.RECIPES["shrec"]()) == ops["shrec"]
    assert translate_transforms(T.RandomScale((0.5, 2))) == [(OP_SCALE, (0.5, 2.0, 0.0))]
    assert translate_transforms(None) == [] and translate_transforms(Compose([])) == []
    # what the loader hands to the kernel: fp32 parameters in list order
    ld = DeviceLoader(_HostStore([4] * 4), 2, transform=R.RECIPES["scanobjectnn"]())
    assert list(ld._codes) == [OP_ROTATE, OP_POINT_JITTER, OP_SCALE, OP_TRANSLATE]
    assert list(ld._params) == [f(v) for v in (-360, 360, 1, 0.01, 0.01, 0.01, 0.8, 1.25, 0, 0.1, 0.1, 0.1)]


def test_parameter_expansion_follows_the_cpu_classes():
    assert translate_transforms(T.RandomRotate(-45, axis=2)) == [(OP_ROTATE, (-45.0, 45.0, 2.0))]        # a Number: (-|d|, |d|)
    assert translate_transforms(T.RandomRotate((10, 20))) == [(OP_ROTATE, (10.0, 20.0, 0.0))]            # axis defaults to 0
    assert translate_transforms(T.RandomTranslateGlobal(-0.3)) == [(OP_TRANSLATE, (0.3, 0.3, 0.3))]      # (-|t|, |t|) per axis
    assert translate_transforms(T.RandomTranslateGlobal((0.1, -0.2, 0))) == [(OP_TRANSLATE, (0.1, 0.2, 0.0))]
    assert translate_transforms(T.RandomNormals(0.05)) == [(OP_NORMAL_JITTER, (0.05, 0.05, 0.05))]
    assert translate_transforms(RandomJitter((0.01, 0.02, 0.03))) == [(OP_POINT_JITTER, (0.01, 0.02, 0.03))]


def test_what_the_kernel_does_not_implement_raises():
    with pytest.raises(ValueError, match="NormalizeScale"):
        translate_transforms(Compose([T.RandomScale((0.8, 1.2)), T.NormalizeScale()]))
    with pytest.raises(ValueError, match="function"):
        translate_transforms([lambda d: d])
    with pytest.raises(ValueError, match="RandomNormals"):
        DeviceLoader(_HostStore([4] * 4, norm=False), 2, transform=[T.RandomNormals(0.1)])
    DeviceLoader(_HostStore([4] * 4, norm=False), 2, transform=[T.RandomScale((0.8, 1.2)), T.RandomRotate(10)])   # normal part skipped
    with pytest.raises(ValueError, match="at most 8"):
        translate_transforms([T.RandomRotate(10)] * 9)
    with pytest.raises(ValueError, match="one per axis"):
        translate_transforms(T.RandomTranslateGlobal((0.1, 0.2)))


def test_random_jitter_cpu_call_is_pyg_random_translate():
    """PyG's RandomTranslate: one uniform_(-|t|, |t|) of n values per axis, in axis order, added to pos."""
    pos = torch.randn(50, 3)
    torch.manual_seed(11)
    out = RandomJitter((0.01, 0.0, 0.5))(Data(pos=pos.clone())).pos
    torch.manual_seed(11)
    ts = [pos.new_empty(50).uniform_(-a, a) for a in (0.01, 0.0, 0.5)]
    assert torch.equal(out, pos + torch.stack(ts, dim=-1))
    d = (RandomJitter(0.25)(Data(pos=pos.clone())).pos - pos).abs()
    assert float(d.max()) <= 0.25 and float(d.max()) > 0.2
    assert repr(RandomJitter(0.25)) == "RandomJitter(0.25)"


# ---- the restated draws ------------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_numpy_philox_known_answers_and_hostcheck():
    """The Random123 known-answer vectors tests/test_hostcheck_nn.py holds nn_math.h to, and hc_philox of libhostcheck.so on
    random counters."""
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == want
    hc_dir = os.path.join(ROOT, "tests", "hostcheck")
    subprocess.run(["make", "-s", "-C", hc_dir], check=True)
    hc = ctypes.CDLL(os.path.join(hc_dir, "libhostcheck.so"))
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(200, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(200, 2), dtype=np.uint64)
    for i in range(200):
        got = np.stack(R.philox4x32_10(*ctr[i], *key[i])).reshape(-1)
        c, out = (ctypes.c_uint32 * 4)(*[int(v) for v in ctr[i]]), (ctypes.c_uint32 * 4)()
        hc.hc_philox(c, ctypes.c_uint32(int(key[i, 0])), ctypes.c_uint32(int(key[i, 1])), out)
        assert [int(v) for v in got] == list(out)
    # vectorised over counters = one at a time
    many = R.philox4x32_10(ctr[:, 0], ctr[:, 1], 7, 9, 1, 2)
    one = R.philox4x32_10(ctr[5, 0], ctr[5, 1], 7, 9, 1, 2)
    assert [int(m[5]) for m in many] == [int(v) for v in one]


def test_counters_are_distinct():
    """(step, op position, cloud, point | per-cloud) -> counter is injective: the words, restated."""
    seen = set()
    for step in (0, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 60 + 5):
        for op in (0, 7):
            for cloud in (0, 1):
                for point in (0, 1, R.PER_CLOUD):
                    seen.add((point, cloud, step & 0xFFFFFFFF, ((step >> 32) << 3) | op))
                    assert ((step >> 32) << 3 | op) < 2 ** 32
    assert len(seen) == 5 * 2 * 2 * 3
    a = R.draw(1, 5, 3, 0, R.PER_CLOUD)
    assert all(tuple(int(v) for v in R.draw(*args)) != tuple(int(v) for v in a)
               for args in ((2, 5, 3, 0, R.PER_CLOUD), (1, 6, 3, 0, R.PER_CLOUD), (1, 5, 4, 0, R.PER_CLOUD),
                            (1, 5, 3, 1, R.PER_CLOUD), (1, 5, 3, 0, 0), (1, 5 + 2 ** 32, 3, 0, R.PER_CLOUD)))


# seed / step of the statistics check: fixed here, used again on the device (tests/test_gpu_loader.py)
STAT_SEED, STAT_STEP, STAT_CLOUDS = 2024, 17, 4096
STAT_TRANSFORMS = lambda: [T.RandomScale((4 / 5, 5 / 4)), T.RandomRotate((0, 90), 2), T.RandomTranslateGlobal((0.1, 0.2, 0.3))]


def check_draw_statistics(values, lo, hi):
    """Over 4096 clouds: the mean within 5 sigma of the midpoint (sigma = (hi - lo) / sqrt(12 * 4096)), the extremes
    within 1 % of the interval's ends, every value inside the interval."""
    v = np.asarray(values, dtype=np.float64)
    assert v.shape[0] == STAT_CLOUDS
    sigma = (hi - lo) / np.sqrt(12 * STAT_CLOUDS)
    assert abs(v.mean() - (lo + hi) / 2) <= 5 * sigma, (v.mean(), lo, hi)
    assert lo <= v.min() <= lo + 0.01 * (hi - lo) and hi - 0.01 * (hi - lo) <= v.max() <= hi, (v.min(), v.max(), lo, hi)


def test_restated_draw_statistics():
    clouds = np.arange(STAT_CLOUDS, dtype=np.uint64)
    sc, rot, tr = (R.cloud_draw(t, STAT_SEED, STAT_STEP, clouds, o) for o, t in enumerate(STAT_TRANSFORMS()))
    for a in range(3):
        check_draw_statistics(sc[:, a], np.float32(4 / 5), np.float32(5 / 4))
        check_draw_statistics(tr[:, a], -np.float32(0.1 * (a + 1)), np.float32(0.1 * (a + 1)))
    check_draw_statistics(rot, 0.0, 90.0)
    # axes, ops, steps and seeds are separate streams
    assert np.mean(sc[:, 0] == sc[:, 1]) < 0.01 and np.mean(sc[:, 0] == tr[:, 0] * 0 + sc[:, 2]) < 0.01
    other_step = R.cloud_draw(STAT_TRANSFORMS()[0], STAT_SEED, STAT_STEP + 1, clouds, 0)
    other_seed = R.cloud_draw(STAT_TRANSFORMS()[0], STAT_SEED + 1, STAT_STEP, clouds, 0)
    assert not np.any(np.all(other_step == sc, axis=1)) and not np.any(np.all(other_seed == sc, axis=1))


# ---- g++ build of batch_math.h ---------------------------------------------------------------------------------------------------
HB_DIR = os.path.join(ROOT, "tests", "hostcheck_batch")


@pytest.fixture(scope="module")
def hb():
    subprocess.run(["make", "-s", "-C", HB_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HB_DIR, "libhostcheck_batch.so"))
    vp, ci, u32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
    lib.hb_cloud_draws.argtypes = [vp, vp, ci, u32, i64, vp, ci, vp]
    lib.hb_point_draws.argtypes = [vp, u32, i64, i64, ci, ci, vp]
    lib.hb_apply.argtypes = [vp, vp, ci, u32, i64, i64, ci, vp, vp, vp, vp]
    lib.hb_cloud_draws.restype = lib.hb_point_draws.restype = lib.hb_apply.restype = None
    return lib


def _op_arrays(transforms, has_norm=True):
    ops = translate_transforms(transforms, has_norm=has_norm)
    codes = np.array([c for c, _ in ops], dtype=np.int32)
    prm = np.array([p for _, p in ops], dtype=np.float32).reshape(-1, 3)
    return codes, prm


P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
ALL = dict(R.SINGLE_OPS, **R.RECIPES)


@pytest.mark.parametrize("name", list(ALL))
def test_drawn_parameters_are_bitwise_the_restated_ones(hb, name):
    transforms = ALL[name]()
    codes, prm = _op_arrays(transforms)
    clouds = np.array([0, 1, 2, 31, 9839, 123456, 2 ** 32 - 2], dtype=np.int64)
    for seed, step in ((0, 0), (1, 7), (2 ** 32 - 1, 2 ** 32 + 3), (77, 2 ** 61 - 1)):
        out = np.full((len(clouds), len(codes), 3), np.nan, dtype=np.float32)
        hb.hb_cloud_draws(P(codes), P(prm), len(codes), seed, step, P(clouds), len(clouds), P(out))
        for o, t in enumerate(transforms):
            if isinstance(t, (T.RandomScale, T.RandomTranslateGlobal)):
                want = R.cloud_draw(t, seed, step, clouds.astype(np.uint64), o)
                assert np.array_equal(out[:, o].view(np.uint32), want.view(np.uint32)), (name, o)
            elif isinstance(t, T.RandomRotate):
                want = R.cloud_draw(t, seed, step, clouds.astype(np.uint64), o)
                assert np.array_equal(out[:, o, 2].view(np.uint32), want.view(np.uint32)), (name, o)      # the degrees
                rad = want.astype(np.float64) * np.pi / 180
                assert np.abs(out[:, o, 0] - np.sin(rad)).max() < 1e-6 and np.abs(out[:, o, 1] - np.cos(rad)).max() < 1e-6
            else:
                assert np.all(out[:, o] == 0)
                jit = np.empty((300, 3), dtype=np.float32)
                for c in (0, 9839):
                    hb.hb_point_draws(P(prm[o]), seed, step, c, o, 300, P(jit))
                    want = R.point_draw(t, seed, step, c, o, 300)
                    assert np.array_equal(jit.view(np.uint32), want.view(np.uint32)), (name, o)


# (RandomNormals on a shape without normals: the loader raises, test_what_the_kernel_does_not_implement_raises)
@pytest.mark.parametrize("name,normals", [(n, True) for n in ALL] + [(n, False) for n in ALL if n != "normals"])
def test_points_and_normals_match_the_cpu_transform_classes(hb, name, normals):
    """hb_apply (the kernel's per-point code, on the host) against the CPU classes in fp64 on the restated draws."""
    transforms = ALL[name]()
    codes, prm = _op_arrays(transforms, has_norm=normals)
    items = R.make_items(4, [257, 64, 1, 300], normals=normals, distinct=4)
    seed, step = 5, 2 ** 33 + 11
    worst = 0.0
    for cloud, item in zip((0, 3, 77, 9000), items):
        pos = item.pos.numpy().copy()
        nrm = item.norm.numpy().copy() if normals else None
        pos_out = np.empty_like(pos)
        nrm_out = np.empty_like(nrm) if normals else None
        hb.hb_apply(P(codes), P(prm), len(codes), seed, step, cloud, pos.shape[0], P(pos), P(nrm), P(pos_out), P(nrm_out))
        want_pos, want_nrm = R.expected(item, transforms, seed, step, cloud)
        err = float((torch.from_numpy(pos_out).double() - want_pos).abs().max())
        assert err <= R.bound(want_pos), (name, cloud, err)
        worst = max(worst, err / R.bound(want_pos))
        if normals:
            got = torch.from_numpy(nrm_out).double()
            err = float((got - want_nrm).abs().max())
            assert err <= R.bound(want_nrm), (name, cloud, err)
            assert float((got.norm(dim=1) - 1).abs().max()) <= R.bound(want_nrm)
            worst = max(worst, err / R.bound(want_nrm))
        else:
            assert want_nrm is None
    print(f"{name} normals={normals}: worst error / bound = {worst:.3f}")
