"""Host side of the device normalisation of a store (deltaconv_amd/csrc/shape_norm_math.h, ``DeviceDataset.normalize``,
``DeviceMeshDataset.normalize``, ``subset``, ``loader.random_split``), without a GPU: a g++ build of shape_norm_math.h
(tests/hostcheck_shapenorm) against the numpy restatement (tests/shape_norm_restate.py) bit for bit, the restatement and the host
transforms ``T.NormalizeScale / NormalizeArea / NormalizeAxes`` against the fp64 formulas within 8 u per op
(u = 2^-24 * scale * max|input|: seven fp32 roundings separate an op's output from its fp64 evaluation), the edge cases of the
axis order, and the host logic of the translator, the subsets and the seeded split."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd import DeviceDataset, DeviceMeshDataset, random_split
from deltaconv_amd.datasets import Compose, Data
from deltaconv_amd.geometry.shape_norm import degenerate_from_stats
from deltaconv_amd.loader import translate_normalize
from tests import shape_norm_restate as R
from tests.helpers import ROOT

HN_DIR = os.path.join(ROOT, "tests", "hostcheck_shapenorm")
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
INF = float("inf")
FACES = (1, 2, 63, 64, 65, 255, 256, 257, 515, 2051, R.T - 1, R.T, R.T + 1)
SINGLE = {"scale2": [R.scale(2)], "scale_inf": [R.scale(INF)], "scale_const": [R.scale(2, 1.7)], "area": [R.area()],
          "axes": [R.axes()]}
HOST = {"scale2": T.NormalizeScale(), "scale_inf": T.NormalizeScale(norm_ord=INF), "scale_const": T.NormalizeScale(scaling_factor=1.7),
        "area": T.NormalizeArea(), "axes": T.NormalizeAxes()}


@pytest.fixture(scope="module")
def hn():
    subprocess.run(["make", "-s", "-C", HN_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HN_DIR, "libhostcheck_shapenorm.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hn_normalize.argtypes, lib.hn_normalize.restype = [vp, i64, vp, i64, vp, vp, i32, vp, vp, vp], ctypes.c_int
    lib.hn_threads.argtypes, lib.hn_threads.restype = [], i32
    assert lib.hn_threads() == R.T
    return lib


def host_normalize(hn, pos, ops, face=None, norm=None, in_place=False):
    pos = np.ascontiguousarray(pos, dtype=np.float32).copy()
    face = None if face is None else np.ascontiguousarray(face, dtype=np.int32)
    out = pos if in_place else np.full_like(pos, np.nan)
    norm = None if norm is None else np.ascontiguousarray(norm, dtype=np.float32).copy()
    codes = np.array([o[0] for o in ops], dtype=np.int32)
    params = np.array([[o[1], o[2]] for o in ops], dtype=np.float32)
    stats = np.full((len(ops), 8), np.nan, dtype=np.float32)
    rc = hn.hn_normalize(P(pos), pos.shape[0], P(face), 0 if face is None else face.shape[0], P(codes), P(params), len(ops), P(out),
                         P(norm), P(stats))
    assert rc == 0
    return out, norm, stats


def small_shape(n_vert, n_face, i):
    """n_vert rows of a stretched test mesh with n_face random triangles over them."""
    pos, _, _ = R.test_mesh(2 * max(n_vert, 9), i)
    rng = np.random.default_rng(50 + i)
    return pos[:n_vert].copy(), rng.integers(0, n_vert, size=(n_face, 3))


_cache = {}


def mesh(i):
    if i not in _cache:
        _cache[i] = R.test_mesh(FACES[i], i)
    return _cache[i]


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


# ---- g++ build of shape_norm_math.h = the restatement, bit for bit -------------------------------------------------------------
CHAINS = dict(SINGLE, area_axes=[R.area(), R.axes()], four=[R.scale(2), R.axes(), R.area(), R.scale(INF)])


@pytest.mark.parametrize("name", CHAINS)
def test_hostcheck_equals_the_restatement_bitwise(hn, name):
    ops = CHAINS[name]
    t = R.T
    shapes = [mesh(i)[:2] for i in (0, 3, 9, 11)]
    shapes += [small_shape(v, f, k) for k, (v, f) in enumerate(((1, 1), (2, 3), (3, 1), (t - 1, t + 1), (t, t), (t + 1, t - 1),
                                                                  (2 * t + 3, 2 * t + 3)))]
    for pos, face in shapes:
        rng = np.random.default_rng(pos.shape[0])
        nrm = rng.standard_normal(pos.shape).astype(np.float32)
        got = host_normalize(hn, pos, ops, face, nrm)
        want = R.normalize(pos, ops, face, nrm)
        assert same_bits(got[0], want[0]) and same_bits(got[2], want[2]) and same_bits(got[1], want[1]), (name, pos.shape)
        assert same_bits(host_normalize(hn, pos, ops, face, in_place=True)[0], want[0])


def test_the_ordered_sum_is_the_strided_partials_and_the_two_trees():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, R.T - 1, R.T, R.T + 1, 2 * R.T + 3):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, size=n)
        part = [0.0] * R.T
        for i, x in enumerate(v):
            part[i % R.T] = part[i % R.T] + float(x)
        for w in range(R.T // 64):
            o = 32
            while o:
                for i in range(o):
                    part[64 * w + i] += part[64 * w + i + o]
                o //= 2
        o = R.T // 128
        while o:
            for i in range(o):
                part[64 * i] += part[64 * (i + o)]
            o //= 2
        assert R.ordered_sum(v) == part[0]


# ---- against the fp64 formulas and the host classes ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_restatement_and_host_class_are_within_8_units_of_fp64(name):
    worst_r = worst_h = 0.0
    for i in range(len(FACES)):
        pos, face, _ = mesh(i)
        want, info = R.exact(pos, SINGLE[name], face)
        u = R.unit(pos, info[0][0])
        got, _, stats = R.normalize(pos, SINGLE[name], face)
        assert stats[0, 4:7].tolist() == info[0][1], (name, FACES[i])
        err_r = float(np.abs(got.astype(np.float64) - want).max()) / u
        host = HOST[name](Data(pos=torch.from_numpy(pos.copy()), face=torch.from_numpy(face))).pos.numpy()
        err_h = float(np.abs(host.astype(np.float64) - want).max()) / u
        print(f"{name} F={FACES[i]}: restatement {err_r:.2f} u, host class {err_h:.2f} u")
        assert err_r <= R.BOUND_UNITS and err_h <= R.BOUND_UNITS, (name, FACES[i], err_r, err_h)
        worst_r, worst_h = max(worst_r, err_r), max(worst_h, err_h)
    print(f"{name}: worst restatement {worst_r:.2f} u, worst host class {worst_h:.2f} u (bound {R.BOUND_UNITS})")


def test_the_permutation_is_the_stable_argsort_of_the_fp64_deviations():
    seen = set()
    for i in range(len(FACES)):
        pos, face, _ = mesh(i)
        std = np.sort(pos.astype(np.float64).std(axis=0, ddof=1))
        assert std[1] / std[0] > 1.13 and std[2] / std[1] > 1.13            # the order does not rest on luck
        want = np.argsort(pos.astype(np.float64).std(axis=0, ddof=1), kind="stable").tolist()
        assert R.normalize(pos, [R.axes()])[2][0, 4:7].tolist() == want
        # after AREA (a uniform scaling) the order is the same
        assert R.normalize(pos, [R.area(), R.axes()], face)[2][1, 4:7].tolist() == want
        seen.add(tuple(want))
    assert len(seen) == 6                                                    # every permutation occurs


def test_a_chain_equals_its_ops_applied_one_at_a_time_bitwise(hn):
    for i in (2, 5, 9, 12):
        pos, face, _ = mesh(i)
        nrm = np.random.default_rng(i).standard_normal(pos.shape).astype(np.float32)
        for ops in ([R.area(), R.axes()], [R.axes(), R.scale(INF), R.axes(), R.area()]):
            whole = host_normalize(hn, pos, ops, face, nrm)
            p, n = pos, nrm
            for k, op in enumerate(ops):
                p, n, st = host_normalize(hn, p, [op], face, n)
                assert same_bits(st[0], whole[2][k])
            assert same_bits(p, whole[0]) and same_bits(n, whole[1])


def test_area_then_axes_equals_centring_then_axes_within_16_units():
    """What survives of NormalizeArea in front of NormalizeAxes is its centring (the uniform scale cancels), so the reference's
    reading of ``face[:, 1]`` and the true area give the same ShapeSeg shapes."""
    for i in range(len(FACES)):
        pos, face, _ = mesh(i)
        a, _, sa = R.normalize(pos, [R.area(), R.axes()], face)
        centred = (pos - R.centre(pos)).astype(np.float32)
        b, _, sb = R.normalize(centred, [R.axes()])
        assert sa[1, 4:7].tolist() == sb[0, 4:7].tolist()
        u = R.unit(pos, float(sa[0, 3]) * float(sa[1, 3]))
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / u
        print(f"F={FACES[i]}: {err:.2f} u")
        assert err <= 2 * R.BOUND_UNITS, (FACES[i], err)


# ---- edge cases ----------------------------------------------------------------------------------------------------------------
def test_exact_ties_and_a_single_point_keep_the_identity_order(hn):
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    for pos in (cube, cube * np.float32(0.375) + np.float32(2.0)):
        got = host_normalize(hn, pos, [R.axes()])
        assert got[2][0, 4:7].tolist() == [0, 1, 2] and same_bits(got[0], R.normalize(pos, [R.axes()])[0])
    assert np.array_equal(host_normalize(hn, cube, [R.axes()])[0], cube * np.float32(0.5))
    one = np.array([[0.3, -1.5, 0.7]], dtype=np.float32)
    got = host_normalize(hn, one, [R.axes()])
    assert got[2][0, 4:7].tolist() == [0, 1, 2] and same_bits(got[0], R.normalize(one, [R.axes()])[0])
    assert np.array_equal(got[0], one * (np.float32(1) / np.float32(1.4)))
    # a NaN variance moves nothing either: two axes tie, the third is NaN
    bad = np.array([[0, 1, np.nan], [1, 0, 0]], dtype=np.float32)
    assert host_normalize(hn, bad, [R.axes()])[2][0, 4:7].tolist() == [0, 1, 2]
    assert R.normalize(bad, [R.axes()])[2][0, 4:7].tolist() == [0, 1, 2]


def test_a_mesh_without_area_gets_an_infinite_scale_and_is_flagged(hn):
    flat = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=np.float32)               # collinear: every face has area 0
    flat_face = np.array([[0, 1, 2], [1, 2, 3], [0, 0, 1]])
    shapes = [mesh(2)[:2], (flat, flat_face), mesh(4)[:2]]
    ops = [R.area(), R.axes()]
    stats = np.stack([host_normalize(hn, p, ops, f)[2] for p, f in shapes])
    assert np.isposinf(stats[1, 0, 3]) and same_bits(stats[1], R.normalize(flat, ops, flat_face)[2])
    assert degenerate_from_stats(stats).tolist() == [False, True, False]
    for k in (0, 2):                                                            # the other shapes are what they are alone
        assert same_bits(host_normalize(hn, *shapes[k][:1], ops, shapes[k][1])[0], R.normalize(shapes[k][0], ops, shapes[k][1])[0])
    # a face with an id out of range counts as zero and indexes nothing
    pos, face, _ = mesh(3)
    mixed = np.concatenate([face[:10], [[0, 1, pos.shape[0]], [-1, 2, 3]], face[10:]])
    assert same_bits(host_normalize(hn, pos, [R.area()], mixed)[0], host_normalize(hn, pos, [R.area()], face)[0])
    assert same_bits(R.normalize(pos, [R.area()], mixed)[0], R.normalize(pos, [R.area()], face)[0])
    # a negative scale is flagged as well
    assert degenerate_from_stats(np.array([[[0, 0, 0, -1, 0, 1, 2, 0]]], dtype=np.float32)).tolist() == [True]


# ---- the translator, the subsets and the split ---------------------------------------------------------------------------------
def test_translate_normalize_maps_the_host_transforms_and_refuses_the_rest():
    assert translate_normalize(T.NormalizeScale())[0][:2] == (1, 2.0) and np.isnan(translate_normalize(T.NormalizeScale())[0][2])
    assert translate_normalize(T.NormalizeScale(norm_ord=INF, scaling_factor=2))[0] == (1, INF, 2.0)
    assert [o[0] for o in translate_normalize([T.NormalizeArea(), T.NormalizeAxes(max_points=1000)], has_face=True)] == [2, 3]
    assert [o[0] for o in translate_normalize(Compose((T.NormalizeScale(), T.NormalizeAxes())))] == [1, 3]
    with pytest.raises(ValueError, match="NormalizeArea"):
        translate_normalize(T.NormalizeArea(), has_face=False)
    with pytest.raises(ValueError, match="RandomScale"):
        translate_normalize([T.NormalizeScale(), T.RandomScale((0.8, 1.2))])
    with pytest.raises(ValueError, match="norm_ord"):
        translate_normalize(T.NormalizeScale(norm_ord=1))
    with pytest.raises(ValueError, match="normalisation ops"):
        translate_normalize([T.NormalizeAxes()] * 5)
    with pytest.raises(ValueError, match="normalisation ops"):
        translate_normalize([])
    pos, face, y = mesh(2)
    item = Data(pos=torch.from_numpy(pos), face=torch.from_numpy(face.T.copy()), y=torch.from_numpy(y))
    with pytest.raises(ValueError, match="NormalizeArea"):
        DeviceDataset.from_dataset([item], "cpu").normalize(T.NormalizeArea())
    with pytest.raises(ValueError, match="GeodesicFPS"):
        DeviceMeshDataset.from_dataset([item], "cpu").normalize([T.NormalizeArea(), T.GeodesicFPS(8)])
    with pytest.raises(ValueError, match="HIP device"):                       # no CPU path
        DeviceMeshDataset.from_dataset([item], "cpu").normalize(T.NormalizeScale())
    with pytest.raises(ValueError, match="shapes_per_launch"):
        DeviceMeshDataset.from_dataset([item], "cpu").normalize(T.NormalizeScale(), shapes_per_launch=0)


def _mesh_items(sizes):
    items = []
    for i, f in enumerate(sizes):
        pos, face, y = R.test_mesh(f, i)
        items.append(Data(pos=torch.from_numpy(pos), face=torch.from_numpy(face.T.copy()), y=torch.from_numpy(y),
                          category=torch.eye(4)[i % 4]))
    return items


def test_subset_carries_rows_offsets_sizes_and_labels():
    items = _mesh_items([5, 40, 1, 17, 64])
    st = DeviceMeshDataset.from_dataset(items, "cpu")
    pick = [3, 0, 3, 4]
    sub = st.subset(pick)
    assert len(sub) == 4 and sub.n_faces.tolist() == [17, 5, 17, 64] and sub.n_verts.tolist() == [items[i].pos.shape[0] for i in pick]
    assert sub.vptr.tolist() == [0] + np.cumsum(sub.n_verts).tolist() and sub.fptr.tolist() == [0, 17, 22, 39, 103]
    for k, i in enumerate(pick):
        assert torch.equal(sub.vert[sub.vptr[k]:sub.vptr[k + 1]], items[i].pos)
        assert torch.equal(sub.face[sub.fptr[k]:sub.fptr[k + 1]].long(), items[i].face.t())
        assert torch.equal(sub.y_vert[sub.vptr[k]:sub.vptr[k + 1]], items[i].y)
        assert torch.equal(sub.category[k], items[i].category)
    assert sub.face.dtype == torch.int32 and sub.vert.is_contiguous() and sub.y_cloud is None
    # a point store: per-point labels, normals and features follow the rows; per-cloud labels follow the clouds
    clouds = [Data(pos=d.pos, norm=d.pos + 1, x=d.pos[:, :2] * 2, y=d.y) for d in items]
    ps = DeviceDataset.from_dataset(clouds, "cpu")
    sub = ps.subset(np.array([4, 1]))
    assert sub.sizes.tolist() == [items[4].pos.shape[0], items[1].pos.shape[0]] and sub.ptr.tolist() == [0] + np.cumsum(sub.sizes).tolist()
    for k, i in enumerate((4, 1)):
        rows = slice(int(sub.ptr[k]), int(sub.ptr[k + 1]))
        assert torch.equal(sub.pos[rows], items[i].pos) and torch.equal(sub.norm[rows], items[i].pos + 1)
        assert torch.equal(sub.x[rows], items[i].pos[:, :2] * 2) and torch.equal(sub.y_point[rows], items[i].y)
    for d, c in zip(clouds, (3, 1, 2, 0, 5)):
        d.y = torch.tensor([c])
    sub = DeviceDataset.from_dataset(clouds, "cpu").subset([2, 2, 0])
    assert sub.y_cloud.tolist() == [2, 2, 3] and sub.y_point is None
    assert len(ps.subset([])) == 0
    for bad in ([5], [-1]):
        with pytest.raises(ValueError, match="indices"):
            ps.subset(bad)
        with pytest.raises(ValueError, match="indices"):
            st.subset(bad)


@pytest.mark.parametrize("n, lengths, seed", [(10, [9, 1], 0), (37, [33, 4], 1), (37, [0.9, 0.1], 1), (8, [3, 3, 2], 7), (5, [5, 0], 3)])
def test_random_split_gives_torchs_index_sets(n, lengths, seed):
    items = _mesh_items([3 + (i % 5) for i in range(n)])
    for d, i in zip(items, range(n)):
        d.y = torch.tensor([i])                                               # the label names the shape
    want = torch.utils.data.random_split(range(n), lengths, generator=torch.Generator().manual_seed(seed))
    for store in (DeviceMeshDataset.from_dataset(items, "cpu"), DeviceDataset.from_dataset(items, "cpu")):
        parts = random_split(store, lengths, seed)
        assert [p.y_cloud.tolist() for p in parts] == [list(w.indices) for w in want]
        assert sorted(sum((p.y_cloud.tolist() for p in parts), [])) == list(range(n))
        sizes = store.n_verts if hasattr(store, "n_verts") else store.sizes
        for p, w in zip(parts, want):
            assert (p.n_verts if hasattr(p, "n_verts") else p.sizes).tolist() == sizes[list(w.indices)].tolist()
