"""Host side of the device surface sampler (deltaconv_amd/meshes.py, csrc/mesh_math.h), without a GPU: a g++ build of
mesh_math.h (tests/hostcheck_mesh) against the numpy restatement (tests/mesh_restate.py) bitwise, against ``T.SamplePoints``
run in fp64 on the restated draws (within 64 * 2^-24 * max(1, max |expected|)), the distribution of the picks and of the
barycentric coordinates (chi-square conditions), the edge cases of the weights, and the host logic of
``DeviceMeshDataset.from_dataset``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from deltaconv_amd.data import synthetic_mesh
from deltaconv_amd.datasets import Data
from deltaconv_amd.meshes import DeviceMeshDataset, MESH_MAX_FACES
from tests import mesh_restate as R
from tests.helpers import ROOT

HM_DIR = os.path.join(ROOT, "tests", "hostcheck_mesh")
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hm():
    subprocess.run(["make", "-s", "-C", HM_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HM_DIR, "libhostcheck_mesh.so"))
    vp, i32, u32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64
    lib.hm_cdf.argtypes, lib.hm_cdf.restype = [vp, i64, vp, i64, vp, vp, vp], u64
    lib.hm_sample.argtypes, lib.hm_sample.restype = [vp, i64, vp, i64, vp, vp, u32, i64, i64, i32, vp, vp, vp, vp, vp], None
    lib.hm_mulhi64.argtypes, lib.hm_mulhi64.restype = [u64, u64], u64
    return lib


def host_cdf(hm, vert, face):
    vert, face = np.ascontiguousarray(vert, dtype=np.float32), np.ascontiguousarray(face, dtype=np.int32)
    f = face.shape[0]
    area, w, cdf = np.empty(f), np.empty(f, dtype=np.uint64), np.empty(f, dtype=np.uint64)
    total = hm.hm_cdf(P(vert), vert.shape[0], P(face), f, P(area), P(w), P(cdf))
    return area, w, cdf, int(total)


def host_sample(hm, vert, face, num, seed=0, rnd=0, mesh=0, y_vert=None):
    vert, face = np.ascontiguousarray(vert, dtype=np.float32), np.ascontiguousarray(face, dtype=np.int32)
    _, w, cdf, total = host_cdf(hm, vert, face)
    pos, norm = np.full((num, 3), np.nan, dtype=np.float32), np.full((num, 3), np.nan, dtype=np.float32)
    y = None if y_vert is None else np.full(num, -7, dtype=np.int64)
    fid, f12 = np.full(num, -7, dtype=np.int32), np.full((num, 2), np.nan, dtype=np.float32)
    yv = None if y_vert is None else np.ascontiguousarray(y_vert, dtype=np.int64)
    hm.hm_sample(P(vert), vert.shape[0], P(face), face.shape[0], P(cdf), P(yv), seed, rnd, mesh, num, P(pos), P(norm), P(y),
                 P(fid), P(f12))
    return dict(face_id=fid.astype(np.int64), f1=f12[:, 0].copy(), f2=f12[:, 1].copy(), pos=pos, norm=norm, y=y, w=w, cdf=cdf,
                total=total)


def mesh_np(n_faces, seed=0, tiny=False, labels=True, **kw):
    """-> (vert float32 [V,3], face int64 [F,3], y_vert int64 [V]) of a synthetic mesh, optionally with a 2^-40 face."""
    pos, face, y = synthetic_mesh(n_faces, seed, labels=True, **kw)
    if tiny:
        pos, face = R.with_tiny_face(pos, face)
        y = torch.cat([y, torch.tensor([1, 2, 3])])
    return pos.numpy(), face.t().contiguous().numpy(), y.numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


MESHES = [dict(n_faces=1), dict(n_faces=2, zero_area=1), dict(n_faces=63, tiny=True), dict(n_faces=300, zero_area=5, shrink=(40, 0.01)),
          dict(n_faces=2051, zero_area=3, tiny=True)]


# ---- g++ build of mesh_math.h = the restatement, bit for bit ------------------------------------------------------------------
def test_mulhi64_is_the_high_half_of_the_product(hm):
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.integers(0, 2 ** 64, size=500, dtype=np.uint64), np.array([0, 1, 2 ** 64 - 1, 2 ** 32, 2 ** 32 - 1], dtype=np.uint64)])
    b = np.concatenate([rng.integers(0, 2 ** 57, size=500, dtype=np.uint64), np.array([2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1, 2 ** 32, 1], dtype=np.uint64)])
    want = [(int(x) * int(y)) >> 64 for x, y in zip(a, b)]
    assert [int(v) for v in R.mulhi64(a, b)] == want
    assert [int(hm.hm_mulhi64(int(x), int(y))) for x, y in zip(a, b)] == want


@pytest.mark.parametrize("spec", MESHES, ids=lambda s: f"F{s['n_faces']}")
def test_hostcheck_equals_the_restatement_bitwise(hm, spec):
    vert, face, y = mesh_np(seed=3, **spec)
    area, w, cdf, total = host_cdf(hm, vert, face)
    assert np.array_equal(area.view(np.uint64), R.areas(vert, face).view(np.uint64))
    rw, rcdf = R.cdf_of(vert, face)
    assert np.array_equal(w, rw) and np.array_equal(cdf, rcdf) and total == int(rcdf[-1]) > 0
    assert int(w.max()) == 2 ** 32 and (w[area == 0] == 0).all()
    for seed, rnd, mesh, num in ((0, 0, 0, 257), (1, 7, 9839, 1000), (2 ** 32 - 1, 2 ** 33 + 3, 2 ** 32 - 1, 64)):
        got = host_sample(hm, vert, face, num, seed, rnd, mesh, y)
        want = R.sample(vert, face, num, seed, rnd, mesh, y)
        assert np.array_equal(got["face_id"], want["face_id"])
        assert np.array_equal(bits(got["f1"]), bits(want["f1"])) and np.array_equal(bits(got["f2"]), bits(want["f2"]))
        assert np.array_equal(bits(got["pos"]), bits(want["pos"])) and np.array_equal(bits(got["norm"]), bits(want["norm"]))
        assert np.array_equal(got["y"], want["y"])
        assert (w[got["face_id"]] > 0).all()                          # zero-weight faces are never picked


# ---- against the host class -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", MESHES[1:], ids=lambda s: f"F{s['n_faces']}")
def test_points_normals_and_labels_match_sample_points_in_fp64(hm, spec):
    vert, face, y = mesh_np(seed=5, **spec)
    worst = 0.0
    for seed, rnd, mesh in ((0, 0, 0), (4, 2, 77)):
        got = host_sample(hm, vert, face, 1000, seed, rnd, mesh, y)
        want_pos, want_norm, want_y = R.expected(vert, face, 1000, seed, rnd, mesh, y)
        for g, w in ((got["pos"], want_pos), (got["norm"], want_norm)):
            err = float((torch.from_numpy(g).double() - w).abs().max())
            assert err <= R.bound(w), (spec, err, R.bound(w))
            worst = max(worst, err / R.bound(w))
        assert np.array_equal(got["y"], want_y.numpy())
    print(f"{spec}: worst error / bound = {worst:.3f}")


# ---- distribution -------------------------------------------------------------------------------------------------------------------
def strip_mesh(widths):
    """One right triangle per entry, in its own plane z = k: legs (width, 1), so the areas are proportional to `widths`."""
    vert, face = [], []
    for k, a in enumerate(widths):
        vert += [[0, 0, k], [a, 0, k], [0, 1, k]]
        face.append([3 * k, 3 * k + 1, 3 * k + 2])
    return np.array(vert, dtype=np.float32), np.array(face, dtype=np.int64)


@pytest.mark.parametrize("seed", range(5))
def test_picks_follow_the_areas_and_the_fold_is_uniform(hm, seed):
    from scipy.stats import chi2
    n = 200_000
    widths = np.arange(1, 65, dtype=np.float64)
    dead = [6, 40]
    widths[dead] = 0
    vert, face = strip_mesh(widths)
    got = host_sample(hm, vert, face, n, seed=seed)
    counts = np.bincount(got["face_id"], minlength=64)
    assert counts[dead].sum() == 0
    live = widths > 0
    want = n * widths[live] / widths[live].sum()
    stat = float((((counts[live] - want) ** 2) / want).sum())
    assert stat < chi2.ppf(0.999, 61), stat
    # the four congruent sub-triangles of the midpoint subdivision of the (f1, f2) triangle
    f1, f2 = got["f1"].astype(np.float64), got["f2"].astype(np.float64)
    # the fold tests the fp32 sum, as the reference does: both fractions are multiples of 2^-24, so the one exact sum above 1
    # that stays unfolded is 1 + 2^-24 (a tie that rounds to the even 1.0f) -- the sample then lies 2^-24 outside the edge
    assert float((got["f1"] + got["f2"]).max()) <= 1.0 and float((f1 + f2).max()) <= 1.0 + 2.0 ** -24
    assert float(f1.min()) >= 0.0 and float(f2.min()) >= 0.0
    region = np.where(f1 >= 0.5, 0, np.where(f2 >= 0.5, 1, np.where(f1 + f2 <= 0.5, 2, 3)))
    cells = np.bincount(region, minlength=4)
    stat2 = float((((cells - n / 4) ** 2) / (n / 4)).sum())
    assert stat2 < chi2.ppf(0.999, 3), stat2
    print(f"seed {seed}: chi2 faces {stat:.1f} (< {chi2.ppf(0.999, 61):.1f}), fold {stat2:.2f} (< {chi2.ppf(0.999, 3):.1f}), "
          f"max(f1 + f2) = {float((f1 + f2).max()):.9f}")


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------
def test_a_face_2_to_the_minus_40_of_the_largest_has_weight_zero(hm):
    pos, face = synthetic_mesh(40, 1)
    pos, face = R.with_tiny_face(pos, face)
    vert, fc = pos.numpy(), face.t().contiguous().numpy()
    area, w, cdf, total = host_cdf(hm, vert, fc)
    ratio = area[-1] / area.max()
    assert 2.0 ** -41 < ratio < 2.0 ** -39 and w[-1] == 0 and cdf[-1] == cdf[-2]
    assert R.cdf_of(vert, fc)[0][-1] == 0
    assert not (host_sample(hm, vert, fc, 5000)["face_id"] == 40).any()
    # 2^-31 of the largest still counts: weight 2
    pos2, face2 = R.with_tiny_face(*synthetic_mesh(40, 1), factor=2.0 ** -31 * 1.0001)
    assert host_cdf(hm, pos2.numpy(), face2.t().contiguous().numpy())[1][-1] == 2


def test_an_all_degenerate_mesh_picks_uniformly_by_index(hm):
    vert = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=np.float32)           # collinear: every area is 0
    face = np.array([[0, 1, 2], [1, 2, 3], [0, 0, 1], [3, 3, 3], [0, 2, 3], [1, 1, 1], [2, 1, 0]], dtype=np.int64)
    got = host_sample(hm, vert, face, 7000, seed=2, y_vert=np.arange(4))
    want = R.sample(vert, face, 7000, seed=2, y_vert=np.arange(4))
    assert got["total"] == 0 == want["total"] and not got["cdf"].any()
    assert np.array_equal(got["face_id"], want["face_id"]) and np.array_equal(bits(got["pos"]), bits(want["pos"]))
    u = R.draws(2, 0, 0, 7000)
    assert np.array_equal(got["face_id"], [((int(x) << 32 | int(y)) * 7) >> 64 for x, y in zip(u[0], u[1])])
    counts = np.bincount(got["face_id"], minlength=7)
    assert counts.min() > 850 and counts.max() < 1150                      # 1000 each, sigma 29
    assert not got["norm"].any() and np.array_equal(got["y"], face[got["face_id"], 0])


def test_a_face_id_out_of_range_is_never_indexed(hm):
    vert, face, y = mesh_np(20, seed=2)
    v = vert.shape[0]
    bad = np.array([[0, 1, v], [-1, 2, 3], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1]], dtype=np.int64)
    mixed = np.concatenate([face[:10], bad, face[10:]])
    area, w, cdf, total = host_cdf(hm, vert, mixed)
    assert (area[10:14] == 0).all() and (w[10:14] == 0).all() and (R.cdf_of(vert, mixed)[1] == cdf).all()
    got = host_sample(hm, vert, mixed, 3000, y_vert=y)
    assert not np.isin(got["face_id"], [10, 11, 12, 13]).any()
    # only such faces: total = 0, the pick is by index and the sample is a zero row with label -1
    got = host_sample(hm, vert, bad, 100, y_vert=y)
    want = R.sample(vert, bad, 100, y_vert=y)
    assert got["total"] == 0 and not got["pos"].any() and not got["norm"].any() and (got["y"] == -1).all()
    assert np.array_equal(got["face_id"], want["face_id"]) and (want["y"] == -1).all() and not want["pos"].any()


def test_the_sample_is_a_function_of_seed_round_and_dataset_index(hm):
    vert, face, y = mesh_np(300, seed=4)
    base = host_sample(hm, vert, face, 500, seed=3, rnd=5, mesh=11)
    again = host_sample(hm, vert, face, 500, seed=3, rnd=5, mesh=11)
    assert all(np.array_equal(bits(base[k]), bits(again[k])) for k in ("pos", "norm")) and np.array_equal(base["face_id"], again["face_id"])
    for other in (dict(seed=4, rnd=5, mesh=11), dict(seed=3, rnd=6, mesh=11), dict(seed=3, rnd=5 + 2 ** 32, mesh=11),
                  dict(seed=3, rnd=5, mesh=12)):
        o = host_sample(hm, vert, face, 500, **other)
        assert np.mean(o["face_id"] == base["face_id"]) < 0.05 and np.mean(np.all(o["pos"] == base["pos"], axis=1)) < 0.01, other


# ---- synthetic meshes and the host logic of the store -----------------------------------------------------------------------------
def test_synthetic_mesh_options():
    pos, face = synthetic_mesh(200, 1)
    assert pos.dtype == torch.float32 and face.dtype == torch.int64 and tuple(face.shape) == (3, 200)
    assert int(face.min()) == 0 and int(face.max()) < pos.shape[0]
    a = R.areas(pos.numpy(), face.t().numpy())
    assert a.min() > 0 and a.max() / a.min() > 1.5                           # areas differ
    assert torch.equal(synthetic_mesh(200, 1)[0], pos) and not torch.equal(synthetic_mesh(200, 2)[0], pos)
    for f in (1, 2, 17, 18, 19, 1023):
        assert synthetic_mesh(f)[1].shape[1] == f
    # a closed torus: every edge is shared by two faces
    pos, face = synthetic_mesh(2 * 12 * 12)
    e = torch.cat([face[[0, 1]], face[[1, 2]], face[[2, 0]]], dim=1).sort(0).values
    assert (torch.unique(e, dim=1, return_counts=True)[1] == 2).all()
    pz, fz = synthetic_mesh(50, 1, zero_area=4)
    az = R.areas(pz.numpy(), fz.t().numpy())
    assert fz.shape[1] == 54 and (az[50:] == 0).all() and (az[:50] > 0).all()
    ps, fs, ys = synthetic_mesh(50, 1, shrink=(10, 0.25), labels=True)
    a0, a1 = R.areas(*[t.numpy() for t in (synthetic_mesh(50, 1)[0], synthetic_mesh(50, 1)[1].t())]), R.areas(ps.numpy(), fs.t().numpy())
    assert np.allclose(a1[:10], a0[:10] / 16, rtol=1e-4) and np.allclose(a1[10:], a0[10:]) and ys.shape == (ps.shape[0],)


def _items(sizes, y="cloud", category=False):
    items = []
    for i, f in enumerate(sizes):
        pos, face, yv = synthetic_mesh(f, i, labels=True)
        d = Data(pos=pos, face=face)
        if y == "cloud":
            d.y = torch.tensor([i % 3])
        elif y == "vertex":
            d.y = yv
        if category:
            d.category = torch.eye(4)[i % 4]
        items.append(d)
    return items


def test_from_dataset_builds_one_store_with_local_face_ids():
    items = _items([5, 40, 1], y="vertex", category=True)
    st = DeviceMeshDataset.from_dataset(items, "cpu")
    assert len(st) == 3 and list(st.n_faces) == [5, 40, 1] and list(st.n_verts) == [d.pos.shape[0] for d in items]
    assert st.face.dtype == torch.int32 and tuple(st.face.shape) == (46, 3) and st.vert.dtype == torch.float32
    assert st.vptr.tolist() == [0] + np.cumsum(st.n_verts).tolist() and st.fptr.tolist() == [0, 5, 45, 46]
    for i, d in enumerate(items):
        assert torch.equal(st.face[st.fptr[i]:st.fptr[i + 1]].long(), d.face.t())                   # local ids, one row per triangle
        assert torch.equal(st.vert[st.vptr[i]:st.vptr[i + 1]], d.pos)
        assert torch.equal(st.y_vert[st.vptr[i]:st.vptr[i + 1]], d.y)
    assert st.y_cloud is None and tuple(st.category.shape) == (3, 4)
    st = DeviceMeshDataset.from_dataset(_items([5, 40, 1], y="cloud"), "cpu")
    assert st.y_vert is None and st.y_cloud.tolist() == [0, 1, 2] and st.category is None

    class _DS:                                       # a dataset object: .items is taken, .transform is not run
        items, transform = _items([3, 4], y=None), staticmethod(lambda d: 1 / 0)
    st = DeviceMeshDataset.from_dataset(_DS(), "cpu")
    assert len(st) == 2 and st.y_vert is None and st.y_cloud is None
    with pytest.raises(ValueError, match="include_labels"):
        st.sample_points(8, include_labels=True)
    with pytest.raises(ValueError, match="HIP device"):      # no CPU path
        st.sample_points(8)


def test_from_dataset_refuses_what_the_kernel_must_not_see():
    ok = _items([6])[0]
    bad = lambda **kw: [Data(**dict(dict(pos=ok.pos, face=ok.face, y=ok.y), **kw))]
    with pytest.raises(ValueError, match="empty"):
        DeviceMeshDataset.from_dataset([], "cpu")
    with pytest.raises(ValueError, match="outside"):
        DeviceMeshDataset.from_dataset(bad(face=torch.tensor([[0], [1], [ok.pos.shape[0]]])), "cpu")
    with pytest.raises(ValueError, match="outside"):
        DeviceMeshDataset.from_dataset(bad(face=torch.tensor([[0], [-1], [2]])), "cpu")
    with pytest.raises(ValueError, match="faces"):
        DeviceMeshDataset.from_dataset(bad(face=torch.zeros((3, 0), dtype=torch.long)), "cpu")
    with pytest.raises(ValueError, match="faces"):
        DeviceMeshDataset.from_dataset(bad(face=torch.zeros((1, 3), dtype=torch.long).expand(MESH_MAX_FACES + 1, 3).t()), "cpu")
    with pytest.raises(ValueError, match=r"\[3,F\]"):
        DeviceMeshDataset.from_dataset(bad(face=ok.face.t().contiguous()[:, :2]), "cpu")
    with pytest.raises(ValueError, match="V >= 1"):
        DeviceMeshDataset.from_dataset(bad(pos=torch.zeros((0, 3))), "cpu")
    with pytest.raises(ValueError, match="no pos / face"):
        DeviceMeshDataset.from_dataset(bad(face=None), "cpu")
    with pytest.raises(ValueError, match="one label per cloud or one per vertex"):
        DeviceMeshDataset.from_dataset(bad(y=torch.tensor([1, 2])), "cpu")
    with pytest.raises(ValueError, match="integers"):
        DeviceMeshDataset.from_dataset(bad(y=torch.tensor([0.5])), "cpu")
    for kw in (dict(num=0), dict(num=4, seed=2 ** 32), dict(num=4, round=-1), dict(num=4, meshes_per_launch=0),
               dict(num=4, meshes_per_launch=65536)):
        with pytest.raises(ValueError, match="sample_points"):
            DeviceMeshDataset.from_dataset([ok], "cpu").sample_points(**kw)
