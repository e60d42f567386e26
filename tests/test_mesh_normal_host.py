"""Host side of the per-vertex normals of a mesh store (csrc/mesh_normal_math.h, deltaconv_amd/geometry/mesh_normals.py,
``DeviceMeshDataset.vertex_cloud``, ``T.GenerateMeshNormals``), without a GPU: a g++ build of mesh_normal_math.h
(tests/hostcheck_mesh_normal) against the numpy restatement (tests/mesh_normal_restate.py) bit for bit -- lists and normals, both
weightings --, the restatement and the host transform against the fp64 evaluation of the same formula within the bound the header
derives, ``((8 sum w_f + (L + 4) sum |t_f|) 2^-24) / |s64| + 4 * 2^-24`` per vertex, the closed torus, and the host logic of
``vertex_cloud``.

Measured with these constants on the seven meshes below (both weightings): largest error / bound 0.075 (restatement) and 0.075
(host transform); largest error 1.4e-7 on the six synthetic meshes and 1.1e-6 on the fan (its hub: the sequential sum of a list
of 300 corners); largest bound of any vertex 6.4e-6 there and 4.5e-5 on the fan -- none above 1e-3, so no
vertex with a non-zero sum is left out of the comparison."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd.datasets import Data
from deltaconv_amd.meshes import DeviceMeshDataset
from tests import mesh_normal_restate as R
from tests.helpers import ROOT

HN_DIR = os.path.join(ROOT, "tests", "hostcheck_mesh_normal")
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
WEIGHTINGS = ("uniform", "area")
CODE = {"uniform": 0, "area": 1}


@pytest.fixture(scope="module")
def hn():
    subprocess.run(["make", "-s", "-C", HN_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HN_DIR, "libhostcheck_mesh_normal.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hn_lists.argtypes, lib.hn_lists.restype = [vp, vp, vp, i32, i64, i64, vp, vp], i64
    lib.hn_normals.argtypes, lib.hn_normals.restype = [vp, vp, vp, vp, i32, i64, i64, vp, vp, i32, vp, vp], None
    lib.hn_contribution.argtypes, lib.hn_contribution.restype = [vp, vp, vp, i32, vp], None
    return lib


def host_lists(hn, face, vptr, fptr, nv):
    vf_ptr, vf_edge = np.full(nv + 1, -7, dtype=np.int64), np.full(3 * face.shape[0], -7, dtype=np.int64)
    n = hn.hn_lists(P(face), P(vptr), P(fptr), len(vptr) - 1, nv, face.shape[0], P(vf_ptr), P(vf_edge))
    return vf_ptr, vf_edge, int(n)


def host_normals(hn, vert, face, vptr, fptr, vf, weighting):
    out = np.full(vert.shape, np.nan, dtype=np.float32)
    zero = np.full(len(vptr) - 1, -7, dtype=np.int32)
    hn.hn_normals(P(vert), P(face), P(vptr), P(fptr), len(vptr) - 1, vert.shape[0], face.shape[0], P(vf[0]), P(vf[1]), CODE[weighting],
                  P(out), P(zero))
    return out, zero


def one(i):
    return R.store_arrays([R.meshes()[i]])


# ---- g++ build of mesh_normal_math.h = the restatement, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize("i", range(7), ids=R.NAMES)
def test_hostcheck_equals_the_restatement_bitwise(hn, i):
    vert, face, vptr, fptr = one(i)
    vf_ptr, vf_edge, n = host_lists(hn, face, vptr, fptr, vert.shape[0])
    want_ptr, want_edge = R.lists(face, vptr, fptr, vert.shape[0])
    assert n == 3 * face.shape[0] and np.array_equal(vf_ptr, want_ptr) and np.array_equal(vf_edge, want_edge)
    for w in WEIGHTINGS:
        got, zero = host_normals(hn, vert, face, vptr, fptr, (vf_ptr, vf_edge), w)
        want, want_zero = R.normals(vert, face, vptr, fptr, w)
        assert np.array_equal(R.bits(got), R.bits(want)), (R.NAMES[i], w)
        assert np.array_equal(zero, want_zero)


def test_hostcheck_equals_the_restatement_on_the_whole_store_and_its_reverse(hn):
    """All seven meshes in one store, forwards and backwards: the same bits per mesh as on its own."""
    alone = [R.normals(*one(i), "uniform")[0] for i in range(7)]
    for order in (list(range(7)), list(range(6, -1, -1))):
        vert, face, vptr, fptr = R.store_arrays([R.meshes()[i] for i in order])
        vf_ptr, vf_edge, _ = host_lists(hn, face, vptr, fptr, vert.shape[0])
        assert np.array_equal(vf_edge, R.lists(face, vptr, fptr, vert.shape[0])[1])
        got, zero = host_normals(hn, vert, face, vptr, fptr, (vf_ptr, vf_edge), "uniform")
        want, want_zero = R.normals(vert, face, vptr, fptr, "uniform")
        assert np.array_equal(R.bits(got), R.bits(want)) and np.array_equal(zero, want_zero)
        for k, i in enumerate(order):
            assert np.array_equal(R.bits(got[vptr[k]:vptr[k + 1]]), R.bits(alone[i])), R.NAMES[i]
    assert want_zero.tolist()[::-1] == [6, 5, 0, 12, 0, 0, 0]         # the unreferenced vertices of F = 1, F = 2 and F = 300


def test_face_contributions(hn):
    rng = np.random.default_rng(5)
    tri = rng.standard_normal((200, 3, 3)).astype(np.float32)
    tri[:5, 1] = tri[:5, 0]                                            # zero area: corner 1 on corner 0
    vert, face = tri.reshape(-1, 3), np.arange(600, dtype=np.int64).reshape(200, 3)
    ptr = np.array([0, 600], dtype=np.int64)
    for w in WEIGHTINGS:
        want = R.contributions(vert, face, ptr, np.array([0, 200]), w)
        got = np.empty_like(want)
        for f in range(200):
            hn.hn_contribution(P(tri[f, 0]), P(tri[f, 1]), P(tri[f, 2]), CODE[w], P(got[f]))
        assert np.array_equal(R.bits(got), R.bits(want)) and not got[:5].any()
    unit = R.contributions(vert, face, ptr, np.array([0, 200]), "uniform")[5:]
    assert np.abs(np.linalg.norm(unit.astype(np.float64), axis=1) - 1).max() <= 4 * R.U


# ---- lists -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(7), ids=R.NAMES)
def test_lists_hold_every_corner_once_in_ascending_order(i):
    vert, face, vptr, fptr = one(i)
    vf_ptr, vf_edge = R.lists(face, vptr, fptr, vert.shape[0])
    assert np.array_equal(np.sort(vf_edge), np.arange(3 * face.shape[0]))                  # every corner exactly once
    assert np.array_equal(np.diff(vf_ptr), np.bincount(face.reshape(-1), minlength=vert.shape[0]))
    owner = np.repeat(np.arange(vert.shape[0]), np.diff(vf_ptr))
    assert np.array_equal(face.reshape(-1)[vf_edge], owner)                                # ... in its own vertex's list
    same = owner[1:] == owner[:-1]
    assert (np.diff(vf_edge)[same] > 0).all()                                              # ascending within a vertex
    if i == R.FAN:
        assert int(np.diff(vf_ptr).max()) == R.FAN_FACES > 64 and int(np.diff(vf_ptr)[0]) == R.FAN_FACES


# ---- against fp64 -------------------------------------------------------------------------------------------------------------------------
def check_against_fp64(n32, vert, face, vptr, fptr, w, what):
    n64, bound, s_zero = R.expected64(vert, face, vptr, fptr, w)
    assert not n32[s_zero].any() and not n64[s_zero].any()            # an exactly zero sum: the zero vector on both sides
    live = ~s_zero
    if not live.any():
        return 0.0, 0.0, 0.0
    err = np.abs(n32[live].astype(np.float64) - n64[live]).max(axis=1)
    ratio = float((err / bound[live]).max())
    print(f"{what} {w}: {int(live.sum())} vertices, largest error {err.max():.3g}, largest error / bound {ratio:.3f}, "
          f"largest bound {bound[live].max():.3g}")
    assert (err <= bound[live]).all(), (what, w, ratio)
    return ratio, float(err.max()), float(bound[live].max())


@pytest.mark.parametrize("i", range(7), ids=R.NAMES)
def test_restatement_matches_fp64_within_the_derived_bound(i):
    vert, face, vptr, fptr = one(i)
    for w in WEIGHTINGS:
        n32, zero = R.normals(vert, face, vptr, fptr, w)
        _, _, worst = check_against_fp64(n32, vert, face, vptr, fptr, w, R.NAMES[i])
        assert worst <= 1e-3                                           # no vertex's bound is too wide to mean anything
        assert int(zero[0]) == {0: 6, 1: 5, R.HOLES: 12}.get(i, 0) == vert.shape[0] - np.unique(face).size      # the unreferenced vertices, and only they


def test_closed_torus_has_no_zero_normal_and_agrees_with_every_incident_face():
    """PyG's weighting: every vertex normal has a positive dot product with every incident unit face normal (smallest: 0.029).
    The seed-3 torus has one fold -- the perturbed quad (66, 82, 83, 67) is not convex, so its thin second triangle faces the other
    way -- and under "area" that thin face weighs little at its own corners: one dot product there is negative (-0.12), in fp64 as
    in fp32.  So "area" is held to the fp64 signs, and to being positive everywhere off that face."""
    vert, face, vptr, fptr = one(R.TORUS)
    assert np.array_equal(np.unique(face), np.arange(vert.shape[0]))                       # every vertex is referenced
    unit = R.contributions(vert, face, vptr, fptr, "uniform")
    unit64 = np.repeat(R.contributions(vert, face, vptr, fptr, "uniform", np.float64), 3, axis=0)
    for w in WEIGHTINGS:
        n, zero = R.normals(vert, face, vptr, fptr, w)
        assert int(zero[0]) == 0 and np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() <= 4 * R.U
        dots = (n[face.reshape(-1)] * np.repeat(unit, 3, axis=0)).sum(axis=1)
        print(f"{w}: smallest dot product of a vertex normal with an incident face normal {float(dots.min()):.3f}")
        if w == "uniform":
            assert float(dots.min()) > 0
        else:
            dots64 = (R.expected64(vert, face, vptr, fptr, w)[0][face.reshape(-1)] * unit64).sum(axis=1)
            assert np.array_equal(dots > 0, dots64 > 0)
            fold = np.flatnonzero(dots <= 0) // 3
            assert set(fold.tolist()) == {133} and sorted(face[133].tolist()) == [66, 67, 83]


# ---- the host transform -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(7), ids=R.NAMES)
def test_generate_mesh_normals_matches_fp64_and_leaves_the_mesh_alone(i):
    vert, face, vptr, fptr = one(i)
    for w in WEIGHTINGS:
        pos, fc = torch.from_numpy(vert.copy()), torch.from_numpy(face.T.astype(np.int64).copy())
        d = T.GenerateMeshNormals(weighting=w)(Data(pos=pos, face=fc))
        assert torch.equal(d.pos, torch.from_numpy(vert)) and torch.equal(d.face, torch.from_numpy(face.T.astype(np.int64)))
        assert d.norm.dtype == torch.float32 and tuple(d.norm.shape) == vert.shape
        check_against_fp64(d.norm.numpy(), vert, face, vptr, fptr, w, f"T.GenerateMeshNormals {R.NAMES[i]}")
    assert repr(T.GenerateMeshNormals()) == "GenerateMeshNormals()" and "area" in repr(T.GenerateMeshNormals("area"))
    with pytest.raises(ValueError, match="weighting"):
        T.GenerateMeshNormals("angle")


# ---- host logic of the store ---------------------------------------------------------------------------------------------------------------
def _store(idx=(0, 3, 5), labels=True):
    items = []
    for i in idx:
        vert, face, y = R.meshes()[i]
        items.append(Data(pos=torch.from_numpy(vert), face=torch.from_numpy(face.T.copy()),
                          y=torch.from_numpy(y) if labels else torch.tensor([i])))
    return DeviceMeshDataset.from_dataset(items, "cpu")


def test_vertex_cloud_argument_errors_and_the_paths_without_a_launch():
    st = _store()
    with pytest.raises(ValueError, match="weighting"):
        st.vertex_cloud(weighting="angle")
    with pytest.raises(ValueError, match="weighting"):
        st.vertex_normals(weighting="angle")
    with pytest.raises(ValueError, match="HIP device"):               # no CPU path
        st.vertex_cloud()
    with pytest.raises(ValueError, match="HIP device"):
        st.vertex_normals()
    assert st.vertex_lists is None
    with pytest.raises(ValueError, match="include_labels"):
        _store(labels=False).vertex_cloud(include_normals=False)
    cloud = st.vertex_cloud(include_normals=False)                     # nothing to launch: works on CPU tensors
    assert cloud.pos.data_ptr() == st.vert.data_ptr() and cloud.norm is None and cloud.zero_normals is None
    assert torch.equal(cloud.ptr, st.vptr) and np.array_equal(cloud.sizes, st.n_verts) and len(cloud) == 3
    assert torch.equal(cloud.y_point, st.y_vert) and cloud.y_cloud is None
    by_cloud = _store(labels=False).vertex_cloud(include_normals=False, include_labels=False)
    assert by_cloud.y_point is None and by_cloud.y_cloud.tolist() == [0, 3, 5]
    from deltaconv_amd.geometry import vertex_face_lists, vertex_normals_batch
    with pytest.raises(ValueError, match="HIP device"):
        vertex_face_lists(st.face, st.vptr, st.fptr, st.vert.shape[0])
    with pytest.raises(ValueError, match="HIP device"):
        vertex_normals_batch(st.vert, st.face, st.vptr, st.fptr)
    with pytest.raises(ValueError, match="weighting"):
        vertex_normals_batch(st.vert, st.face, st.vptr, st.fptr, weighting=1)


def test_zero_normals_are_refused_by_name():
    DeviceMeshDataset._refuse_zero_normals(np.zeros(9, dtype=np.int64))
    counts = np.array([0, 12, 0, 1, 3, 5, 7, 9, 0], dtype=np.int64)
    with pytest.raises(ValueError) as e:
        DeviceMeshDataset._refuse_zero_normals(counts)
    msg = str(e.value)
    assert "6 of 9 meshes" in msg and "mesh 1: 12, mesh 3: 1, mesh 4: 3, mesh 5: 5, mesh 6: 7, ..." in msg
    assert "mesh 7" not in msg and "allow_zero_normals=True" in msg


def test_subset_and_a_new_normalised_store_start_without_lists():
    st = _store()
    st.vertex_lists = (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))      # as if built
    sub = st.subset([2, 0])
    assert sub.vertex_lists is None and len(sub) == 2 and st.vertex_lists is not None
    fresh = DeviceMeshDataset(st.vert, st.face, st.vptr, st.fptr, st.n_verts, st.n_faces)
    assert fresh.vertex_lists is None
