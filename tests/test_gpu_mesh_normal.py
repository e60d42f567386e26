"""The per-vertex normals of a mesh store on the MI355X (csrc/mesh_normal.hip: ``dc_mesh_vertex_faces``, ``dc_mesh_vertex_normals``;
``geometry.vertex_face_lists``, ``geometry.vertex_normals_batch``; ``DeviceMeshDataset.vertex_normals`` / ``vertex_cloud``) against
the numpy restatement of csrc/mesh_normal_math.h (tests/mesh_normal_restate.py, itself held to a g++ build of that header and to
the fp64 formula by tests/test_mesh_normal_host.py): lists, normals and zero counts bit for bit, for both weightings; the same bits
whatever the grouping and the place of a mesh in the store; and the vertex cloud through the stages that follow it."""
import functools

import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from tests import mesh_normal_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHTINGS = ("uniform", "area")


def _items(ms):
    from deltaconv_amd.datasets import Data
    return [Data(pos=torch.from_numpy(v), face=torch.from_numpy(f.T.copy()), y=torch.from_numpy(y)) for v, f, y in ms]


@functools.lru_cache(maxsize=None)
def store():
    """The seven meshes of the host tests in one store."""
    from deltaconv_amd import DeviceMeshDataset
    return DeviceMeshDataset.from_dataset(_items(R.meshes()), DEV)


@functools.lru_cache(maxsize=None)
def restated(weighting):
    """(normals, zero counts) of the whole store, computed once per weighting and shared."""
    return R.normals(*R.store_arrays(R.meshes()), weighting)


@functools.lru_cache(maxsize=None)
def tori():
    """Three closed tori of 512 faces (seeds 1 .. 3), their vertex cloud normalised and cut to 64 geodesic-farthest vertices."""
    from deltaconv_amd import DeviceMeshDataset
    meshes = DeviceMeshDataset.from_dataset(_items([R.torus(s) for s in (1, 2, 3)]), DEV)
    sub = meshes.vertex_cloud().normalize(T.NormalizeScale()).geodesic_subsample(64, seed=1)
    return meshes, sub


def test_lists_normals_and_zero_counts_equal_the_restatement_bitwise():
    from deltaconv_amd.geometry import vertex_face_lists, vertex_normals_batch
    st = store()
    vert, face, vptr, fptr = R.store_arrays(R.meshes())
    assert np.array_equal(st.face.cpu().numpy(), face) and np.array_equal(st.vptr.cpu().numpy(), vptr)
    vf_ptr, vf_edge = vertex_face_lists(st.face, st.vptr, st.fptr, st.vert.shape[0])
    want_ptr, want_edge = R.lists(face, vptr, fptr, vert.shape[0])
    assert vf_ptr.dtype == vf_edge.dtype == torch.int64 and tuple(vf_edge.shape) == (3 * face.shape[0],)
    assert np.array_equal(vf_ptr.cpu().numpy(), want_ptr) and np.array_equal(vf_edge.cpu().numpy(), want_edge)
    for w in WEIGHTINGS:
        zero = torch.full((len(st),), -7, dtype=torch.int32, device=DEV)
        out = torch.full_like(st.vert, float("nan"))
        got = vertex_normals_batch(st.vert, st.face, st.vptr, st.fptr, (vf_ptr, vf_edge), w, out=out, zero_count=zero)
        want, want_zero = restated(w)
        assert got is out and np.array_equal(R.bits(got.cpu().numpy()), R.bits(want)), w
        assert np.array_equal(zero.cpu().numpy(), want_zero) and want_zero.tolist() == [6, 5, 0, 12, 0, 0, 0]
        # the lists are built where none are given; the store builds them once and keeps them
        assert np.array_equal(R.bits(vertex_normals_batch(st.vert, st.face, st.vptr, st.fptr, weighting=w).cpu().numpy()), R.bits(want))
        assert np.array_equal(R.bits(st.vertex_normals(w).cpu().numpy()), R.bits(want))
    assert torch.equal(st.vertex_lists[0], vf_ptr) and torch.equal(st.vertex_lists[1], vf_edge)
    kept = st.vertex_lists
    st.vertex_normals()
    assert st.vertex_lists is kept


def test_a_slice_of_the_offsets_writes_only_its_meshes():
    from deltaconv_amd.geometry import vertex_normals_batch
    st = store()
    vptr = st.vptr.cpu().numpy()
    out = torch.full_like(st.vert, 5.0)
    zero = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    vertex_normals_batch(st.vert, st.face, st.vptr[2:6], st.fptr[2:6], out=out, zero_count=zero)
    got, (want, want_zero) = out.cpu().numpy(), restated("uniform")
    lo, hi = int(vptr[2]), int(vptr[5])
    assert np.array_equal(R.bits(got[lo:hi]), R.bits(want[lo:hi])) and (got[:lo] == 5).all() and (got[hi:] == 5).all()
    assert np.array_equal(zero.cpu().numpy(), want_zero[2:5])


@pytest.mark.parametrize("w", WEIGHTINGS)
def test_the_bits_do_not_depend_on_grouping_placement_or_the_run(w):
    st = store()
    vptr = st.vptr.cpu().numpy()
    whole = st.vertex_normals(w).cpu().numpy()
    assert np.array_equal(R.bits(st.vertex_normals(w).cpu().numpy()), R.bits(whole))                # a second run
    for i in range(len(st)):                                                                       # every mesh as a store of its own
        alone = st.subset([i])
        assert alone.vertex_lists is None
        assert np.array_equal(R.bits(alone.vertex_normals(w).cpu().numpy()), R.bits(whole[vptr[i]:vptr[i + 1]])), R.NAMES[i]
    order = list(range(len(st)))[::-1]
    rev = st.subset(order)
    got, rptr = rev.vertex_normals(w).cpu().numpy(), rev.vptr.cpu().numpy()
    for k, i in enumerate(order):
        assert np.array_equal(R.bits(got[rptr[k]:rptr[k + 1]]), R.bits(whole[vptr[i]:vptr[i + 1]])), R.NAMES[i]


def test_vertex_cloud_is_the_store_seen_as_clouds():
    st = store()
    pair = st.subset([R.TORUS, 4])                                     # the closed torus and F = 2051
    cloud = pair.vertex_cloud()
    assert cloud.pos.data_ptr() == pair.vert.data_ptr() and cloud.pos.shape == pair.vert.shape
    assert torch.equal(cloud.ptr, pair.vptr) and np.array_equal(cloud.sizes, pair.n_verts) and len(cloud) == 2
    assert torch.equal(cloud.y_point, pair.y_vert) and cloud.y_cloud is None and cloud.zero_normals.tolist() == [0, 0]
    vptr, want = st.vptr.cpu().numpy(), restated("uniform")[0]
    rows = np.concatenate([np.arange(vptr[i], vptr[i + 1]) for i in (R.TORUS, 4)])
    assert np.array_equal(R.bits(cloud.norm.cpu().numpy()), R.bits(want[rows]))
    area = pair.vertex_cloud(weighting="area", include_labels=False)
    assert area.y_point is None and np.array_equal(R.bits(area.norm.cpu().numpy()), R.bits(restated("area")[0][rows]))
    # unreferenced vertices: refused by name unless allowed
    holes = st.subset([R.TORUS, R.HOLES])
    with pytest.raises(ValueError, match=r"1 of 2 meshes.*mesh 1: 12.*allow_zero_normals=True"):
        holes.vertex_cloud()
    kept = holes.vertex_cloud(allow_zero_normals=True)
    assert kept.zero_normals.tolist() == [0, 12] and int((~kept.norm.any(dim=1)).sum()) == 12
    # a normalisation that makes a new store starts without lists, one in place keeps them
    assert holes.vertex_lists is not None and holes.normalize(T.NormalizeScale()).vertex_lists is None
    lists = holes.vertex_lists
    assert holes.normalize(T.NormalizeScale(), out=holes).vertex_lists is lists


def test_the_vertex_cloud_runs_through_normalisation_sampling_loader_and_model():
    import deltaconv_amd as dc
    meshes, sub = tori()
    assert len(sub) == 3 and sub.sizes.tolist() == [64, 64, 64] and tuple(sub.norm.shape) == (192, 3) and tuple(sub.y_point.shape) == (192,)
    batch = next(iter(dc.DeviceLoader(sub, 3)))
    assert tuple(batch.pos.shape) == (192, 3) and batch.num_graphs == 3
    length = np.linalg.norm(batch.norm.cpu().numpy().astype(np.float64), axis=1)
    assert np.abs(length - 1).max() <= 4 * R.U, np.abs(length - 1).max()
    torch.manual_seed(2)
    model = dc.models.DeltaNetSegmentation(in_channels=3, num_classes=8, conv_channels=[16, 32], mlp_depth=1, embedding_size=64,
                                           num_neighbors=8).to(DEV).eval()
    with torch.no_grad():
        logits = model(batch)
    assert tuple(logits.shape) == (192, 8) and bool(torch.isfinite(logits).all())


def test_a_vertex_sampled_store_and_its_mesh_line_up_in_the_propagator():
    from deltaconv_amd import Propagator
    meshes, sub = tori()
    rows = int(meshes.vert.shape[0])
    x = torch.randn(192, 5, generator=torch.Generator().manual_seed(4)).to(DEV)
    up = Propagator(sub, meshes, k=3).apply(x)
    assert tuple(up.shape) == (rows, 5) and bool(torch.isfinite(up).all())
    # in the coordinates the samples were taken in, every sampled vertex finds itself: k = 1 hands it its own row back
    same = meshes.normalize(T.NormalizeScale())
    back = Propagator(sub, same, k=1).apply(sub.pos)
    hit = (back == same.vert).all(dim=1).cpu().numpy()
    vptr = same.vptr.cpu().numpy()
    assert [int(hit[vptr[i]:vptr[i + 1]].sum()) for i in range(3)] == [64, 64, 64]
    assert torch.equal(Propagator(sub, same, k=1).labels(sub.y_point)[torch.from_numpy(hit).to(DEV)],
                       same.y_vert[torch.from_numpy(hit).to(DEV)])


def test_argument_errors_return_dc_err_arg_without_a_launch():
    from deltaconv_amd._lib import lib
    faces, normals = lib.raw("dc_mesh_vertex_faces"), lib.raw("dc_mesh_vertex_normals")
    st = store()
    p = lambda t: t.data_ptr()
    nv, nf = int(st.vert.shape[0]), int(st.face.shape[0])
    assert faces(None, None, None, 1, 8, 8, None, None, None, 0, None) == -1 and "null" in lib.last_error()
    assert faces(p(st.face), p(st.vptr), p(st.fptr), -1, nv, nf, None, None, None, 0, None) == -1 and "B = -1" in lib.last_error()
    vf_ptr = torch.empty(nv + 1, dtype=torch.int64, device=DEV)
    vf_edge = torch.empty(3 * nf, dtype=torch.int64, device=DEV)
    assert faces(p(st.face), p(st.vptr), p(st.fptr), len(st), nv, nf, p(vf_ptr), p(vf_edge), None, 0, None) == -1
    assert "workspace" in lib.last_error()
    assert faces(p(st.face), p(st.vptr), p(st.fptr), len(st), -1, nf, p(vf_ptr), p(vf_edge), None, 0, None) == -1
    assert lib.raw("dc_mesh_vertex_faces_workspace_bytes")(-1, 5) == 0
    assert lib.raw("dc_mesh_vertex_faces_workspace_bytes")(2048, 10) == 8 * (2048 + 2 + 30)
    assert normals(None, None, None, None, 1, 8, 8, None, None, 0, None, None, None) == -1 and "null" in lib.last_error()
    assert normals(None, None, None, None, -1, 8, 8, None, None, 0, None, None, None) == -1 and "B = -1" in lib.last_error()
    out = torch.empty_like(st.vert)
    lists = st.vertex_lists or (vf_ptr, vf_edge)
    assert normals(p(st.vert), p(st.face), p(st.vptr), p(st.fptr), len(st), nv, nf, p(lists[0]), p(lists[1]), 2, p(out), None,
                   None) == -1 and "weighting" in lib.last_error()
