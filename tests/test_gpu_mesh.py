"""The device surface sampler on the MI355X (csrc/mesh.hip: ``dc_mesh_sample``, ``geometry.sample_points_batch``,
``DeviceMeshDataset.sample_points``) against the numpy restatement of csrc/mesh_math.h (tests/mesh_restate.py, itself held
to a g++ build of that header and to ``T.SamplePoints`` by tests/test_mesh_host.py): the cdf and every sample bit for bit.
Face counts sit around the cdf kernel's scan iteration T (``dc_mesh_scan_faces``); sample counts around the 256 samples of
a sampling workgroup."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NUMS = (1, 255, 256, 257, 1000)
SEED, ROUND, FIRST = 7, 2 ** 32 + 3, 1000


def scan_faces():
    from deltaconv_amd._lib import lib
    return int(lib.raw("dc_mesh_scan_faces")())


def make_mesh(f, seed):
    """A mesh of exactly f faces with per-vertex labels; from 63 faces on, three of them have zero area and one is 2^-40 of
    the largest (f = 2: one live face and a zero-area one)."""
    from deltaconv_amd.data import synthetic_mesh
    from deltaconv_amd.datasets import Data
    if f >= 63:
        pos, face, y = synthetic_mesh(f - 4, seed, zero_area=3, shrink=(5, 0.1), labels=True)
        pos, face = R.with_tiny_face(pos, face)
        y = torch.cat([y, torch.tensor([1, 2, 3])])
    elif f == 2:
        pos, face, y = synthetic_mesh(1, seed, zero_area=1, labels=True)
    else:
        pos, face, y = synthetic_mesh(f, seed, labels=True)
    assert face.shape[1] == f
    return Data(pos=pos, face=face, y=y)


@functools.lru_cache(maxsize=None)
def fixture_store():
    """-> (items, DeviceMeshDataset) of the face counts {1, 2, 63, 64, 65, T-1, T, T+1, 2T+3}."""
    from deltaconv_amd import DeviceMeshDataset
    t = scan_faces()
    items = [make_mesh(f, 10 + i) for i, f in enumerate((1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 3))]
    return items, DeviceMeshDataset.from_dataset(items, DEV)


@functools.lru_cache(maxsize=None)
def restated(i, num):
    """The restated sample of fixture mesh i, computed once per (mesh, num) and shared."""
    d = fixture_store()[0][i]
    return R.sample(d.pos.numpy(), d.face.t().numpy(), num, SEED, ROUND, FIRST + i, d.y.numpy())


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def test_cdf_and_total_equal_the_restatement_exactly():
    from deltaconv_amd.geometry import sample_points_batch
    items, st = fixture_store()
    assert scan_faces() >= 64 and list(st.n_faces) == [d.face.shape[1] for d in items]
    *_, total, cdf = sample_points_batch(st.vert, st.face, st.vptr, st.fptr, 1, return_cdf=True, n_faces=int(st.n_faces.sum()))
    cdf, total = cdf.cpu().numpy().view(np.uint64), total.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(st.n_faces)])
    for i, d in enumerate(items):
        w, want = R.cdf_of(d.pos.numpy(), d.face.t().numpy())
        got = cdf[off[i]:off[i + 1]]
        assert np.array_equal(got, want), (i, d.face.shape[1], int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max()))
        assert int(total[i]) == int(want[-1]) > 0
        if d.face.shape[1] >= 63:
            assert (w[-4:] == 0).all() and (got[-4:] == got[-5]).all()           # the zero-area faces and the 2^-40 face


@pytest.mark.parametrize("num", NUMS)
def test_samples_equal_the_restatement_bitwise(num):
    from deltaconv_amd.geometry import sample_points_batch
    items, st = fixture_store()
    pos, norm, y, fid, total = sample_points_batch(st.vert, st.face, st.vptr, st.fptr, num, first_mesh_index=FIRST, seed=SEED,
                                                   round=ROUND, y_vert=st.y_vert, labels=True, face_ids=True,
                                                   n_faces=int(st.n_faces.sum()))
    pos, norm, y, fid = bits(pos), bits(norm), y.cpu().numpy(), fid.cpu().numpy()
    for i in range(len(items)):
        want, rows = restated(i, num), slice(i * num, (i + 1) * num)
        assert np.array_equal(fid[rows], want["face_id"]), (i, num)
        assert np.array_equal(pos[rows], want["pos"].view(np.uint32)), (i, num)
        assert np.array_equal(norm[rows], want["norm"].view(np.uint32)), (i, num)
        assert np.array_equal(y[rows], want["y"]), (i, num)
        assert (want["w"][fid[rows]] > 0).all()


def ragged_items():
    from deltaconv_amd.datasets import Data
    t = scan_faces()
    items = [make_mesh(f, 40 + i) for i, f in enumerate((1, 37, 300, t + 5, 64))]
    flat = torch.tensor([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=torch.float32)       # collinear: every face degenerate
    items.insert(2, Data(pos=flat, face=torch.tensor([[0, 1, 0], [1, 2, 0], [2, 3, 1]]), y=torch.arange(4)))
    return items


def test_one_call_over_ragged_meshes_equals_the_single_mesh_calls():
    from deltaconv_amd import DeviceMeshDataset
    from deltaconv_amd.geometry import sample_points_batch
    items = ragged_items()
    st = DeviceMeshDataset.from_dataset(items, DEV)
    kw = dict(seed=3, round=1, y_vert=st.y_vert, labels=True, face_ids=True)
    whole = sample_points_batch(st.vert, st.face, st.vptr, st.fptr, 300, first_mesh_index=5, **kw)
    for i in range(len(items)):
        one = sample_points_batch(st.vert, st.face, st.vptr[i:i + 2], st.fptr[i:i + 2], 300, first_mesh_index=5 + i, **kw)
        for a, b in zip(whole[:4], one[:4]):
            assert torch.equal(a[i * 300:(i + 1) * 300], b), i
        assert torch.equal(whole[4][i:i + 1], one[4])
    assert whole[4].cpu().tolist()[2] == 0 and (whole[4].cpu() > 0).sum() == 5
    # the all-degenerate mesh: uniform by index, the restated picks, zero normals
    want = R.sample(items[2].pos.numpy(), items[2].face.t().numpy(), 300, 3, 1, 7, items[2].y.numpy())
    assert np.array_equal(whole[3][600:900].cpu().numpy(), want["face_id"]) and not whole[1][600:900].any()
    assert np.array_equal(bits(whole[0][600:900]), want["pos"].view(np.uint32)) and set(want["face_id"]) == {0, 1, 2}


def test_store_sampling_is_independent_of_the_launch_grouping_and_repeatable():
    from deltaconv_amd import DeviceMeshDataset
    st = DeviceMeshDataset.from_dataset(ragged_items(), DEV)
    a = st.sample_points(200, include_labels=True, seed=2, round=4)
    b = st.sample_points(200, include_labels=True, seed=2, round=4, meshes_per_launch=1)
    c = st.sample_points(200, include_labels=True, seed=2, round=4, meshes_per_launch=4)
    again = st.sample_points(200, include_labels=True, seed=2, round=4)
    for other in (b, c, again):
        assert torch.equal(a.pos, other.pos) and torch.equal(a.norm, other.norm) and torch.equal(a.y_point, other.y_point)
        assert torch.equal(a.total, other.total) and np.array_equal(a.degenerate, other.degenerate)
    assert a.degenerate.tolist() == [False, False, True, False, False, False] and st.degenerate is again.degenerate
    fresh = st.sample_points(200, include_labels=True, seed=2, round=5)
    assert float((fresh.pos == a.pos).all(dim=1).float().mean()) < 0.02 and torch.equal(fresh.total, a.total)
    assert not torch.equal(st.sample_points(200, seed=3, round=4).pos, a.pos)


def test_sample_points_builds_a_device_dataset_and_chains_with_fps():
    from deltaconv_amd import DeviceDataset, DeviceMeshDataset
    from deltaconv_amd.geometry import geodesic_fps_batch, sample_points_batch
    items = [make_mesh(f, 60 + i) for i, f in enumerate((200, 64, 500))]
    st = DeviceMeshDataset.from_dataset(items, DEV)
    store = st.sample_points(256, include_labels=True, seed=1)
    assert isinstance(store, DeviceDataset) and len(store) == 3 and store.sizes.tolist() == [256] * 3
    assert store.ptr.tolist() == [0, 256, 512, 768] and store.x is None and store.y_cloud is None and store.category is None
    pos, norm, y, _, total = sample_points_batch(st.vert, st.face, st.vptr, st.fptr, 256, seed=1, y_vert=st.y_vert, labels=True)
    assert torch.equal(store.pos, pos) and torch.equal(store.norm, norm) and torch.equal(store.y_point, y)
    assert torch.equal(store.total, total) and not store.degenerate.any()
    assert float((store.norm.norm(dim=1) - 1).abs().max()) < 1e-5
    # chained with the device FPS = the two steps by hand
    sub = store.geodesic_subsample(32, seed=1)
    ids = geodesic_fps_batch(pos, store.ptr, 32, seed=1)
    rows = (ids + store.ptr[:-1, None]).reshape(-1)
    assert torch.equal(sub.pos, pos[rows]) and torch.equal(sub.norm, norm[rows]) and torch.equal(sub.y_point, y[rows])
    assert sub.sizes.tolist() == [32] * 3
    # flags off; per-cloud labels and category pass through
    for d, c in zip(items, (3, 1, 2)):
        d.y, d.category = torch.tensor([c]), torch.eye(4)[c]
    st2 = DeviceMeshDataset.from_dataset(items, DEV)
    plain = st2.sample_points(256, include_normals=False, seed=1)
    assert plain.norm is None and plain.y_point is None and torch.equal(plain.pos, pos)
    assert plain.y_cloud.tolist() == [3, 1, 2] and torch.equal(plain.category.cpu(), torch.eye(4)[[3, 1, 2]])
    with pytest.raises(ValueError, match="include_labels"):
        st2.sample_points(16, include_labels=True)


def test_argument_errors_raise_with_a_message_and_launch_nothing():
    from deltaconv_amd._lib import lib
    _, st = fixture_store()
    b, num = len(st), 4
    pos = torch.full((b * num, 3), -5.0, device=DEV)
    total = torch.full((b,), -5, dtype=torch.int64, device=DEV)
    need = int(lib.raw("dc_mesh_sample_workspace_bytes")(int(st.n_faces.sum())))
    assert need == 8 * int(st.n_faces.sum()) and int(lib.raw("dc_mesh_sample_workspace_bytes")(0)) == 0
    ws = torch.full((need // 8,), -5, dtype=torch.int64, device=DEV)
    y = torch.empty(b * num, dtype=torch.int64, device=DEV)

    def call(B=b, n=num, seed=0, rnd=0, first=0, y_vert=None, y_out=None, ws_bytes=need):
        lib.call("dc_mesh_sample", st.vert, st.face, st.vptr, st.fptr, B, first, n, seed, rnd, y_vert, pos, None, y_out, None, total,
                 ws, ws_bytes)

    for kw, msg in ((dict(n=0), "num = 0"), (dict(B=65536), "65535"), (dict(seed=2 ** 32), "seed"), (dict(seed=-1), "seed"),
                    (dict(rnd=-1), "round"), (dict(first=2 ** 32), "dataset indices"), (dict(y_out=y), "y_vert"),
                    (dict(ws_bytes=8 * b - 1), "workspace")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((pos == -5).all()) and bool((total == -5).all()) and bool((ws == -5).all())
    call(B=0)
    torch.cuda.synchronize()
    assert bool((pos == -5).all())
    # a workspace that passes the host's check (8 bytes per mesh) but cannot hold every cdf: the kernels skip what does not fit
    cap = int(st.n_faces[:5].sum())
    call(ws_bytes=8 * cap)
    torch.cuda.synchronize()
    assert (total[:5] > 0).all() and (total[5:] == -1).all() and bool((ws[cap:] == -5).all())
    assert not pos[5 * num:].any() and bool((pos[:5 * num] != -5).all())
    call()
    assert bool((total > 0).all())
