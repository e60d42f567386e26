"""The device normalisation of a store on the MI355X (csrc/shape_norm.hip: ``dc_shape_normalize``,
``geometry.normalize_shapes_batch``, ``DeviceMeshDataset.normalize``, ``DeviceDataset.normalize``) against the numpy restatement
of csrc/shape_norm_math.h (tests/shape_norm_restate.py, itself held to a g++ build of that header, to the fp64 formulas and to
the host transforms by tests/test_shape_norm_host.py): rows, ``stats`` and permuted normals bit for bit.  Vertex and face counts
sit around the threads T of the parameter workgroup (``dc_shape_normalize_threads``), on which the order of the fp64 sums
depends.  A NaN (0 * inf in a shape without extent or area) has no agreed sign between the host and the device: it is compared
as a NaN, everything else by its bits."""
import functools

import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from tests import shape_norm_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
MESH_CHAINS = {"scale2": [R.scale(2)], "scale_inf": [R.scale(INF)], "scale_const": [R.scale(2, 1.7)], "area": [R.area()],
               "axes": [R.axes()], "area_axes": [R.area(), R.axes()]}
CLOUD_CHAINS = {"scale2": [R.scale(2)], "scale_inf": [R.scale(INF)], "scale_const": [R.scale(INF, 0.8)], "axes": [R.axes()],
                "scale_axes": [R.scale(2), R.axes()]}
FLAT = 7                                                      # the mesh without area


def threads():
    from deltaconv_amd._lib import lib
    return int(lib.raw("dc_shape_normalize_threads")())


def same(got, want):
    """Equal bits, a NaN matching any NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(R.bits(got)[~nan], R.bits(want)[~nan])


@functools.lru_cache(maxsize=None)
def mesh_items():
    """Nine meshes: vertex counts {3, 4, 5, T-1, T, T+1, 2T+3} with face counts {1, 2, 3, T+1, T, T-1, 2T+3} (rows of a stretched,
    permuted, shifted synthetic mesh under random triangles), a collinear mesh whose faces all have area 0, and a whole
    stretched synthetic mesh of 515 faces."""
    from deltaconv_amd.datasets import Data
    t = threads()
    assert t == R.T
    items = []
    for i, (v, f) in enumerate(((3, 1), (4, 2), (5, 3), (t - 1, t + 1), (t, t), (t + 1, t - 1), (2 * t + 3, 2 * t + 3))):
        pos, _, y = R.test_mesh(2 * max(v, 9), i)
        rng = np.random.default_rng(70 + i)
        face = np.stack([rng.permutation(v)[:3] for _ in range(f)])             # three different corners per face
        items.append(Data(pos=torch.from_numpy(pos[:v].copy()), face=torch.from_numpy(face.T.copy()), y=torch.from_numpy(y[:v].copy())))
    flat = torch.tensor([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=torch.float32)
    items.append(Data(pos=flat, face=torch.tensor([[0, 1, 0], [1, 2, 0], [2, 3, 1]]), y=torch.arange(4)))
    pos, face, y = R.test_mesh(515, 8)
    items.append(Data(pos=torch.from_numpy(pos), face=torch.from_numpy(face.T.copy()), y=torch.from_numpy(y)))
    assert len(items) == 9 and FLAT == 7
    return items


@functools.lru_cache(maxsize=None)
def mesh_store():
    from deltaconv_amd import DeviceMeshDataset
    return DeviceMeshDataset.from_dataset(mesh_items(), DEV)


@functools.lru_cache(maxsize=None)
def cloud_items():
    """Nine clouds of {1, 2, 3, T-1, T, T+1, 2T+3, 64, 65} points with unit normals and per-point labels."""
    from deltaconv_amd.datasets import Data
    t = threads()
    items = []
    for i, n in enumerate((1, 2, 3, t - 1, t, t + 1, 2 * t + 3, 64, 65)):
        pos, _, y = R.test_mesh(2 * max(n, 9), 20 + i)
        nrm = np.random.default_rng(90 + i).standard_normal((n, 3)).astype(np.float32)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        items.append(Data(pos=torch.from_numpy(pos[:n].copy()), norm=torch.from_numpy(nrm), y=torch.from_numpy(y[:n].copy())))
    return items


@functools.lru_cache(maxsize=None)
def cloud_store():
    from deltaconv_amd import DeviceDataset
    return DeviceDataset.from_dataset(cloud_items(), DEV)


@functools.lru_cache(maxsize=None)
def restated_mesh(name):
    """The restated chain of every fixture mesh, computed once per chain and shared -> [(pos, None, stats)]."""
    return [R.normalize(d.pos.numpy(), MESH_CHAINS[name], d.face.t().numpy()) for d in mesh_items()]


@functools.lru_cache(maxsize=None)
def restated_cloud(name):
    return [R.normalize(d.pos.numpy(), CLOUD_CHAINS[name], None, d.norm.numpy()) for d in cloud_items()]


def check(got_pos, got_norm, got_stats, want, offsets, what):
    got_pos, got_stats = got_pos.cpu().numpy(), got_stats.cpu().numpy()
    got_norm = None if got_norm is None else got_norm.cpu().numpy()
    for i, (pos, norm, stats) in enumerate(want):
        rows = slice(int(offsets[i]), int(offsets[i + 1]))
        assert same(got_stats[i], stats), (what, i, got_stats[i], stats)
        assert same(got_pos[rows], pos), (what, i)
        if norm is not None and got_norm is not None:
            assert same(got_norm[rows], norm), (what, i)


@pytest.mark.parametrize("name", MESH_CHAINS)
def test_a_mesh_store_equals_the_restatement_bitwise(name):
    from deltaconv_amd.geometry import normalize_shapes_batch
    st = mesh_store()
    before = st.vert.clone()
    pos, _, stats = normalize_shapes_batch(st.vert, st.vptr, MESH_CHAINS[name], st.face, st.fptr, n_rows=int(st.n_verts.sum()))
    assert tuple(stats.shape) == (9, len(MESH_CHAINS[name]), 8) and torch.equal(st.vert, before)
    check(pos, None, stats, restated_mesh(name), st.vptr.cpu().numpy(), name)
    if "area" in name:
        assert np.isposinf(stats[FLAT, 0, 3].item())


@pytest.mark.parametrize("name", CLOUD_CHAINS)
def test_a_point_store_and_its_normals_equal_the_restatement_bitwise(name):
    from deltaconv_amd.geometry import normalize_shapes_batch
    st = cloud_store()
    norm = st.norm.clone()
    pos, norm_out, stats = normalize_shapes_batch(st.pos, st.ptr, CLOUD_CHAINS[name], norm=norm)      # n_rows read from the device
    assert norm_out is norm
    check(pos, norm, stats, restated_cloud(name), st.ptr.cpu().numpy(), name)
    if "axes" not in name:
        assert torch.equal(norm, st.norm)
    else:
        assert not torch.equal(norm, st.norm)                                 # some cloud's columns did move


def test_the_grouping_into_launches_and_the_position_in_the_store_change_no_bit():
    st = mesh_store()
    chain = [T.NormalizeArea(), T.NormalizeAxes()]
    whole = st.normalize(chain)
    for per in (1, 4):
        other = st.normalize(chain, shapes_per_launch=per)
        assert torch.equal(whole.vert.view(torch.int32), other.vert.view(torch.int32))
        assert torch.equal(whole.norm_stats.view(torch.int32), other.norm_stats.view(torch.int32))
        assert np.array_equal(whole.degenerate, other.degenerate)
    check(whole.vert, None, whole.norm_stats, restated_mesh("area_axes"), st.vptr.cpu().numpy(), "store")
    # the same meshes in another order and another store: a mesh's rows are a function of the mesh alone
    order = [8, 2, 6, 0, 4]
    moved = st.subset(order).normalize(chain)
    check(moved.vert, None, moved.norm_stats, [restated_mesh("area_axes")[i] for i in order], moved.vptr.cpu().numpy(), "moved")
    cl = cloud_store()
    a, b = cl.normalize(T.NormalizeScale()), cl.normalize(T.NormalizeScale(), shapes_per_launch=1)
    assert torch.equal(a.pos.view(torch.int32), b.pos.view(torch.int32)) and torch.equal(a.norm_stats.view(torch.int32), b.norm_stats.view(torch.int32))
    check(a.pos, None, a.norm_stats, restated_cloud("scale2"), cl.ptr.cpu().numpy(), "cloud store")


def test_in_place_equals_out_of_place_and_the_result_shares_the_other_tensors():
    from deltaconv_amd import DeviceDataset, DeviceMeshDataset
    st = mesh_store()
    chain = [T.NormalizeArea(), T.NormalizeAxes()]
    fresh = st.normalize(chain)
    assert fresh is not st and fresh.face is st.face and fresh.vptr is st.vptr and fresh.fptr is st.fptr and fresh.y_vert is st.y_vert
    assert fresh.vert.data_ptr() != st.vert.data_ptr() and torch.equal(st.vert.cpu(), torch.cat([d.pos for d in mesh_items()]))
    own = DeviceMeshDataset.from_dataset(mesh_items(), DEV)
    ptr = own.vert.data_ptr()
    assert own.normalize(chain, out=own) is own and own.vert.data_ptr() == ptr
    assert torch.equal(own.vert.view(torch.int32), fresh.vert.view(torch.int32))
    assert torch.equal(own.norm_stats.view(torch.int32), fresh.norm_stats.view(torch.int32))
    built = DeviceMeshDataset.from_dataset(mesh_items(), DEV, normalize=chain)                # the construction shortcut
    assert torch.equal(built.vert.view(torch.int32), fresh.vert.view(torch.int32)) and built.degenerate.tolist() == fresh.degenerate.tolist()
    # a point store with normals: an axes op permutes a copy of them, or them in place
    cl = cloud_store()
    chain = [T.NormalizeScale(), T.NormalizeAxes()]
    fresh = cl.normalize(chain)
    assert fresh.norm is not cl.norm and fresh.y_point is cl.y_point and fresh.ptr is cl.ptr
    assert cl.normalize(T.NormalizeScale()).norm is cl.norm                               # nothing permuted: shared
    check(fresh.pos, fresh.norm, fresh.norm_stats, restated_cloud("scale_axes"), cl.ptr.cpu().numpy(), "cloud chain")
    own = DeviceDataset.from_dataset(cloud_items(), DEV)
    ptrs = own.pos.data_ptr(), own.norm.data_ptr()
    assert own.normalize(chain, out=own) is own and (own.pos.data_ptr(), own.norm.data_ptr()) == ptrs
    assert torch.equal(own.pos.view(torch.int32), fresh.pos.view(torch.int32)) and torch.equal(own.norm.view(torch.int32), fresh.norm.view(torch.int32))
    built = DeviceDataset.from_dataset(cloud_items(), DEV, normalize=chain, fps=16, fps_seed=1)   # normalised before the FPS
    want = fresh.geodesic_subsample(16, seed=1)
    assert torch.equal(built.pos.view(torch.int32), want.pos.view(torch.int32)) and torch.equal(built.norm.view(torch.int32), want.norm.view(torch.int32))


def test_sampling_the_normalised_store_equals_sampling_the_host_normalised_items():
    from deltaconv_amd import DeviceMeshDataset
    from deltaconv_amd.datasets import Data
    keep = [i for i in range(9) if i != FLAT]                                 # a mesh of NaN rows has no sample to compare
    st = mesh_store().subset(keep)
    got = st.normalize([T.NormalizeArea(), T.NormalizeAxes()]).sample_points(256, include_labels=True, seed=5, round=3)
    items = [Data(pos=torch.from_numpy(restated_mesh("area_axes")[i][0]), face=mesh_items()[i].face, y=mesh_items()[i].y) for i in keep]
    want = DeviceMeshDataset.from_dataset(items, DEV).sample_points(256, include_labels=True, seed=5, round=3)
    assert torch.equal(got.pos.view(torch.int32), want.pos.view(torch.int32)) and torch.equal(got.norm.view(torch.int32), want.norm.view(torch.int32))
    assert torch.equal(got.y_point, want.y_point) and torch.equal(got.total, want.total) and not got.degenerate.any()


def test_degenerate_marks_the_mesh_without_area_only():
    st = mesh_store()
    for chain in (T.NormalizeArea(), [T.NormalizeArea(), T.NormalizeAxes()]):
        res = st.normalize(chain)
        assert res.degenerate.dtype == bool and res.degenerate.tolist() == [i == FLAT for i in range(9)]
        assert res.norm_stats.shape[1] == (2 if isinstance(chain, list) else 1)
    assert not st.normalize(T.NormalizeScale()).degenerate.any()
    # a cloud of one point has no extent: its 2-norm scale is infinite
    assert cloud_store().normalize(T.NormalizeScale()).degenerate.tolist() == [True] + [False] * 8


def test_the_pass_is_capturable_and_replays_to_the_same_bits():
    from deltaconv_amd.geometry import normalize_shapes_batch
    st = mesh_store()
    src, out = st.vert.clone(), torch.zeros_like(st.vert)
    n_rows, chain = int(st.n_verts.sum()), MESH_CHAINS["area_axes"]
    run = lambda: normalize_shapes_batch(src, st.vptr, chain, st.face, st.fptr, out=out, n_rows=n_rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                 # loads the code objects outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, _, stats = run()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check(out, None, stats, restated_mesh("area_axes"), st.vptr.cpu().numpy(), "replay")
    # new contents of the same buffers: the replay normalises them (a shifted, doubled store has the same normal form up to rounding)
    src.copy_(st.vert * 2 + 1)
    graph.replay()
    torch.cuda.synchronize()
    eager = normalize_shapes_batch(src, st.vptr, chain, st.face, st.fptr, n_rows=n_rows)
    assert torch.equal(out.view(torch.int32)[~out.isnan()], eager[0].view(torch.int32)[~eager[0].isnan()])
    assert torch.equal(stats.view(torch.int32), eager[2].view(torch.int32))


def test_random_split_subsets_feed_a_loader_like_the_parent_store():
    from deltaconv_amd import DeviceLoader, random_split
    st = cloud_store().normalize(T.NormalizeScale(norm_ord=float("inf"), scaling_factor=0.8))       # finite rows: torch.equal compares them
    assert not bool(st.pos.isnan().any())
    parts = random_split(st, [7, 2], seed=3)
    want = torch.utils.data.random_split(range(9), [7, 2], generator=torch.Generator().manual_seed(3))
    parent = DeviceLoader(st, 3)
    for part, w in zip(parts, want):
        idx = list(w.indices)
        assert part.sizes.tolist() == st.sizes[idx].tolist()
        batches = list(DeviceLoader(part, 3))
        assert len(batches) == -(-len(idx) // 3)
        for k, got in enumerate(batches):
            ref = parent.assemble(idx[3 * k:3 * k + 3])
            for name in ("pos", "norm", "y", "batch", "ptr"):
                assert torch.equal(getattr(got, name), getattr(ref, name)), (name, k)


def test_argument_errors_raise_with_a_message_and_launch_nothing():
    import ctypes
    from deltaconv_amd._lib import lib
    st = mesh_store()
    out = torch.full_like(st.vert, -5.0)
    stats = torch.full((9, 4, 8), -5.0, device=DEV)
    n_rows = int(st.n_verts.sum())

    def call(codes=(2, 3), params=(0, 0, 0, 0), n_ops=None, B=9, face=st.face, fptr=st.fptr, table=stats, ws=None, ws_bytes=0):
        n_ops = len(codes) if n_ops is None else n_ops
        lib.call("dc_shape_normalize", st.vert, st.vptr, face, fptr, B, n_rows, (ctypes.c_int32 * 8)(*codes),
                 (ctypes.c_float * 16)(*params), n_ops, out, None, table, ws, ws_bytes)

    for kw, msg in ((dict(codes=(2, 9)), "unknown code 9"), (dict(codes=(0,)), "unknown code 0"), (dict(n_ops=0), "n_ops = 0"),
                    (dict(codes=(3,) * 5, params=(0,) * 10), "n_ops = 5"), (dict(B=65536), "65535"),
                    (dict(face=None), "area op"), (dict(fptr=None), "area op"),
                    (dict(codes=(1,), params=(1.0, float("nan"))), "norm_ord = 1"), (dict(codes=(1,), params=(-INF, 1.0)), "norm_ord"),
                    (dict(table=None), "workspace"), (dict(table=None, ws=stats, ws_bytes=9 * 2 * 32 - 1), "workspace")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and bool((stats == -5).all())
    call(B=0)
    torch.cuda.synchronize()
    assert bool((out == -5).all()) and bool((stats == -5).all())
    # without stats the table lives in the workspace: the same rows
    ws = torch.empty(9 * 2 * 8, device=DEV)
    call(table=None, ws=ws, ws_bytes=9 * 2 * 32)
    check(out, None, ws.view(9, 2, 8), restated_mesh("area_axes"), st.vptr.cpu().numpy(), "workspace")
