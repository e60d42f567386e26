"""The device geodesic farthest-point sampler for clouds above the LDS kernel's cap on the MI355X (csrc/fps.hip:
``fps_sample_global_kernel`` behind ``dc_geodesic_fps_large``; ``geometry.geodesic_fps_batch(large=True)``;
``DeviceDataset.geodesic_subsample(large="device")``).

Two yardsticks.  Where the LDS kernel takes the cloud too (n <= 16 384) both kernels read the same graph and run the same
arithmetic, so the picks are EQUAL: no tolerance, no excused round.  Above the cap the acceptance rule of tests/test_gpu_fps.py
holds (``replay(...) == 0``); the fixtures were checked on the CPU with the host library's picks: no excused round, smallest
relative gap 1.2e-4."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests.test_fps_host import doubled_cloud, shell, two_clusters
from tests.test_gpu_fps import knn_graph_f64, replay

pytestmark = pytest.mark.gpu
DEV = "cuda"


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def large_entry(clouds, m, starts, dtype=torch.float32):
    """``dc_geodesic_fps_large`` itself, one launch pair over `clouds` whatever their sizes -> int64 [B, m] on the host."""
    from deltaconv_amd.geometry.fps import _fps_device
    pos = torch.from_numpy(np.concatenate(clouds)).to(dtype).to(DEV)
    out = _fps_device(pos, offsets([len(c) for c in clouds]), m, np.asarray(starts, dtype=np.int32), large=True)
    assert out.dtype == torch.int32 and out.shape == (len(clouds), m) and out.is_cuda
    return out.cpu().numpy().astype(np.int64)


def batch(clouds, m, starts, dtype=torch.float32, **kw):
    from deltaconv_amd.geometry import geodesic_fps_batch
    pos = torch.from_numpy(np.concatenate(clouds)).to(dtype).to(DEV)
    out = geodesic_fps_batch(pos, torch.from_numpy(offsets([len(c) for c in clouds])), m, start=starts, **kw)
    assert out.dtype == torch.int64 and out.shape == (len(clouds), m) and out.is_cuda
    return out.cpu().numpy()


# ---- 1. the same bits as the LDS kernel ---------------------------------------------------------------------------------------
SMALL = [(1, 0), (7, 6), (33, 32), (64, 63), (65, 64), (200, 5), (1000, 999), (2500, 1234)]    # (n, start): word edges start at the last bit


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_same_picks_as_the_lds_kernel(dt):
    dtype = torch.float32 if dt == "f32" else torch.float64
    rng = np.random.default_rng(31)
    clouds = [rng.random((n, 3)).astype(np.float32) for n, _ in SMALL]
    starts = [s for _, s in SMALL]
    want = batch(clouds, 40, starts, dtype)
    for i, c in enumerate(clouds):                       # alone: the LDS of the launch is sized by this cloud
        got = large_entry([c], 40, [starts[i]], dtype)[0]
        assert np.array_equal(got, want[i]), (len(c), np.flatnonzero(got != want[i])[:5])
    assert np.array_equal(large_entry(clouds, 40, starts, dtype), want)      # and ragged in one launch


@pytest.mark.parametrize("make,m", [(two_clusters, 30), (doubled_cloud, 130)])
def test_same_picks_on_disconnected_and_duplicated_clouds(make, m):
    pos = make()
    want = batch([pos], m, [2])[0]
    assert np.array_equal(large_entry([pos], m, [2])[0], want)
    if make is two_clusters:
        side = pos[want, 0] > 50
        assert side.any() and not side.all()             # the +inf round crossed over


# ---- 2. above the cap: the acceptance rule -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(kind, n, m, seed):
    """-> (pos float32 [n,3], its fp64 graph, the start: the first pick of the host library for this seed)."""
    from deltaconv_amd.geometry import geodesic_fps
    pos = (np.random.default_rng(seed).random((n, 3)) if kind == "random" else shell(n, seed)).astype(np.float32)
    return pos, knn_graph_f64(pos), int(np.atleast_1d(geodesic_fps(pos, m, seed=seed))[0])


FIXTURES = [("random", 16385, 8, 6), ("random", 16390, 8, 6), ("random", 20000, 16, 7), ("shell", 20000, 16, 3), ("shell", 17000, 24, 4)]


@pytest.mark.parametrize("kind,n,m,seed", FIXTURES)
def test_picks_above_the_cap_replay_as_farthest_points(kind, n, m, seed):
    pos, graph, start = fixture(kind, n, m, seed)
    got = batch([pos], m, [start], large=True)[0]
    assert got[0] == start
    assert replay(graph, got) == 0                       # no round of these fixtures is close enough to be excused


# ---- 3. one ragged launch over both size classes -------------------------------------------------------------------------------
def test_ragged_launch_over_both_size_classes():
    m = 8
    rng = np.random.default_rng(41)
    big_a, big_b = fixture("random", 16390, 8, 6), fixture("shell", 17000, 24, 4)     # their first 8 picks: a prefix of the fixture's
    clouds = [rng.random((50, 3)).astype(np.float32), big_a[0], rng.random((1, 3)).astype(np.float32),
              rng.random((300, 3)).astype(np.float32), big_b[0]]
    assert [len(c) for c in clouds] == [50, 16390, 1, 300, 17000]
    starts = [7, big_a[2], 0, 299, big_b[2]]
    got = batch(clouds, m, starts, large=True)
    assert got[:, 0].tolist() == starts                                               # rows in input order
    small = [0, 2, 3]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(got[small], batch([clouds[i] for i in small], m, [starts[i] for i in small]))
    assert replay(big_a[1], got[1]) == 0 and replay(big_b[1], got[4]) == 0
    assert np.array_equal(batch(clouds, m, starts, large=True), got)                  # the same bits again
    for i in (1, 4):
        assert np.array_equal(batch([clouds[i]], m, [starts[i]], large=True)[0], got[i])


# ---- 4. the store ---------------------------------------------------------------------------------------------------------------
def test_store_samples_every_cloud_on_the_device():
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry import geodesic_fps_batch
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS, fps_starts
    from deltaconv_amd.loader import DeviceDataset
    g = torch.Generator().manual_seed(8)
    sizes, m = [50, FPS_MAX_POINTS + 6, 80], 8
    items = [Data(pos=torch.rand(n, 3, generator=g), norm=torch.rand(n, 3, generator=g), y=torch.randint(0, 9, (n,), generator=g))
             for n in sizes]
    store = DeviceDataset.from_dataset(items, DEV)
    sub = store.geodesic_subsample(m, seed=2, large="device")
    ids = geodesic_fps_batch(store.pos, store.ptr, m, start=fps_starts(sizes, 2), large=True)
    assert ids[:, 0].tolist() == fps_starts(sizes, 2).tolist()
    rows = (ids + store.ptr[:-1, None]).reshape(-1)
    for name in ("pos", "norm", "y_point"):
        assert torch.equal(getattr(sub, name), getattr(store, name)[rows]), name
    assert np.array_equal(sub.sizes, [m] * 3) and sub.ptr.tolist() == [0, m, 2 * m, 3 * m]
    split = store.geodesic_subsample(m, seed=2, large="device", clouds_per_launch=1)
    via = DeviceDataset.from_dataset(items, DEV, fps=m, fps_seed=2, fps_large="device")
    for other in (split, via):
        assert torch.equal(other.pos, sub.pos) and torch.equal(other.norm, sub.norm) and torch.equal(other.y_point, sub.y_point)
    # an explicit start reaches the big cloud (the host path refuses it)
    first = store.geodesic_subsample(m, start=[3, 12345, 9], large="device")
    want = geodesic_fps_batch(store.pos, store.ptr, m, start=[3, 12345, 9], large=True)
    assert torch.equal(first.pos, store.pos[(want + store.ptr[:-1, None]).reshape(-1)])
    assert torch.equal(first.pos[m], store.pos[50 + 12345])
    with pytest.raises(ValueError, match="start"):
        store.geodesic_subsample(m, start=[3, 12345, 9])


def test_vertex_clouds_of_a_mesh_store_with_a_large_mesh():
    from deltaconv_amd.data import synthetic_mesh
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry import geodesic_fps_batch
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS, fps_starts
    from deltaconv_amd.meshes import DeviceMeshDataset
    items = []
    for i, faces in enumerate((400, 33800, 1200)):       # 33 800 faces: a 130 x 130 grid torus of 16 900 vertices
        pos, face, y = synthetic_mesh(faces, 50 + i, labels=True)
        items.append(Data(pos=pos, face=face, y=y))
    cloud = DeviceMeshDataset.from_dataset(items, DEV).vertex_cloud()
    assert cloud.sizes.max() > FPS_MAX_POINTS and cloud.sizes.min() <= FPS_MAX_POINTS
    sub = cloud.geodesic_subsample(64, seed=1, large="device")
    ids = geodesic_fps_batch(cloud.pos, cloud.ptr, 64, start=fps_starts(cloud.sizes, 1), large=True)
    rows = (ids + cloud.ptr[:-1, None]).reshape(-1)
    assert sub.pos.shape == (3 * 64, 3) and np.array_equal(sub.sizes, [64] * 3)
    for name in ("pos", "norm", "y_point"):
        assert torch.equal(getattr(sub, name), getattr(cloud, name)[rows]), name
    for row in ids.cpu().numpy():                        # farthest points of a connected surface: no vertex is taken twice
        assert len(set(row.tolist())) == 64


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from deltaconv_amd.geometry import geodesic_fps_batch
    pos = torch.zeros(262145, 3, device=DEV)
    with pytest.raises(ValueError, match="262144"):
        geodesic_fps_batch(pos, torch.tensor([0, 262145]), 4, large=True)
    with pytest.raises(ValueError, match="at most 16384 per cloud"):
        geodesic_fps_batch(pos[:16385], torch.tensor([0, 16385]), 4)
    with pytest.raises(ValueError, match="empty"):
        geodesic_fps_batch(pos[:10], torch.tensor([0, 10, 10]), 4, large=True)
    with pytest.raises(ValueError, match="start"):
        geodesic_fps_batch(pos[:20000], torch.tensor([0, 20000]), 4, start=[20000], large=True)
