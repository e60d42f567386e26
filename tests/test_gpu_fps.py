"""The device geodesic farthest-point sampler on the MI355X (csrc/fps.hip: ``dc_geodesic_fps_batch``,
``geometry.geodesic_fps_batch``, ``DeviceDataset.geodesic_subsample``).

Acceptance rule, implemented once (``replay``): the k = 10 graph is rebuilt in numpy fp64 with the sampler's own expression and
tie rule, then heap Dijkstra is replayed ALONG THE DEVICE'S OWN PICKS.  In every round the pick must reach the maximum of the
replayed distance vector (relative 1e-12), and it must be the FIRST arg-max wherever the maximum is +inf or 0, or is separated
from the second-largest value by a relative gap above 1e-9 (or by none at all: an exact tie).  Only rounds with a finite, non-zero
gap <= 1e-9 are not held to the exact index -- the one thing a device fp64 ``sqrt`` that is not correctly rounded could move --
and the fixtures have none (smallest gaps 4.7e-5 .. 1.4e-3 on the CPU): the tests assert that count to be 0."""
import functools
import heapq
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests.test_fps_host import doubled_cloud, two_clusters

pytestmark = pytest.mark.gpu
DEV = "cuda"


def knn_graph_f64(pos):
    """-> (nbr [n,kk], w [n,kk]): per row the kk = min(10, n-1) smallest ((dx*dx + dy*dy) + dz*dz, j), the point itself left out.
    Row-chunked; a stable argsort restricted to the candidates not above the row's kk-th smallest value (the same first kk
    entries as a stable argsort of the whole row, without sorting 16 384 values per row)."""
    p = np.asarray(pos, dtype=np.float64)
    n = p.shape[0]
    kk = min(10, n - 1)
    nbr, w = np.zeros((n, kk), dtype=np.int64), np.zeros((n, kk))
    if kk == 0:
        return nbr, w

    def rows(lo):
        hi = min(n, lo + 512)
        dx, dy, dz = (p[None, :, a] - p[lo:hi, None, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(hi - lo), np.arange(lo, hi)] = np.inf
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        for r in range(hi - lo):
            c = np.flatnonzero(d2[r] <= kth[r])
            c = c[np.argsort(d2[r, c], kind="stable")][:kk]
            nbr[lo + r], w[lo + r] = c, np.sqrt(d2[r, c])

    with ThreadPoolExecutor(8) as pool:                  # numpy releases the interpreter lock inside its loops
        list(pool.map(rows, range(0, n, 512)))
    return nbr, w


def replay(graph, picks):
    """-> the number of rounds NOT held to the exact index (finite, non-zero relative gap <= 1e-9); asserts the rule above."""
    nbr, w = graph
    n = nbr.shape[0]
    picks = [int(v) for v in picks]
    assert all(0 <= v < n for v in picks)
    nbr_l, w_l = nbr.tolist(), w.tolist()
    D = np.full(n, np.inf)
    loose = 0
    for r in range(1, len(picks)):
        src = picks[r - 1]
        D[src] = 0.0
        heap = [(0.0, src)]
        while heap:
            du, u = heapq.heappop(heap)
            for v, wv in zip(nbr_l[u], w_l[u]):
                nd = du + wv
                if nd < D[v]:
                    D[v] = nd
                    heapq.heappush(heap, (nd, v))
        pick, first = picks[r], int(np.argmax(D))
        mx = D[first]
        assert D[pick] >= mx * (1 - 1e-12) if np.isfinite(mx) else D[pick] == mx, (r, pick, first, D[pick], mx)
        second = np.partition(D, -2)[-2] if n > 1 else mx
        gap = 0.0 if (not np.isfinite(mx) or mx == 0) else (mx - second) / mx
        if np.isfinite(mx) and mx != 0 and 0 < gap <= 1e-9:
            loose += 1
        else:
            assert pick == first, (r, pick, first, gap)
    return loose


def device_fps(clouds, m, starts, dtype=torch.float32):
    from deltaconv_amd.geometry import geodesic_fps_batch
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(c) for c in clouds])]), dtype=torch.int64)
    pos = torch.from_numpy(np.concatenate(clouds)).to(dtype).to(DEV)
    out = geodesic_fps_batch(pos, ptr, m, start=starts)
    assert out.dtype == torch.int64 and out.shape == (len(clouds), m) and out.is_cuda
    return out.cpu().numpy()


# ---- 1. the fixtures of the acceptance rule ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(n, seed):
    pos = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    return pos, knn_graph_f64(pos)


FIXTURES = [(200, 50, 0, "f32"), (1000, 128, 1, "f32"), (2500, 64, 2, "f32"), (8193, 32, 5, "f32"), (16384, 8, 4, "f32"),
            (200, 50, 0, "f64"), (1000, 128, 1, "f64"), (2500, 64, 2, "f64")]


@pytest.mark.parametrize("n,m,seed,dt", FIXTURES)
def test_picks_replay_as_farthest_points(n, m, seed, dt):
    pos, graph = fixture(n, seed)
    got = device_fps([pos], m, [0], torch.float32 if dt == "f32" else torch.float64)[0]
    assert got[0] == 0
    assert replay(graph, got) == 0                       # no round of these fixtures is close enough to be excused


# ---- 2. ragged launch, degenerate clouds ---------------------------------------------------------------------------------------
def test_ragged_clouds_in_one_launch():
    from deltaconv_amd.geometry import geodesic_fps
    sizes, m = [1, 7, 64, 333, 1000], 40
    rng = np.random.default_rng(21)
    clouds = [rng.random((n, 3)).astype(np.float32) for n in sizes]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        host = [np.atleast_1d(geodesic_fps(c, m, seed=3)) for c in clouds[:2]]
    starts = [int(host[0][0]), int(host[1][0]), 5, 100, 999]
    got = device_fps(clouds, m, starts)
    for c, row, s in zip(clouds, got, starts):
        assert row[0] == s
        assert replay(knn_graph_f64(c), row) == 0
    # n = 1 and n = 7 (complete graphs, then all-zero rounds): structural ties only, equal to the host library exactly
    assert np.array_equal(got[0], host[0]) and np.array_equal(got[1], host[1])


@pytest.mark.parametrize("make,m", [(two_clusters, 30), (doubled_cloud, 130)])
def test_disconnected_and_duplicated_clouds(make, m):
    pos = make()
    got = device_fps([pos], m, [2])[0]
    assert replay(knn_graph_f64(pos), got) == 0
    if make is two_clusters:
        side = pos[got, 0] > 50
        assert side.any() and not side.all()             # the +inf round crossed over


def test_reproducible_and_independent_of_the_batch():
    rng = np.random.default_rng(22)
    clouds = [rng.random((n, 3)).astype(np.float32) for n in (500, 64, 1500, 9, 300)]
    starts = [1, 2, 3, 4, 5]
    a, b = device_fps(clouds, 48, starts), device_fps(clouds, 48, starts)
    assert np.array_equal(a, b)
    for i in (0, 2, 3):
        assert np.array_equal(device_fps([clouds[i]], 48, [starts[i]])[0], a[i])


def test_seeded_starts_do_not_depend_on_launch_grouping():
    from deltaconv_amd.geometry import geodesic_fps_batch
    from deltaconv_amd.geometry.fps import fps_starts
    from tests import batch_restate as R
    from deltaconv_amd.loader import DeviceDataset
    sizes = [40, 90, 33, 120, 64]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]))
    pos = torch.rand(int(ptr[-1]), 3, device=DEV)
    a = geodesic_fps_batch(pos, ptr, 16, seed=7)
    assert torch.equal(a, geodesic_fps_batch(pos, ptr.to(DEV), 16, seed=7))
    assert np.array_equal(a[:, 0].cpu().numpy(), fps_starts(sizes, 7))
    store = DeviceDataset.from_dataset(R.make_items(5, sizes), DEV)
    whole, split = store.geodesic_subsample(16, seed=7), store.geodesic_subsample(16, seed=7, clouds_per_launch=2)
    assert torch.equal(whole.pos, split.pos) and torch.equal(whole.norm, split.norm)


# ---- 3. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from deltaconv_amd.geometry import geodesic_fps_batch
    pos = torch.rand(16385, 3, device=DEV)
    with pytest.raises(ValueError, match="16384"):
        geodesic_fps_batch(pos, torch.tensor([0, 16385]), 4)
    with pytest.raises(ValueError, match="empty"):
        geodesic_fps_batch(pos[:10], torch.tensor([0, 10, 10]), 4)
    with pytest.raises(ValueError, match="start"):
        geodesic_fps_batch(pos[:10], torch.tensor([0, 4, 10]), 4, start=[0, 6])
    with pytest.raises(ValueError, match="start"):
        geodesic_fps_batch(pos[:10], torch.tensor([0, 4, 10]), 4, start=[-1, 0])
    with pytest.raises(ValueError, match="HIP device"):
        geodesic_fps_batch(pos[:10].cpu(), torch.tensor([0, 10]), 4)
    with pytest.raises(ValueError, match="ptr"):
        geodesic_fps_batch(pos[:10], torch.tensor([0, 9]), 4)
    assert geodesic_fps_batch(pos[:10], torch.tensor([0, 10]), 4, start=[9]).tolist()[0][0] == 9


# ---- 4. the store ----------------------------------------------------------------------------------------------------------------
def test_device_dataset_subsamples_every_attribute():
    import deltaconv_amd as dc
    from deltaconv_amd.geometry import geodesic_fps_batch
    from deltaconv_amd.geometry.fps import fps_starts
    from deltaconv_amd.loader import DeviceDataset, DeviceLoader
    from tests import batch_restate as R
    sizes, m = [20, 500, 33, 257, 128, 31], 32
    items = R.make_items(len(sizes), sizes)
    g = torch.Generator().manual_seed(4)
    for d in items:
        d.y = torch.randint(0, 50, (d.pos.shape[0],), generator=g)          # per-point labels
        d.x = torch.randn(d.pos.shape[0], 5, generator=g)
    plain = DeviceDataset.from_dataset(items, DEV)
    store = DeviceDataset.from_dataset(items, DEV, fps=m, fps_seed=3)
    assert len(store) == len(sizes) and np.array_equal(store.sizes, np.full(len(sizes), m))
    assert torch.equal(store.ptr, torch.arange(len(sizes) + 1, device=DEV) * m) and store.ptr.dtype == torch.int64
    ids = geodesic_fps_batch(plain.pos, plain.ptr, m, start=fps_starts(sizes, 3)).cpu()
    rows = []
    for i, n in enumerate(sizes):                                            # the tiling rule of T.GeodesicFPS
        idx = ids[i]
        if n < m:
            idx = idx[:n].repeat(-(-m // n))
        rows.append(idx[:m] + int(plain.ptr[i]))
    rows = torch.cat(rows).to(DEV)
    for name in ("pos", "norm", "x", "y_point"):
        assert torch.equal(getattr(store, name), getattr(plain, name)[rows]), name
    assert store.y_cloud is None and store.category is None
    for i in (0, 5):                                                         # clouds below m: every point, then again from the top
        assert sorted(ids[i][:sizes[i]].tolist()) == list(range(sizes[i]))
    # per-cloud labels pass through, and a loader over the result feeds the classification model
    items = R.make_items(len(sizes), sizes)
    store = DeviceDataset.from_dataset(items, DEV, fps=m, fps_seed=3)
    assert torch.equal(store.y_cloud.cpu(), torch.cat([d.y for d in items]))
    batch = next(iter(DeviceLoader(store, 4)))
    assert batch.pos.shape == (4 * m, 3) and batch.num_graphs == 4
    torch.manual_seed(5)
    model = dc.models.DeltaNetClassification(in_channels=3, num_classes=40, num_neighbors=20).to(DEV).eval()
    with torch.no_grad():
        logits = model(batch)
    assert logits.shape == (4, 40) and bool(torch.isfinite(logits).all())


def test_clouds_above_the_cap_take_the_host_path_beside_the_device_ones():
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry import geodesic_fps, geodesic_fps_batch
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS, fps_starts
    from deltaconv_amd.loader import DeviceDataset
    g = torch.Generator().manual_seed(8)
    sizes, m = [50, FPS_MAX_POINTS + 6, 80], 8
    items = [Data(pos=torch.rand(n, 3, generator=g), norm=torch.rand(n, 3, generator=g)) for n in sizes]
    sub = DeviceDataset.from_dataset(items, DEV).geodesic_subsample(m, seed=2)
    starts = fps_starts(sizes, 2)
    small = torch.cat([items[0].pos, items[2].pos]).to(DEV)
    ids = geodesic_fps_batch(small, torch.tensor([0, 50, 130]), m, start=starts[[0, 2]]).cpu()
    host_seed = int(np.random.Generator(np.random.Philox(key=[2, 1])).integers(0, 2 ** 31))
    want = [ids[0], torch.from_numpy(geodesic_fps(items[1].pos.numpy(), m, seed=host_seed).astype(np.int64)), ids[1]]
    for i, (d, idx) in enumerate(zip(items, want)):
        assert torch.equal(sub.pos[m * i:m * (i + 1)].cpu(), d.pos[idx]), i
        assert torch.equal(sub.norm[m * i:m * (i + 1)].cpu(), d.norm[idx]), i
