"""The device geodesic farthest-point sampler (csrc/fps.hip) without a GPU: a g++ build of its shared arithmetic
(csrc/fps_math.h) drives a serial emulation of both kernels (tests/hostcheck_fps) -- the top-10 rule per query, the
sweep-until-stable relaxation over two frontier flag arrays, the (value, index) arg-max combine.  Its picks equal the host
library's (``geodesic_fps``, heap Dijkstra) EXACTLY: on the CPU both sides share IEEE arithmetic (no contraction, the same
``sqrt``), so equality holds at ties as well.  Also: the stand-alone sanitizer build of the emulation, the entry point's argument
errors, and the seed -> start derivation of ``geodesic_fps_batch``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import fps as ofps
from tests.helpers import ROOT

HF_DIR = os.path.join(ROOT, "tests", "hostcheck_fps")


@pytest.fixture(scope="module")
def hf():
    subprocess.run(["make", "-s", "-C", HF_DIR], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "deltaconv_amd", "csrc_host")], check=True)
    lib = ctypes.CDLL(os.path.join(HF_DIR, "libhostcheck_fps.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.hf_fps.argtypes = [vp, i32, i32, i32, vp]
    lib.hf_fps.restype = ctypes.c_int
    lib.hf_workspace_bytes.argtypes = [ctypes.c_int64]
    lib.hf_workspace_bytes.restype = ctypes.c_uint64
    return lib


def emulate(hf, pos, m, start):
    pts = np.ascontiguousarray(pos, dtype=np.float64)
    out = np.empty(m, dtype=np.int32)
    assert hf.hf_fps(pts.ctypes.data, pts.shape[0], m, int(start), out.ctypes.data) == 0
    return out


def shell(n, seed):
    """The shapes of tests/test_fps.py: a noisy spherical shell."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * (1 + 0.2 * rng.random((n, 1)))


def grid_cloud():
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float64)                                           # massive ties in the kNN order and in D


def doubled_cloud():
    p = np.random.default_rng(11).random((60, 3)).astype(np.float32)
    return np.concatenate([p, p])                                         # every point twice: neighbours at distance 0


def two_clusters():
    p = np.random.default_rng(12).random((30, 3)).astype(np.float32)
    p[15:, 0] += 100.0                                                    # k = 10 < 14: no edge crosses, rounds with max(D) = +inf
    return p


CASES = {
    "shell200": (lambda: shell(200, 0), 50, 0), "shell333": (lambda: shell(333, 1), 333, 1), "shell64": (lambda: shell(64, 2), 10, 2),
    "grid": (grid_cloud, 200, 3), "doubled": (doubled_cloud, 130, 4), "two_clusters": (two_clusters, 30, 5),
    "n1": (lambda: np.array([[0.5, 0.25, 1.0]]), 5, 6), "n7_m40": (lambda: shell(7, 7), 40, 7), "n11": (lambda: shell(11, 8), 11, 8),
}


@pytest.mark.parametrize("case", list(CASES))
def test_emulation_picks_the_host_librarys_points(hf, case):
    import warnings
    from deltaconv_amd.geometry import geodesic_fps
    make, m, seed = CASES[case]
    pos = make()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # "more samples than points" is the case under test
        want = np.atleast_1d(geodesic_fps(pos, m, seed=seed))
    got = emulate(hf, pos, m, want[0])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    if case == "two_clusters":                                             # the +inf rounds were there: both clusters are reached
        side = pos[want, 0] > 50
        assert side.any() and not side.all()


@pytest.mark.parametrize("n,m,seed", [(200, 50, 0), (333, 333, 1), (64, 10, 2)])
def test_emulation_matches_the_python_oracle(hf, n, m, seed):
    pos = shell(n, seed)
    start = int(np.random.default_rng(seed).integers(0, n))
    assert np.array_equal(emulate(hf, pos, m, start), ofps.geodesic_fps(pos, m, start=start))


def test_sanitizer_build_of_the_emulation_runs_clean(hf):
    """The stand-alone program (own main, -fsanitize=address,undefined) checks the emulation against its own heap Dijkstra."""
    r = subprocess.run([os.path.join(HF_DIR, "hostcheck_fps_san")], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_entry_point_argument_errors(hf):
    """Every check sits in front of the first device call, so they run without a GPU."""
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS
    assert hf.hf_max_points() == FPS_MAX_POINTS == 16384 and hf.hf_k() == 10
    header = open(os.path.join(ROOT, "include", "deltaconv_hip.h")).read()
    assert "#define DC_FPS_MAX_POINTS (16384)" in header
    ws_bytes = lib.raw("dc_geodesic_fps_workspace_bytes")
    assert ws_bytes(1000) == hf.hf_workspace_bytes(1000) >= 1000 * 10 * 12
    fn = lib.raw("dc_geodesic_fps_batch")
    A = lambda a, t: np.asarray(a, dtype=t)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    dummy = ctypes.c_void_p(256)                                           # never dereferenced: the argument checks come first

    def call(ptr, start, B=None, m=8, mx=None, ws=1 << 30):
        ptr, start = A(ptr, np.int64), A(start, np.int32)
        B = len(ptr) - 1 if B is None else B
        mx = int(np.diff(ptr).max()) if mx is None else mx
        return fn(dummy, 0, P(ptr), B, mx, m, P(start), dummy, dummy, ws, None)

    assert call([0, 5], [0], B=0) == 0                                     # B = 0: nothing to do
    assert call([0, 16385], [0]) == -1 and "16384" in lib.last_error()     # above the cap
    assert call([0, 5, 5], [0, 0]) == -1 and "empty" in lib.last_error()
    assert call([0, 5, 9], [0, 4]) == -1 and "start" in lib.last_error()
    assert call([0, 5, 9], [-1, 0]) == -1 and "start" in lib.last_error()
    assert call([0, 5], [0], m=0) == -1 and "n_samples" in lib.last_error()
    assert call([0, 5], [0], mx=4) == -1 and "max_cloud_size" in lib.last_error()
    assert call([3, 5], [0]) == -1 and "ptr[0]" in lib.last_error()
    assert call([0, 5], [0], B=-1) == -1
    assert call([0, 5], [0], ws=16) == -3 and "workspace" in lib.last_error()
    assert fn(None, 0, None, 1, 1, 1, None, None, None, 0, None) == -1 and "null" in lib.last_error()


def test_start_points_follow_seed_and_cloud_index_only():
    from deltaconv_amd.geometry.fps import fps_starts
    sizes = np.array([1, 7, 64, 333, 1000, 20, 16384])
    a = fps_starts(sizes, seed=3)
    assert a.dtype == np.int32 and np.array_equal(a, fps_starts(sizes, seed=3))            # reproducible
    assert (a >= 0).all() and (a < sizes).all() and a[0] == 0
    # however the clouds are grouped into launches: a group starting at cloud `first` draws what the whole list draws
    for first in (0, 2, 5):
        assert np.array_equal(fps_starts(sizes[first:first + 2], seed=3, first=first), a[first:first + 2])
    assert not np.array_equal(fps_starts(sizes, seed=4)[2:], a[2:])
    many = fps_starts(np.full(400, 50), seed=9)
    assert len(np.unique(many)) > 25                                                        # the key really includes the cloud
    r = fps_starts(sizes, seed=None)
    assert (r >= 0).all() and (r < sizes).all()
    with pytest.raises(ValueError):
        fps_starts([5, 0], seed=1)


def test_batch_sampler_refuses_host_tensors():
    import torch
    from deltaconv_amd.geometry import geodesic_fps_batch
    with pytest.raises(ValueError, match="HIP device"):
        geodesic_fps_batch(torch.rand(10, 3), torch.tensor([0, 10]), 4)


def test_store_sends_clouds_above_the_cap_through_the_host_library():
    """A store of clouds above the cap only never reaches the device sampler: host picks, gathered with torch indexing."""
    import torch
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry import geodesic_fps
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS
    from deltaconv_amd.loader import DeviceDataset
    g = torch.Generator().manual_seed(6)
    items = [Data(pos=torch.rand(n, 3, generator=g), norm=torch.rand(n, 3, generator=g), y=torch.randint(0, 9, (n,), generator=g))
             for n in (FPS_MAX_POINTS + 1, FPS_MAX_POINTS + 40)]
    store = DeviceDataset.from_dataset(items, "cpu")
    sub = store.geodesic_subsample(6, seed=5)
    assert np.array_equal(sub.sizes, [6, 6]) and sub.ptr.tolist() == [0, 6, 12]
    for i, d in enumerate(items):
        host_seed = int(np.random.Generator(np.random.Philox(key=[5, i])).integers(0, 2 ** 31))
        idx = torch.from_numpy(geodesic_fps(d.pos.numpy(), 6, seed=host_seed).astype(np.int64))
        assert torch.equal(sub.pos[6 * i:6 * i + 6], d.pos[idx]) and torch.equal(sub.norm[6 * i:6 * i + 6], d.norm[idx])
        assert torch.equal(sub.y_point[6 * i:6 * i + 6], d.y[idx])
    with pytest.raises(ValueError, match="start"):
        store.geodesic_subsample(6, start=[0, 0])
