"""The device geodesic farthest-point sampler for clouds above the LDS kernel's cap (csrc/fps.hip: ``fps_sample_global_kernel``
behind ``dc_geodesic_fps_large``) without a GPU: a g++ build of the shared arithmetic (csrc/fps_math.h) drives a serial emulation
of the kernel (tests/hostcheck_fps_large) -- D as 64-bit patterns lowered by an unsigned minimum, two frontier bit sets of exactly
``bitset_words(n)`` words scanned by word, the same arg-max combine.  Its picks equal the host library's (``geodesic_fps``, heap
Dijkstra) EXACTLY, as those of tests/test_fps_host.py do.  Also: the stand-alone sanitizer build of the emulation, the entry
point's argument errors and workspace size, and the ``large=`` dispatch of ``DeviceDataset.geodesic_subsample``."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest

from tests.helpers import ROOT
from tests.test_fps_host import CASES, shell

HFL_DIR = os.path.join(ROOT, "tests", "hostcheck_fps_large")


@pytest.fixture(scope="module")
def hfl():
    subprocess.run(["make", "-s", "-C", HFL_DIR], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "deltaconv_amd", "csrc_host")], check=True)
    lib = ctypes.CDLL(os.path.join(HFL_DIR, "libhostcheck_fps_large.so"))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.hfl_fps.argtypes = [vp, i32, i32, i32, vp]
    lib.hfl_fps.restype = ctypes.c_int
    lib.hfl_workspace_bytes.argtypes = [ctypes.c_int64]
    lib.hfl_workspace_bytes.restype = ctypes.c_uint64
    lib.hfl_lds_bytes.argtypes = [i32]
    lib.hfl_lds_bytes.restype = ctypes.c_uint64
    return lib


def emulate(hfl, pos, m, start):
    pts = np.ascontiguousarray(pos, dtype=np.float64)
    out = np.empty(m, dtype=np.int32)
    assert hfl.hfl_fps(pts.ctypes.data, pts.shape[0], m, int(start), out.ctypes.data) == 0
    return out


# the cases of tests/test_fps_host.py, then the bit-set word edges and the first size the LDS kernel does not take
LARGE_CASES = dict(CASES)
LARGE_CASES.update({"n33": (lambda: shell(33, 9), 33, 9), "n64_full": (lambda: shell(64, 10), 64, 10),
                    "n65": (lambda: shell(65, 11), 65, 11), "n16385": (lambda: shell(16385, 12), 12, 12)})


@pytest.mark.parametrize("case", list(LARGE_CASES))
def test_emulation_picks_the_host_librarys_points(hfl, case):
    from deltaconv_amd.geometry import geodesic_fps
    make, m, seed = LARGE_CASES[case]
    pos = make()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # "more samples than points" is the case under test
        want = np.atleast_1d(geodesic_fps(pos, m, seed=seed))
    got = emulate(hfl, pos, m, want[0])
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    if case == "two_clusters":                                             # the +inf rounds were there: both clusters are reached
        side = pos[want, 0] > 50
        assert side.any() and not side.all()


@pytest.mark.parametrize("n", [33, 64, 65])
def test_emulation_from_the_last_vertex(hfl, n):
    """The start is the last bit of the last word; every point is taken, so every bit of every word is set at some time."""
    from deltaconv_amd.geometry import geodesic_fps
    pos = shell(n, n)
    for seed in range(200):                                                # a host seed whose start is the last vertex
        want = np.atleast_1d(geodesic_fps(pos, n, seed=seed))
        if want[0] == n - 1:
            break
    else:
        pytest.fail("no seed below 200 starts at the last vertex")
    got = emulate(hfl, pos, n, n - 1)
    assert np.array_equal(got, want) and sorted(got.tolist()) == list(range(n))


def test_sanitizer_build_of_the_emulation_runs_clean(hfl):
    """The stand-alone program (own main, -fsanitize=address,undefined) checks the emulation against its own heap Dijkstra."""
    r = subprocess.run([os.path.join(HFL_DIR, "hostcheck_fps_large_san")], capture_output=True, text=True)
    assert r.returncode == 0 and "all ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_workspace_and_lds_sizes(hfl):
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry.fps import FPS_LARGE_MAX_POINTS
    assert hfl.hfl_max_points() == FPS_LARGE_MAX_POINTS == 262144 and hfl.hfl_k() == 10
    header = open(os.path.join(ROOT, "include", "deltaconv_hip.h")).read()
    assert "#define DC_FPS_LARGE_MAX_POINTS (262144)" in header
    small, large = lib.raw("dc_geodesic_fps_workspace_bytes"), lib.raw("dc_geodesic_fps_large_workspace_bytes")
    for n in (0, 1, 1000, 16385, 262144, 1 << 20):
        assert large(n) == hfl.hfl_workspace_bytes(n) >= small(n) + 8 * n
        assert large(n) <= 140 * n + 2048                                  # the 140 bytes per point the launch groups are sized by
    assert [hfl.hfl_bitset_words(n) for n in (1, 31, 32, 33, 64, 65)] == [1, 1, 1, 2, 2, 3]
    assert hfl.hfl_lds_bytes(262144) == 65536


def test_entry_point_argument_errors():
    """Every check sits in front of the first device call, so they run without a GPU."""
    from deltaconv_amd._lib import lib
    fn = lib.raw("dc_geodesic_fps_large")
    A = lambda a, t: np.asarray(a, dtype=t)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    dummy = ctypes.c_void_p(256)                                           # never dereferenced: the argument checks come first

    def call(ptr, start, B=None, m=8, mx=None, ws=1 << 30):
        ptr, start = A(ptr, np.int64), A(start, np.int32)
        B = len(ptr) - 1 if B is None else B
        mx = int(np.diff(ptr).max()) if mx is None else mx
        return fn(dummy, 0, P(ptr), B, mx, m, P(start), dummy, dummy, ws, None)

    assert call([0, 5], [0], B=0) == 0                                     # B = 0: nothing to do
    assert call([0, 262145], [0]) == -1 and "262144" in lib.last_error() and "dc_geodesic_fps_large" in lib.last_error()
    assert call([0, 5, 5], [0, 0]) == -1 and "empty" in lib.last_error()
    assert call([0, 5, 9], [0, 4]) == -1 and "start" in lib.last_error()
    assert call([0, 5, 9], [-1, 0]) == -1 and "start" in lib.last_error()
    assert call([0, 5], [0], m=0) == -1 and "n_samples" in lib.last_error()
    assert call([0, 5], [0], mx=4) == -1 and "max_cloud_size" in lib.last_error()
    assert call([0, 5], [0], mx=262145) == -1 and "max_cloud_size" in lib.last_error()
    assert call([3, 5], [0]) == -1 and "ptr[0]" in lib.last_error()
    assert call([0, 5], [0], B=-1) == -1
    assert call([0, 5], [0], ws=16) == -3 and "workspace" in lib.last_error()
    # a workspace that the LDS kernel's entry would accept is short here: D is missing
    short = int(lib.raw("dc_geodesic_fps_workspace_bytes")(20000))
    assert call([0, 20000], [0], ws=short) == -3 and "workspace" in lib.last_error()
    assert fn(None, 0, None, 1, 1, 1, None, None, None, 0, None) == -1 and "null" in lib.last_error()


def test_store_dispatch_of_large_clouds():
    import torch
    from deltaconv_amd.datasets import Data
    from deltaconv_amd.geometry.fps import FPS_MAX_POINTS
    from deltaconv_amd.loader import DeviceDataset
    g = torch.Generator().manual_seed(6)
    items = [Data(pos=torch.rand(n, 3, generator=g), norm=torch.rand(n, 3, generator=g), y=torch.randint(0, 9, (n,), generator=g))
             for n in (FPS_MAX_POINTS + 1, FPS_MAX_POINTS + 40)]
    store = DeviceDataset.from_dataset(items, "cpu")
    with pytest.raises(ValueError, match="large"):
        store.geodesic_subsample(6, seed=5, large="bogus")
    with pytest.raises(ValueError, match="HIP device"):
        store.geodesic_subsample(6, seed=5, large="device")
    with pytest.raises(ValueError, match="HIP device"):
        DeviceDataset.from_dataset(items, "cpu", fps=6, fps_seed=5, fps_large="device")
    plain, host = store.geodesic_subsample(6, seed=5), store.geodesic_subsample(6, seed=5, large="host")
    for name in ("pos", "norm", "y_point"):
        assert torch.equal(getattr(plain, name), getattr(host, name)), name
    via = DeviceDataset.from_dataset(items, "cpu", fps=6, fps_seed=5, fps_large="host")
    assert torch.equal(via.pos, plain.pos)


def test_large_launch_groups_are_bounded_by_points(monkeypatch):
    """Groups of large clouds hold at most FPS_LARGE_POINTS_PER_LAUNCH points (140 bytes of workspace each) unless one cloud alone
    is larger, and at most ``clouds_per_launch`` clouds; rows, offsets and start points stay in step."""
    import torch
    from deltaconv_amd.geometry import fps
    calls = []

    def fake(pos, ptr_host, n_samples, start_host, large=False):
        calls.append((int(pos.shape[0]), ptr_host.tolist(), [int(s) for s in start_host], large))
        return torch.tensor(start_host, dtype=torch.int32).reshape(-1, 1).repeat(1, n_samples)

    monkeypatch.setattr(fps, "_fps_device", fake)
    sizes = np.array([600000, 500000, 10, 600000, 5, 20], dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    pos = torch.zeros(int(ptr[-1]), 3)
    out = fps._fps_launches(pos, ptr, 4, np.arange(6), 1024, large=True)
    assert out[:, 0].tolist() == list(range(6))
    assert [c[1] for c in calls] == [[0, 600000], [0, 500000, 500010], [0, 600000, 600005, 600025]] and all(c[3] for c in calls)
    assert [c[2] for c in calls] == [[0], [1, 2], [3, 4, 5]]
    assert all(c[0] <= fps.FPS_LARGE_POINTS_PER_LAUNCH for c in calls)
    calls.clear()
    fps._fps_launches(pos, ptr, 4, np.arange(6), 2, large=True)
    assert [c[2] for c in calls] == [[0], [1, 2], [3, 4], [5]]
    calls.clear()                                                          # the LDS kernel's grouping is what it was
    fps._fps_launches(pos[:35], ptr[-3:] - ptr[-3], 4, np.arange(2), 1)
    assert [(c[1], c[3]) for c in calls] == [([0, 5], False), ([0, 20], False)]
