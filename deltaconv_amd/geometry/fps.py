"""Geodesic farthest-point sampling (reference: deltaconv/geometry/fps.py:5-17 over the pybind module
of deltaconv/cpp).  Same validation, same return value; the native part is the dependency-free C++
restatement in deltaconv_amd/csrc_host/fps.cpp behind a C ABI (include/deltaconv_host.h).

``geodesic_fps_batch`` is the same sampler for a batch of clouds that already live on the device (csrc/fps.hip behind
``dc_geodesic_fps_batch``): the same picks as ``geodesic_fps`` from the same start point, all clouds in two launches.  With
``large=True`` clouds above that kernel's cap go through ``dc_geodesic_fps_large``, whose distance vector lives in global memory.

``fps`` is plain EUCLIDEAN farthest-point sampling for use inside a training step (csrc/fps_euclid.hip behind ``dc_fps_batch``):
device offsets, one launch, nothing read on the host, capturable.  ``fps(method="grid")`` is the same sampler on a uniform cell
grid (csrc/fps_grid.hip behind ``dc_fps_grid``) for clouds above that kernel's cap: the same picks, bit for bit."""
import ctypes
import os
import warnings

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LIB_PATH = os.path.join(_PKG, "lib", "libdeltaconv_host.so")
_lib = None


def _host():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"{HOST_LIB_PATH} is not built (make -C deltaconv_amd/csrc_host)")
        lib = ctypes.CDLL(HOST_LIB_PATH)
        lib.dc_geodesic_fps.restype = ctypes.c_int
        lib.dc_geodesic_fps.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p]
        _lib = lib
    return _lib


def geodesic_fps(points, n_samples, seed=None):
    """points: float [V,3] numpy array -> int32 [n_samples] sample indices.  ``seed=None`` starts from a
    random point like the reference (sampling.cpp:34-40); an integer makes the start reproducible."""
    if n_samples > points.shape[0]:
        warnings.warn("Number of samples is larger than number of points.")
    if type(points) is not np.ndarray:
        raise ValueError("`points` should be a numpy array")
    if (len(points.shape) != 2) or (points.shape[1] != 3):
        raise ValueError("`points` should have shape (V,3), shape is " + str(points.shape))
    pts = np.ascontiguousarray(points, dtype=np.float64)
    out = np.empty(int(n_samples), dtype=np.int32)
    rc = _host().dc_geodesic_fps(pts.ctypes.data, pts.shape[0], int(n_samples), -1 if seed is None else int(seed),
                                 out.ctypes.data)
    if rc != 0:
        raise ValueError("geodesic_fps: bad arguments")
    return out.squeeze()


FPS_MAX_POINTS = 16384        # DC_FPS_MAX_POINTS: a cloud's distance vector lives in the LDS of one workgroup (csrc/fps_math.h)
FPS_LARGE_MAX_POINTS = 262144 # DC_FPS_LARGE_MAX_POINTS: the distance vector in global memory, two frontier bit sets in LDS
FPS_LARGE_POINTS_PER_LAUNCH = 1 << 20   # points of a group of large clouds: its workspace holds 140 bytes per point (140 MiB)
FPS_EUCLID_MAX_POINTS = 16384 # DC_FPS_EUCLID_MAX_POINTS: a cloud's positions and minima live in the registers of one workgroup
FPS_GRID_MAX_POINTS = 262144  # DC_FPS_GRID_MAX_POINTS: one key per 64 of a cloud's at most 2 n cells lives in the LDS of one workgroup
# The sampler behind ``fps`` / ``fps_levels`` where the call names none: "brute" (dc_fps_batch, the register kernel) or "grid" (the
# exact sampler over a uniform cell grid, csrc/fps_grid.hip: the same picks bit for bit, clouds up to FPS_GRID_MAX_POINTS).
# DC_FPS=brute|grid; no policy picks by size.
FPS_METHODS = ("brute", "grid")
FPS_METHOD = [os.environ.get("DC_FPS", "") or "brute"]
FPS_GRID_TARGET = 0.5         # mean points per cell where the call names none (csrc/fps_grid_math.h: DEFAULT_TARGET; README: measured)


def fps_method(fn, method):
    """The `method` argument of a sampler, None = the switch -> "brute" | "grid"."""
    method = FPS_METHOD[0] if method is None else method
    if method not in FPS_METHODS:
        raise ValueError(f"{fn}: method = {method!r} (DC_FPS where the call names none), known: {', '.join(FPS_METHODS)}")
    return method


def coarse_sizes(ratio, largest, smallest):
    """(largest, smallest) cloud of the level below one with those: ``ceil(n / ratio)``, the arithmetic of ``prefix_levels``."""
    return -(-int(largest) // ratio), -(-int(smallest) // ratio)


def coarse_offsets(ptr, b, ratio, largest, smallest):
    """The output offsets of a ``ratio`` level over the int64 device offsets ``ptr`` -> (optr int64 [B+1], rows in all), as
    ``prefix_levels`` derives them: a uniform batch synchronises nothing, a ragged one reads its total once."""
    import torch
    mx, mn = coarse_sizes(ratio, largest, smallest)
    if largest == smallest:
        return torch.arange(b + 1, dtype=torch.int64, device=ptr.device) * mx, b * mx
    optr = torch.zeros(b + 1, dtype=torch.int64, device=ptr.device)
    optr[1:] = torch.cumsum((ptr[1:] - ptr[:-1] + (ratio - 1)) // ratio, 0)
    return optr, int(optr[-1])                 # the one host read


def fps_launch(pos, ptr, optr, b, max_cloud, max_samples, total, start=None, out=None):
    """``dc_fps_batch`` on checked arguments: fp32 [N,3] positions, int64 device offsets in and out -> rows int64 [total]."""
    import torch
    from .._lib import lib
    fn = "fps"
    if max_cloud > FPS_EUCLID_MAX_POINTS:
        raise ValueError(f"{fn}: a cloud of {max_cloud} points; the sampler takes at most {FPS_EUCLID_MAX_POINTS} per cloud "
                         "(FPS_EUCLID_MAX_POINTS: a cloud lives in the registers of one workgroup)")
    if start is not None:
        if not torch.is_tensor(start) or not start.is_cuda or start.dim() != 1 or start.shape[0] != b or \
                start.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{fn}: `start` must be a device int32 / int64 tensor of {b} ids local to their clouds")
        start = start.to(torch.int32).contiguous()
    if out is None:
        out = torch.empty(total, dtype=torch.int64, device=pos.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.int64 or tuple(out.shape) != (total,) or \
            not out.is_contiguous():
        raise ValueError(f"{fn}: `out` must be a contiguous device int64 tensor of {total} rows")
    if b and total:
        lib.call("dc_fps_batch", pos, ptr, optr, b, int(max_cloud), int(max_samples), start, out)
    return out


def fps_grid_launch(pos, ptr, optr, b, max_cloud, max_samples, total, start=None, out=None, grid_target=None, stats=False):
    """``dc_fps_grid`` on checked arguments, the workspace from torch's allocator -> rows int64 [total], or (rows, stats int64
    [b,2]) with ``stats``."""
    import torch
    from .._lib import lib
    fn = "fps"
    if max_cloud > FPS_GRID_MAX_POINTS:
        raise ValueError(f"{fn}: a cloud of {max_cloud} points; the grid sampler takes at most {FPS_GRID_MAX_POINTS} per cloud "
                         "(FPS_GRID_MAX_POINTS: the keys of a cloud's cell blocks live in the LDS of one workgroup)")
    target = float(FPS_GRID_TARGET if grid_target is None else grid_target)
    if not (target > 0.0 and target < float("inf")):
        raise ValueError(f"{fn}: grid_target = {grid_target!r} must be positive and finite")
    if start is not None:
        if not torch.is_tensor(start) or not start.is_cuda or start.dim() != 1 or start.shape[0] != b or \
                start.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{fn}: `start` must be a device int32 / int64 tensor of {b} ids local to their clouds")
        start = start.to(torch.int32).contiguous()
    if out is None:
        out = torch.empty(total, dtype=torch.int64, device=pos.device)
    elif not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.int64 or tuple(out.shape) != (total,) or \
            not out.is_contiguous():
        raise ValueError(f"{fn}: `out` must be a contiguous device int64 tensor of {total} rows")
    st = torch.zeros((b, 2), dtype=torch.int64, device=pos.device) if stats else None
    if b and total:
        nbytes = int(lib.raw("dc_fps_grid_workspace_bytes")(int(pos.shape[0]), int(b)))
        if nbytes == 0:
            raise ValueError(f"{fn}: {int(pos.shape[0])} points in {b} clouds are out of range")
        work = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=pos.device)
        lib.call("dc_fps_grid", pos, ptr, optr, b, int(max_cloud), int(max_samples), start, target, out, st, work, nbytes)
    return (out, st) if stats else out


def fps(pos, ptr=None, batch=None, ratio=None, n_samples=None, start=None, ptr_info=None, out=None, method=None, grid_target=None,
        stats=False):
    """Euclidean farthest-point sampling of every cloud of a batch on the device, in ONE launch that reads nothing on the host
    (``torch_cluster.fps(pos, batch, ratio)``; csrc/fps_euclid.hip behind ``dc_fps_batch``).

    pos: DEVICE float32 [N,3].  The clouds: ``ptr_info`` (a ``PtrInfo``: offsets, B, largest cloud, ``min_cloud`` -- nothing is
    read), or ``ptr`` (B+1 absolute offsets; largest and smallest cloud are read once), or a sorted ``batch`` vector (one read), or
    one cloud of N rows.  Exactly one of ``ratio`` (an integer >= 1: ``ceil(n_b / ratio)`` picks of cloud b, the sizes of
    ``prefix_levels``; a ragged batch reads its total once) and ``n_samples`` (that many picks of every cloud; a smaller cloud
    raises).  ``start``: DEVICE int32 / int64 [B], the first pick of every cloud as an id local to it (an id outside its cloud is
    read as 0); None starts every cloud at its row 0.
    -> ``(rows int64 [N_out], optr int64 [B+1])``: ``rows[optr[b] + r]`` is the GLOBAL row of cloud b's pick r, in pick order.

    The rules (csrc/fps_euclid_math.h): the fp32 distance ``(dx*dx + dy*dy) + dz*dz``, a running minimum per point, the next pick
    is the FIRST index of its maximum; points with a non-finite coordinate are picked last.  The picks are pairwise distinct, a
    function of the inputs only, and the first m' picks of m are the m'-pick sample -- a cloud whose rows are re-ordered to
    ``pos[rows]`` samples to the identity prefix, which is what ``prefix_levels`` rests on.  Clouds above
    ``FPS_EUCLID_MAX_POINTS`` = 16 384 points, empty clouds where the host knows of them, host tensors and anything but float32
    [N,3] raise ``ValueError``; a ``pos`` that requires grad raises (nothing here is differentiable).  The call can be captured
    by ``torch.cuda.graph`` when the sizes come from ``ptr_info`` and the batch is uniform or ``n_samples`` is given.

    ``method``: "brute" (``dc_fps_batch``, the register kernel above) or "grid" (``dc_fps_grid``, csrc/fps_grid.hip: the SAME
    picks bit for bit, found on a uniform cell grid -- a pick updates only the points near it; clouds up to
    ``FPS_GRID_MAX_POINTS`` = 262 144 points; six launches and a workspace from torch's allocator, still nothing read on the
    host), None = ``FPS_METHOD[0]`` (``DC_FPS``, default "brute").  ``grid_target``: the grid's mean points per cell (None =
    ``FPS_GRID_TARGET``); it cannot change a pick, and with "brute" it raises.  ``stats=True`` (grid only) adds a third result,
    int64 [B,2]: per cloud the point updates evaluated and the cells visited, summed over its picks."""
    import torch
    from . import _cross
    from .graph import _min_cloud, _ptr_from_batch
    fn = "fps"
    method = fps_method(fn, method)
    if method != "grid" and grid_target is not None:
        raise ValueError(f"{fn}: grid_target sizes the cells of method='grid'; it cannot be combined with method='brute'")
    if method != "grid" and stats:
        raise ValueError(f"{fn}: stats are the grid sampler's (method='grid')")
    if not torch.is_tensor(pos) or not pos.is_cuda:
        raise ValueError(f"{fn}: `pos` must be a tensor on a HIP device (there is no CPU path)")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
        raise ValueError(f"{fn}: `pos` must be float32 [N,3], got {pos.dtype} {tuple(pos.shape)}")
    _cross.no_grad_inputs(fn, pos=pos)
    if (ratio is None) == (n_samples is None):
        raise ValueError(f"{fn}: give exactly one of ratio and n_samples")
    if ratio is not None and (int(ratio) != ratio or int(ratio) < 1):
        raise ValueError(f"{fn}: ratio must be an integer >= 1, got {ratio!r}")
    if n_samples is not None and (int(n_samples) != n_samples or int(n_samples) < 1):
        raise ValueError(f"{fn}: n_samples must be an integer >= 1, got {n_samples!r}")
    if sum(a is not None for a in (ptr, batch, ptr_info)) > 1:
        raise ValueError(f"{fn}: give one of ptr, batch and ptr_info")
    n, dev = int(pos.shape[0]), pos.device
    if ptr_info is not None:
        b, mx, mn = int(ptr_info[1]), int(ptr_info[2]), _min_cloud(ptr_info)
        ptr = ptr_info[0].to(device=dev, dtype=torch.int64).contiguous()
    elif ptr is not None:
        ptr = torch.as_tensor(ptr).to(device=dev, dtype=torch.int64).contiguous()
        if ptr.dim() != 1 or ptr.numel() < 1:
            raise ValueError(f"{fn}: `ptr` must hold B+1 offsets")
        b = int(ptr.numel()) - 1
        sizes = ptr[1:] - ptr[:-1]
        lo, hi, mn, mx = (torch.stack([ptr[0], ptr[-1], sizes.min(), sizes.max()]).tolist() if b else (0, 0, 1, 1))   # one read
        if lo < 0 or hi > n:
            raise ValueError(f"{fn}: `ptr` runs from {lo} to {hi}, `pos` has {n} rows")
    else:
        if batch is not None and (not torch.is_tensor(batch) or batch.dim() != 1 or batch.shape[0] != n):
            raise ValueError(f"{fn}: `batch` must hold one cloud id per row")
        if n == 0:
            raise ValueError(f"{fn}: empty cloud")
        info = _ptr_from_batch(None if batch is None else batch.to(dev), n, dev)
        ptr, b, mx, mn = info[0].to(torch.int64), int(info[1]), int(info[2]), int(info.min_cloud)
    if ptr.numel() != b + 1:
        raise ValueError(f"{fn}: {b} clouds need {b + 1} offsets, got {ptr.numel()}")
    if b and mn < 1:
        raise ValueError(f"{fn}: empty cloud")
    if b and method == "brute" and mx > FPS_EUCLID_MAX_POINTS:
        raise ValueError(f"{fn}: a cloud of {mx} points; the sampler takes at most {FPS_EUCLID_MAX_POINTS} per cloud "
                         "(FPS_EUCLID_MAX_POINTS: a cloud lives in the registers of one workgroup)")
    if b and method == "grid" and mx > FPS_GRID_MAX_POINTS:
        raise ValueError(f"{fn}: a cloud of {mx} points; the grid sampler takes at most {FPS_GRID_MAX_POINTS} per cloud "
                         "(FPS_GRID_MAX_POINTS: the keys of a cloud's cell blocks live in the LDS of one workgroup)")
    if ratio is not None:
        optr, total = coarse_offsets(ptr, b, int(ratio), mx, mn)
        most = coarse_sizes(int(ratio), mx, mn)[0]
    else:
        most = int(n_samples)
        if b and mn < most:
            raise ValueError(f"{fn}: n_samples = {most}, but a cloud has only {mn} points")
        optr, total = torch.arange(b + 1, dtype=torch.int64, device=dev) * most, b * most
    if method == "grid":
        got = fps_grid_launch(pos.detach().contiguous(), ptr, optr, b, mx if b else 0, most, total, start, out, grid_target, stats)
        return (got[0], optr, got[1]) if stats else (got, optr)
    return fps_launch(pos.detach().contiguous(), ptr, optr, b, mx if b else 0, most, total, start, out), optr


def fps_starts(sizes, seed=None, first=0):
    """The start point of every cloud: ``sizes[i]`` points, cloud index ``first + i``.  With a seed it is a function of
    ``(seed, cloud index, size)`` only -- a counter-based generator keyed by the pair, as ``loader.epoch_permutation`` keys its
    own by (seed, epoch) -- so it does not depend on how clouds are grouped into launches; ``seed=None`` draws at random like
    the reference (sampling.cpp:34-40).  -> int32 [len(sizes)]"""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if sizes.size and sizes.min() < 1:
        raise ValueError("geodesic_fps_batch: empty cloud")
    if seed is None:
        return np.random.default_rng().integers(0, sizes).astype(np.int32)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("geodesic_fps_batch: seed in [0, 2^64)")
    return np.array([np.random.Generator(np.random.Philox(key=[int(seed), int(first) + i])).integers(0, int(n))
                     for i, n in enumerate(sizes)], dtype=np.int32).reshape(-1)


def _fps_device(pos, ptr_host, n_samples, start_host, large=False):
    """One launch pair over the clouds ptr_host (numpy int64 [B+1], ptr_host[0] = 0) of pos -> int32 [B, n_samples] on the device.
    ``large``: through ``dc_geodesic_fps_large`` (clouds of 1 .. FPS_LARGE_MAX_POINTS points) instead of the LDS kernel."""
    import torch
    from .._lib import lib
    b = int(ptr_host.shape[0]) - 1
    out = torch.empty((b, int(n_samples)), dtype=torch.int32, device=pos.device)
    if b == 0:
        return out
    ptr_host = np.ascontiguousarray(ptr_host, dtype=np.int64)
    start_host = np.ascontiguousarray(start_host, dtype=np.int32)
    entry, sizer = (("dc_geodesic_fps_large", "dc_geodesic_fps_large_workspace_bytes") if large else
                    ("dc_geodesic_fps_batch", "dc_geodesic_fps_workspace_bytes"))
    need = int(lib.raw(sizer)(int(ptr_host[-1])))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=pos.device)
    sizes = ptr_host[1:] - ptr_host[:-1]
    lib.call(entry, pos, 1 if pos.dtype == torch.float64 else 0, ctypes.c_void_p(ptr_host.ctypes.data), b,
             int(sizes.max()), int(n_samples), ctypes.c_void_p(start_host.ctypes.data), out, ws, need)
    return out


def _fps_launches(pos, ptr_host, n_samples, start_host, clouds_per_launch=1024, large=False):
    """The clouds in groups of at most `clouds_per_launch` (the workspace holds 132 bytes per point of a group) -> int32 [B, n_samples].
    ``large``: groups of at most FPS_LARGE_POINTS_PER_LAUNCH points as well (one cloud at least; 140 bytes per point)."""
    import torch
    b = int(ptr_host.shape[0]) - 1
    if not large:
        if b <= clouds_per_launch:
            return _fps_device(pos, ptr_host, n_samples, start_host)
        bounds = list(range(0, b, clouds_per_launch)) + [b]
    else:
        bounds = [0]
        for i in range(b):                               # cloud i opens a group where the open one is full by count or by points
            lo = bounds[-1]
            if i > lo and (i - lo >= clouds_per_launch or ptr_host[i + 1] - ptr_host[lo] > FPS_LARGE_POINTS_PER_LAUNCH):
                bounds.append(i)
        bounds.append(b)
    parts = [_fps_device(pos[int(ptr_host[lo]):int(ptr_host[hi])], ptr_host[lo:hi + 1] - ptr_host[lo], n_samples, start_host[lo:hi],
                         large) for lo, hi in zip(bounds[:-1], bounds[1:])]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def _fps_by_size_class(pos, ptr_host, n_samples, start_host, clouds_per_launch=1024):
    """Every cloud on the device, whatever its size up to FPS_LARGE_MAX_POINTS: clouds of at most FPS_MAX_POINTS points through
    the LDS kernel, the others through the global-memory kernel; rows in input order -> int64 [B, n_samples].  Both kernels give
    a cloud the same picks, so the result does not depend on which side of the cap a cloud falls."""
    import torch
    sizes = ptr_host[1:] - ptr_host[:-1]
    big = sizes > FPS_MAX_POINTS
    if not big.any():
        return _fps_launches(pos, ptr_host, n_samples, start_host, clouds_per_launch).long()
    if big.all():
        return _fps_launches(pos, ptr_host, n_samples, start_host, clouds_per_launch, large=True).long()
    dev = pos.device
    ids = torch.empty((sizes.size, int(n_samples)), dtype=torch.int64, device=dev)
    for mask, is_large in ((~big, False), (big, True)):
        sel = np.flatnonzero(mask)
        rows = torch.from_numpy(np.concatenate([np.arange(ptr_host[i], ptr_host[i + 1]) for i in sel])).to(dev)
        ptr_sel = np.zeros(sel.size + 1, dtype=np.int64)
        ptr_sel[1:] = np.cumsum(sizes[sel])
        ids[torch.from_numpy(sel).to(dev)] = _fps_launches(pos[rows], ptr_sel, n_samples, start_host[sel], clouds_per_launch,
                                                           large=is_large).long()
    return ids


def geodesic_fps_batch(pos, ptr, n_samples, start=None, seed=None, large=False):
    """Geodesic farthest-point sampling of every cloud of a batch on the device (reference: transforms/geodesic_fps.py:14-43
    over cpp/sampling.cpp:5-81, one host call per shape).

    pos: DEVICE float32 / float64 [N,3]; ptr: int64 [B+1] cloud offsets (tensor on any device, or array), ptr[0] = 0 and
    ptr[B] = N.  -> DEVICE int64 [B, n_samples], ids local to the cloud: row b is what ``geodesic_fps(pos[ptr[b]:ptr[b+1]],
    n_samples)`` returns when it starts from the same point.  ``start``: the first sample of every cloud (B ids local to the
    cloud); otherwise ``fps_starts(sizes, seed)``.  Clouds of more than ``FPS_MAX_POINTS`` = 16 384 points, empty clouds, a
    start outside its cloud and host tensors raise ``ValueError``; there is no CPU path (``geodesic_fps`` is the host sampler).
    ``large=True``: clouds above ``FPS_MAX_POINTS`` are sampled too, by the kernel that keeps the distance vector in global
    memory (``dc_geodesic_fps_large``, up to ``FPS_LARGE_MAX_POINTS`` = 262 144 points; above that ``ValueError``); the others
    still go to the LDS kernel, and the rows come back in input order."""
    import torch
    if not torch.is_tensor(pos) or not pos.is_cuda:
        raise ValueError("geodesic_fps_batch: `pos` must be a tensor on a HIP device (geodesic_fps samples host arrays)")
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"geodesic_fps_batch: `pos` must be float32 / float64 [N,3], got {pos.dtype} {tuple(pos.shape)}")
    ptr_host = (ptr.detach().cpu().numpy() if torch.is_tensor(ptr) else np.asarray(ptr)).astype(np.int64).reshape(-1)
    if ptr_host.size < 1 or ptr_host[0] != 0 or ptr_host[-1] != pos.shape[0]:
        raise ValueError("geodesic_fps_batch: `ptr` must hold B+1 offsets from 0 to the number of points")
    if int(n_samples) < 1:
        raise ValueError("geodesic_fps_batch: n_samples >= 1")
    sizes = ptr_host[1:] - ptr_host[:-1]
    if sizes.size and sizes.min() < 1:
        raise ValueError("geodesic_fps_batch: empty cloud")
    if large and sizes.size and sizes.max() > FPS_LARGE_MAX_POINTS:
        raise ValueError(f"geodesic_fps_batch: a cloud of {int(sizes.max())} points; the device sampler for large clouds takes "
                         f"at most {FPS_LARGE_MAX_POINTS} per cloud (use geodesic_fps on the host for larger ones)")
    if not large and sizes.size and sizes.max() > FPS_MAX_POINTS:
        raise ValueError(f"geodesic_fps_batch: a cloud of {int(sizes.max())} points; the device sampler takes at most "
                         f"{FPS_MAX_POINTS} per cloud (use geodesic_fps on the host for larger ones)")
    if start is None:
        start_host = fps_starts(sizes, seed)
    else:
        start_host = (start.detach().cpu().numpy() if torch.is_tensor(start) else np.asarray(start)).astype(np.int64).reshape(-1)
        if start_host.shape != sizes.shape or (start_host < 0).any() or (start_host >= sizes).any():
            raise ValueError("geodesic_fps_batch: `start` must hold one point of every cloud (ids local to the cloud)")
    if large:
        return _fps_by_size_class(pos.contiguous(), ptr_host, n_samples, start_host)
    return _fps_launches(pos.contiguous(), ptr_host, n_samples, start_host).long()


class _CallableModule(type(os)):             # type(os): types.ModuleType
    """``geometry.fps`` names this module (``geometry.fps.fps_starts``, ``from deltaconv_amd.geometry import fps``) AND the
    sampler users expect under that name: calling the module is calling ``fps.fps``."""

    def __call__(self, *args, **kwargs):
        return fps(*args, **kwargs)


import sys as _sys  # noqa: E402
_sys.modules[__name__].__class__ = _CallableModule
