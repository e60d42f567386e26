"""Voxel-grid subsampling benchmark (csrc/voxel.hip behind ``geometry.voxel_subsample``).  Whole passes, each ending in a device
synchronise:

  (a) a torch composition on the device: per-cloud minimum (``scatter_reduce`` amin), floor-divide, packed keys,
      ``torch.unique(return_inverse=True)``, a ``scatter_reduce`` minimum of the row index -- this is ``pick="first"``
  (b) ``geometry.voxel_subsample(pos, size, ptr=ptr, pick="first")``: seven launches and one read

on 32 x 8 192, 8 x 65 536 and 1 x 262 144 surface points from ``deltaconv_amd.data`` and on the vertex clouds of the 128-mesh
synthetic store of the other tools (1 k .. 200 k faces a mesh), each at two edge lengths found by bisection so that roughly 1/4 and
1/16 of the points are kept.  The representatives and the clusters of the two legs are asserted equal here (as sets of rows: (a)
orders a cloud's cells by key, (b) by row).  (b) with ``pick="centre"``, the default, is timed next to them.

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run and
its run-to-run spread.  No speed-up is claimed in advance.  The expectation: (b) no slower than (a) beyond (a)'s spread -- reported
per shape either way.  These are wall-clock windows of a few launches, not kernel times.

One descriptive row: ``vertex_cloud().geodesic_subsample(1024, large="device")`` alone against ``voxel_subsample(S)`` followed by
``geodesic_subsample(1024, large="device")`` on the same store.  The two produce different samples: times only.  Needs an MI355X.

    python tools/bench_voxel_subsample.py --out profiles/device_voxel_subsample.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_batch, synthetic_mesh
from deltaconv_amd.datasets import Data
from deltaconv_amd.geometry import voxel_subsample
from deltaconv_amd.meshes import DeviceMeshDataset

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)
AXIS = 1 << 16                                # cells per axis the packed key of leg (a) has room for


def torch_first(pos, batch, b, size):
    """Leg (a) -> (rows of the representatives, unordered; cluster id per point; the largest cell index)."""
    origin = torch.zeros(b, 3, device=pos.device).scatter_reduce(0, batch[:, None].expand(-1, 3), pos, "amin", include_self=False)
    t = torch.floor((pos - origin[batch]) / size).long()          # size: a device tensor (a host scalar would become a reciprocal)
    key = ((batch * AXIS + t[:, 2]) * AXIS + t[:, 1]) * AXIS + t[:, 0]
    uniq, inv = torch.unique(key, return_inverse=True)
    rows = torch.full((uniq.numel(),), pos.shape[0], dtype=torch.int64, device=pos.device)
    rows.scatter_reduce_(0, inv, torch.arange(pos.shape[0], device=pos.device), "amin")
    return rows, inv, t.max()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[32, 8192, 8, 65536, 1, 262144], help="clouds points ...")
    ap.add_argument("--meshes", type=int, default=128, help="meshes of the vertex store; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--keep", type=float, nargs="+", default=[0.25, 0.0625], help="fractions of the points to keep")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fps-repeats", type=int, default=2, help="repeats of the descriptive geodesic row (0: leave it out)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_voxel_subsample.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    def size_for(pos, ptr, keep):
        """The edge length at which about `keep` of the points survive (bisection in log space; outside every timing)."""
        lo, hi = 1e-5, 10.0
        for _ in range(24):
            mid = (lo * hi) ** 0.5
            kept = voxel_subsample(pos, mid, ptr=ptr, pick="first")[0].numel() / pos.shape[0]
            lo, hi = (mid, hi) if kept > keep else (lo, mid)
        return (lo * hi) ** 0.5

    held = []

    def compare(what, pos, ptr):
        b, n = ptr.numel() - 1, pos.shape[0]
        batch = torch.repeat_interleave(torch.arange(b, device=dev), ptr[1:] - ptr[:-1])
        for keep in args.keep:
            size = size_for(pos, ptr, keep)
            size_dev = torch.tensor(size, dtype=torch.float32, device=dev)
            leg_a = lambda: torch_first(pos, batch, b, size_dev)
            leg_b = lambda: voxel_subsample(pos, size, ptr=ptr, pick="first")
            leg_c = lambda: voxel_subsample(pos, size, ptr=ptr)
            (ra, inv, most), (rb, _, cb), _ = leg_a(), leg_b(), leg_c()           # warm-up passes; they double as the equality check
            assert int(most) < AXIS, f"{what}: leg (a)'s packed key has no room for cell {int(most)}"
            assert torch.equal(torch.sort(ra).values, rb), f"{what}: the representatives differ"
            assert torch.equal(ra[inv], rb[cb]), f"{what}: the clusters differ"
            kept = rb.numel()
            del ra, inv, rb, cb
            times = {"a": [], "b": [], "c": []}
            for _ in range(args.repeats):
                times["a"].append(timed(leg_a))
                times["b"].append(timed(leg_b))
                times["c"].append(timed(leg_c))
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            say(f"## {what}: {n} points in {b} clouds, size {size:.5g} keeps {kept} rows = 1/{n / kept:.2f}")
            for k, name in (("a", "torch composition, first"), ("b", "voxel_subsample, pick='first'"), ("c", "voxel_subsample, pick='centre'")):
                say(f"({k}) {name}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.3f} ms")
            spread = max(times["a"]) - min(times["a"])
            ok = med["b"] <= med["a"] + spread
            held.append(ok)
            say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %")
            say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians), same rows and clusters: yes -> (b) no slower than (a) beyond (a)'s "
                f"spread: {'yes' if ok else 'NO'}")
        return size                                                              # of the last `keep`

    say(f"# voxel-grid subsampling benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass, wall clock, device "
        f"synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats")
    for b, n in zip(args.shapes[::2], args.shapes[1::2]):
        pos = synthetic_batch(b, n, seed=3, normals=False).pos.float().to(dev).contiguous()
        compare(f"{b} x {n} surface points", pos, (torch.arange(b + 1, dtype=torch.int64) * n).to(dev))
        del pos
    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0] + 0.25 * i, face=base[f][1]) for i, f in ((i, FACES[i % len(FACES)]) for i in range(args.meshes))]
    cloud = DeviceMeshDataset.from_dataset(items, dev).vertex_cloud(include_labels=False)
    size = compare(f"vertex clouds of {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces", cloud.pos, cloud.ptr)
    say(f"## the expectation held at {sum(held)} of {len(held)} rows")
    if args.fps_repeats > 0:
        alone = lambda: cloud.geodesic_subsample(1024, seed=1, large="device")
        thinned = lambda: cloud.voxel_subsample(size).geodesic_subsample(1024, seed=1, large="device")
        largest = int(cloud.voxel_subsample(size).sizes.max())
        alone(), thinned()                                                       # warm-up
        ta, tb = [], []
        for _ in range(args.fps_repeats):
            ta.append(timed(alone))
            tb.append(timed(thinned))
        say(f"## descriptive (different samples, times only): the vertex store ({int(cloud.sizes.max())} vertices in its largest cloud) "
            f"to 1 024 points a cloud")
        say("    geodesic_subsample(1024, large='device') alone: " + ", ".join(f"{t * 1e3:.1f}" for t in ta) + " ms / pass")
        say(f"    voxel_subsample({size:.5g}) (largest cloud then {largest}) + geodesic_subsample(1024, large='device'): "
            + ", ".join(f"{t * 1e3:.1f}" for t in tb) + " ms / pass")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
