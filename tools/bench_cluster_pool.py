"""Cluster pooling benchmark (csrc/cluster.hip behind ``geometry.cluster_pool``): per-point features pooled over the cells of a
voxel thinning AND the gradient brought back to the points -- whole forward + backward passes on FINISHED member lists, each ending
in a device synchronise:

  (a) ``torch.zeros(M, C).scatter_reduce(0, cluster, x, "amax" | "sum" | "mean", include_self=False)`` and autograd's backward, on
      the device (floating-point atomics: torch gives NO run-to-run guarantee for it)
  (b) ``cluster_pool(x, cluster, M, reduce, lists=lists, differentiable=True)`` and its backward: ``dc_cluster_pool`` +
      ``dc_cluster_pool_backward`` (ordered sums, no atomics, the same bits every run)

on 8 x 65 536 surface points thinned to about 1/16 at C = 64 and 128, and on the vertex clouds of the 128-mesh synthetic store of
tools/bench_voxel_subsample.py (3.1 M vertices) at C = 64.  The list build (``cluster_lists``), which runs once per thinning and
serves every pooling over it, is timed on its own.

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run and
its run-to-run spread.  No ratio is claimed in advance.  The expectation: (b) no slower than (a) beyond (a)'s spread -- reported per
row either way.  These are wall-clock windows of a few launches, not kernel times.  The largest |(b) - (a)| is reported, not
asserted: sums differ by the order of the additions, and a max gradient differs wherever two members of a cell tie in a channel
(torch splits the gradient between them, (b) sends it to the lower row).

One descriptive row: 65 536 rows in a SINGLE cell (the quadratic ranking pass of the list build and the serial walk of the
pooling), run in a child process under a time limit of its own.  Sized from the code: the ranking is 65 536 threads of 65 536
cached 8-byte compares each (4.3e9 in all: well under a second), the walk 16 threads of 16 384 groups of four loads in flight (a
few microseconds a group: well under a second), times a warm-up and ``--repeats`` passes, plus starting a process and loading the
library: 120 s.  Needs an MI355X.

    python tools/bench_cluster_pool.py --out profiles/device_cluster_pool.txt
"""
import argparse
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.geometry import cluster_lists, cluster_pool, voxel_subsample

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)
TORCH_NAME = {"max": "amax", "sum": "sum", "mean": "mean"}
SINGLE_CELL_LIMIT = 120                       # seconds; see the module docstring


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def single_cell(rows, channels, repeats):
    """The descriptive row, in this (child) process: prints one line."""
    dev = torch.device("cuda", 0)
    cluster = torch.zeros(rows, dtype=torch.int64, device=dev)
    x = torch.randn(rows, channels, device=dev)
    build = lambda: cluster_lists(cluster, 1)
    lists = build()
    pool = lambda: cluster_pool(x, cluster, 1, "max", lists=lists)
    pool()
    tb = [timed(build, dev) for _ in range(repeats)]
    tp = [timed(pool, dev) for _ in range(repeats)]
    assert torch.equal(lists[1], torch.arange(rows, device=dev)) and torch.equal(pool()[0], x.amax(0))
    print(f"## descriptive: {rows} rows in ONE cell, C = {channels} (quadratic ranking, serial walk): cluster_lists "
          + ", ".join(f"{t * 1e3:.2f}" for t in tb) + " ms; cluster_pool (max, forward only) " + ", ".join(f"{t * 1e3:.2f}" for t in tp)
          + " ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--keep", type=float, default=0.0625, help="fraction of the points a thinning keeps")
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--meshes", type=int, default=128, help="meshes of the vertex store (0: leave it out)")
    ap.add_argument("--mesh-channels", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--single-cell", type=int, default=65536, help="rows of the descriptive single-cell row (0: leave it out)")
    ap.add_argument("--single-cell-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cluster_pool.py needs an MI355X: neither leg has a CPU form")
    if args.single_cell_child:
        return single_cell(args.single_cell, args.channels[0], args.repeats)
    dev = torch.device("cuda", 0)
    lines, held, worst = [], [], 0.0

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def size_for(pos, ptr, keep):
        """The edge length at which about `keep` of the points survive (bisection in log space; outside every timing)."""
        lo, hi = 1e-5, 10.0
        for _ in range(24):
            mid = (lo * hi) ** 0.5
            kept = voxel_subsample(pos, mid, ptr=ptr)[0].numel() / pos.shape[0]
            lo, hi = (mid, hi) if kept > keep else (lo, mid)
        return (lo * hi) ** 0.5

    def compare(what, pos, ptr, channels):
        nonlocal worst
        n = pos.shape[0]
        size = size_for(pos, ptr, args.keep)
        rows, _, cluster = voxel_subsample(pos, size, ptr=ptr)
        m = rows.numel()
        assert int(cluster.min()) >= 0
        build = lambda: cluster_lists(cluster, m)
        lists = build()
        tl = [timed(build, dev) for _ in range(args.repeats)]
        lengths = (lists[0][1:] - lists[0][:-1]).float()
        say(f"## {what}: {n} points, size {size:.5g} keeps {m} cells = 1/{n / m:.2f}; members per cell mean {float(lengths.mean()):.2f}, "
            f"largest {int(lengths.max())}")
        say("    cluster_lists (once per thinning): " + ", ".join(f"{t * 1e3:.3f}" for t in tl) + f" ms; median {sorted(tl)[len(tl) // 2] * 1e3:.3f} ms")
        gen = torch.Generator().manual_seed(1)
        for c in channels:
            values = torch.randn(n, c, generator=gen).to(dev)
            grad = torch.randn(m, c, generator=gen).to(dev)
            index = cluster[:, None].expand(-1, c)
            for reduce in ("max", "sum", "mean"):
                def leg_a(x):
                    out = torch.zeros(m, c, device=dev).scatter_reduce(0, index, x, TORCH_NAME[reduce], include_self=False)
                    out.backward(grad)
                    torch.cuda.synchronize(dev)
                    return out

                def leg_b(x):
                    out = cluster_pool(x, cluster, m, reduce, lists=lists, differentiable=True)
                    out.backward(grad)
                    torch.cuda.synchronize(dev)
                    return out

                outs, grads, same = {}, {}, {}
                for key, fn in (("a", leg_a), ("b", leg_b)):                    # the warm-up passes double as the comparison
                    x = values.clone().requires_grad_(True)
                    outs[key], grads[key] = fn(x).detach(), x.grad
                for key, fn in (("a", leg_a), ("b", leg_b)):
                    x = values.clone().requires_grad_(True)
                    again = fn(x).detach()
                    same[key] = bool(torch.equal(again, outs[key]) and torch.equal(x.grad, grads[key]))
                dfwd, dbwd = float((outs["b"] - outs["a"]).abs().max()), float((grads["b"] - grads["a"]).abs().max())
                worst = max(worst, dfwd, dbwd)
                del outs, grads
                times = {"a": [], "b": []}
                for _ in range(args.repeats):
                    for key, fn in (("a", leg_a), ("b", leg_b)):
                        x = values.clone().requires_grad_(True)
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        fn(x)
                        times[key].append(time.perf_counter() - t0)
                med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
                spread = max(times["a"]) - min(times["a"])
                ok = med["b"] <= med["a"] + spread
                held.append(ok)
                say(f"### C = {c}, reduce = {reduce}: largest |(b) - (a)| forward {dfwd:.3e}, gradient {dbwd:.3e}; a second run gives the "
                    f"same bits: (a) {'yes' if same['a'] else 'no'}, (b) {'yes' if same['b'] else 'NO'}")
                for key, name in (("a", f"scatter_reduce({TORCH_NAME[reduce]}) + autograd"), ("b", "cluster_pool + gather backward")):
                    say(f"({key}) {name}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.3f} ms")
                say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %; (a) / (b) = "
                    f"{med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: {'yes' if ok else 'NO'}")
            del values, grad, index

    say(f"# cluster pooling benchmark on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward pass on finished "
        f"member lists, wall clock, device synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} "
        f"repeats.  Leg (a) uses floating-point atomics and has no reproducibility guarantee")
    from deltaconv_amd.data import synthetic_batch
    b, n = args.clouds, args.points
    pos = synthetic_batch(b, n, seed=3, normals=False).pos.float().to(dev).contiguous()
    compare(f"{b} x {n} surface points", pos, (torch.arange(b + 1, dtype=torch.int64) * n).to(dev), args.channels)
    del pos
    if args.meshes > 0:
        from deltaconv_amd.data import synthetic_mesh
        from deltaconv_amd.datasets import Data
        from deltaconv_amd.meshes import DeviceMeshDataset
        base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
        items = [Data(pos=base[f][0] + 0.25 * i, face=base[f][1]) for i, f in ((i, FACES[i % len(FACES)]) for i in range(args.meshes))]
        cloud = DeviceMeshDataset.from_dataset(items, dev).vertex_cloud(include_labels=False)
        compare(f"vertex clouds of {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces", cloud.pos, cloud.ptr, [args.mesh_channels])
    say(f"## the expectation held at {sum(held)} of {len(held)} rows; largest |(b) - (a)| over all rows {worst:.3e}")
    if args.single_cell > 0:
        cmd = [sys.executable, os.path.abspath(__file__), "--single-cell-child", "--single-cell", str(args.single_cell), "--channels",
               str(args.channels[0]), "--repeats", str(min(args.repeats, 3))]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=SINGLE_CELL_LIMIT)
            say(res.stdout.strip() if res.returncode == 0 else f"## descriptive single-cell row failed (exit {res.returncode}): {res.stderr.strip()[-400:]}")
        except subprocess.TimeoutExpired:
            say(f"## descriptive single-cell row: not finished inside {SINGLE_CELL_LIMIT} s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
