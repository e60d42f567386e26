"""Vector cluster pooling benchmark (csrc/cluster_vectors.hip behind ``geometry.cluster_pool_vectors`` / ``cluster_unpool_vectors``):
tangent-vector features pooled over the cells of a voxel thinning (max / sum / mean), or carried back up to the points, AND the
gradient brought back -- whole forward + backward passes on FINISHED member lists and rotation tables, each ending in a device
synchronise:

  (a) a torch composition on the device: the gather of both coefficient rows, the batched 2 x 2 products with the per-point
      rotation, ``scatter_reduce`` (amax of the squared norms, amin of the winning rows) / ``index_add_`` / a gather by
      ``cluster``, and autograd's backward (floating-point atomics: torch gives NO run-to-run guarantee for it)
  (b) ``cluster_pool_vectors(v, cluster, lists=..., rotation=..., differentiable=True)`` / ``cluster_unpool_vectors`` and their
      backwards: ``dc_cluster_pool_vectors`` + ``dc_cluster_pool_vectors_backward``, ``dc_cluster_unpool_vectors`` +
      ``dc_cluster_unpool_vectors_backward`` (ordered sums, no atomics, the same bits every run)

on 8 x 65 536 surface points thinned to about 1/16 at C = 64 and 128, and on the vertex clouds of the 128-mesh synthetic store of
tools/bench_cluster_pool.py (3.1 M vertices) at C = 64.  The two table builds (``cluster_rotation``), which run once per thinning,
are timed on their own.

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each, and the results of the two legs are
asserted close; the yardstick is leg (a) of the same run and its run-to-run spread.  No ratio is claimed in advance.  The
expectation: (b) no slower than (a) beyond (a)'s spread -- reported per row either way.  These are wall-clock windows of a few
launches, not kernel times.  Needs an MI355X.

    python tools/bench_cluster_pool_vectors.py --out profiles/device_cluster_pool_vectors.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.geometry import (cluster_lists, cluster_pool_vectors, cluster_rotation, cluster_unpool_vectors,
                                    voxel_subsample)
from tools.bench_cluster_pool import FACES, timed

KINDS = ("max", "sum", "mean", "up")


def frames_of(normal):
    """(normal, x, y) of unit normals: the x-axis across a fixed direction, as build_tangent_basis picks it."""
    n = torch.nn.functional.normalize(normal, dim=1)
    t = torch.zeros_like(n)
    alt = n[:, 0].abs() > 0.9
    t[:, 0], t[:, 1] = (~alt).float(), alt.float()
    x = torch.nn.functional.normalize(torch.linalg.cross(t, n), dim=1)
    return n.contiguous(), x.contiguous(), torch.nn.functional.normalize(torch.linalg.cross(n, x), dim=1).contiguous()


def interleave(u, w):
    return torch.stack([u, w], 1).reshape(2 * u.shape[0], u.shape[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--points", type=int, default=65536)
    ap.add_argument("--keep", type=float, default=0.0625, help="fraction of the points a thinning keeps")
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--meshes", type=int, default=128, help="meshes of the vertex store (0: leave it out)")
    ap.add_argument("--mesh-channels", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cluster_pool_vectors.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines, held = [], []

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

    def compare(what, pos, normal, ptr, channels):
        n = pos.shape[0]
        size = size_for(pos, ptr, args.keep)
        rows, _, cluster = voxel_subsample(pos, size, ptr=ptr)
        m = rows.numel()
        assert int(cluster.min()) >= 0
        fine = frames_of(normal)
        coarse = tuple(t[rows].contiguous() for t in fine)
        lists = cluster_lists(cluster, m)
        build = {d: (lambda d=d: cluster_rotation(cluster, m, fine, coarse, d)) for d in ("down", "up")}
        table = {d: build[d]() for d in build}
        lengths = (lists[0][1:] - lists[0][:-1]).float()
        count = lengths[:, None]
        say(f"## {what}: {n} points, size {size:.5g} keeps {m} cells = 1/{n / m:.2f}; members per cell mean {float(lengths.mean()):.2f}, "
            f"largest {int(lengths.max())}")
        for d in build:
            tl = [timed(build[d], dev) for _ in range(args.repeats)]
            say(f"    cluster_rotation({d!r}) (once per thinning): " + ", ".join(f"{t * 1e3:.3f}" for t in tl)
                + f" ms; median {sorted(tl)[len(tl) // 2] * 1e3:.3f} ms")
        gen = torch.Generator().manual_seed(1)
        every = torch.arange(n, device=dev)[:, None]
        for c in channels:
            index = cluster[:, None].expand(-1, c)
            data = {"down": (torch.randn(2 * n, c, generator=gen).to(dev), torch.randn(2 * m, c, generator=gen).to(dev))}
            data["up"] = (data["down"][1], data["down"][0])
            for kind in KINDS:
                values, grad = data["up" if kind == "up" else "down"]
                r = table["up" if kind == "up" else "down"]
                r00, r01, r10, r11 = (r[:, i, None] for i in range(4))

                def leg_a(v):
                    if kind == "up":
                        x0, x1 = v[0::2][cluster], v[1::2][cluster]
                        out = interleave(r00 * x0 + r01 * x1, r10 * x0 + r11 * x1)
                    else:
                        v0, v1 = v[0::2], v[1::2]
                        tu, tv = r00 * v0 + r01 * v1, r10 * v0 + r11 * v1
                        if kind == "max":
                            with torch.no_grad():
                                key = v0 * v0 + v1 * v1
                                top = torch.zeros(m, c, device=dev).scatter_reduce(0, index, key, "amax", include_self=False)
                                arg = torch.full((m, c), n, device=dev).scatter_reduce(0, index, torch.where(key == top[cluster], every, n),
                                                                                       "amin", include_self=False)
                            out = interleave(tu.gather(0, arg), tv.gather(0, arg))
                        else:
                            ou = torch.zeros(m, c, device=dev).index_add_(0, cluster, tu)
                            ov = torch.zeros(m, c, device=dev).index_add_(0, cluster, tv)
                            out = interleave(ou / count, ov / count) if kind == "mean" else interleave(ou, ov)
                    out.backward(grad)
                    torch.cuda.synchronize(dev)
                    return out

                def leg_b(v):
                    if kind == "up":
                        out = cluster_unpool_vectors(v, cluster, lists=lists, rotation=r, differentiable=True)
                    else:
                        out = cluster_pool_vectors(v, cluster, num_clusters=m, reduce=kind, lists=lists, rotation=r, differentiable=True)
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
                # sums differ by the order of the additions alone: a few units of 2^-24 of a sum of about `largest` terms of size 1.
                # A maximum may fall on another member where two squared norms agree to the last bit or two (torch is free to
                # contract v0*v0 + v1*v1): such entries are counted, and at most one in 10^5 may differ
                off = [float(((p - q).abs() > 1e-4 + 1e-4 * q.abs()).float().mean()) for p, q in ((outs["b"], outs["a"]), (grads["b"], grads["a"]))]
                assert max(off) <= (1e-5 if kind == "max" else 0.0), (kind, c, off)
                del outs, grads
                times = {"a": [], "b": []}
                for _ in range(args.repeats):
                    for key, fn in (("a", leg_a), ("b", leg_b)):
                        x = values.clone().requires_grad_(True)
                        torch.cuda.synchronize(dev)
                        t0 = time.perf_counter()
                        fn(x)
                        times[key].append(time.perf_counter() - t0)
                med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
                spread = max(times["a"]) - min(times["a"])
                ok = med["b"] <= med["a"] + spread
                held.append(ok)
                name = "un-pooling (up)" if kind == "up" else f"pooling (down), reduce = {kind}"
                say(f"### C = {c}, {name}: largest |(b) - (a)| forward {dfwd:.3e}, gradient {dbwd:.3e} (asserted close; entries apart: "
                    f"{off[0]:.1e}, {off[1]:.1e}); a second run gives "
                    f"the same bits: (a) {'yes' if same['a'] else 'no'}, (b) {'yes' if same['b'] else 'NO'}")
                for key, label in (("a", "torch composition + autograd"), ("b", "cluster_*_vectors + its backward")):
                    say(f"({key}) {label}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.3f} ms")
                say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %; (a) / (b) = "
                    f"{med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: {'yes' if ok else 'NO'}")
            del data, index

    say(f"# vector cluster pooling benchmark on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward pass on "
        f"finished member lists and rotation tables, wall clock (a window of a few launches, not a kernel time), device synchronise at "
        f"the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats.  Leg (a) uses floating-point atomics and "
        f"has no reproducibility guarantee")
    from deltaconv_amd.data import synthetic_batch
    b, n = args.clouds, args.points
    batch = synthetic_batch(b, n, seed=3, normals=True)
    compare(f"{b} x {n} surface points", batch.pos.float().to(dev).contiguous(), batch.norm.float().to(dev),
            (torch.arange(b + 1, dtype=torch.int64) * n).to(dev), args.channels)
    del batch
    if args.meshes > 0:
        from deltaconv_amd.data import synthetic_mesh
        from deltaconv_amd.datasets import Data
        from deltaconv_amd.meshes import DeviceMeshDataset
        base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
        items = [Data(pos=base[f][0] + 0.25 * i, face=base[f][1]) for i, f in ((i, FACES[i % len(FACES)]) for i in range(args.meshes))]
        cloud = DeviceMeshDataset.from_dataset(items, dev).vertex_cloud(include_normals=False, include_labels=False)
        # a smooth unit field stands in for the normals: the times do not depend on the frames' values
        compare(f"vertex clouds of {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces", cloud.pos, cloud.pos + 1e-3, cloud.ptr,
                [args.mesh_channels])
    say(f"## the expectation held at {sum(held)} of {len(held)} rows")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
