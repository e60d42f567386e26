"""Propagation benchmark: per-point values of sampled clouds (1 024 points, 50 channels) interpolated back to the vertices of the
meshes they were sampled from -- a set of synthetic meshes with mixed face counts (1 k .. 200 k), whole passes, each ending in a
device synchronise:

  (a) the host form a user without PyG writes: per cloud ``scipy.spatial.cKDTree(samples).query(vertices, k)`` and the
      inverse-squared-distance weights in numpy, in a Python loop (inputs and result in host memory)
  (b) ``Propagator(sampled, meshes, k)`` -- the search over the whole set -- plus ``apply(values)``: stores and values resident on
      the device, the result left there

The two legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same
run and its run-to-run spread.  Needs an MI355X.

    python tools/bench_propagate.py --out profiles/device_propagate.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_mesh
from deltaconv_amd.datasets import Data
from deltaconv_amd.meshes import DeviceMeshDataset
from deltaconv_amd.propagate import Propagator

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128, help="meshes of a pass; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--num", type=int, default=1024, help="sampled points per mesh")
    ap.add_argument("--channels", type=int, default=50)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_propagate.py needs an MI355X: leg (b) has no CPU form")
    from scipy.spatial import cKDTree
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0], face=base[f][1]) for f in (FACES[i % len(FACES)] for i in range(args.meshes))]
    meshes = DeviceMeshDataset.from_dataset(items, dev)
    sampled = meshes.sample_points(args.num, include_normals=False, seed=1)
    values = torch.randn(args.meshes * args.num, args.channels, generator=torch.Generator().manual_seed(1)).to(dev)
    verts = int(meshes.n_verts.sum())
    say(f"# propagation benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, device "
        f"synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({verts} vertices in all), {args.num} sampled points each, "
        f"{args.channels} channels, k = {args.k}: {verts * args.num / 1e9:.2f} G distance evaluations, "
        f"{verts * (4 * args.channels * (args.k + 1) + 8 * args.k) / 1e6:.0f} MB of algorithmic interpolation traffic")
    # host copies for leg (a): what a host pipeline holds
    voff = np.concatenate([[0], np.cumsum(meshes.n_verts)])
    h_vert, h_pos, h_val = meshes.vert.cpu().numpy(), sampled.pos.cpu().numpy(), values.cpu().numpy()

    def leg_a():
        out = np.empty((verts, args.channels), dtype=np.float32)
        for c in range(args.meshes):
            src = h_pos[c * args.num:(c + 1) * args.num]
            dist, idx = cKDTree(src).query(h_vert[voff[c]:voff[c + 1]], k=args.k)
            dist, idx = dist.reshape(-1, args.k), idx.reshape(-1, args.k)
            w = (1.0 / np.maximum(dist * dist, 1e-16)).astype(np.float32)
            x = h_val[c * args.num:(c + 1) * args.num][idx]                      # [V, k, C]
            out[voff[c]:voff[c + 1]] = (w[:, :, None] * x).sum(axis=1) / w.sum(axis=1, keepdims=True)
        return out

    def leg_b():
        out = Propagator(sampled, meshes, k=args.k).apply(values)
        torch.cuda.synchronize(dev)
        return out

    want = leg_a()
    got = leg_b()
    err = float(np.abs(got.cpu().numpy() - want).max())
    times = {"a": [], "b": []}
    for _ in range(args.repeats):
        for key, fn in (("a", leg_a), ("b", leg_b)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[key].append(time.perf_counter() - t0)
    med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
    for key, what in (("a", "host cKDTree + numpy loop"), ("b", "Propagator(...) + apply on the device")):
        say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.2f} ms = "
            f"{med[key] / args.meshes * 1e3:.3f} ms / mesh")
    spread = max(times["a"]) - min(times["a"])
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    say(f"    largest |(b) - (a)| over the {verts} x {args.channels} results: {err:.3e} (fp32 against fp64 distances)")
    # the two stages of (b) on their own, by device events
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    prop = Propagator(sampled, meshes, k=args.k)
    ev[1].record()
    for _ in range(5):
        prop.apply(values)
    ev[2].record()
    torch.cuda.synchronize(dev)
    say(f"    (b) by device events: search {ev[0].elapsed_time(ev[1]):.3f} ms, interpolation {ev[1].elapsed_time(ev[2]) / 5:.3f} ms / pass "
        f"(5 back to back, allocation of the {verts * args.channels * 4 / 1e6:.0f} MB result included)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
