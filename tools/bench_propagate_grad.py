"""Differentiable propagation benchmark: per-point values of sampled clouds (1 024 points, 50 channels) interpolated to the
vertices of the meshes they were sampled from AND the gradient brought back to the sampled rows -- the synthetic meshes of
tools/bench_propagate.py (mixed face counts, 1 k .. 200 k), whole forward + backward passes on a finished search, each ending in
a device synchronise:

  (a) a torch restatement on the device: gather ``x[idx]``, the weights ``1 / clamp(d2, 1e-16)``, the weighted mean, and
      autograd's backward of the gather (an ``index_add_`` / ``index_put_(accumulate=True)`` that may use floating-point atomics:
      torch gives no run-to-run guarantee for it)
  (b) ``Propagator(sampled, meshes, k, differentiable=True).apply(x)`` and its backward: ``dc_knn_interpolate`` +
      ``dc_knn_interpolate_backward`` on the transposed lists built once (ordered sums, no atomics, the same bits every run)

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  The transposed build (once per store) is reported on its own.  Needs an MI355X.

    python tools/bench_propagate_grad.py --out profiles/device_propagate_grad.txt
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
from deltaconv_amd.geometry import knn_cross_transpose
from deltaconv_amd.meshes import DeviceMeshDataset
from deltaconv_amd.propagate import Propagator

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128, help="meshes of a pass; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--num", type=int, default=1024, help="sampled points per mesh")
    ap.add_argument("--channels", type=int, default=50)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_propagate_grad.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0], face=base[f][1]) for f in (FACES[i % len(FACES)] for i in range(args.meshes))]
    meshes = DeviceMeshDataset.from_dataset(items, dev)
    sampled = meshes.sample_points(args.num, include_normals=False, seed=1)
    gen = torch.Generator().manual_seed(1)
    verts, rows, c, k = int(meshes.n_verts.sum()), args.meshes * args.num, args.channels, args.k
    values = torch.randn(rows, c, generator=gen).to(dev)
    grad = torch.randn(verts, c, generator=gen).to(dev)
    prop = Propagator(sampled, meshes, k=k, differentiable=True)
    torch.cuda.synchronize(dev)
    tptr = prop.lists[0]
    lengths = (tptr[1:] - tptr[:-1]).cpu().numpy()
    edges = int(tptr[-1])
    say(f"# differentiable propagation benchmark on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward pass "
        f"over the set on a finished search, wall clock, device synchronise at the end, after one warm-up pass per leg; the legs "
        f"alternate, {args.repeats} repeats")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({verts} vertices in all), {args.num} sampled points each, "
        f"{c} channels, k = {k}: {edges} in-edges, per sampled row median {int(np.median(lengths))}, mean {lengths.mean():.1f}, "
        f"largest {int(lengths.max())}")
    say(f"## algorithmic bytes of the backward: {(edges * (4 * c + 12) + rows * (4 * c + 8)) / 1e6:.0f} MB (per in-edge a {4 * c}-byte "
        f"row of g, an 8-byte edge id and a 4-byte coefficient; per sampled row {4 * c} bytes of dx and an 8-byte list offset)")

    # leg (a): what the search result looks like to torch -- absolute source rows and a validity mask, prepared once
    sizes = torch.from_numpy(np.asarray(meshes.n_verts, dtype=np.int64)).to(dev)
    first = torch.repeat_interleave(prop.sptr[:-1], sizes, output_size=verts)
    ok = prop.idx >= 0
    absolute = (first[:, None] + prop.idx.clamp(min=0).long())

    def leg_a(x):
        w = torch.where(ok, 1.0 / prop.d2.clamp(min=1e-16), torch.zeros_like(prop.d2))
        out = (w[:, :, None] * x[absolute]).sum(dim=1) / w.sum(dim=1, keepdim=True)
        out.backward(grad)
        torch.cuda.synchronize(dev)
        return out

    def leg_b(x):
        out = prop.apply(x)
        out.backward(grad)
        torch.cuda.synchronize(dev)
        return out

    grads, outs = {}, {}
    for key, fn in (("a", leg_a), ("b", leg_b)):                                # the warm-up passes double as the comparison
        x = values.clone().requires_grad_(True)
        outs[key] = fn(x).detach()
        grads[key] = x.grad
    x = values.clone().requires_grad_(True)
    leg_b(x)
    same_b = bool(torch.equal(x.grad, grads["b"]))
    x = values.clone().requires_grad_(True)
    leg_a(x)
    same_a = bool(torch.equal(x.grad, grads["a"]))
    scale = float(grads["a"].abs().max())
    say(f"    largest |(b) - (a)|: forward {float((outs['b'] - outs['a']).abs().max()):.3e}, gradient "
        f"{float((grads['b'] - grads['a']).abs().max()):.3e} (largest |gradient| {scale:.3e}); a second run gives the same gradient "
        f"bits: (a) {'yes' if same_a else 'no'}, (b) {'yes' if same_b else 'NO'}")
    del outs
    times = {"a": [], "b": []}
    for _ in range(args.repeats):
        for key, fn in (("a", leg_a), ("b", leg_b)):
            x = values.clone().requires_grad_(True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(x)
            times[key].append(time.perf_counter() - t0)
    med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
    for key, what in (("a", "torch gather + weights, autograd's index_add_ backward"),
                      ("b", "Propagator(differentiable=True).apply + ordered backward")):
        say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.2f} ms")
    spread = max(times["a"]) - min(times["a"])
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    # the stages of (b) on their own, by device events
    g = grad
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    lists = knn_cross_transpose(prop.idx, prop.d2, prop.tptr, prop.sptr, num_ref=rows)
    ev[1].record()
    for _ in range(5):
        prop.apply(values)
    ev[2].record()
    from deltaconv_amd.geometry import interpolate_rows_backward
    rel = prop.cloud_range((0, len(prop)))[1]
    for _ in range(5):
        interpolate_rows_backward(g, rel, lists[0], lists[1], lists[2], k, int(prop.ssizes.max()), n_ref=rows)
    ev[3].record()
    torch.cuda.synchronize(dev)
    say(f"    (b) by device events: transposed build (once per store) {ev[0].elapsed_time(ev[1]):.3f} ms, forward "
        f"{ev[1].elapsed_time(ev[2]) / 5:.3f} ms / pass, backward {ev[2].elapsed_time(ev[3]) / 5:.3f} ms / pass (5 back to back, "
        f"allocation of the results included)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
