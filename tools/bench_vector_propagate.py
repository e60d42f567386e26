"""Vector-stream propagation benchmark: tangent-vector features of sampled clouds (1 024 points, 64 channels, two rows a point)
interpolated to the vertices of the meshes they were sampled from -- every neighbour's vector carried into the vertex's frame by
parallel transport -- AND the gradient brought back to the sampled rows.  The synthetic meshes of tools/bench_propagate.py (mixed
face counts, 1 k .. 200 k), whole forward + backward passes on a finished search and a finished table, each ending in a device
synchronise:

  (a) a torch composition on the device: the connection of every slot from the existing ``build_transport`` on expanded pairs and
      the weights ``1 / clamp(d2, 1e-16)``, both ONCE outside the timed window; inside it the gather of the rows, the weighted
      2 x 2 products, the sum over k, and autograd's backward of the gather (an ``index_add_`` that may use floating-point atomics:
      torch gives no run-to-run guarantee for it)
  (b) ``Propagator(sampled, meshes, k, differentiable=True, frames="normals").apply_vectors(v)`` and its backward:
      ``dc_knn_interpolate_vectors`` + ``dc_knn_interpolate_vectors_backward`` on the table and the transposed lists built once
      (ordered sums, no atomics, the same bits every run)

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  The table build (once per store) is reported on its own, by device events.  Needs an MI355X.

    python tools/bench_vector_propagate.py --out profiles/device_vector_propagate.txt
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
from deltaconv_amd.geometry import build_tangent_basis, build_transport, knn_cross_transport
from deltaconv_amd.meshes import DeviceMeshDataset
from deltaconv_amd.propagate import Propagator

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128, help="meshes of a pass; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--num", type=int, default=1024, help="sampled points per mesh")
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_vector_propagate.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0], face=base[f][1]) for f in (FACES[i % len(FACES)] for i in range(args.meshes))]
    meshes = DeviceMeshDataset.from_dataset(items, dev)
    sampled = meshes.sample_points(args.num, include_normals=True, seed=1)
    gen = torch.Generator().manual_seed(1)
    verts, rows, c, k = int(meshes.n_verts.sum()), args.meshes * args.num, args.channels, args.k
    values = torch.randn(2 * rows, c, generator=gen).to(dev)
    grad = torch.randn(2 * verts, c, generator=gen).to(dev)
    vn = meshes.vertex_normals()
    tframes = (vn,) + tuple(build_tangent_basis(vn))
    sframes = (sampled.norm,) + tuple(build_tangent_basis(sampled.norm))
    prop = Propagator(sampled, meshes, k=k, differentiable=True, frames=(sframes, tframes))
    torch.cuda.synchronize(dev)
    tptr = prop.lists[0]
    lengths = (tptr[1:] - tptr[:-1]).cpu().numpy()
    edges = int(tptr[-1])
    say(f"# vector-stream propagation benchmark on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward pass "
        f"over the set on a finished search and table, wall clock, device synchronise at the end, after one warm-up pass per leg; "
        f"the legs alternate, {args.repeats} repeats")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({verts} vertices in all), {args.num} sampled points each, "
        f"{c} channels (two rows a point), k = {k}: {edges} in-edges, per sampled point median {int(np.median(lengths))}, mean "
        f"{lengths.mean():.1f}, largest {int(lengths.max())}")
    say(f"## algorithmic bytes: table build {verts * (8 * k + 36 + 24 * k + 16 * k) / 1e6:.0f} MB (per vertex {8 * k} B of idx / d2, "
        f"36 B of its frame, {24 * k} B of gathered source frames, {16 * k} B written); forward "
        f"{verts * (k * (16 + 8 * c) + 8 * c) / 1e6:.0f} MB (per vertex k x (16 + {8 * c}) B read, {8 * c} B written); backward "
        f"{(edges * (8 * c + 24) + rows * (8 * c + 8)) / 1e6:.0f} MB (per in-edge two {4 * c}-byte rows of g, a 16-byte matrix and an "
        f"8-byte edge id; per sampled point {8 * c} B of dv and an 8-byte list offset)")

    # leg (a): what the search result looks like to torch -- absolute source rows, the connection of every slot from the existing
    # build_transport on expanded pairs and the normalised weights, prepared once outside the timed window
    sizes = torch.from_numpy(np.asarray(meshes.n_verts, dtype=np.int64)).to(dev)
    first = torch.repeat_interleave(prop.sptr[:-1], sizes, output_size=verts)
    ok = prop.idx >= 0
    absolute = first[:, None] + prop.idx.clamp(min=0).long()
    tgt = torch.arange(verts, device=dev)[:, None].expand(verts, k).reshape(-1)
    src = absolute.reshape(-1)
    conn = build_transport(tframes[0][tgt], tframes[1][tgt], tframes[2][tgt], sframes[0][src], sframes[1][src]).view(verts, k, 2, 2)
    w = torch.where(ok, 1.0 / prop.d2.clamp(min=1e-16), torch.zeros_like(prop.d2))
    w = w / w.sum(dim=1, keepdim=True)
    del tgt, src
    torch.cuda.synchronize(dev)

    def leg_a(x):
        pair = x.view(rows, 2, c)[absolute]                                     # [verts, k, 2, C]
        out = (w[:, :, None, None] * torch.matmul(conn, pair)).sum(dim=1).reshape(2 * verts, c)
        out.backward(grad)
        torch.cuda.synchronize(dev)
        return out

    def leg_b(x):
        out = prop.apply_vectors(x)
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
    for key, what in (("a", "torch gather + weighted 2 x 2 products, autograd's index_add_ backward"),
                      ("b", "Propagator(differentiable=True, frames=...).apply_vectors + ordered backward")):
        say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.2f} ms")
    spread = max(times["a"]) - min(times["a"])
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    # the table build (once per store) on its own, by device events
    mq = int(np.asarray(meshes.n_verts).max())
    knn_cross_transport(prop.idx, prop.d2, prop.tptr, prop.sptr, tframes, sframes, max_query_cloud=mq)      # warm
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    tmat = knn_cross_transport(prop.idx, prop.d2, prop.tptr, prop.sptr, tframes, sframes, max_query_cloud=mq)
    ev[1].record()
    torch.cuda.synchronize(dev)
    say(f"    (b) table build (once per store) by device events: {ev[0].elapsed_time(ev[1]):.3f} ms for {verts * k} slots (the zero "
        f"fill of the {tmat.numel() * 4 / 1e6:.0f} MB table included); the same bits as the propagator's: "
        f"{'yes' if torch.equal(tmat, prop.tmat) else 'NO'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
