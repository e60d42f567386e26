"""Transported vector sum benchmark: the mean over the k neighbours of every point of their tangent vectors brought into the
point's frame, AND the gradient with respect to the vectors -- 32 clouds of 1 024 points, k = 20, 64 and 128 channels, whole
forward + backward passes on a finished graph and connection, each ending in a device synchronise:

  (a) a torch composition on the device: gather the neighbours' rows ``v[nbr]``, multiply by the 2 x 2 blocks, sum over k, and
      autograd's backward of the gather (an ``index_add_`` / ``index_put_(accumulate=True)`` that may use floating-point atomics:
      torch gives no run-to-run guarantee for it)
  (b) ``transport_sum(v, connection, graph, reduce="mean")`` and its backward: ``dc_transport_sum`` + ``dc_transport_sum_backward``
      over the graph's CSC (ordered sums, no atomics, the same bits every run)

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  One more line compares ``build_graph_transport`` (one launch, no expansion) with the same connection
composed in torch on the expanded ``[E,3]`` rows.  Needs an MI355X.

    python tools/bench_transport.py --out profiles/device_transport.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.geometry import Graph, build_graph_transport, build_tangent_basis, transport_sum


def torch_transport(tn, tx, ty, sn, sx, non_oriented=True):
    """the connection composed from torch operators on expanded rows (the formulas of DESIGN.md 3.4i; trig through atan2)"""
    dot = lambda a, b: (a * b).sum(dim=1, keepdim=True)
    unit = lambda a: a / torch.linalg.norm(a, dim=1, keepdim=True).clamp(1e-8)
    inverted = dot(sn, tn) < 0
    tn, ty = torch.where(inverted, -tn, tn), torch.where(inverted, -ty, ty)
    axis = torch.linalg.cross(tn, sn)
    an = torch.linalg.norm(axis, dim=1, keepdim=True)
    axis = torch.where(an > 1e-6, axis / an, sx)
    up = unit(sn - dot(sn, axis) * axis)
    by = unit(torch.linalg.cross(axis, up))
    angle = torch.atan2(dot(tn, by), dot(tn, up))
    par = axis * dot(sx, axis)
    tc = sx - par
    tl = torch.linalg.norm(tc, dim=1, keepdim=True).clamp(1e-8)
    bx = tc / tl
    rot = tl * (torch.cos(angle) * bx + torch.sin(angle) * torch.linalg.cross(axis, bx)) + par
    ab = torch.cat([dot(rot, tx), dot(rot, ty)], dim=1)
    l = torch.linalg.norm(ab, dim=1, keepdim=True)
    ab = torch.where(l > 1e-6, ab / l, torch.tensor([1.0, 0.0], device=ab.device))
    conj = torch.where(inverted[:, 0] & non_oriented, -1.0, 1.0)
    return torch.stack([ab[:, 0], -ab[:, 1], ab[:, 1] * conj, ab[:, 0] * conj], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_transport.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gen = torch.Generator().manual_seed(1)
    n, k = args.clouds * args.points, args.k
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=1)
    pos = (nrm * (1 + 0.1 * torch.rand(n, 1, generator=gen))).to(dev)          # bumpy spheres, outward normals
    nrm = nrm.to(dev)
    batch = torch.arange(args.clouds, device=dev).repeat_interleave(args.points)
    graph = Graph.knn(pos, k, batch)
    xb, yb = build_tangent_basis(nrm)
    conn = build_graph_transport(nrm, xb, yb, graph)
    graph.csc()
    torch.cuda.synchronize(dev)
    e = n * k
    say(f"# transported vector sum benchmark on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward pass on a "
        f"finished graph and connection, wall clock, device synchronise at the end, after one warm-up pass per leg; the legs "
        f"alternate, {args.repeats} repeats")
    say(f"## {args.clouds} clouds of {args.points} points, k = {k}: {e} edges")
    nbr = graph.nbr.long()
    blocks = conn.view(n, k, 2, 2)

    for c in args.channels:
        values = torch.randn(2 * n, c, generator=gen).to(dev)
        grad = torch.randn(2 * n, c, generator=gen).to(dev)
        say(f"## C = {c}: algorithmic bytes of a pass, forward and backward each: {(20 * e + 16 * c * n) / 1e6:.0f} MB (per edge a 16-byte "
            f"connection and a 4-byte id; per point {8 * c} bytes of vectors in and {8 * c} out)")

        def leg_a(x):
            out = (blocks[:, :, :, :, None] * x.view(n, 2, c)[nbr][:, :, None, :, :]).sum(dim=(1, 3)).reshape(2 * n, c) / k
            out.backward(grad)
            torch.cuda.synchronize(dev)
            return out

        def leg_b(x):
            out = transport_sum(x, conn, graph, reduce="mean")
            out.backward(grad)
            torch.cuda.synchronize(dev)
            return out

        grads, outs = {}, {}
        for key, fn in (("a", leg_a), ("b", leg_b)):                            # the warm-up passes double as the comparison
            x = values.clone().requires_grad_(True)
            outs[key] = fn(x).detach()
            grads[key] = x.grad
        same = {}
        for key, fn in (("b", leg_b), ("a", leg_a)):
            x = values.clone().requires_grad_(True)
            fn(x)
            same[key] = bool(torch.equal(x.grad, grads[key]))
        say(f"    largest |(b) - (a)|: forward {float((outs['b'] - outs['a']).abs().max()):.3e}, gradient "
            f"{float((grads['b'] - grads['a']).abs().max()):.3e} (largest |gradient| {float(grads['a'].abs().max()):.3e}); a second run "
            f"gives the same gradient bits: (a) {'yes' if same['a'] else 'no'}, (b) {'yes' if same['b'] else 'NO'}")
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
        for key, what in (("a", "torch gather, 2 x 2 products, sum over k, autograd's index_add_ backward"),
                          ("b", "transport_sum + ordered backward")):
            say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.3f} ms")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
            f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")

    # the connection itself: one launch on the graph against the torch composition of the expanded call
    row, col = graph.edge_index

    def expanded():
        return torch_transport(nrm[row], xb[row], yb[row], nrm[col], xb[col])

    def one_launch():
        return build_graph_transport(nrm, xb, yb, graph)

    ref, got = expanded(), one_launch()
    torch.cuda.synchronize(dev)
    times = {"torch": [], "hip": []}
    for _ in range(args.repeats):
        for key, fn in (("torch", expanded), ("hip", one_launch)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[key].append(time.perf_counter() - t0)
    med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
    say(f"## build_graph_transport, {e} edges: torch composition on expanded rows {med['torch'] * 1e3:.3f} ms, one launch "
        f"{med['hip'] * 1e3:.3f} ms (medians of {args.repeats}, spread of the torch leg "
        f"{(max(times['torch']) - min(times['torch'])) * 1e3:.3f} ms); largest difference {float((got - ref).abs().max()):.3e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
