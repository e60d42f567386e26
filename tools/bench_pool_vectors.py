"""Cross-cloud pooling of tangent-vector features: vectors of full clouds pooled down to sampled ones AND the gradient brought
back to the full rows -- 32 clouds of 8 192 points down to 1 024 each (every 8th point), k = 16, C = 64 and 128, ``reduce="max"``;
whole forward + backward passes on a finished search and rotation table, each ending in a device synchronise:

  (a) a torch composition on the device: the gather of both coefficient rows (``[Nq, k, C]`` intermediates), the batched 2 x 2
      products with the table, the squared norm, ``argmax`` over the slots, ``take_along_dim``, and autograd's backward of all of it
  (b) ``CloudPair.down_vectors(v, "max")`` and its backward: ``dc_knn_pool_vectors`` + ``dc_knn_pool_vectors_backward`` on the
      transposed lists built once (ordered sums, no atomics, the same bits every run)

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  No speed-up is claimed in advance: the expectation is "(b) no slower than (a) beyond (a)'s spread".
Needs an MI355X.

    python tools/bench_pool_vectors.py --out profiles/device_pool_vectors.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.geometry import CloudPair, build_tangent_basis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=8192, help="points of a full cloud")
    ap.add_argument("--num", type=int, default=1024, help="points of a sampled cloud (every points/num-th point)")
    ap.add_argument("--channels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pool_vectors.py needs an MI355X: neither leg has a CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    b, n, m, k = args.clouds, args.points, args.num, args.k
    gen = torch.Generator().manual_seed(1)
    normal = torch.nn.functional.normalize(torch.randn(b * n, 3, generator=gen), dim=1).to(dev)
    pos = (normal * (1 + 0.1 * torch.rand(b * n, 1, generator=gen).to(dev))).contiguous()
    frames = (normal,) + tuple(build_tangent_basis(normal))
    pick = (torch.arange(b)[:, None] * n + torch.arange(0, n, n // m)[None, :m]).reshape(-1).to(dev)
    fptr = (torch.arange(b + 1, dtype=torch.int64) * n).to(dev)
    cptr = (torch.arange(b + 1, dtype=torch.int64) * m).to(dev)
    pair = CloudPair(pos, pos[pick].contiguous(), fptr, cptr, k_down=k, frames_fine=frames,
                     frames_coarse=tuple(t[pick].contiguous() for t in frames), max_fine_cloud=n, max_coarse_cloud=m)
    pair.prepare(vector_pool=True)
    idx, tptr, rmat = pair.search("down")[0], pair.lists("down")[0], pair.rotation("down")
    torch.cuda.synchronize(dev)
    lengths = (tptr[1:] - tptr[:-1]).float()
    say(f"# transported pooling of vector features on {torch.cuda.get_device_name(0)}: every time is one whole forward + backward "
        f"pass on a finished search and table, wall clock, device synchronise at the end, after one warm-up pass per leg; the legs "
        f"alternate, {args.repeats} repeats; reduce = max")
    say(f"## {b} clouds of {n} points down to {m}, k = {k}: {int(tptr[-1])} in-edges, per full-cloud row mean {float(lengths.mean()):.2f}, "
        f"largest {int(lengths.max())}, rows without one {int((lengths == 0).sum())}")
    assert bool((idx >= 0).all())
    ids = (fptr[:-1].repeat_interleave(m)[:, None] + idx.long())                # absolute source rows, prepared once
    R = rmat.view(b * m, k, 2, 2)

    def leg_a(v, grad):
        w = torch.stack([v[0::2][ids], v[1::2][ids]], 2)                         # [Nq, k, 2, C]
        at = (w * w).sum(2).argmax(1, keepdim=True)                              # [Nq, 1, C]
        moved = torch.matmul(R, w)                                               # [Nq, k, 2, C]
        out = torch.take_along_dim(moved, at[:, :, None, :], 1)[:, 0].reshape(2 * b * m, -1)
        out.backward(grad)
        torch.cuda.synchronize(dev)
        return out

    def leg_b(v, grad):
        out = pair.down_vectors(v, "max")
        out.backward(grad)
        torch.cuda.synchronize(dev)
        return out

    for c in args.channels:
        values = torch.randn(2 * b * n, c, generator=gen).to(dev)
        grad = torch.randn(2 * b * m, c, generator=gen).to(dev)
        say(f"## C = {c}")
        grads, outs = {}, {}
        for key, fn in (("a", leg_a), ("b", leg_b)):                            # the warm-up passes double as the comparison
            x = values.clone().requires_grad_(True)
            outs[key] = fn(x, grad).detach()
            grads[key] = x.grad
        same = {}
        for key, fn in (("a", leg_a), ("b", leg_b)):
            x = values.clone().requires_grad_(True)
            fn(x, grad)
            same[key] = bool(torch.equal(x.grad, grads[key]))
        say(f"    largest |(b) - (a)|: forward {float((outs['b'] - outs['a']).abs().max()):.3e}, gradient "
            f"{float((grads['b'] - grads['a']).abs().max()):.3e} (largest |gradient| {float(grads['a'].abs().max()):.3e}); a second "
            f"run gives the same gradient bits: (a) {'yes' if same['a'] else 'no'}, (b) {'yes' if same['b'] else 'NO'}")
        del outs, grads
        times = {"a": [], "b": []}
        for _ in range(args.repeats):
            for key, fn in (("a", leg_a), ("b", leg_b)):
                x = values.clone().requires_grad_(True)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn(x, grad)
                times[key].append(time.perf_counter() - t0)
        med = {key: sorted(t)[len(t) // 2] for key, t in times.items()}
        for key, what in (("a", "torch gather + 2 x 2 products + argmax + take_along_dim, autograd's backward"),
                          ("b", "CloudPair.down_vectors(v, 'max') + ordered backward")):
            say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.3f} ms")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
            f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
