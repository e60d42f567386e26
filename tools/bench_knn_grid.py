"""k-nearest-neighbour search benchmark: where the brute-force graph starts to dominate, and what the exact grid search
(csrc/knn_grid.hip) does about it.  Surfaces from ``deltaconv_amd.data``, k = 20, at 32 x 1 024, 8 x 16 384, 4 x 65 536 and
1 x 262 144 points; whole searches, each ending in a device synchronise:

  (a) ``Graph.knn(method="brute")``: ``dc_knn``, n^2 distances per cloud (above 4 096 points the sorted-insertion kernel)
  (b) ``Graph.knn(method="grid")``: ``dc_knn_grid``, seven launches; its table is asserted ``torch.equal`` to (a)'s here

and a cross leg, 8 x 65 536 points searched from 8 x 16 384 sampled ones (every 4th point), k = 16: ``knn_cross`` with
``method="brute"`` against ``method="grid"``, ``idx`` and the bits of ``d2`` asserted equal.

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  Leg (a) is code this search does not touch, so it stands for the library without it.  No speed-up is
claimed in advance.  The expectation: at 65 536 points a cloud and above (b) is no slower than (a) beyond (a)'s spread; at
1 024 points the build's launches may well lose -- reported either way.  ``--targets`` times (b) at several mean points per cell
on every shape; the library's default is whichever does best at 65 536 points.  Needs an MI355X.

    python tools/bench_knn_grid.py --out profiles/device_knn_grid.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_batch
from deltaconv_amd.geometry import Graph, knn_cross
from deltaconv_amd.geometry.graph import GRID_TARGET, PtrInfo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[32, 1024, 8, 16384, 4, 65536, 1, 262144], help="clouds points ...")
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--cross", type=int, nargs=3, default=[8, 65536, 16384], help="clouds, reference points, query points")
    ap.add_argument("--cross-k", type=int, default=16)
    ap.add_argument("--targets", type=float, nargs="+", default=[0.5, 1.0, 2.0, 4.0, 8.0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_knn_grid.py needs an MI355X: neither leg has a CPU form")
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

    def compare(what, leg_a, leg_b, same, sweep):
        """Warm-up passes (they double as the equality check), alternating repeats, the report; then the target sweep of (b)."""
        ra, rb = leg_a(), leg_b(None)
        torch.cuda.synchronize(dev)
        assert same(ra, rb), f"{what}: the grid search differs from brute force"
        del ra, rb
        times = {"a": [], "b": []}
        for _ in range(args.repeats):
            times["a"].append(timed(leg_a))
            times["b"].append(timed(lambda: leg_b(None)))
        med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
        for key, name in (("a", "brute force"), ("b", f"grid, target {GRID_TARGET:g}")):
            say(f"({key}) {name}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / search; median {med[key] * 1e3:.3f} ms")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians), same table: yes -> (b) no slower than (a) beyond (a)'s spread: "
            f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
        for target in sweep:
            leg_b(target)                                                       # warm-up
            ts = sorted(timed(lambda: leg_b(target)) for _ in range(args.repeats))
            say(f"    (b) at target {target:g}: median {ts[len(ts) // 2] * 1e3:.3f} ms (min {ts[0] * 1e3:.3f}, max {ts[-1] * 1e3:.3f})")
        return med

    say(f"# k-NN search benchmark on {torch.cuda.get_device_name(0)}: every time is one whole search, wall clock, device synchronise "
        f"at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats")
    wins = []
    for b, n in zip(args.shapes[::2], args.shapes[1::2]):
        pos = synthetic_batch(b, n, seed=3, normals=False).pos.float().to(dev)
        info = PtrInfo((torch.arange(b + 1, dtype=torch.int32) * n).to(dev), b, n, n)
        say(f"## graph: {b} clouds of {n} points, k = {args.k}: brute force evaluates {b * n * n:.3e} distances")
        med = compare(f"{b} x {n}", lambda: Graph.knn(pos, args.k, ptr_info=info, method="brute").nbr,
                      lambda t: Graph.knn(pos, args.k, ptr_info=info, method="grid", grid_target=t).nbr, torch.equal, args.targets)
        if med["b"] < med["a"]:
            wins.append(n)
        del pos
    say(f"## the smallest measured cloud size at which (b)'s median beats (a)'s: {min(wins) if wins else 'none'} points "
        f"(a measurement of these shapes, not a policy)")
    b, n, m = args.cross
    ref = synthetic_batch(b, n, seed=4, normals=False).pos.float().to(dev)
    qry = ref.view(b, n, 3)[:, ::n // m][:, :m].reshape(b * m, 3).contiguous()
    rptr, qptr = (torch.arange(b + 1, dtype=torch.int64) * n).to(dev), (torch.arange(b + 1, dtype=torch.int64) * m).to(dev)
    say(f"## cross: {b} clouds of {m} queries into {n} reference points, k = {args.cross_k}: brute force evaluates {b * n * m:.3e} distances")
    kw = dict(ptr_query=qptr, ptr_ref=rptr, max_query_cloud=m)
    compare("cross", lambda: knn_cross(qry, ref, args.cross_k, method="brute", **kw),
            lambda t: knn_cross(qry, ref, args.cross_k, method="grid", grid_target=t, **kw),
            lambda x, y: torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32)), args.targets)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
