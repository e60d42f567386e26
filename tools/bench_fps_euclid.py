"""Euclidean farthest-point sampling benchmark: ``geometry.fps`` (csrc/fps_euclid.hip, one launch, every pick inside it) beside
the batched torch composition a user without it would write.  Surfaces from ``deltaconv_amd.data`` at 32 x 1 024 -> 256,
16 x 2 048 -> 512, 32 x 8 192 -> 1 024 and one cloud at the sampler's cap (16 384 -> 1 024); whole passes, each ending in a device
synchronise:

  (a) torch: a ``[B, n]`` minimum-distance tensor, per pick one gather of the picked rows, the distance in the contract's
      association ``(dx*dx + dy*dy) + dz*dz``, one ``minimum`` and one ``argmax``
  (b) ``geometry.fps(pos, ptr_info=..., n_samples=m)``; its rows are asserted ``torch.equal`` to (a)'s here

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  No ratio is promised.  The expectation: (b) is no slower than (a) beyond (a)'s spread.  Needs an
MI355X.

    python tools/bench_fps_euclid.py --out profiles/device_fps_euclid.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_batch
from deltaconv_amd.geometry import fps
from deltaconv_amd.geometry.fps import FPS_EUCLID_MAX_POINTS
from deltaconv_amd.geometry.graph import PtrInfo


def torch_fps(pos, b, n, m):
    """(a): pos [B*n,3] -> global rows int64 [B*m] in pick order, every cloud from its row 0."""
    p = pos.view(b, n, 3)
    cloud = torch.arange(b, device=pos.device)
    md = torch.full((b, n), float("inf"), device=pos.device)
    cur = torch.zeros(b, dtype=torch.int64, device=pos.device)
    picks = torch.empty((b, m), dtype=torch.int64, device=pos.device)
    for r in range(m):
        picks[:, r] = cur
        d = p - p[cloud, cur][:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        md = torch.minimum(md, d2)
        md[cloud, cur] = -1.0
        cur = torch.argmax(md, dim=1)
    return (picks + (cloud * n)[:, None]).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[32, 1024, 256, 16, 2048, 512, 32, 8192, 1024, 1, FPS_EUCLID_MAX_POINTS, 1024],
                    help="clouds points picks ...")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fps_euclid.py needs an MI355X: neither leg has a CPU form")
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

    say(f"# Euclidean farthest-point sampling on {torch.cuda.get_device_name(0)}: every time is one whole pass, wall clock, device "
        f"synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats")
    for b, n, m in zip(args.shapes[::3], args.shapes[1::3], args.shapes[2::3]):
        pos = synthetic_batch(b, n, seed=3, normals=False).pos.float().to(dev).contiguous()
        info = PtrInfo((torch.arange(b + 1, dtype=torch.int32) * n).to(dev), b, n, n)
        leg_a = lambda: torch_fps(pos, b, n, m)
        leg_b = lambda: fps(pos, ptr_info=info, n_samples=m)[0]
        ra, rb = leg_a(), leg_b()                                               # warm-up passes; they double as the equality check
        torch.cuda.synchronize(dev)
        assert torch.equal(ra, rb), f"{b} x {n} -> {m}: geometry.fps differs from the torch composition"
        times = {"a": [], "b": []}
        for _ in range(args.repeats):
            times["a"].append(timed(leg_a))
            times["b"].append(timed(leg_b))
        med = {key: sorted(v)[len(v) // 2] for key, v in times.items()}
        say(f"## {b} clouds of {n} points -> {m} picks each")
        for key, name in (("a", "torch composition"), ("b", "geometry.fps")):
            say(f"({key}) {name}: " + ", ".join(f"{t * 1e3:.3f}" for t in times[key]) + f" ms / pass; median {med[key] * 1e3:.3f} ms "
                f"= {med[key] / m * 1e6:.2f} us / pick")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians), same picks: yes -> (b) no slower than (a) beyond (a)'s spread: "
            f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
        del pos
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
