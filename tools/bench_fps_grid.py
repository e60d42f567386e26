"""Farthest-point sampling on a cell grid: ``geometry.fps(method="grid")`` (csrc/fps_grid.hip, exact, clouds up to 262 144 points)
beside the register kernel ``method="brute"`` (csrc/fps_euclid.hip) where the cloud fits its cap of 16 384.  Surfaces from
``deltaconv_amd.data`` at 32 x 1 024 -> 256, 32 x 8 192 -> 1 024, 1 x 16 384 -> 4 096, 8 x 65 536 -> 1 024 and -> 16 384,
1 x 262 144 -> 1 024 and -> 65 536; whole calls, each ending in a device synchronise:

  (a) ``fps(method="brute")``: one launch (no leg above 16 384 points: it raises there)
  (b) ``fps(method="grid", stats=True)``: the grid build, the workspace allocation and the sampling launch, all inside the window;
      its rows are asserted ``torch.equal`` to (a)'s here where (a) exists

The legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same run
and its run-to-run spread.  No speed-up is promised: at small clouds (b) is expected to lose (six launches against one, a pick
of a few barriers against one).  Then targets 0.5, 1, 2, 4, 8 at 8 x 65 536 -> 16 384; the default ``grid_target`` is the best
median there.  Needs an MI355X.

    python tools/bench_fps_grid.py --out profiles/device_fps_grid.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_batch
from deltaconv_amd.geometry import fps
from deltaconv_amd.geometry.fps import FPS_EUCLID_MAX_POINTS, FPS_GRID_MAX_POINTS, FPS_GRID_TARGET
from deltaconv_amd.geometry.graph import PtrInfo

SHAPES = [32, 1024, 256, 32, 8192, 1024, 1, 16384, 4096, 8, 65536, 1024, 8, 65536, 16384, 1, FPS_GRID_MAX_POINTS, 1024,
          1, FPS_GRID_MAX_POINTS, 65536]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=SHAPES, help="clouds points picks ...")
    ap.add_argument("--targets", type=float, nargs="*", default=[0.5, 1.0, 2.0, 4.0, 8.0], help="grid targets tried at --target-shape")
    ap.add_argument("--target-shape", type=int, nargs=3, default=[8, 65536, 16384], help="clouds points picks of the target sweep")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fps_grid.py needs an MI355X: neither leg has a CPU form")
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

    def cloud(b, n):
        pos = synthetic_batch(b, n, seed=3, normals=False).pos.float().to(dev).contiguous()
        return pos, PtrInfo((torch.arange(b + 1, dtype=torch.int32) * n).to(dev), b, n, n)

    median = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: ", ".join(f"{t * 1e3:.3f}" for t in v)
    say(f"# farthest-point sampling on a cell grid on {torch.cuda.get_device_name(0)}: every time is one whole call, wall clock, "
        f"device synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats; "
        f"default grid_target = {FPS_GRID_TARGET}")
    for b, n, m in zip(args.shapes[::3], args.shapes[1::3], args.shapes[2::3]):
        pos, info = cloud(b, n)
        has_a = n <= FPS_EUCLID_MAX_POINTS
        leg_a = lambda: fps(pos, ptr_info=info, n_samples=m, method="brute")[0]
        leg_b = lambda: fps(pos, ptr_info=info, n_samples=m, method="grid", stats=True)
        rb, _, stats = leg_b()                                                  # warm-up passes; they double as the equality check
        if has_a:
            assert torch.equal(leg_a(), rb), f"{b} x {n} -> {m}: the grid sampler differs from the register kernel"
        torch.cuda.synchronize(dev)
        times = {"a": [], "b": []}
        for _ in range(args.repeats):
            if has_a:
                times["a"].append(timed(leg_a))
            times["b"].append(timed(leg_b))
        say(f"## {b} clouds of {n} points -> {m} picks each")
        if has_a:
            say(f"(a) method=brute: {fmt(times['a'])} ms / call; median {median(times['a']) * 1e3:.3f} ms = "
                f"{median(times['a']) / m * 1e6:.2f} us / pick")
        else:
            say(f"(a) method=brute: no leg (above its cap of {FPS_EUCLID_MAX_POINTS} points)")
        mb = median(times["b"])
        per_pick = float(stats[:, 0].double().mean()) / max(m - 1, 1)
        say(f"(b) method=grid:  {fmt(times['b'])} ms / call; median {mb * 1e3:.3f} ms = {mb / m * 1e6:.2f} us / pick; "
            f"points updated a pick {per_pick:.0f} of {n} ({per_pick / n * 100:.2f} %), cells a pick "
            f"{float(stats[:, 1].double().mean()) / max(m - 1, 1):.0f}")
        if has_a:
            ma, spread = median(times["a"]), max(times["a"]) - min(times["a"])
            say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.3f} ms = {spread / ma * 100:.2f} %")
            say(f"    (a) / (b) = {ma / mb:.2f} (medians), same picks: yes -> (b) no slower than (a) beyond (a)'s spread: "
                f"{'yes' if mb <= ma + spread else 'NO'}")
        del pos
    if args.targets:
        b, n, m = args.target_shape
        pos, info = cloud(b, n)
        say(f"## grid_target at {b} clouds of {n} points -> {m} picks each")
        want, best = None, None
        for t in args.targets:
            leg = lambda: fps(pos, ptr_info=info, n_samples=m, method="grid", grid_target=t, stats=True)
            rows, _, stats = leg()
            want = rows if want is None else want
            assert torch.equal(rows, want), f"grid_target = {t} changed a pick"
            ts = [timed(leg) for _ in range(args.repeats)]
            say(f"target {t:g}: {fmt(ts)} ms / call; median {median(ts) * 1e3:.3f} ms; points updated a pick "
                f"{float(stats[:, 0].double().mean()) / max(m - 1, 1):.0f}")
            best = (median(ts), t) if best is None or median(ts) < best[0] else best
        say(f"    best median: target {best[1]:g} ({best[0] * 1e3:.3f} ms); the default is {FPS_GRID_TARGET:g}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
