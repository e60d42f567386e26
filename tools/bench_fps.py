"""Geodesic farthest-point sampling benchmark: whole passes over a synthetic dataset, each ending in a device synchronise,
in the two recipes the reference prepares its data with -- ModelNet / ShapeSeg (256 clouds x 8 192 points -> 1 024 samples:
``sampling_margin = 8``) and ShapeNet (256 clouds x 2 048 points -> 2 048 samples):

  (a) the host form: ``geodesic_fps`` per cloud in a Python loop, as ``T.GeodesicFPS`` runs inside ``pre_transform`` (the
      library's kNN stage uses the OpenMP threads the machine grants, 16 here; its Dijkstra rounds are serial)
  (b) ``geodesic_fps_batch``: all clouds of the pass on the device, positions already resident (``DeviceDataset``)

The two legs alternate in one process, ``--repeats`` times each after a warm-up pass each, from the same start points; the
yardstick is leg (a) of the same run and its run-to-run spread.  The picks of both legs are compared.  Needs an MI355X.

    python tools/bench_fps.py --out profiles/device_fps.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_cloud
from deltaconv_amd.geometry import geodesic_fps, geodesic_fps_batch

SETS = {"modelnet": dict(clouds=256, points=8192, samples=1024), "shapenet": dict(clouds=256, points=2048, samples=2048)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="modelnet,shapenet")
    ap.add_argument("--clouds", type=int, default=None, help="override the cloud count of every set (quick runs)")
    ap.add_argument("--distinct", type=int, default=32, help="different surfaces generated per set (the clouds cycle through them)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fps.py needs an MI355X: leg (b) has no CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# geodesic FPS benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, device "
        f"synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats; host threads: "
        f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}")
    for name in filter(None, args.sets.split(",")):
        spec = SETS[name]
        clouds, n, m = args.clouds or spec["clouds"], spec["points"], spec["samples"]
        base = [synthetic_cloud(n, 9000 + i, normals=False)[0].numpy() for i in range(min(args.distinct, clouds))]
        host = [base[i % len(base)] for i in range(clouds)]
        pos = torch.from_numpy(np.concatenate(host)).to(dev)
        ptr = torch.arange(clouds + 1, dtype=torch.int64) * n
        say(f"## {name}: {clouds} clouds x {n} points -> {m} samples")

        def leg_a():
            return np.stack([geodesic_fps(p, m, seed=i) for i, p in enumerate(host)])

        starts = None

        def leg_b():
            out = geodesic_fps_batch(pos, ptr, m, start=starts)
            torch.cuda.synchronize(dev)
            return out

        want = leg_a()                                       # warm-up pass of (a); its start points serve (b)
        starts = want[:, 0].copy()
        got = leg_b().cpu().numpy()                          # warm-up pass of (b)
        times = {"a": [], "b": []}
        for _ in range(args.repeats):
            for k, fn in (("a", leg_a), ("b", leg_b)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, what in (("a", "host geodesic_fps loop"), ("b", "geodesic_fps_batch on the device")):
            say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.1f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.1f} ms = "
                f"{med[k] / clouds * 1e3:.3f} ms / cloud = {clouds / med[k]:.0f} clouds/s")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.1f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) faster than (a) beyond (a)'s spread: "
            f"{'yes' if med['a'] - med['b'] > spread else 'NO'}")
        same = int((got == want).all(axis=1).sum())
        say(f"    clouds whose {m} picks equal the host library's: {same} of {clouds}; samples that differ: {int((got != want).sum())}")
        del pos
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
