"""Geodesic farthest-point sampling of clouds above the LDS kernel's cap of 16 384 points: whole passes over a synthetic set,
each ending in a device synchronise.

Leg pair 1, host against device, on ``65k`` (8 clouds x 65 536 points -> 1 024 samples) and ``262k`` (4 clouds x 262 144 -> 1 024):
  (a) the host form: ``geodesic_fps`` per cloud in a Python loop (what ``geodesic_subsample(large="host")`` runs after a download;
      the library's kNN stage uses the OpenMP threads the machine grants, capped at 16 here; its Dijkstra rounds are serial)
  (b) ``geodesic_fps_batch(..., large=True)``: all clouds of the pass on the device, positions already resident
Leg pair 2, the cost of keeping the distance vector in global memory, on ``cap`` (32 clouds x 16 384 -> 1 024), a size both
kernels take:
  (c) the LDS kernel (``dc_geodesic_fps_batch``)        (d) the global-memory kernel (``dc_geodesic_fps_large``)
The ratio of pair 2 decides nothing: the LDS kernel keeps every cloud it can hold.

The legs of a pair alternate in one process, ``--repeats`` times each after a warm-up pass each, from the same start points; the
yardstick of pair 1 is leg (a) of the same run and its run-to-run spread.  The picks of both legs are compared.  Needs an MI355X.

    python tools/bench_fps_large.py --out profiles/device_fps_large.txt
"""
import argparse
import os
import sys
import time

os.environ["OMP_NUM_THREADS"] = str(min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))     # leg (a): 16 threads, never more

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deltaconv_amd.data import synthetic_cloud
from deltaconv_amd.geometry import geodesic_fps, geodesic_fps_batch
from deltaconv_amd.geometry.fps import _fps_device

SETS = {"65k": dict(clouds=8, points=65536, samples=1024), "262k": dict(clouds=4, points=262144, samples=1024),
        "cap": dict(clouds=32, points=16384, samples=1024)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="65k,262k,cap")
    ap.add_argument("--clouds", type=int, default=None, help="override the cloud count of every set (quick runs)")
    ap.add_argument("--samples", type=int, default=None, help="override the sample count of every set (quick runs)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fps_large.py needs an MI355X: the device legs have no CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                         # rewritten as the run goes: a pass of leg (a) takes minutes
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    say(f"# geodesic FPS of large clouds on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, "
        f"device synchronise at the end, after one warm-up pass per leg; the legs of a pair alternate, {args.repeats} repeats; host "
        f"threads: OMP_NUM_THREADS={os.environ['OMP_NUM_THREADS']}")
    for name in filter(None, args.sets.split(",")):
        spec = SETS[name]
        clouds, n, m = args.clouds or spec["clouds"], spec["points"], args.samples or spec["samples"]
        host = [synthetic_cloud(n, 9100 + i, normals=False)[0].numpy() for i in range(clouds)]
        pos = torch.from_numpy(np.concatenate(host)).to(dev)
        ptr = np.arange(clouds + 1, dtype=np.int64) * n
        say(f"## {name}: {clouds} clouds x {n} points -> {m} samples")
        starts = None
        if name == "cap":
            starts = np.array([(7919 * i) % n for i in range(clouds)], dtype=np.int32)
            legs = (("c", "LDS kernel (dc_geodesic_fps_batch)", lambda: _fps_device(pos, ptr, m, starts)),
                    ("d", "global-memory kernel (dc_geodesic_fps_large)", lambda: _fps_device(pos, ptr, m, starts, large=True)))
        else:
            legs = (("a", "host geodesic_fps loop", lambda: np.stack([geodesic_fps(p, m, seed=i) for i, p in enumerate(host)])),
                    ("b", "geodesic_fps_batch(large=True) on the device",
                     lambda: geodesic_fps_batch(pos, torch.from_numpy(ptr), m, start=starts, large=True)))
        (ka, what_a, leg_a), (kb, what_b, leg_b) = legs
        want = leg_a()                                       # warm-up pass of the first leg; on pair 1 its start points serve (b)
        if starts is None:
            starts = want[:, 0].copy()
        got = leg_b()                                        # warm-up pass of the second leg
        torch.cuda.synchronize(dev)
        want, got = (v.cpu().numpy() if torch.is_tensor(v) else v for v in (want, got))
        times = {ka: [], kb: []}
        for _ in range(args.repeats):
            for k, fn in ((ka, leg_a), (kb, leg_b)):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                times[k].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, what in ((ka, what_a), (kb, what_b)):
            say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.1f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.1f} ms = "
                f"{med[k] / clouds * 1e3:.3f} ms / cloud")
        spread = max(times[ka]) - min(times[ka])
        say(f"    spread of ({ka}) over its repeats (max - min): {spread * 1e3:.1f} ms = {spread / med[ka] * 100:.2f} %")
        if name == "cap":
            say(f"    (d) / (c) = {med[kb] / med[ka]:.2f} (medians): the cost of the distance vector in global memory at the cap")
        else:
            say(f"    (a) / (b) = {med[ka] / med[kb]:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
                f"{'yes' if med[kb] - med[ka] <= spread else 'NO'}")
        same = int((got == want).all(axis=1).sum())
        say(f"    clouds whose {m} picks equal the {'LDS kernel' if name == 'cap' else 'host library'}'s: {same} of {clouds}; "
            f"samples that differ: {int((got != want).sum())}")
        del pos
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
