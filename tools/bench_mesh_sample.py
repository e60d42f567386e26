"""Surface sampling benchmark: whole passes over a set of synthetic meshes with mixed face counts (1 k .. 200 k), each ending
in a device synchronise, 8 192 points with normals per mesh as the ModelNet recipe draws them (1 024 points x
``sampling_margin = 8``):

  (a) the host form: ``T.SamplePoints(8192, include_normals=True)`` per mesh in a Python loop, as it runs inside
      ``pre_transform`` (torch's CPU threads as the machine grants them)
  (b) ``DeviceMeshDataset.sample_points(8192)``: all meshes of the pass on the device, the store already resident; the pass
      includes the one synchronise that fills ``degenerate``

The two legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same
run and its run-to-run spread.  The two legs draw different samples (other generators): what is compared is the time.  Needs an
MI355X.

    python tools/bench_mesh_sample.py --out profiles/device_mesh_sample.txt
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd.transforms as T
from deltaconv_amd.data import synthetic_mesh
from deltaconv_amd.datasets import Data
from deltaconv_amd.meshes import DeviceMeshDataset

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128, help="meshes of a pass; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--num", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mesh_sample.py needs an MI355X: leg (b) has no CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0], face=base[f][1]) for f in (FACES[i % len(FACES)] for i in range(args.meshes))]
    faces = sum(int(d.face.shape[1]) for d in items)
    store = DeviceMeshDataset.from_dataset(items, dev)
    say(f"# surface sampling benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, "
        f"device synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats; host threads: "
        f"torch.get_num_threads() = {torch.get_num_threads()}")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({faces} faces in all) -> {args.num} points with normals each")
    host = T.SamplePoints(args.num, include_normals=True)

    def leg_a():
        return [host(Data(pos=d.pos, face=d.face)) for d in items]

    def leg_b():
        out = store.sample_points(args.num, seed=1)
        torch.cuda.synchronize(dev)
        return out

    leg_a()
    got = leg_b()
    times = {"a": [], "b": []}
    for _ in range(args.repeats):
        for k, fn in (("a", leg_a), ("b", leg_b)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, what in (("a", "host T.SamplePoints loop"), ("b", "DeviceMeshDataset.sample_points on the device")):
        say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.2f} ms = "
            f"{med[k] / args.meshes * 1e3:.3f} ms / mesh = {args.meshes / med[k]:.0f} meshes/s")
    spread = max(times["a"]) - min(times["a"])
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    # the two launches of one pass on their own, by events (the pass above adds the allocations and the synchronise)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(5):
        store.sample_points(args.num, seed=1)
    ev[1].record()
    torch.cuda.synchronize(dev)
    say(f"    (b) by device events, 5 passes back to back: {ev[0].elapsed_time(ev[1]) / 5:.3f} ms / pass; "
        f"degenerate meshes: {int(got.degenerate.sum())}; points: {tuple(got.pos.shape)}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
