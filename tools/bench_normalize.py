"""Normalisation benchmark: whole passes over a set of synthetic meshes with mixed face counts (1 k .. 200 k), each ending in a
device synchronise, the ShapeSeg chain ``NormalizeArea`` + ``NormalizeAxes`` (experiments/train_shapeseg.py:28-30):

  (a) the host form: ``T.NormalizeArea()`` then ``T.NormalizeAxes()`` per mesh in a Python loop, as it runs inside
      ``pre_transform`` (torch's CPU threads as the machine grants them); faces as ``[F,3]``, the layout in which the host class
      computes the surface area
  (b) ``DeviceMeshDataset.normalize([T.NormalizeArea(), T.NormalizeAxes()])``: all meshes of the pass on the device, the store
      already resident; the pass includes the clone of the vertex rows and the one synchronise that fills ``degenerate``

The two legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same
run and its run-to-run spread.  No speed-up is claimed in advance: the expectation is that (b) is no slower than (a) beyond
(a)'s spread.  One workgroup per mesh builds the parameters, so a 200 k-face mesh is one workgroup's work.  Needs an MI355X.

    python tools/bench_normalize.py --out profiles/device_normalize.txt
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
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_normalize.py needs an MI355X: leg (b) has no CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stretch = torch.tensor([1.0, 0.55, 1.7])                     # distinct deviations per axis, as in the tests
    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0] * stretch + 0.25 * i, face=base[f][1]) for i, f in
             ((i, FACES[i % len(FACES)]) for i in range(args.meshes))]
    faces, verts = sum(int(d.face.shape[1]) for d in items), sum(int(d.pos.shape[0]) for d in items)
    rows = [d.face.t().contiguous() for d in items]              # [F,3] for the host class
    store = DeviceMeshDataset.from_dataset(items, dev)
    chain = [T.NormalizeArea(), T.NormalizeAxes()]
    say(f"# normalisation benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, "
        f"device synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats; host threads: "
        f"torch.get_num_threads() = {torch.get_num_threads()}")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({faces} faces, {verts} vertices in all), chain "
        "NormalizeArea + NormalizeAxes")

    def leg_a():
        return [chain[1](chain[0](Data(pos=d.pos, face=f))) for d, f in zip(items, rows)]

    def leg_b():
        out = store.normalize(chain)
        torch.cuda.synchronize(dev)
        return out

    want = leg_a()
    got = leg_b()
    worst = max(float((got.vert[int(store.vptr[i]):int(store.vptr[i + 1])].cpu() - w.pos).abs().max()) for i, w in enumerate(want))
    times = {"a": [], "b": []}
    for _ in range(args.repeats):
        for k, fn in (("a", leg_a), ("b", leg_b)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, what in (("a", "host T.NormalizeArea + T.NormalizeAxes loop"), ("b", "DeviceMeshDataset.normalize on the device")):
        say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.2f} ms = "
            f"{med[k] / args.meshes * 1e3:.3f} ms / mesh = {args.meshes / med[k]:.0f} meshes/s")
    spread = max(times["a"]) - min(times["a"])
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / (b) = {med['a'] / med['b']:.2f} (medians) -> (b) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if med['b'] <= med['a'] + spread else 'NO'}")
    # the two launches of one pass on their own, by events (the pass above adds the clone, the allocations and the synchronise)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    scratch = store.normalize(chain)
    ev[0].record()
    for _ in range(5):
        store.normalize(chain, out=scratch)                      # from the raw store into the same rows: no clone
    ev[1].record()
    torch.cuda.synchronize(dev)
    per = ev[0].elapsed_time(ev[1]) / 5
    algo = 3 * 12 * verts + 12 * faces + 3 * 12 * faces + 2 * 12 * verts     # three row passes, ids + three gathered rows, read + write
    say(f"    (b) by device events, 5 passes back to back (each with its synchronise): {per:.3f} ms / pass; algorithmic bytes "
        f"{algo / 1e6:.1f} MB -> {algo / per / 1e6:.1f} GB/s; degenerate meshes: {int(got.degenerate.sum())}; "
        f"largest |device - host| coordinate: {worst:.3g}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
