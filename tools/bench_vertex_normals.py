"""Vertex-normal benchmark: whole passes over a set of synthetic meshes with mixed face counts (1 k .. 200 k), each ending in a
device synchronise -- ``GenerateMeshNormals()`` of the ShapeSeg ``pre_transform`` (experiments/train_shapeseg.py:31):

  (a) the host form: ``T.GenerateMeshNormals()`` per mesh in a Python loop, as it runs inside ``pre_transform`` (torch's CPU
      threads as the machine grants them)
  (b) the list build: ``geometry.vertex_face_lists`` over the whole store (count, scan, fill, rank), the store already resident;
      the pass includes its allocations
  (c) ``DeviceMeshDataset.vertex_normals()`` on finished lists: one launch, plus the allocation of the result

The three legs alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is leg (a) of the same
run and its run-to-run spread.  No speed-up is claimed in advance: the expectation is that (b) + (c) is no slower than (a) beyond
(a)'s spread.  One thread per vertex walks its list, so a hub vertex is one thread's work.  Needs an MI355X.

    python tools/bench_vertex_normals.py --out profiles/device_vertex_normals.txt
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
from deltaconv_amd.geometry import vertex_face_lists
from deltaconv_amd.meshes import DeviceMeshDataset

FACES = (1000, 2000, 5000, 10000, 20000, 50000, 100000, 200000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", type=int, default=128, help="meshes of a pass; their face counts cycle through 1 k .. 200 k")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_vertex_normals.py needs an MI355X: legs (b) and (c) have no CPU form")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = {f: synthetic_mesh(f, 9000 + i) for i, f in enumerate(FACES)}
    items = [Data(pos=base[f][0] + 0.25 * i, face=base[f][1]) for i, f in ((i, FACES[i % len(FACES)]) for i in range(args.meshes))]
    faces, verts = sum(int(d.face.shape[1]) for d in items), sum(int(d.pos.shape[0]) for d in items)
    store = DeviceMeshDataset.from_dataset(items, dev)
    host = T.GenerateMeshNormals()
    say(f"# vertex-normal benchmark on {torch.cuda.get_device_name(0)}: every time is one whole pass over the set, wall clock, "
        f"device synchronise at the end, after one warm-up pass per leg; the legs alternate, {args.repeats} repeats; host threads: "
        f"torch.get_num_threads() = {torch.get_num_threads()}")
    say(f"## {args.meshes} meshes of {min(FACES)} .. {max(FACES)} faces ({faces} faces, {verts} vertices in all), weighting uniform")

    def leg_a():
        return [host(Data(pos=d.pos, face=d.face)).norm for d in items]

    def leg_b():
        out = vertex_face_lists(store.face, store.vptr, store.fptr, verts)
        torch.cuda.synchronize(dev)
        return out

    def leg_c():
        out = store.vertex_normals()
        torch.cuda.synchronize(dev)
        return out

    want = torch.cat(leg_a())
    store.vertex_lists = leg_b()
    zero = torch.empty(len(store), dtype=torch.int32, device=dev)
    got = store.vertex_normals(zero_count=zero)
    worst = float((got.cpu() - want).abs().max())
    times = {"a": [], "b": [], "c": []}
    for _ in range(args.repeats):
        for k, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times[k].append(time.perf_counter() - t0)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    for k, what in (("a", "host T.GenerateMeshNormals loop"), ("b", "geometry.vertex_face_lists on the device (once per store)"),
                    ("c", "DeviceMeshDataset.vertex_normals on finished lists")):
        say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.2f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.2f} ms = "
            f"{med[k] / args.meshes * 1e3:.3f} ms / mesh = {args.meshes / med[k]:.0f} meshes/s")
    spread = max(times["a"]) - min(times["a"])
    both = med["b"] + med["c"]
    say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.2f} ms = {spread / med['a'] * 100:.2f} %")
    say(f"    (a) / ((b) + (c)) = {med['a'] / both:.2f} (medians) -> (b) + (c) no slower than (a) beyond (a)'s spread: "
        f"{'yes' if both <= med['a'] + spread else 'NO'}")
    # the launch of one normals pass on its own, by events (the pass above adds the allocation and the synchronise)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    from deltaconv_amd.geometry import vertex_normals_batch
    ev[0].record()
    for _ in range(5):
        vertex_normals_batch(store.vert, store.face, store.vptr, store.fptr, store.vertex_lists, out=got)
    ev[1].record()
    torch.cuda.synchronize(dev)
    per = ev[0].elapsed_time(ev[1]) / 5
    algo = (24 + 12) * faces + (8 + 12 + 12) * verts             # list entries + ids per face; list offsets, the row, the normal per vertex
    say(f"    (c) by device events, 5 launches back to back: {per:.3f} ms / pass; algorithmic bytes {algo / 1e6:.1f} MB -> "
        f"{algo / per / 1e6:.1f} GB/s; vertices with a zero normal: {int(zero.sum())}; largest |device - host| component: {worst:.3g}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
