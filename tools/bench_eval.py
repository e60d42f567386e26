"""Evaluation benchmark: whole test passes, each ending in a device synchronise, on synthetic test sets of the ModelNet40
shape (2 468 clouds x 1 024 points with normals, batch 32, the C2 classifier) and of the ShapeNet shape (2 874 shapes x
2 048 points, 16 categories, 50 parts, batch 16, the C4 segmentation net), both resident on the device and served by a
``DeviceLoader`` in all three forms:

  (a) the existing host form: eager eval forward per batch, then the host metrics -- ``evaluate()`` of
      examples/train_modelnet_like.py (a synchronising ``int(...)`` per batch) / examples/train_shapenet_like.py (arg-max,
      copies to the host, ``calc_shape_IoU`` per batch)
  (b) ``DeviceEvaluator(graphed=False)``: eager forward, metrics in one launch per batch, one synchronise per pass
  (c) ``DeviceEvaluator(graphed=True)``: the forward replayed from one captured graph

The three forms alternate in one process, ``--repeats`` times each after a warm-up pass each; the yardstick is form (a) of
the same run.  Needs an MI355X; there is no CPU form of any of it.

    python tools/bench_eval.py --out profiles/device_eval.txt
    python tools/bench_eval.py --sets shapenet --votes 10          # the multi-vote test of experiments/test_shapenet.py
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as dc
from deltaconv_amd.configs import build_model
from deltaconv_amd.data import synthetic_cloud
from deltaconv_amd.datasets import Data
from deltaconv_amd.evaluate import part_tables
from deltaconv_amd.utils import calc_shape_IoU, evaluate_votes

SETS = {"modelnet": dict(config="C2", clouds=2468, points=1024, batch=32, task="classification"),
        "shapenet": dict(config="C4", clouds=2874, points=2048, batch=16, task="segmentation")}


def make_items(spec, clouds, distinct):
    base = [synthetic_cloud(spec["points"], 9000 + i) for i in range(distinct)]
    start, count = part_tables()
    g = torch.Generator().manual_seed(1)
    items = []
    for i in range(clouds):
        pos, norm = base[i % distinct]
        if spec["task"] == "classification":
            items.append(Data(pos=pos, norm=norm, y=torch.tensor([i % 40])))
        else:
            k = i % 16
            cat = torch.zeros(1, 16)
            cat[0, k] = 1
            items.append(Data(pos=pos, norm=norm, category=cat,
                              y=torch.randint(start[k], start[k] + count[k], (spec["points"],), generator=g)))
    return items


@torch.no_grad()
def host_classification(model, loader):
    """evaluate() of examples/train_modelnet_like.py (without the operator cache: the loader builds new batches)."""
    model.eval()
    correct = count = 0
    for data in loader:
        correct += int((model(data).argmax(1) == data.y).sum())
        count += data.num_graphs
    return correct / count


@torch.no_grad()
def host_segmentation(model, loader):
    """evaluate() of examples/train_shapenet_like.py."""
    model.eval()
    ious = []
    for data in loader:
        pred = model(data).argmax(1).view(data.num_graphs, -1).cpu().numpy()
        true = data.y.view(data.num_graphs, -1).cpu().numpy()
        label = data.category.argmax(1).cpu().numpy()
        ious += calc_shape_IoU(pred, true, label, None)
    return float(np.mean(ious))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="modelnet,shapenet")
    ap.add_argument("--clouds", type=int, default=None, help="override the cloud count of every set (quick runs)")
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--votes", type=int, default=1, help="> 1: form (a) becomes utils.evaluate_votes (segmentation only)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_eval.py needs an MI355X: nothing here can be measured on a CPU")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# device evaluation benchmark on {torch.cuda.get_device_name(0)}: every time is one whole test pass ({args.votes} vote(s)), "
        f"wall clock, device synchronise at the end, after one warm-up pass per form; the forms alternate, {args.repeats} repeats")
    for name in filter(None, args.sets.split(",")):
        spec = SETS[name]
        clouds = args.clouds or spec["clouds"]
        seg = spec["task"] == "segmentation"
        store = dc.DeviceDataset.from_dataset(make_items(spec, clouds, args.distinct), dev)
        torch.manual_seed(1)
        model = build_model(spec["config"]).to(dev).eval()
        mk = lambda: dc.DeviceLoader(store, spec["batch"])
        nb = len(mk())
        say(f"## {name}: {clouds} clouds x {spec['points']} points, batch {spec['batch']} ({nb} batches, the last one "
            f"{'short' if clouds % spec['batch'] else 'full'}), model {spec['config']}")
        la = mk()
        if args.votes > 1 and seg:
            form_a = lambda: evaluate_votes(model, la, num_votes=args.votes)["mean_iou"]
        else:
            form_a = (lambda: host_segmentation(model, la)) if seg else (lambda: host_classification(model, la))
        key = "mean_iou" if seg else "accuracy"
        evs = {g: dc.DeviceEvaluator(model, mk(), spec["task"], num_votes=args.votes if seg else 1, graphed=g) for g in (False, True)}
        forms = [("a", "host form: eager forward + host metrics", form_a),
                 ("b", "DeviceEvaluator, eager forward", lambda: evs[False].run()[key]),
                 ("c", "DeviceEvaluator, captured forward", lambda: evs[True].run()[key])]
        times, values = {k: [] for k, _, _ in forms}, {}
        for k, _, fn in forms:
            values[k] = fn()                                 # warm-up pass
        for _ in range(args.repeats):
            for k, _, fn in forms:
                t, values[k] = timed(fn, dev)
                times[k].append(t)
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for k, what, _ in forms:
            say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.1f}" for t in times[k]) + f" ms / pass; median {med[k] * 1e3:.1f} ms = "
                f"{med[k] / nb / max(args.votes if seg else 1, 1) * 1e3:.3f} ms / batch = {clouds / med[k]:.0f} clouds/s; {key} {values[k]:.6f}")
        spread = max(times["a"]) - min(times["a"])
        say(f"    spread of (a) over its repeats (max - min): {spread * 1e3:.1f} ms = {spread / med['a'] * 100:.2f} %")
        say(f"    (a) / (b) = {med['a'] / med['b']:.3f}, (a) / (c) = {med['a'] / med['c']:.3f}, medians -> (c) no slower than (a) by more "
            f"than (a)'s spread: {'yes' if med['c'] - med['a'] <= spread else 'NO'}")
        say(f"    |{key} (c) - (a)| = {abs(values['c'] - values['a']):.3e}, |(b) - (a)| = {abs(values['b'] - values['a']):.3e}")
        del evs, store, model
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
