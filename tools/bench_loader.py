"""Input-pipeline benchmark: the host DataLoader paths against the device-resident loader (deltaconv_amd/loader.py), on a
ModelNet40-shaped dataset -- 9 840 clouds x 1024 points with normals from ``synthetic_cloud`` (a few hundred distinct clouds,
repeated), batch 32, the ModelNet recipe RandomScale((4/5, 5/4)) + RandomTranslateGlobal(0.1).  Every figure is the wall time
of a whole epoch that ends in a device synchronise, after a warm-up epoch:

  (a) datasets.DataLoader with the per-shape transforms + ``.to(device)``           (the shipped path)
  (b) datasets.DataLoader without transforms + ``.to(device)`` + the per-batch device form of the two transforms
  (c) DeviceLoader iteration alone                                                 (one launch per batch)
  (d) a GraphedTrainStep epoch fed by ``loader.into(step.static)``
  (e) the same step fed batches already resident on the device through ``load()``  (the best case without the loader)

(d) and (e) alternate in one process, ``--repeats`` times each.  Needs an MI355X; there is no CPU form of any of it.

    python tools/bench_loader.py --out profiles/device_loader.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_loader.py --only c      # the assembly kernel's own time
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as dc
import deltaconv_amd.transforms as T
from deltaconv_amd.configs import build_model, build_optimizer
from deltaconv_amd.data import synthetic_cloud
from deltaconv_amd.datasets import Compose, Data, DataLoader
from deltaconv_amd.graph_step import GraphedTrainStep
from deltaconv_amd.utils import calc_loss


class ListDataset(torch.utils.data.Dataset):
    """``items`` + ``transform`` on a copy at every access, as the dataset classes of deltaconv_amd.datasets do."""

    def __init__(self, items, transform=None):
        self.items, self.transform = items, transform

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        data = self.items[i].clone()
        return data if self.transform is None else self.transform(data)


def recipe():
    return Compose((T.RandomScale((4 / 5, 5 / 4)), T.RandomTranslateGlobal(0.1)))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=9840)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="abcde", help="which of the legs a..e to run")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_loader.py needs an MI355X: nothing here can be measured on a CPU")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = [synthetic_cloud(args.points, 5000 + i) for i in range(args.distinct)]
    items = [Data(pos=base[i % args.distinct][0], norm=base[i % args.distinct][1], y=torch.tensor([i % 40]))
             for i in range(args.clouds)]
    nb = args.clouds // args.batch
    say(f"# device loader benchmark: {args.clouds} clouds x {args.points} points with normals ({args.distinct} distinct), batch "
        f"{args.batch}, {nb} batches per epoch (drop_last), recipe RandomScale((4/5, 5/4)) + RandomTranslateGlobal(0.1)")
    say(f"# device: {torch.cuda.get_device_name(0)}; every time: one whole epoch, wall clock, device synchronise at the end, "
        "after one warm-up epoch")
    res = {}

    def report(key, what, secs):
        res[key] = secs
        say(f"({key}) {what}: {secs * 1e3:9.1f} ms / epoch = {secs / nb * 1e6:8.1f} us / batch = {nb * args.batch / secs:10.0f} clouds/s")

    if "a" in args.only:
        loader = DataLoader(ListDataset(items, recipe()), batch_size=args.batch, shuffle=True, drop_last=True)
        epoch = lambda: [b.to(dev) for b in loader][-1]
        epoch()
        report("a", "DataLoader, per-shape transforms, .to(device)", timed(epoch, dev))
    if "b" in args.only:
        loader = DataLoader(ListDataset(items), batch_size=args.batch, shuffle=True, drop_last=True)
        aug = recipe()
        epoch = lambda: [aug(b.to(dev)) for b in loader][-1]
        epoch()
        report("b", "DataLoader, collate, .to(device), per-batch device transforms", timed(epoch, dev))

    store = dc.DeviceDataset.from_dataset(items, dev)
    dl = dc.DeviceLoader(store, args.batch, shuffle=True, drop_last=True, transform=recipe(), seed=1)
    if "c" in args.only:
        def epoch():
            for b in dl:
                pass
        epoch()
        report("c", "DeviceLoader iteration alone (one launch per batch)", timed(epoch, dev))
        if "a" in res:
            say(f"    (a) / (c) = {res['a'] / res['c']:.1f}")

    if "d" in args.only or "e" in args.only:
        torch.manual_seed(1)
        model = build_model("C2").to(dev).train()
        opt = build_optimizer("C2", model.parameters())
        step = GraphedTrainStep(model, calc_loss, dl.static_batch(), optimizer=opt)
        dl.set_epoch(0)
        resident = [b for b in dl]                       # (e): the epoch's batches, built beforehand, resident on the device

        def epoch_d():
            for _ in dl.into(step.static):
                step()

        def epoch_e():
            for b in resident:
                step(b)
        epoch_d()
        epoch_e()
        td, te = [], []
        for _ in range(args.repeats):                    # alternating, one process
            td.append(timed(epoch_d, dev))
            te.append(timed(epoch_e, dev))
        for key, what, ts in (("d", "GraphedTrainStep fed by loader.into(step.static)", td),
                              ("e", "GraphedTrainStep fed resident batches through load()", te)):
            say(f"({key}) {what}: " + ", ".join(f"{t * 1e3:.1f}" for t in ts) + f" ms / epoch; median {sorted(ts)[len(ts) // 2] * 1e3:.1f} ms "
                f"= {sorted(ts)[len(ts) // 2] / nb * 1e3:.4f} ms / step")
        md, me = sorted(td)[len(td) // 2], sorted(te)[len(te) // 2]
        spread = max(te) - min(te)
        say(f"    spread of (e) over its repeats (max - min): {spread * 1e3:.1f} ms = {spread / me * 100:.2f} %")
        say(f"    (d) - (e), medians: {(md - me) * 1e3:+.1f} ms / epoch = {(md - me) / nb * 1e6:+.2f} us / step "
            f"-> (d) no slower than (e) by more than (e)'s spread: {'yes' if md - me <= spread else 'NO'}")
        say(f"    final loss {float(step.loss):.4f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
