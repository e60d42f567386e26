"""Training-epoch benchmark: whole epochs, each ending in a device synchronise, on a synthetic ModelNet40-shaped store
(2 048 clouds x 1 024 points with normals from ``synthetic_cloud``, batch 32, the ModelNet recipe RandomScale((4/5, 5/4)) +
RandomTranslateGlobal(0.1), the C2 classifier, SGD), resident on the device and served by a ``DeviceLoader`` in three forms:

  (a) the eager loop of examples/train_modelnet_like.py (``train_epoch``): ~124 launches per step through Python, autograd and
      ctypes, ``float(loss)`` and the arg-max count read back on every step
  (b) a bare ``GraphedTrainStep`` fed by ``loader.into(step.static)``: no loss trace, no metrics
  (c) ``DeviceTrainer.run_epoch``: (b) + one 4-byte copy and one ``dc_eval_metrics`` launch per step, one synchronise and the
      host reduction at the end

Each form has its own model, optimizer and loader from the same seeds.  The forms alternate in one process, ``--repeats`` times
each after a warm-up epoch each; reported are the median and the run-to-run spread (max - min) of every form, (a) / (c) and
(c) / (b), and whether (c) - (b) lies inside (b)'s own spread.  A last, untimed-as-a-whole epoch of (c) clocks the host side of
its four calls per step (assembly, replay, loss copy, metric launch: enqueue times, no synchronise) -- where (c) - (b) comes
from when it exceeds the spread.  Needs an MI355X; there is no CPU form of any of it.

    python tools/bench_train_epoch.py --out profiles/device_train.txt
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/bench_train_epoch.py --forms c    # then, for the
    python tools/step_timeline.py <dir> batch_assemble_kernel                        # device's view of one step of (c) (or b)
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
from deltaconv_amd.datasets import Data
from deltaconv_amd.dp import FlatGradDataParallel
from deltaconv_amd.graph_step import GraphedTrainStep
from deltaconv_amd.utils import calc_loss


def train_epoch(ddp, opt, loader):
    """train_epoch() of examples/train_modelnet_like.py."""
    ddp.module.train()
    total, correct, count = 0.0, 0, 0
    for data in loader:
        ddp.zero_grad()
        out = ddp(data)
        loss = calc_loss(out, data.y)
        loss.backward()
        ddp.reduce_gradients()
        opt.step()
        total += float(loss) * data.num_graphs
        correct += int((out.argmax(1) == data.y).sum())
        count += data.num_graphs
    return total / count, correct / count


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=2048)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--forms", default="abc", help="which of the forms a, b, c to run (one alone: for a kernel trace of it)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("tools/bench_train_epoch.py: at least five repeats (the spread of a form is part of the result)")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_train_epoch.py needs an MI355X: nothing here can be measured on a CPU")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    base = [synthetic_cloud(args.points, 5000 + i) for i in range(args.distinct)]
    items = [Data(pos=base[i % args.distinct][0], norm=base[i % args.distinct][1], y=torch.tensor([i % 40])) for i in range(args.clouds)]
    store = dc.DeviceDataset.from_dataset(items, dev)
    nb = args.clouds // args.batch
    say(f"# training-epoch benchmark on {torch.cuda.get_device_name(0)}: {args.clouds} clouds x {args.points} points with normals "
        f"({args.distinct} distinct), batch {args.batch}, {nb} steps per epoch (shuffle, drop_last), recipe RandomScale((4/5, 5/4)) + "
        "RandomTranslateGlobal(0.1), model C2, SGD(0.1, momentum 0.9, wd 1e-4)")
    say(f"# every time: one whole epoch, wall clock, device synchronise at the end, after one warm-up epoch per form; the forms "
        f"alternate in one process, {args.repeats} repeats")

    def parts():
        torch.manual_seed(1)
        model = build_model("C2").to(dev).train()
        loader = dc.DeviceLoader(store, args.batch, shuffle=True, drop_last=True,
                                 transform=[T.RandomScale((4 / 5, 5 / 4)), T.RandomTranslateGlobal(0.1)], seed=1)
        return model, build_optimizer("C2", model.parameters()), loader

    if "a" in args.forms:
        model_a, opt_a, loader_a = parts()
        ddp = FlatGradDataParallel(model_a)
    if "b" in args.forms:
        model_b, opt_b, loader_b = parts()
        step = GraphedTrainStep(model_b, calc_loss, loader_b.static_batch(), optimizer=opt_b)
    if "c" in args.forms:
        model_c, opt_c, loader_c = parts()
        trainer = dc.DeviceTrainer(model_c, loader_c, opt_c, task="classification")

    def epoch_b():
        for _ in loader_b.into(step.static):
            step()
        return None

    forms = [("a", "eager train_epoch of the example over the iterated DeviceLoader", lambda: train_epoch(ddp, opt_a, loader_a)[0]),
             ("b", "bare GraphedTrainStep fed by loader.into, no metrics", epoch_b),
             ("c", "DeviceTrainer.run_epoch", lambda: trainer.run_epoch()["loss"])]
    forms = [f for f in forms if f[0] in args.forms]
    times, values = {k: [] for k, _, _ in forms}, {}
    for k, _, fn in forms:
        fn()                                                 # warm-up epoch
    for _ in range(args.repeats):
        for k, _, fn in forms:
            t, values[k] = timed(fn, dev)
            times[k].append(t)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    spread = {k: max(v) - min(v) for k, v in times.items()}
    for k, what, _ in forms:
        say(f"({k}) {what}: " + ", ".join(f"{t * 1e3:.1f}" for t in times[k]) + f" ms / epoch; median {med[k] * 1e3:.1f} ms = "
            f"{med[k] / nb * 1e3:.3f} ms / step = {nb * args.batch / med[k]:.0f} clouds/s; spread (max - min) {spread[k] * 1e3:.1f} ms = "
            f"{spread[k] / med[k] * 100:.2f} %")
    if len(forms) < 3:
        return
    say(f"    (a) / (c) = {med['a'] / med['c']:.3f}, (c) / (b) = {med['c'] / med['b']:.3f} (medians)")
    say(f"    (c) - (b), medians: {(med['c'] - med['b']) * 1e3:+.1f} ms / epoch = {(med['c'] - med['b']) / nb * 1e6:+.2f} us / step -> inside "
        f"(b)'s own spread of {spread['b'] * 1e3:.1f} ms: {'yes' if med['c'] - med['b'] <= spread['b'] else 'NO'}")
    say(f"    last epoch's loss: (a) {values['a']:.4f}, (c) {values['c']:.4f} (separate models on separate trajectories: eager and "
        "replayed steps from the same seeds, not compared bit for bit)")

    # the host side of (c)'s calls, step by step: enqueue times of one more epoch (no synchronise inside; the sum is the host's
    # share of the epoch -- where it is below the epoch time the device is the bound and the added calls ride in its shadow)
    clock = dict(assemble=0.0, replay=0.0, loss_copy=0.0, metrics=0.0)
    torch.cuda.synchronize(dev)
    t_epoch = time.perf_counter()
    it = iter(loader_c.into(trainer.step.static))
    for i in range(nb):
        t0 = time.perf_counter()
        next(it)
        t1 = time.perf_counter()
        loss = trainer.step()
        t2 = time.perf_counter()
        trainer._rows[i][0].copy_(loss)
        t3 = time.perf_counter()
        trainer._metrics(i)
        t4 = time.perf_counter()
        clock["assemble"] += t1 - t0
        clock["replay"] += t2 - t1
        clock["loss_copy"] += t3 - t2
        clock["metrics"] += t4 - t3
    for _ in it:
        pass
    t_host = time.perf_counter() - t_epoch
    torch.cuda.synchronize(dev)
    t_epoch = time.perf_counter() - t_epoch
    say("    host timeline of (c), one more epoch, us / step enqueued: " + ", ".join(f"{k} {v / nb * 1e6:.1f}" for k, v in clock.items())
        + f"; host total {t_host / nb * 1e6:.1f} us / step of {t_epoch / nb * 1e6:.1f} us / step with the final synchronise")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
