"""A captured training step of ``DeltaNetMultiscaleSegmentation`` beside the single-resolution ``DeltaNetSegmentation`` step on
the same batch: forward + loss + backward + SGD update replayed from a HIP graph (``GraphedTrainStep``).  Reported per model: the
library launches of one eager step (calls through the C ABI; torch's own kernels are not counted), ms per step (HIP events
around ``--steps`` back-to-back replays, ``--repeats`` times, legs alternating) and the run-to-run spread.  Descriptive: the two
networks do different work and neither is expected to beat the other.  ``--sampling fps`` adds the multi-resolution step with
``sampling="fps"`` (one Euclidean farthest-point sampling launch inside the captured step, ``geometry.fps_levels``) as a third
leg and reports its cost against the ``"prefix"`` step of the same run.  Needs an MI355X.

    python tools/bench_multiscale.py --out profiles/device_multiscale.txt
    python tools/bench_multiscale.py --sampling fps --out profiles/device_multiscale_fps.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as dc
from deltaconv_amd._lib import lib
from deltaconv_amd.data import synthetic_batch
from deltaconv_amd.graph_step import GraphedTrainStep
from deltaconv_amd.utils import calc_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=16)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sampling", choices=("prefix", "fps"), default="prefix",
                    help="fps: a third leg, the multi-scale step with sampling=\"fps\", against the prefix step of this run")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_multiscale.py needs an MI355X")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    loss_fn = lambda out, y: calc_loss(out, y, smoothing=False)
    make_batch = lambda: synthetic_batch(args.clouds, args.points, seed=7, num_classes=args.classes, per_point_labels=True).to(dev)
    models = {
        "multi-scale (enc (64, 64) / (128) / (256), dec (128, 128), ratios (4, 4), vector_pool max)":
            lambda: dc.models.DeltaNetMultiscaleSegmentation(3, args.classes, num_neighbors=args.k),
        "single resolution (conv_channels [64, 128, 256], mlp_depth 2)":
            lambda: dc.models.DeltaNetSegmentation(3, args.classes, num_neighbors=args.k),
    }
    prefix_name = next(iter(models))
    fps_name = "multi-scale, sampling=\"fps\" (the same network; level 1 sampled inside the step)"
    if args.sampling == "fps":
        models[fps_name] = lambda: dc.models.DeltaNetMultiscaleSegmentation(3, args.classes, num_neighbors=args.k, sampling="fps")
    say(f"# captured training steps on {torch.cuda.get_device_name(0)}: {args.clouds} clouds of {args.points} points, k = {args.k}, "
        f"{args.classes} classes; ms per step = HIP events around {args.steps} back-to-back replays, {args.repeats} repeats, the "
        f"models alternating")
    steps = {}
    for name, build in models.items():
        torch.manual_seed(1)
        model = build().to(dev).train()
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        names, call = [], lib.call
        lib.call = lambda n, *a: (names.append(n), call(n, *a))[1]
        try:
            b = make_batch()
            loss_fn(model(b), b.y).backward()
        finally:
            lib.call = call
        model.zero_grad(set_to_none=True)
        steps[name] = GraphedTrainStep(model, loss_fn, make_batch(), optimizer=opt)
        say(f"## {name}: {sum(p.numel() for p in model.parameters())} parameters, {len(names)} library launches in one eager "
            f"forward + backward ({len(set(names))} different entry points)")
    times = {name: [] for name in steps}
    for _ in range(args.repeats):
        for name, step in steps.items():
            step()
            torch.cuda.synchronize(dev)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                step()
            t1.record()
            torch.cuda.synchronize(dev)
            times[name].append(t0.elapsed_time(t1) / args.steps)
    for name, t in times.items():
        med = sorted(t)[len(t) // 2]
        say(f"{name}: " + ", ".join(f"{x:.3f}" for x in t) + f" ms / step; median {med:.3f} ms, spread (max - min) "
            f"{max(t) - min(t):.3f} ms = {(max(t) - min(t)) / med * 100:.2f} %")
    if args.sampling == "fps":
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        spread = max(max(times[n]) - min(times[n]) for n in (prefix_name, fps_name))
        say(f"sampling=\"fps\" against sampling=\"prefix\" (medians of this run): {med[fps_name] - med[prefix_name]:+.3f} ms / step = "
            f"{(med[fps_name] / med[prefix_name] - 1) * 100:+.2f} %; the larger spread of the two legs is {spread:.3f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
