"""Training loop with the semantics of the reference's experiments/train_modelnet.py (:20-142): SGD(lr 0.1,
momentum 0.9, wd 1e-4) + cosine annealing to 1e-3, label-smoothed cross entropy, train / evaluate per
epoch, state_dict checkpoints with the reference's key names -- on the MI355X path, data-parallel over
the GPUs of one node.  No dataset ships with this repo (the reference downloads ModelNet40), so by default
the clouds are synthetic; with `--data <ModelNet40 root>` (raw/<category>/<train|test>/*.off) the reference's
pipeline runs instead: NormalizeScale -> SamplePoints -> GeodesicFPS once, RandomScale + RandomTranslateGlobal
per access (train_modelnet.py:29-49), through `deltaconv_amd.datasets`.  `--device-loader` keeps the prepared clouds on
the GPU; `--device-fps` and `--device-sample` move GeodesicFPS, and SamplePoints with it, there as well, `--device-normalize`
NormalizeScale too; `--device-train` runs
the epochs themselves there (deltaconv_amd.DeviceTrainer: captured step, loss and accuracy read once per epoch).

    python examples/train_modelnet_like.py --epochs 3
    python examples/train_modelnet_like.py --data /data/ModelNet40 --epochs 50
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_modelnet_like.py
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as deltaconv                       # the drop-in: was `import deltaconv`
from deltaconv_amd.models import DeltaNetClassification
from deltaconv_amd.utils import calc_loss
from deltaconv_amd.dp import FlatGradDataParallel
from deltaconv_amd.data import synthetic_batch


def make_split(num_batches, batch_size, points, seed, device, num_classes=30):
    """Synthetic stand-in for the ModelNet40 loaders: the label IS the shape family of the cloud (30 families of closed surfaces
    r = 1 + a sin(m theta) cos(l phi), randomly rotated: deltaconv_amd.data.shape_family) -- a learnable task."""
    out = []
    for b in range(num_batches):
        data = synthetic_batch(batch_size, points, seed=seed + b, num_classes=num_classes, learnable=True)
        out.append(data.to(device))
    return out


def train_epoch(ddp, opt, loader):
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


@torch.no_grad()
def evaluate(model, loader):
    model.eval()
    model.deltanet_base.cache_operators = True          # static test set: keep the operators
    correct = count = 0
    for data in loader:
        correct += int((model(data).argmax(1) == data.y).sum())
        count += data.num_graphs
    model.deltanet_base.cache_operators = False
    return correct / count


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--num_points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--grad_regularizer", type=float, default=0.001)
    ap.add_argument("--train_batches", type=int, default=8)
    ap.add_argument("--logdir", default="runs/modelnet_like")
    ap.add_argument("--data", default=None, help="ModelNet40 root with raw/<category>/<train|test>/*.off")
    ap.add_argument("--sampling_margin", type=int, default=8)
    ap.add_argument("--device-loader", action="store_true",
                    help="with --data: keep the prepared dataset on the GPU, build and augment every batch in one launch "
                         "(deltaconv_amd.DeviceLoader) instead of per-shape transforms + collate + upload on the host")
    ap.add_argument("--device-eval", action="store_true",
                    help="with --device-loader: the per-epoch evaluation on the device (deltaconv_amd.DeviceEvaluator: captured "
                         "forward, metrics in one launch per batch, one synchronise per pass) instead of evaluate() below")
    ap.add_argument("--device-fps", action="store_true",
                    help="with --device-loader: GeodesicFPS leaves pre_transform; the oversampled clouds are reduced to num_points on "
                         "the device, all shapes in a few launches (DeviceDataset.geodesic_subsample) instead of one host call per shape")
    ap.add_argument("--device-fps-large", action="store_true",
                    help="with --device-fps or --device-sample: clouds of more than 16 384 points (num_points * sampling_margin above that) are reduced "
                         "on the device too (geodesic_subsample(large='device'), up to 262 144 points) instead of through the host "
                         "library")
    ap.add_argument("--device-sample", action="store_true",
                    help="with --device-loader: SamplePoints and GeodesicFPS leave pre_transform (NormalizeScale alone stays); the "
                         "meshes go to the GPU and are sampled and reduced there, all shapes in a few launches "
                         "(DeviceMeshDataset.sample_points, then DeviceDataset.geodesic_subsample)")
    ap.add_argument("--device-normalize", action="store_true",
                    help="with --device-sample: NormalizeScale leaves pre_transform as well (nothing stays); the raw meshes go to the "
                         "GPU and are normalised there, all shapes in two launches (DeviceMeshDataset.normalize)")
    ap.add_argument("--device-train", action="store_true",
                    help="with --device-loader: the training epoch on the device (deltaconv_amd.DeviceTrainer: the step replayed from "
                         "one captured graph, loss and accuracy kept on the device, one synchronise per epoch) instead of "
                         "train_epoch() below; also writes the trainer's state next to last.pt")
    ap.add_argument("--resume", default=None,
                    help="with --device-train: continue from the trainer state a run with --device-train wrote (last_trainer.pt; "
                         "'{rank}' in the name is replaced by the rank)")
    args = ap.parse_args(argv)
    if args.device_train and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-train trains from a device-resident training set: it needs --data and --device-loader")
    if args.resume is not None and not args.device_train:
        raise SystemExit("--resume continues from the state of a device trainer: it needs --device-train")
    if args.device_sample and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-sample samples device-resident meshes: it needs --data and --device-loader")
    if args.device_normalize and not args.device_sample:
        raise SystemExit("--device-normalize normalises the device-resident meshes of --device-sample: it needs --device-sample")
    if args.device_fps and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-fps samples a device-resident dataset: it needs --data and --device-loader")
    if args.device_fps_large and not (args.device_fps or args.device_sample):
        raise SystemExit("--device-fps-large moves the large clouds of --device-fps / --device-sample to the device: it needs one of them")
    if args.device_eval and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-eval evaluates from a device-resident test set: it needs --data and --device-loader")

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(1)
    model = DeltaNetClassification(3, 40, num_neighbors=args.k, grad_regularizer=args.grad_regularizer).to(dev)
    ddp = FlatGradDataParallel(model)
    opt = deltaconv.optim.SGD(model.parameters(), lr=args.lr, momentum=0.9, weight_decay=1e-4)   # torch.optim.SGD, step = one launch
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, args.epochs, eta_min=0.001)
    if args.data is None:
        train = make_split(args.train_batches, args.batch_size, args.num_points, 1000 * (rank + 1), dev)
        test = make_split(4, args.batch_size, args.num_points, 777000, dev)
    else:
        import deltaconv_amd.transforms as T
        from deltaconv_amd.datasets import Compose, DataLoader, ModelNet
        pre = (T.NormalizeScale(), T.SamplePoints(args.num_points * args.sampling_margin, include_normals=True))
        pre = Compose(pre if args.device_fps else pre + (T.GeodesicFPS(args.num_points),))
        if args.device_sample:                                   # the meshes themselves are stored: faces stay
            pre = None if args.device_normalize else T.NormalizeScale()
        aug = Compose((T.RandomScale((4 / 5, 5 / 4)), T.RandomTranslateGlobal(0.1)))
        tr = ModelNet(args.data, None, "40", True, transform=aug, pre_transform=pre)
        te = ModelNet(args.data, None, "40", False, pre_transform=pre)
    if args.data is not None and args.device_loader:
        # the same recipe, drawn and applied on the device; every rank takes its share of one permutation per epoch
        fps = args.num_points if args.device_fps else None      # same start points on every rank: one dataset, many shares
        fps_large = "device" if args.device_fps_large else "host"
        if args.device_sample:                                  # same draws on every rank: seeds, not the global generator
            norm = T.NormalizeScale() if args.device_normalize else None
            store = lambda ds: deltaconv.DeviceMeshDataset.from_dataset(ds, dev, normalize=norm).sample_points(
                args.num_points * args.sampling_margin, seed=1).geodesic_subsample(args.num_points, seed=1, large=fps_large)
        else:
            store = lambda ds: deltaconv.DeviceDataset.from_dataset(ds, dev, fps=fps, fps_seed=1, fps_large=fps_large)
        train = deltaconv.DeviceLoader(store(tr), args.batch_size, shuffle=True, drop_last=True, transform=aug, seed=1, rank=rank,
                                       world=world)
        test = deltaconv.DeviceLoader(store(te), args.batch_size)
        args.train_batches = len(train)
        if args.device_eval:                 # equal-size clouds (GeodesicFPS to num_points): the full batches replay one graph
            evaluator = deltaconv.DeviceEvaluator(model, test, task="classification")
        if args.device_train:                # the capture's warm-up steps leave model and optimizer where they were
            trainer = deltaconv.DeviceTrainer(model, train, opt, task="classification", reducer=ddp)
    elif args.data is not None:
        sampler = torch.utils.data.distributed.DistributedSampler(tr) if world > 1 else None
        on_dev = lambda loader: (b.to(dev) for b in loader)      # each rank collates and uploads its own shard
        train_loader = DataLoader(tr, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler, drop_last=True)
        test_loader = DataLoader(te, batch_size=args.batch_size, shuffle=False, drop_last=False)
        args.train_batches = len(train_loader)

        class _OnDevice:
            def __init__(self, loader): self.loader = loader
            def __iter__(self): return on_dev(self.loader)
        train, test = _OnDevice(train_loader), _OnDevice(test_loader)
    os.makedirs(args.logdir, exist_ok=True)
    first_epoch = 0
    trainer_file = "last_trainer.pt" if world == 1 else f"last_trainer.rank{rank}.pt"      # every rank has its own loader share
    if args.resume is not None:
        saved = torch.load(args.resume.format(rank=rank), map_location=dev)
        trainer.load_state_dict(saved["trainer"])
        sched.load_state_dict(saved["scheduler"])
        first_epoch = saved["trainer"]["epoch"]
    for epoch in range(first_epoch, args.epochs):
        t0 = time.perf_counter()
        if args.device_train:
            res = trainer.run_epoch(epoch)
            loss, acc = res["loss"], res["accuracy"]
        else:
            loss, acc = train_epoch(ddp, opt, train)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        test_acc = evaluator.run()["accuracy"] if args.device_eval else evaluate(model, test)
        sched.step()
        if args.device_train:
            torch.save(dict(trainer=trainer.state_dict(), scheduler=sched.state_dict()), os.path.join(args.logdir, trainer_file))
        if rank == 0:
            print(json.dumps(dict(epoch=epoch, loss=round(loss, 4), train_acc=round(acc, 4), test_acc=round(test_acc, 4),
                                  clouds_per_s=round(world * args.train_batches * args.batch_size / dt, 1))))
            torch.save(model.state_dict(), os.path.join(args.logdir, "last.pt"))   # reference key names
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
