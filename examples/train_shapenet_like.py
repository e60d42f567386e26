"""Part-segmentation training loop with the semantics of the reference's experiments/train_shapenet.py (:20-189):
DeltaNetSegmentation(conv_channels [64,128,256], mlp_depth 2, embedding 1024, categorical vector),
SGD(100 * lr, momentum 0.9, wd 1e-4) + cosine annealing to lr, plain mean cross entropy over the points,
mean part-IoU per shape (experiments/utils.py:27-51) after every epoch, state_dict checkpoint with the
reference's key names -- on the MI355X path, data-parallel over the GPUs of one node.

    python examples/train_shapenet_like.py --epochs 2                           # synthetic clouds
    python examples/train_shapenet_like.py --data /data/ShapeNet --epochs 200   # raw/<synset>/*.txt + train_test_split/
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_shapenet_like.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as deltaconv                       # the drop-in: was `import deltaconv`
from deltaconv_amd.models import DeltaNetMultiscaleSegmentation, DeltaNetSegmentation
from deltaconv_amd.utils import calc_loss, calc_shape_IoU
from deltaconv_amd.dp import FlatGradDataParallel
from deltaconv_amd.data import synthetic_batch


def shapenet_model(args, num_classes):
    """train_shapenet.py:76-89; --multiscale: the multi-resolution network over prefix levels (rows in FPS pick order, as
    geodesic_subsample writes them, make the levels an FPS hierarchy); --sampling fps samples level 1 inside every step instead
    (Euclidean farthest-point sampling, geometry.fps_levels): an FPS hierarchy whatever the order of the rows."""
    if getattr(args, "multiscale", False):
        return DeltaNetMultiscaleSegmentation(in_channels=3, num_classes=num_classes, mlp_depth=2, embedding_size=1024,
                                              num_neighbors=args.k, grad_regularizer=args.grad_regularizer,
                                              grad_kernel_width=args.grad_kernel, categorical_vector=True,
                                              sampling=getattr(args, "sampling", "prefix"),
                                              fps_method=getattr(args, "fps_method", None))
    return DeltaNetSegmentation(in_channels=3, num_classes=num_classes, conv_channels=[64, 128, 256], mlp_depth=2,
                                embedding_size=1024, num_neighbors=args.k, grad_regularizer=args.grad_regularizer,
                                grad_kernel_width=args.grad_kernel, categorical_vector=True)


def synthetic_split(num_batches, args, seed, device):
    """Stand-in for the ShapeNet loaders: 16 categories, per-point labels inside the category's part range."""
    starts = [0, 4, 6, 8, 12, 16, 19, 22, 24, 28, 30, 36, 38, 41, 44, 47]
    parts = [4, 2, 2, 4, 4, 3, 3, 2, 4, 2, 6, 2, 3, 3, 3, 3]
    out = []
    g = torch.Generator().manual_seed(seed)
    for b in range(num_batches):
        data = synthetic_batch(args.batch_size, args.num_points, seed=seed + b, per_point_labels=True, categories=16,
                               num_classes=50)
        cat = torch.randint(0, 16, (args.batch_size,), generator=g)
        data.category = torch.nn.functional.one_hot(cat, 16).float()
        height = data.pos[:, 2].view(args.batch_size, -1)                      # the part = a height band of the shape
        band = ((height - height.min(1, keepdim=True).values) / (height.max(1, keepdim=True).values
                - height.min(1, keepdim=True).values + 1e-9) * torch.tensor(parts)[cat].view(-1, 1)).long()
        band = torch.minimum(band, (torch.tensor(parts)[cat] - 1).view(-1, 1))
        data.y = (band + torch.tensor(starts)[cat].view(-1, 1)).reshape(-1)
        out.append(data.to(device))
    return out


def shapenet_sets(root, num_points, full_resolution=False):
    """-> (trainval set, test set, augmentation).  The training shapes are NormalizeScale + GeodesicFPS(num_points), cached under
    ``root/processed``.  With `full_resolution` the test shapes keep every point (NormalizeScale alone).  ShapeNet keys its cache
    by the categories only and writes all splits with the pre_transform of whoever comes first, so the un-subsampled split has a
    cache of its own, ``root/processed_full``, that the subsampled one cannot shadow."""
    import deltaconv_amd.transforms as T
    from deltaconv_amd.datasets import Compose, ShapeNet
    pre = Compose((T.NormalizeScale(), T.GeodesicFPS(num_points)))                          # train_shapenet.py:30-33
    aug = Compose((T.RandomScale((2 / 3, 3 / 2)), T.RandomTranslateGlobal(0.2)))            # train_shapenet.py:35-38
    tr = ShapeNet(root, split="trainval", transform=aug, pre_transform=pre)
    if full_resolution:
        te = ShapeNet(root, split="test", pre_transform=T.NormalizeScale(), processed_dir=os.path.join(root, "processed_full"))
    else:
        te = ShapeNet(root, split="test", pre_transform=pre)
    return tr, te, aug


def require_full_resolution(sizes, num_points):
    """Refuse a "full-resolution" store that is the subsampled one under another name: every cloud holding exactly num_points
    points is what GeodesicFPS(num_points) leaves (a stale or shared cache), and the score on it is the sampled-resolution score."""
    sizes = [int(n) for n in sizes]
    if sizes and all(n == num_points for n in sizes):
        raise SystemExit(f"--eval-full-resolution: every one of the {len(sizes)} test shapes has exactly {num_points} points, the "
                         "size GeodesicFPS leaves -- this is the subsampled split, not the shapes as read; remove the stale "
                         "processed_full cache or lower --num_points")


def train_epoch(ddp, opt, loader):
    ddp.module.train()
    total, count = 0.0, 0
    for data in loader:
        ddp.zero_grad()
        loss = calc_loss(ddp(data), data.y, smoothing=False)
        loss.backward()
        ddp.reduce_gradients()
        opt.step()
        total += float(loss) * data.num_graphs
        count += data.num_graphs
    return total / count


@torch.no_grad()
def evaluate(model, loader):
    """Mean part IoU per shape (train_shapenet.py:137-160)."""
    model.eval()
    ious = []
    for data in loader:
        pred = model(data).argmax(1).view(data.num_graphs, -1).cpu().numpy()
        true = data.y.view(data.num_graphs, -1).cpu().numpy()
        label = data.category.argmax(1).cpu().numpy()
        ious += calc_shape_IoU(pred, true, label, None)
    return float(np.mean(ious))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--num_points", type=int, default=2048)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--grad_regularizer", type=float, default=0.001)
    ap.add_argument("--grad_kernel", type=float, default=1)
    ap.add_argument("--train_batches", type=int, default=4)
    ap.add_argument("--logdir", default="runs/shapenet_like")
    ap.add_argument("--data", default=None, help="ShapeNet part root (raw/<synset>/*.txt, raw/train_test_split/*.json)")
    ap.add_argument("--multiscale", action="store_true",
                    help="DeltaNetMultiscaleSegmentation: three levels (ratios 4, 4) with transported max-pooling of the vector stream")
    ap.add_argument("--sampling", choices=("prefix", "fps"), default="prefix",
                    help="with --multiscale: prefix = the coarser levels are the first rows of every cloud (rows in FPS pick order); "
                         "fps = Euclidean farthest-point sampling inside the step (rows in any order)")
    ap.add_argument("--fps-method", choices=("brute", "grid"), default=None,
                    help="with --sampling fps: brute = the register kernel (clouds up to 16 384 points), grid = the exact sampler on a "
                         "cell grid (the same picks, clouds up to 262 144 points); default: the DC_FPS switch")
    ap.add_argument("--device-loader", action="store_true",
                    help="with --data: keep the prepared dataset on the GPU, build and augment every batch in one launch "
                         "(deltaconv_amd.DeviceLoader) instead of per-shape transforms + collate + upload on the host")
    ap.add_argument("--device-eval", action="store_true",
                    help="with --device-loader: the per-epoch evaluation on the device (deltaconv_amd.DeviceEvaluator: captured "
                         "forward, metrics in one launch per batch, one synchronise per pass) instead of evaluate() below")
    ap.add_argument("--eval-full-resolution", action="store_true",
                    help="with --device-eval: keep the test shapes as read (every point, before GeodesicFPS) on the device as well, "
                         "subsample them there, and report the mean IoU on ALL points of every shape -- the sampled points' vote "
                         "sums interpolated back by deltaconv_amd.Propagator (k = 3, inference only)")
    ap.add_argument("--device-train", action="store_true",
                    help="with --device-loader: the training epoch on the device (deltaconv_amd.DeviceTrainer: the step replayed from "
                         "one captured graph, loss and the part IoU of the training forward kept on the device, one synchronise per "
                         "epoch) instead of train_epoch() below; prints train_miou and writes the trainer's state next to last.pt")
    ap.add_argument("--resume", default=None,
                    help="with --device-train: continue from the trainer state a run with --device-train wrote (last_trainer.pt; "
                         "'{rank}' in the name is replaced by the rank)")
    args = ap.parse_args(argv)
    if args.device_train and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-train trains from a device-resident training set: it needs --data and --device-loader")
    if args.resume is not None and not args.device_train:
        raise SystemExit("--resume continues from the state of a device trainer: it needs --device-train")
    if args.eval_full_resolution and not args.device_eval:
        raise SystemExit("--eval-full-resolution scores the pre-FPS store through the device evaluator: it needs --device-eval")
    if args.device_eval and not (args.data is not None and args.device_loader):
        raise SystemExit("--device-eval evaluates from a device-resident test set: it needs --data and --device-loader")

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    torch.manual_seed(1)
    model = shapenet_model(args, 50).to(dev)
    ddp = FlatGradDataParallel(model)
    opt = deltaconv.optim.SGD(model.parameters(), lr=100 * args.lr, momentum=args.momentum, weight_decay=1e-4)   # torch.optim.SGD, step = one launch
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, args.epochs, eta_min=args.lr)
    if args.data is None:
        train = synthetic_split(args.train_batches, args, 1000 * (rank + 1), dev)
        test = synthetic_split(2, args, 777000, dev)
    else:
        from deltaconv_amd.datasets import DataLoader
        # --eval-full-resolution: the test shapes keep every point; the subsampling happens on the device below
        tr, te, aug = shapenet_sets(args.data, args.num_points, args.eval_full_resolution)
    if args.data is not None and args.device_loader:
        # the same recipe, drawn and applied on the device; every rank takes its share of one permutation per epoch
        train = deltaconv.DeviceLoader(deltaconv.DeviceDataset.from_dataset(tr, dev), args.batch_size, shuffle=True,
                                       drop_last=True, transform=aug, seed=1, rank=rank, world=world)
        test_store = full_store = deltaconv.DeviceDataset.from_dataset(te, dev)
        if args.eval_full_resolution:        # the pre-FPS store stays; the network sees its geodesic subsample
            require_full_resolution(full_store.sizes, args.num_points)
            test_store = full_store.geodesic_subsample(args.num_points, seed=1)
        test = deltaconv.DeviceLoader(test_store, args.batch_size)
        args.train_batches = len(train)
        if args.device_eval:                 # equal-size clouds (GeodesicFPS to num_points): the full batches replay one graph
            evaluator = deltaconv.DeviceEvaluator(model, test, task="segmentation",
                                                  propagate_to=full_store if args.eval_full_resolution else None)
        if args.device_train:                # the capture's warm-up steps leave model and optimizer where they were
            trainer = deltaconv.DeviceTrainer(model, train, opt, task="segmentation", reducer=ddp)
    elif args.data is not None:
        sampler = torch.utils.data.distributed.DistributedSampler(tr) if world > 1 else None

        class _OnDevice:
            def __init__(self, loader):
                self.loader = loader

            def __iter__(self):
                return (b.to(dev) for b in self.loader)
        train = _OnDevice(DataLoader(tr, batch_size=args.batch_size, shuffle=sampler is None, sampler=sampler, drop_last=True))
        test = _OnDevice(DataLoader(te, batch_size=args.batch_size, shuffle=False, drop_last=False))
        args.train_batches = len(train.loader)
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
            loss = res["loss"]
        else:
            loss = train_epoch(ddp, opt, train)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        miou = evaluator.run()["mean_iou"] if args.device_eval else evaluate(model, test)
        sched.step()
        if args.device_train:
            torch.save(dict(trainer=trainer.state_dict(), scheduler=sched.state_dict()), os.path.join(args.logdir, trainer_file))
        if rank == 0:
            train_miou = dict(train_miou=round(res["mean_iou"], 4)) if args.device_train else {}    # of the training forward
            print(json.dumps(dict(epoch=epoch, loss=round(loss, 4), **train_miou, test_mean_iou=round(miou, 4),
                                  clouds_per_s=round(world * args.train_batches * args.batch_size / dt, 1))))
            torch.save(model.state_dict(), os.path.join(args.logdir, "last.pt"))   # reference key names
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
