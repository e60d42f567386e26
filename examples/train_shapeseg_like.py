"""Mesh-segmentation training loop with the semantics of the reference's experiments/train_shapeseg.py (:18-141):
DeltaNetSegmentation(conv_channels [128] * 8, mlp_depth 1, embedding 512, 8 classes), Adam(lr 0.005) + StepLR(30, 0.1), plain
mean cross entropy over the points, a seeded 90/10 train/validation split, validation and test accuracy after every epoch,
``best.pt`` = the model with the best validation accuracy -- with the whole data side on the MI355X: the raw meshes go to the
device once and

    DeviceMeshDataset.from_dataset(...).normalize([NormalizeArea, NormalizeAxes])
        .sample_points(num_points * sampling_margin, include_labels=True).geodesic_subsample(num_points)

replaces the per-shape ``pre_transform`` (train_shapeseg.py:28-34; GenerateMeshNormals is left out there: SamplePoints overwrites
the normals it computes).  ``--vertex-clouds`` trains on the meshes' own vertices instead of surface samples:
``meshes.vertex_cloud().geodesic_subsample(num_points)``, the vertex normals being the device form of GenerateMeshNormals
(train_shapeseg.py:31).  ``deltaconv_amd.random_split`` the split of :46-50, ``DeviceLoader`` the augmentation of :37-41,
``DeviceTrainer`` the epoch and ``DeviceEvaluator`` the two evaluations.  No per-shape host call is left.  The device
``NormalizeArea`` is the surface area over face rows; in front of ``NormalizeAxes`` only its centring survives, so the shapes
are the reference's.

    python examples/train_shapeseg_like.py --epochs 2                          # synthetic labelled meshes
    python examples/train_shapeseg_like.py --data /data/ShapeSeg --epochs 50   # raw/ShapeSeg/<SET>/raw/{meshes,segs}
    python examples/train_shapeseg_like.py --epochs 2 --vertex-clouds          # vertices + vertex normals, no surface sampling
    python examples/train_shapeseg_like.py --epochs 2 --vertex-clouds --voxel-size 0.02   # one vertex per grid cell, then geodesic FPS
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deltaconv_amd as deltaconv                       # the drop-in: was `import deltaconv`
import deltaconv_amd.transforms as T
from deltaconv_amd.data import synthetic_mesh
from deltaconv_amd.datasets import Data
from deltaconv_amd.models import DeltaNetSegmentation


def shapeseg_model(args):
    """train_shapeseg.py:68-78."""
    return DeltaNetSegmentation(in_channels=3, num_classes=8, conv_channels=[args.channels] * args.layers, mlp_depth=1,
                                embedding_size=512, num_neighbors=args.k, grad_regularizer=args.grad_regularizer,
                                grad_kernel_width=args.grad_kernel)


def synthetic_items(count, faces, seed):
    """Stand-in for the ShapeSeg reader: stretched, shifted tori with one of 8 labels per vertex."""
    items = []
    for i in range(count):
        pos, face, y = synthetic_mesh(faces, seed + i, labels=True)
        items.append(Data(pos=pos * torch.tensor([1.0, 0.55, 1.7]) + 0.1 * (i % 7), face=face, y=y))
    return items


def prepare(items, dev, args):
    """Raw meshes -> the store the network trains on; the meshes themselves are kept for nothing else."""
    meshes = deltaconv.DeviceMeshDataset.from_dataset(items, dev).normalize([T.NormalizeArea(), T.NormalizeAxes()])
    if meshes.degenerate.any():
        raise SystemExit(f"{int(meshes.degenerate.sum())} meshes without surface area or extent: nothing to normalise them by")
    if args.vertex_clouds:
        cloud = meshes.vertex_cloud()
        if args.voxel_size is not None:                 # one vertex per grid cell first: linear, and it evens out the tessellation
            cloud = cloud.voxel_subsample(args.voxel_size, reduce=args.voxel_reduce)
        return cloud.geodesic_subsample(args.num_points, seed=args.seed, large="device" if args.device_fps_large else "host")
    return meshes.sample_points(args.num_points * args.sampling_margin, include_normals=True, include_labels=True,
                                seed=args.seed).geodesic_subsample(args.num_points, seed=args.seed)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--num_points", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--grad_kernel", type=float, default=1)
    ap.add_argument("--grad_regularizer", type=float, default=0.001)
    ap.add_argument("--sampling_margin", type=int, default=8)
    ap.add_argument("--vertex-clouds", action="store_true",
                    help="train on the meshes' vertices and vertex normals instead of surface samples")
    ap.add_argument("--device-fps-large", action="store_true",
                    help="with --vertex-clouds: meshes of more than 16 384 vertices are reduced on the device too "
                         "(geodesic_subsample(large='device'), up to 262 144 vertices) instead of through the host library")
    ap.add_argument("--voxel-size", type=float, default=None,
                    help="with --vertex-clouds: thin every vertex cloud to one vertex per grid cell of this edge length "
                         "(DeviceDataset.voxel_subsample; the meshes are normalised to about unit extent) before the geodesic sampling")
    ap.add_argument("--voxel-reduce", choices=["mean"], default=None,
                    help="with --voxel-size: 'mean' pools every cell's attributes (barycentre, mean normal, majority label) instead "
                         "of keeping its representative's (DeviceDataset.voxel_subsample(reduce='mean'))")
    ap.add_argument("--layers", type=int, default=8, help="convolution layers (train_shapeseg.py:71: 8)")
    ap.add_argument("--channels", type=int, default=128, help="channels of every layer (train_shapeseg.py:71: 128)")
    ap.add_argument("--seed", type=int, default=1, help="of the split, the surface samples, the FPS starts and the loader")
    ap.add_argument("--logdir", default="runs/shapeseg_like")
    ap.add_argument("--data", default=None, help="ShapeSeg root (raw/ShapeSeg/<SET>/raw/{meshes,segs}); default: synthetic meshes")
    ap.add_argument("--train_meshes", type=int, default=40, help="synthetic training meshes (before the 90/10 split)")
    ap.add_argument("--test_meshes", type=int, default=8)
    ap.add_argument("--mesh_faces", type=int, default=4000, help="faces of a synthetic mesh")
    ap.add_argument("--resume", default=None, help="continue from the state a run of this script wrote (last_trainer.pt)")
    args = ap.parse_args(argv)
    if args.device_fps_large and not args.vertex_clouds:
        raise SystemExit("--device-fps-large samples the vertex clouds of --vertex-clouds: it needs --vertex-clouds")
    if args.voxel_size is not None and not args.vertex_clouds:
        raise SystemExit("--voxel-size thins the vertex clouds of --vertex-clouds: it needs --vertex-clouds")
    if args.voxel_reduce is not None and args.voxel_size is None:
        raise SystemExit("--voxel-reduce pools the cells of --voxel-size: it needs --voxel-size")

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    if args.data is None:
        train_items = synthetic_items(args.train_meshes, args.mesh_faces, 1000)
        test_items = synthetic_items(args.test_meshes, args.mesh_faces, 777000)
    else:
        from deltaconv_amd.datasets import ShapeSeg
        train_items, test_items = ShapeSeg(args.data, True).items, ShapeSeg(args.data, False).items    # no pre_transform: raw meshes
    full = prepare(train_items, dev, args)
    num_train = int(len(full) * 0.9)                                                                 # train_shapeseg.py:47-50
    train_store, val_store = deltaconv.random_split(full, [num_train, len(full) - num_train], seed=args.seed)
    test_store = prepare(test_items, dev, args)
    aug = [T.RandomScale((0.8, 1.2)), T.RandomRotate(360, axis=2), T.RandomTranslateGlobal(0.1)]     # train_shapeseg.py:37-41
    train = deltaconv.DeviceLoader(train_store, args.batch_size, shuffle=True, drop_last=True, transform=aug, seed=args.seed)
    val = deltaconv.DeviceLoader(val_store, args.batch_size)
    test = deltaconv.DeviceLoader(test_store, args.batch_size)

    model = shapeseg_model(args).to(dev)
    opt = deltaconv.optim.Adam(model.parameters(), lr=args.lr)                                       # torch.optim.Adam, step = one launch
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=30, gamma=0.1)
    trainer = deltaconv.DeviceTrainer(model, train, opt, task="segmentation")
    val_eval = deltaconv.DeviceEvaluator(model, val, task="segmentation")
    test_eval = deltaconv.DeviceEvaluator(model, test, task="segmentation")

    os.makedirs(args.logdir, exist_ok=True)
    first_epoch, best_val, best_val_test = 0, 0.0, 0.0
    if args.resume is not None:
        saved = torch.load(args.resume, map_location=dev)
        trainer.load_state_dict(saved["trainer"])
        sched.load_state_dict(saved["scheduler"])
        first_epoch, best_val, best_val_test = saved["trainer"]["epoch"], saved["best_validation"], saved["best_validation_test"]
    for epoch in range(first_epoch, args.epochs):
        t0 = time.perf_counter()
        res = trainer.run_epoch(epoch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        val_acc, test_acc = val_eval.run()["accuracy"], test_eval.run()["accuracy"]
        if val_acc > best_val:                                                                       # train_shapeseg.py:98-101
            best_val, best_val_test = val_acc, test_acc
            torch.save(model.state_dict(), os.path.join(args.logdir, "best.pt"))                     # reference key names
        sched.step()
        torch.save(dict(trainer=trainer.state_dict(), scheduler=sched.state_dict(), best_validation=best_val,
                        best_validation_test=best_val_test), os.path.join(args.logdir, "last_trainer.pt"))
        print(json.dumps(dict(epoch=epoch, loss=round(res["loss"], 4), train_acc=round(res["accuracy"], 4),
                              validation_acc=round(val_acc, 4), test_acc=round(test_acc, 4),
                              clouds_per_s=round(len(train) * args.batch_size / dt, 1))))
    print(f"Test accuracy: {best_val_test}")


if __name__ == "__main__":
    main()
