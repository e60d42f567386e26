"""The host side of ``DeviceTrainer`` (deltaconv_amd/train.py), no GPU: the reduction of an epoch's per-step losses and integer
counts (``reduce_epoch``), the mapping from result rows to dataset indices (``epoch_indices``) and the argument checks of the
examples' ``--device-train`` / ``--resume``."""
import importlib.util
import os

import numpy as np
import pytest

from deltaconv_amd.loader import DeviceLoader, epoch_permutation
from deltaconv_amd.train import DeviceTrainer, epoch_indices, reduce_epoch   # noqa: F401  (the class imports without a device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts(true, pred, classes, groups):
    """What the metric launches leave: per group of rows, hits and label counts per class, and the labels outside the classes."""
    hit, cnt, ign = (np.zeros((groups, classes), np.int32), np.zeros((groups, classes), np.int32), np.zeros(groups, np.int32))
    for g, (t, p) in enumerate(zip(np.array_split(true, groups), np.array_split(pred, groups))):
        ok = (t >= 0) & (t < classes)
        cnt[g] = np.bincount(t[ok], minlength=classes)
        hit[g] = np.bincount(t[ok & (t == p)], minlength=classes)
        ign[g] = np.sum(~ok)
    return hit, cnt, ign


def test_loss_in_the_reference_accumulation_order():
    rng = np.random.default_rng(0)
    losses = (rng.random(37) * np.float32(3.0) + np.float32(1e-3)).astype(np.float32)
    losses[5] = np.float32(1e4)                             # an order that matters
    true = rng.integers(0, 7, size=37 * 32)
    hit, cnt, ign = _counts(true, rng.integers(0, 7, size=true.size), 7, 37)
    got = reduce_epoch(losses, 32, hit, cnt, ign)
    total, count = 0.0, 0
    for v in losses:                                        # total += float(loss) * data.num_graphs; count += data.num_graphs
        total += float(v) * 32
        count += 32
    assert got["loss"] == total / count and got["steps"] == 37 and got["clouds"] == 37 * 32
    assert got["losses"].dtype == np.float32 and np.array_equal(got["losses"], losses)
    single = np.float32(0.0)
    for v in losses:
        single += v * np.float32(32)
    assert float(single) != total                           # (the check above can tell Python floats from an fp32 running sum)
    assert "indices" not in got and "mean_iou" not in got
    empty = reduce_epoch(np.zeros(0, np.float32), 32, hit[:0], cnt[:0], ign[:0])
    assert np.isnan(empty["loss"]) and np.isnan(empty["accuracy"]) and empty["clouds"] == 0


@pytest.mark.parametrize("groups", [1, 16])
def test_accuracies_against_sklearn(groups):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(groups)
    true = rng.integers(0, 9, size=640)
    true[true == 4] = 3                                     # a class no row carries
    pred = np.where(rng.random(640) < 0.6, true, rng.integers(0, 10, size=640))
    hit, cnt, ign = _counts(true, pred, 10, groups)
    got = reduce_epoch(np.ones(groups, np.float32), 640 // groups, hit, cnt, ign, indices=np.arange(640))
    assert got["ignored"] == 0 and np.array_equal(got["indices"], np.arange(640))
    assert abs(got["accuracy"] - metrics.accuracy_score(true, pred)) <= 1e-15
    assert abs(got["balanced_accuracy"] - metrics.balanced_accuracy_score(true, pred)) <= 1e-15


def test_ignored_rows_are_misses_and_ious_pass_through():
    true = np.array([0, 1, 1, 2, -1, 3, 0, 0])
    pred = np.array([0, 1, 0, 2, 1, 0, 0, 1])
    hit, cnt, ign = _counts(true, pred, 3, 2)
    got = reduce_epoch(np.array([1.0, 2.0], np.float32), 4, hit, cnt, ign, iou=np.array([0.5, 0.25]), label=np.array([3, 7]))
    assert got["ignored"] == 2 and got["accuracy"] == 4 / 8
    assert got["balanced_accuracy"] == float(np.mean(np.array([2, 1, 1]) / np.array([3, 2, 1])))
    assert got["ious"] == [0.5, 0.25] and got["mean_iou"] == 0.375 and np.array_equal(got["label"], [3, 7])
    assert got["loss"] == (1.0 * 4 + 2.0 * 4) / 8


class _Store:
    """What ``DeviceLoader`` asks of a store on the host: a length (and whether it has normals)."""
    norm = None

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("shuffle", [True, False])
def test_indices_follow_the_rank_share(world, shuffle):
    n, bs, seed = 43, 4, 11
    seen = []
    for rank in range(world):
        loader = DeviceLoader(_Store(n), bs, shuffle=shuffle, drop_last=True, seed=seed, rank=rank, world=world)
        for epoch in (0, 3):
            perm = epoch_permutation(n, seed, epoch, shuffle)
            share = perm[:(n // world) * world][rank::world]             # DeviceLoader.rank_share, written out
            steps = (n // world) // bs
            got = epoch_indices(loader, epoch)
            assert got.dtype == np.int64 and got.shape == (steps * bs,) and steps == len(loader)
            assert np.array_equal(got, share[:steps * bs])
            if epoch == 3:
                seen.append(got)
        loader.set_epoch(3)
        assert np.array_equal(epoch_indices(loader), seen[-1])           # default: the loader's current epoch
    both = np.concatenate(seen)
    assert len(set(both.tolist())) == both.size                          # the ranks' rows are disjoint clouds


def _example(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["train_modelnet_like", "train_shapenet_like"])
def test_examples_refuse_device_train_without_its_inputs(name, tmp_path):
    main = _example(name).main
    with pytest.raises(SystemExit, match="--device-train .* needs --data and --device-loader"):
        main(["--device-train"])
    with pytest.raises(SystemExit, match="--device-train .* needs --data and --device-loader"):
        main(["--device-train", "--data", str(tmp_path)])
    with pytest.raises(SystemExit, match="--device-train .* needs --data and --device-loader"):
        main(["--device-train", "--device-loader"])
    with pytest.raises(SystemExit, match="--resume .* needs --device-train"):
        main(["--resume", str(tmp_path / "last_trainer.pt")])
    with pytest.raises(SystemExit, match="--resume .* needs --device-train"):
        main(["--resume", str(tmp_path / "last_trainer.pt"), "--data", str(tmp_path), "--device-loader"])
