"""``examples/train_shapenet_like.py --eval-full-resolution`` must hand the evaluator the test shapes AS READ.  ``ShapeNet`` caches
its processed splits by category only and writes all of them with the first constructor's ``pre_transform``, so the un-subsampled
test split lives in a cache of its own (``processed_dir``) that the GeodesicFPS cache of the training run cannot shadow.  A tiny
fake ShapeNet root, no GPU."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_POINTS = 8
FILES = {"train": [("02691156", "a1", 20), ("03001627", "c1", 23)], "val": [("03001627", "c2", 17)],
         "test": [("02691156", "a3", 21), ("04379243", "t1", 26), ("03001627", "c3", NUM_POINTS)]}


@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location("train_shapenet_like", os.path.join(ROOT, "examples", "train_shapenet_like.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_root(root):
    g = torch.Generator().manual_seed(3)
    os.makedirs(os.path.join(root, "raw", "train_test_split"))
    for split, lst in FILES.items():
        with open(os.path.join(root, "raw", "train_test_split", f"shuffled_{split}_file_list.json"), "w") as fh:
            json.dump([f"shape_data/{syn}/{name}" for syn, name, _ in lst], fh)
        for syn, name, n in lst:
            os.makedirs(os.path.join(root, "raw", syn), exist_ok=True)
            lo = {"02691156": 0, "03001627": 12, "04379243": 47}[syn]
            tab = torch.cat([torch.randn(n, 3, generator=g), torch.nn.functional.normalize(torch.randn(n, 3, generator=g)),
                             torch.randint(lo, lo + 3, (n, 1), generator=g).float()], 1)
            with open(os.path.join(root, "raw", syn, name + ".txt"), "w") as fh:
                for row in tab.tolist():
                    fh.write(" ".join(f"{v:.6f}" for v in row) + "\n")
    return root


RAW_TEST = [n for _, _, n in FILES["test"]]


@pytest.mark.parametrize("sampled_cache_first", [True, False], ids=["fps-cache-exists", "fresh-root"])
def test_the_full_resolution_test_split_keeps_the_raw_point_counts(example, tmp_path, sampled_cache_first):
    root = make_root(str(tmp_path / "ShapeNet"))
    if sampled_cache_first:                                 # an earlier run without the flag left the subsampled cache of ALL splits
        tr, te, _ = example.shapenet_sets(root, NUM_POINTS)
        assert [d.pos.shape[0] for d in te.items] == [NUM_POINTS] * 3
    tr, te, aug = example.shapenet_sets(root, NUM_POINTS, full_resolution=True)
    assert [d.pos.shape[0] for d in te.items] == RAW_TEST   # every point of every test shape, labels and normals with them
    assert all(d.y.shape[0] == d.pos.shape[0] == d.norm.shape[0] for d in te.items)
    assert [d.pos.shape[0] for d in tr.items] == [NUM_POINTS] * 3 and tr.transform is aug
    example.require_full_resolution([d.pos.shape[0] for d in te.items], NUM_POINTS)
    # and the flag does not disturb a later run without it
    assert [d.pos.shape[0] for d in example.shapenet_sets(root, NUM_POINTS)[1].items] == [NUM_POINTS] * 3


def test_processed_dir_separates_two_preparations_of_one_root(tmp_path):
    import deltaconv_amd.transforms as T
    from deltaconv_amd.datasets import Compose, ShapeNet
    root = make_root(str(tmp_path / "ShapeNet"))
    pre = Compose((T.NormalizeScale(), T.GeodesicFPS(NUM_POINTS)))
    assert [d.pos.shape[0] for d in ShapeNet(root, split="test", pre_transform=pre).items] == [NUM_POINTS] * 3
    # the default cache is keyed by category only: another pre_transform reads what is there
    assert [d.pos.shape[0] for d in ShapeNet(root, split="test", pre_transform=T.NormalizeScale()).items] == [NUM_POINTS] * 3
    full = ShapeNet(root, split="test", pre_transform=T.NormalizeScale(), processed_dir=os.path.join(root, "processed_full"))
    assert [d.pos.shape[0] for d in full.items] == RAW_TEST
    assert sorted(os.listdir(os.path.join(root, "processed_full"))) == sorted(os.listdir(os.path.join(root, "processed")))


def test_a_subsampled_store_is_refused_as_full_resolution(example):
    with pytest.raises(SystemExit, match="exactly 8 points"):
        example.require_full_resolution([8, 8, 8], 8)
    example.require_full_resolution([8, 9, 8], 8)           # one shape of exactly num_points points among others is data, not a cache
    example.require_full_resolution([], 8)
