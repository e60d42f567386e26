"""The device-resident loader on the MI355X (deltaconv_amd/loader.py, csrc/batch.hip: dc_batch_assemble): the pure gather
against ``collate`` bit for bit, every augmentation op and the five recipes of the reference's training scripts against the
CPU transform classes in fp64 on the bit-exact restated draws (tests/batch_restate.py), independence of a cloud's rows from
its batch, and in-place assembly in front of a captured training step."""
import numpy as np
import pytest
import torch

import deltaconv_amd.transforms as T
from deltaconv_amd.datasets import Data, collate
from deltaconv_amd.loader import DeviceDataset, DeviceLoader, RandomJitter
from tests import batch_restate as R
from tests.test_loader_host import (STAT_CLOUDS, STAT_SEED, STAT_STEP, STAT_TRANSFORMS, check_draw_statistics)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _equal_to_collate(got, items, idx):
    want = collate([items[i] for i in idx]).to(DEV)
    for name in ("pos", "norm", "x", "y", "batch", "category"):
        g, w = getattr(got, name), getattr(want, name)
        assert (g is None) == (w is None), name
        if w is not None:
            assert g.dtype == w.dtype and torch.equal(g, w), name
    assert got.num_graphs == want.num_graphs == len(idx)
    assert got.ptr.dtype == torch.int32 and torch.equal(got.ptr, want.ptr)
    sizes = [items[i].pos.shape[0] for i in idx]
    info = got._ptr_info
    assert info[0] is got.ptr and tuple(info[1:]) == (len(idx), max(sizes)) and info.min_cloud == min(sizes)


# ---- 1. no transform: the gather is collate, bit for bit -------------------------------------------------------------------
def _dress(items, per_point=False, category=False, x=False):
    g = torch.Generator().manual_seed(3)
    for i, d in enumerate(items):
        n = d.pos.shape[0]
        if per_point:
            d.y = torch.randint(0, 50, (n,), generator=g)
        if category:
            d.category = torch.zeros(1, 16)
            d.category[0, i % 16] = 1
        if x:
            d.x = torch.randn(n, 5, generator=g)
    return items


RAGGED = [300, 1, 1024, 17, 256, 257, 64, 1024, 2, 511, 1, 700]
GATHER_CASES = {
    "equal": lambda: R.make_items(12, 256),
    "ragged": lambda: R.make_items(12, RAGGED),
    "per_point_labels": lambda: _dress(R.make_items(12, RAGGED), per_point=True),
    "category_and_x": lambda: _dress(R.make_items(12, RAGGED), per_point=True, category=True, x=True),
    "no_normals": lambda: R.make_items(12, RAGGED, normals=False),
}


@pytest.mark.parametrize("case", list(GATHER_CASES))
def test_gather_equals_collate(case):
    items = GATHER_CASES[case]()
    store = DeviceDataset.from_dataset(items, DEV)
    assert len(store) == 12 and store.sizes.tolist() == [d.pos.shape[0] for d in items]
    # batch 5 of 12: two full batches and the short last one, shuffled and in order
    for shuffle in (False, True):
        loader = DeviceLoader(store, 5, shuffle=shuffle, seed=4)
        loader.set_epoch(2)
        idx_lists = loader.batch_indices(2)
        assert [len(i) for i in idx_lists] == [5, 5, 2]
        batches = list(loader)
        assert len(batches) == len(loader) == 3
        for got, idx in zip(batches, idx_lists):
            _equal_to_collate(got, items, idx)
    for got, idx in zip(DeviceLoader(store, 1), [[i] for i in range(12)]):           # B = 1, the 1-point clouds included
        _equal_to_collate(got, items, idx)
    whole = list(DeviceLoader(store, 12))                                              # the max-size clouds next to 1-point ones
    assert len(whole) == 1
    _equal_to_collate(whole[0], items, list(range(12)))
    _equal_to_collate(DeviceLoader(store, 4).assemble([7, 7, 1, 10]), items, [7, 7, 1, 10])   # any index list, repeats too


def test_dataset_objects_and_bad_input():
    """``from_dataset`` takes ``ds.items`` without running ``ds.transform``; `normal` is taken as `norm` like collate does."""
    items = R.make_items(6, 64)

    class _DS:
        def __init__(self):
            self.items, self.transform = items, lambda d: 1 / 0

    for d in items:
        d.normal, d.norm = d.norm, None
    store = DeviceDataset.from_dataset(_DS(), DEV)
    _equal_to_collate(next(iter(DeviceLoader(store, 6))), items, list(range(6)))
    with pytest.raises(ValueError, match="empty"):
        DeviceDataset.from_dataset([], DEV)
    with pytest.raises(ValueError, match="one label per cloud or one per point"):
        DeviceDataset.from_dataset([Data(pos=torch.zeros(4, 3), y=torch.zeros(2, dtype=torch.long))], DEV)
    with pytest.raises(ValueError, match="dataset indices"):
        DeviceLoader(store, 2).assemble([6])


# ---- 2. every op alone and the five recipes ------------------------------------------------------------------------------------
ALL = dict(R.SINGLE_OPS, **R.RECIPES)
_ITEMS = {}


def _items(n, normals):
    if (n, normals) not in _ITEMS:
        _ITEMS[(n, normals)] = R.make_items(40, n, normals=normals)
    return _ITEMS[(n, normals)]


# ScanObjectNN ships positions only (experiments/datasets/scanobjectnn.py): its recipe runs on a store without normals too,
# and so do a scale and a rotation alone (the normal part is skipped, as in the CPU classes)
AUG_CASES = [(name, n, True) for name in ALL for n in (1024, 2048)] + \
            [(name, 1024, False) for name in ("scanobjectnn", "scale", "rotate1")]


@pytest.mark.parametrize("name,n,normals", AUG_CASES)
def test_augmentation_matches_cpu_classes_on_restated_draws(name, n, normals):
    """B = 32 clouds of 1024 / 2048 points.  Per tensor |got - expected| <= 64 * 2^-24 * max(1, max |expected|); normals of
    unit length within the same bound.  Largest error observed: 0.081 of the bound (shapeseg recipe) in the g++ build of the
    same per-point code (tests/test_loader_host.py); the device figures are printed per case before the assertion (run with
    -s) and were NOT yet recorded from an MI355X run when this was written."""
    items = _items(n, normals)
    transforms = ALL[name]()
    store = DeviceDataset.from_dataset(items, DEV)
    loader = DeviceLoader(store, 32, shuffle=True, transform=transforms, seed=11)
    epoch = 3
    loader.set_epoch(epoch)
    idx = loader.batch_indices(epoch)[0]
    got = next(iter(loader))
    step = epoch * len(loader) + 0
    assert got.num_graphs == 32 and got.pos.shape == (32 * n, 3)
    pos, nrm = got.pos.double().cpu(), None if got.norm is None else got.norm.double().cpu()
    want = [R.expected(items[i], transforms, 11, step, i) for i in idx]
    want_pos = torch.cat([w[0] for w in want])
    err_p = float((pos - want_pos).abs().max())
    line = f"{name} n={n} normals={normals}: pos err {err_p:.3e} = {err_p / R.bound(want_pos):.3f} of the bound"
    if normals:
        want_nrm = torch.cat([w[1] for w in want])
        err_n = float((nrm - want_nrm).abs().max())
        err_l = float((nrm.norm(dim=1) - 1).abs().max())
        line += f"; norm err {err_n:.3e} = {err_n / R.bound(want_nrm):.3f}, |norm| - 1: {err_l:.3e}"
    print(line)
    assert err_p <= R.bound(want_pos), line
    if normals:
        assert err_n <= R.bound(want_nrm) and err_l <= R.bound(want_nrm), line
    else:
        assert got.norm is None
    # what no op touches is the gather
    assert torch.equal(got.y.cpu(), torch.cat([items[i].y for i in idx]))
    assert torch.equal(got.batch.cpu(), torch.arange(32).repeat_interleave(n))
    assert torch.equal(got.ptr.cpu(), (torch.arange(33) * n).int())


# ---- 3. independence and determinism -------------------------------------------------------------------------------------------
def _rows(batch, slot):
    lo, hi = batch.ptr[slot].item(), batch.ptr[slot + 1].item()
    return batch.pos[lo:hi].clone(), batch.norm[lo:hi].clone()


def test_a_clouds_rows_do_not_depend_on_its_batch():
    items = R.make_items(40, [1024 if i % 3 else 700 for i in range(40)])
    transforms = [T.RandomRotate(360, 1), RandomJitter(0.01), T.RandomScale((4 / 5, 5 / 4)), T.RandomNormals(0.05),
                  T.RandomTranslateGlobal(0.1)]
    store = DeviceDataset.from_dataset(items, DEV)
    loader = DeviceLoader(store, 32, transform=transforms, seed=5)
    c, step = 23, 41
    others = [i for i in range(40) if i != c]
    alone = _rows(loader.assemble([c], step), 0)
    first = _rows(loader.assemble([c] + others[:31], step), 0)
    last = _rows(loader.assemble(others[:31] + [c], step), 31)
    eight = _rows(loader.assemble(others[33:36] + [c] + others[:4], step), 3)
    for other in (first, last, eight):
        assert torch.equal(alone[0], other[0]) and torch.equal(alone[1], other[1])
    # the same (seed, step, idx) twice: the same bits; another step or another seed: other rows
    idx = [c] + others[:31]
    a, b = loader.assemble(idx, step), loader.assemble(idx, step)
    assert torch.equal(a.pos, b.pos) and torch.equal(a.norm, b.norm)
    assert not torch.equal(a.pos, loader.assemble(idx, step + 1).pos)
    assert not torch.equal(a.pos, DeviceLoader(store, 32, transform=transforms, seed=6).assemble(idx, step).pos)


def test_draws_on_the_device_are_the_restated_bits():
    """4096 one-point clouds at one step: a point at (1, 1, 1) scaled IS the factor triple, a point at the origin
    translated IS the offset triple -- bitwise the numpy restatement, which passes the statistics check on the CPU
    (tests/test_loader_host.py: test_restated_draw_statistics); the angle is read back from the rotated (1, 0, 0)."""
    scale, rot, tr = STAT_TRANSFORMS()
    clouds = np.arange(STAT_CLOUDS, dtype=np.uint64)
    idx = list(range(STAT_CLOUDS))

    def run(point, transform, seed=STAT_SEED, step=STAT_STEP):
        items = [Data(pos=torch.tensor([point], dtype=torch.float32)) for _ in range(STAT_CLOUDS)]
        loader = DeviceLoader(DeviceDataset.from_dataset(items, DEV), STAT_CLOUDS, transform=[transform], seed=seed)
        out = loader.assemble(idx, step)
        assert torch.equal(out.ptr.cpu(), torch.arange(STAT_CLOUDS + 1).int())
        return out.pos.cpu().numpy()

    sc = run([1.0, 1.0, 1.0], scale)
    assert np.array_equal(sc.view(np.uint32), R.cloud_draw(scale, STAT_SEED, STAT_STEP, clouds, 0).view(np.uint32))
    off = run([0.0, 0.0, 0.0], tr)
    assert np.array_equal(off.view(np.uint32), R.cloud_draw(tr, STAT_SEED, STAT_STEP, clouds, 0).view(np.uint32))
    xy = run([1.0, 0.0, 0.0], rot).astype(np.float64)              # (1, 0, 0) @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] = (c, s, 0)
    deg = np.degrees(np.arctan2(xy[:, 1], xy[:, 0]))
    assert np.abs(deg - R.cloud_draw(rot, STAT_SEED, STAT_STEP, clouds, 0)).max() < 1e-4
    for a in range(3):
        check_draw_statistics(sc[:, a], np.float32(4 / 5), np.float32(5 / 4))
        check_draw_statistics(off[:, a], -np.float32(0.1 * (a + 1)), np.float32(0.1 * (a + 1)))
    check_draw_statistics(np.clip(deg, 0, 90), 0.0, 90.0)
    # another step, another seed: other parameters for EVERY cloud
    assert not np.any(np.all(run([1.0, 1.0, 1.0], scale, step=STAT_STEP + 1) == sc, axis=1))
    assert not np.any(np.all(run([1.0, 1.0, 1.0], scale, seed=STAT_SEED + 1) == sc, axis=1))


# ---- 4. in front of a captured step ---------------------------------------------------------------------------------------------
def _model():
    import deltaconv_amd as dc
    torch.manual_seed(5)
    m = dc.models.DeltaNetClassification(in_channels=3, num_classes=40, num_neighbors=20, grad_regularizer=1e-3).to(DEV)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    return m


def test_in_place_assembly_feeds_a_captured_step():
    """Three batches through a GraphedTrainStep by ``loader.into(step.static)`` == the same three batches, obtained by
    iterating the loader, handed to ``step(batch)`` (the copy launch of GraphedTrainStep.load): losses and final parameters
    bit for bit, every data_ptr of the static batch unchanged."""
    from deltaconv_amd.graph_step import GraphedTrainStep
    from deltaconv_amd.utils import calc_loss
    items = R.make_items(16, 256)
    store = DeviceDataset.from_dataset(items, DEV)
    recipe = R.RECIPES["modelnet"]

    def run(in_place):
        loader = DeviceLoader(store, 4, shuffle=True, drop_last=True, transform=recipe(), seed=2)
        m = _model().train()
        opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        step = GraphedTrainStep(m, calc_loss, loader.static_batch(), optimizer=opt, warmup=2)
        loader.set_epoch(1)
        losses = []
        if in_place:
            names = ("pos", "norm", "y", "batch", "ptr")
            ptrs = {k: getattr(step.static, k).data_ptr() for k in names}
            for i, b in enumerate(loader.into(step.static)):
                assert b is step.static and {k: getattr(b, k).data_ptr() for k in names} == ptrs
                losses.append(step().clone())
                if i == 2:
                    break
        else:
            for i, b in enumerate(loader):
                assert b is not step.static
                losses.append(step(b).clone())
                if i == 2:
                    break
        return torch.stack(losses), m.state_dict()

    la, sa = run(True)
    lb, sb = run(False)
    assert la.shape == (3,) and torch.equal(la, lb), (la, lb)
    assert len(set(la.tolist())) == 3                                 # three different batches went through
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


def test_into_refuses_other_shapes():
    store = DeviceDataset.from_dataset(R.make_items(10, [256] * 9 + [255]), DEV)
    loader = DeviceLoader(store, 4, drop_last=True)
    static = loader.static_batch()
    assert len(list(loader.into(static))) == 2
    with pytest.raises(ValueError, match="shape of the static batch"):
        list(DeviceLoader(store, 4).into(static))                     # the short last batch
    with pytest.raises(ValueError, match="shape of the static batch"):
        list(DeviceLoader(store, 4, drop_last=True).into(collate(R.make_items(4, 128)).to(DEV)))
    ragged = DeviceDataset.from_dataset(R.make_items(8, [256, 255, 257, 256] * 2), DEV)     # same Nt, other offsets
    with pytest.raises(ValueError, match="cloud sizes"):
        list(DeviceLoader(ragged, 4).into(static))


def test_eval_forward_on_a_loader_batch_equals_collate():
    items = R.make_items(8, [256, 300, 256, 512, 256, 256, 400, 256])
    store = DeviceDataset.from_dataset(items, DEV)
    m = _model().eval()
    with torch.no_grad():
        for got, idx in zip(DeviceLoader(store, 4), ([0, 1, 2, 3], [4, 5, 6, 7])):
            ref = collate([items[i] for i in idx]).to(DEV)
            assert torch.equal(m(got), m(ref))
