"""``DeviceTrainer`` on the MI355X (deltaconv_amd/train.py): whole epochs through the captured step with the loss trace and the
metrics kept on the device -- the same trajectory as a ``GraphedTrainStep`` driven by hand, a capture that leaves parameters,
buffers and optimizer state where they were, the part IoU of the training forward against ``utils.calc_shape_IoU``, stop and
resume, and the refusals.

``torch.nn.Dropout`` modules are in eval mode everywhere (the trainer takes a model in train mode module by module), so no
bit equality hinges on a random stream.  Shapes: clouds of 128 points, 8 or 16 clouds, batches of 4, conv_channels [16, 32],
8 neighbours -- two to four steps an epoch."""
import numpy as np
import pytest
import torch

import deltaconv_amd as dc
from deltaconv_amd.evaluate import part_tables
from deltaconv_amd.graph_step import GraphedTrainStep
from deltaconv_amd.loader import DeviceDataset, DeviceLoader
from deltaconv_amd.utils import calc_loss, calc_shape_IoU
from tests import batch_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
POINTS, BATCH, CLASSES = 128, 4, 10


def _train_mode(model):
    model.train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.eval()
    return model


def _cls_model(burn=0):
    torch.manual_seed(8)
    torch.randn(burn)                                   # other initial weights under the same process seed
    return _train_mode(dc.models.DeltaNetClassification(in_channels=3, num_classes=CLASSES, conv_channels=[16, 32],
                                                        num_neighbors=8).to(DEV))


def _seg_model(burn=0, categories=True):
    torch.manual_seed(7)
    torch.randn(burn)
    return _train_mode(dc.models.DeltaNetSegmentation(in_channels=3, num_classes=50, conv_channels=[16, 32], mlp_depth=1,
                                                      embedding_size=64, num_neighbors=8, categorical_vector=categories).to(DEV))


def _cls_items(n=16, sizes=POINTS):
    items = R.make_items(n, sizes)
    for i, d in enumerate(items):
        d.y = torch.tensor([(7 * i) % CLASSES])
    return items


def _seg_items(n=8, categories=True):
    start, count = part_tables()
    items = R.make_items(n, POINTS)
    g = torch.Generator().manual_seed(6)
    for i, d in enumerate(items):
        k = (3 * i) % 16
        if categories:
            d.category = torch.zeros(1, 16)
            d.category[0, k] = 1
        d.y = torch.randint(start[k], start[k] + count[k], (POINTS,), generator=g)
    return items


_STORES = {}


def _store(kind):
    """The stores, made once, shared, left unchanged."""
    if kind not in _STORES:
        _STORES[kind] = DeviceDataset.from_dataset({"cls": _cls_items, "seg": _seg_items,
                                                    "seg_plain": lambda: _seg_items(categories=False)}[kind](), DEV)
    return _STORES[kind]


def _cls_loader(seed=2, **kw):
    kw = dict(dict(shuffle=True, drop_last=True, transform=R.RECIPES["modelnet"](), seed=seed), **kw)
    return DeviceLoader(_store("cls"), BATCH, **kw)


def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _copy_state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# ---- 1. the same trajectory as the step driven by hand ----------------------------------------------------------------------------
def test_same_trajectory_as_the_step_driven_by_hand():
    def parts():
        model = _cls_model()
        opt = dc.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        return model, opt, torch.optim.lr_scheduler.StepLR(opt, 1, gamma=0.5), _cls_loader()

    # leg A: the trainer
    model, opt, sched, loader = parts()
    trainer = dc.DeviceTrainer(model, loader, opt, task="classification", warmup=2)
    res = [trainer.run_epoch(0)]
    sched.step()
    res.append(trainer.run_epoch(1))
    final_a = _copy_state(model)
    assert model.training and loader.epoch == 2

    # leg B: a bare step; the test undoes the warm-up itself
    model, opt, sched, loader = parts()
    init = _copy_state(model)
    step = GraphedTrainStep(model, calc_loss, loader.static_batch(), optimizer=opt, warmup=2)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(init[k])
        for st in opt.state.values():
            st["momentum_buffer"].zero_()
    losses, preds = [[], []], [[], []]
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        for _ in loader.into(step.static):
            step()
            losses[epoch].append(step.loss.clone())
            preds[epoch].append(step.out.argmax(1))
        if epoch == 0:
            sched.step()
    _same_state(final_a, model.state_dict())

    y_all = _store("cls").y_cloud.cpu().numpy()
    for epoch in (0, 1):
        got = res[epoch]
        want = torch.stack(losses[epoch]).cpu().numpy()
        assert got["losses"].dtype == np.float32 and got["losses"].shape == (4,)
        assert np.array_equal(got["losses"].view(np.uint32), want.view(np.uint32)), (epoch, got["losses"], want)
        assert len(set(want.tolist())) == 4                                 # four different steps
        total, count = 0.0, 0
        for v in want:
            total += float(v) * BATCH
            count += BATCH
        assert got["loss"] == total / count and got["steps"] == 4 and got["clouds"] == 16
        indices = np.concatenate(loader.batch_indices(epoch))
        assert np.array_equal(got["indices"], indices) and sorted(indices.tolist()) == list(range(16))
        pred, true = torch.cat(preds[epoch]).cpu().numpy(), y_all[indices]
        assert got["accuracy"] == float(np.float64(int((pred == true).sum())) / np.float64(16))
        hit, cnt = (np.bincount(v, minlength=CLASSES) for v in (true[pred == true], true))
        seen = cnt > 0
        print(f"epoch {epoch}: loss {got['loss']!r} accuracy {got['accuracy']!r} balanced {got['balanced_accuracy']!r}")
        assert got["balanced_accuracy"] == float(np.mean(hit[seen] / cnt[seen])) and got["ignored"] == 0
        assert "mean_iou" not in got
    assert not np.array_equal(res[0]["indices"], res[1]["indices"])         # the epochs shuffle differently


# ---- 2. the capture leaves no trace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["SGD", "Adam"])
def test_the_capture_leaves_no_trace(which):
    model = _cls_model()
    if which == "SGD":
        opt = dc.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    else:
        opt = dc.optim.Adam(model.parameters(), lr=1e-3)
    before = _copy_state(model)
    assert any(k.endswith("num_batches_tracked") for k in before)
    tensors = {k: v for k, v in model.state_dict().items()}
    trainer = dc.DeviceTrainer(model, _cls_loader(), opt, warmup=3)
    after = model.state_dict()
    _same_state(before, after)
    assert all(after[k] is tensors[k] or after[k].data_ptr() == tensors[k].data_ptr() for k in tensors)     # in place
    state = [v for st in opt.state.values() for v in st.values() if torch.is_tensor(v)]
    assert len(state) >= len(opt.state) > 0                                 # the warm-up created it ...
    assert all(not bool(v.count_nonzero()) for v in state)                  # ... and it is the initial state again
    assert model.training and trainer.step is not None


def test_sgd_with_dampening_and_no_state_is_refused():
    model = _cls_model()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, dampening=0.1)
    before = _copy_state(model)
    with pytest.raises(ValueError, match="dampening"):
        dc.DeviceTrainer(model, _cls_loader(), opt)
    _same_state(before, model.state_dict())                                 # refused before anything ran
    assert not opt.state


# ---- 3. segmentation with categories ---------------------------------------------------------------------------------------------------
def test_segmentation_part_iou_of_the_training_forward():
    items = _seg_items()
    items[5].y = items[5].y.clone()
    items[5].y[17] = 50                                                      # one label outside the 50 classes
    store = DeviceDataset.from_dataset(items, DEV)
    loader = DeviceLoader(store, BATCH, shuffle=True, drop_last=True, transform=R.RECIPES["shapenet"](), seed=4)
    model = _seg_model()
    opt = dc.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    # (the loss kernel answers a label outside the classes with NaN: this loss clamps it, the metrics see the label as stored)
    trainer = dc.DeviceTrainer(model, loader, opt, task="segmentation", warmup=2,
                               loss_fn=lambda out, y: calc_loss(out, y.clamp(0, 49), smoothing=False))
    seen, launch = [], trainer._metrics

    def spy(i):                                                             # what the metric launch of step i reads
        s = trainer.step.static
        seen.append((trainer.step.out.argmax(1), s.y.clone(), s.category.argmax(1)))
        launch(i)
    trainer._metrics = spy
    got = trainer.run_epoch(0)
    assert len(seen) == 2 and np.all(np.isfinite(got["losses"]))
    pred, true = (torch.cat([s[j] for s in seen]).cpu().numpy().reshape(8, POINTS) for j in (0, 1))
    label = torch.cat([s[2] for s in seen]).cpu().numpy()
    indices = np.concatenate(loader.batch_indices(0))
    assert np.array_equal(got["indices"], indices)
    assert np.array_equal(got["label"], label) and np.array_equal(label, (3 * indices) % 16)
    want = calc_shape_IoU(pred, true, label, None)
    print("ious", got["ious"], "reference", [float(v) for v in want])
    assert got["ious"] == [float(v) for v in want]
    assert got["mean_iou"] == float(np.mean(want))
    assert got["ignored"] == 1 and int((true == 50).sum()) == 1
    assert got["accuracy"] == float(np.float64(int((pred == true).sum())) / np.float64(8 * POINTS))
    ok = true < 50
    hit, cnt = (np.bincount(v, minlength=50) for v in (true[ok & (pred == true)], true[ok]))
    assert got["balanced_accuracy"] == float(np.mean(hit[cnt > 0] / cnt[cnt > 0]))


# ---- 4. stop and resume ------------------------------------------------------------------------------------------------------------------
def test_resume_continues_bit_for_bit():
    store = _store("seg_plain")                                              # no categories: default loss, no IoU

    def parts(burn=0):
        model = _seg_model(burn, categories=False)
        opt = dc.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        loader = DeviceLoader(store, BATCH, shuffle=True, drop_last=True, transform=R.RECIPES["shapenet"](), seed=4)
        return model, dc.DeviceTrainer(model, loader, opt, task="segmentation", warmup=2)

    model, straight = parts()
    for epoch in range(3):
        want = straight.run_epoch(epoch)
    assert "mean_iou" not in want and want["steps"] == 2
    final = _copy_state(model)

    _, first = parts()
    for epoch in range(2):
        first.run_epoch(epoch)
    sd = first.state_dict()
    assert sd["epoch"] == 2 and sd["loader"] == dict(seed=4, shuffle=True, batch_size=BATCH, rank=0, world=1)
    assert sd["initial_seed"] == torch.initial_seed() and sd["cuda_rng_state"].dtype == torch.uint8
    first.run_epoch(2)                                                       # moves on: the saved copy must not follow
    fresh, second = parts(burn=5)
    assert not torch.equal(next(iter(fresh.parameters())), next(iter(model.parameters())))
    mine = second.loader
    second.loader = DeviceLoader(store, BATCH, shuffle=True, drop_last=True, transform=R.RECIPES["shapenet"](), seed=5)
    with pytest.raises(ValueError, match="loader settings"):
        second.load_state_dict(sd)
    second.loader = mine
    second.load_state_dict(sd)
    assert mine.epoch == 2
    got = second.run_epoch()                                                 # the loader's own epoch: 2
    assert np.array_equal(got["indices"], want["indices"])
    assert np.array_equal(got["losses"].view(np.uint32), want["losses"].view(np.uint32)), (got["losses"], want["losses"])
    assert got["accuracy"] == want["accuracy"]
    _same_state(final, fresh.state_dict())


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    model = _cls_model()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    with pytest.raises(ValueError, match="drop_last"):
        dc.DeviceTrainer(model, _cls_loader(drop_last=False), opt)
    ragged = DeviceDataset.from_dataset(_cls_items(8, [POINTS] * 7 + [POINTS - 1]), DEV)
    with pytest.raises(ValueError, match="same size"):
        dc.DeviceTrainer(model, DeviceLoader(ragged, BATCH, drop_last=True), opt)
    with pytest.raises(ValueError, match="one label per point"):
        dc.DeviceTrainer(model, _cls_loader(), opt, task="segmentation")
    with pytest.raises(ValueError, match="one label per cloud"):
        dc.DeviceTrainer(model, DeviceLoader(_store("seg"), BATCH, drop_last=True), opt, task="classification")
    with pytest.raises(ValueError, match="no full batch"):
        dc.DeviceTrainer(model, DeviceLoader(_store("cls"), 32, drop_last=True), opt)
    with pytest.raises(ValueError, match="task must be"):
        dc.DeviceTrainer(model, _cls_loader(), opt, task="regression")
    assert not opt.state                                                     # none of them ran a step
    # a torch optimizer has its learning rate baked into the capture
    trainer = dc.DeviceTrainer(model, _cls_loader(), opt, warmup=2)
    first = trainer.run_epoch(0)
    assert first["steps"] == 4 and np.all(np.isfinite(first["losses"]))
    opt.param_groups[0]["lr"] = 0.025
    keep = _copy_state(model)
    with pytest.raises(ValueError, match="learning rates changed"):
        trainer.run_epoch(1)
    _same_state(keep, model.state_dict())
