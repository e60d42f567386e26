"""Device-side training epochs: the captured step (``GraphedTrainStep``) fed in place by a ``DeviceLoader``, the loss of every
step and the training-side metrics -- accuracy, balanced accuracy, for part segmentation the IoU per shape -- kept on the device,
ONE synchronise at the end of the epoch (``DeviceTrainer``).

What it replaces: the reference's training loops (experiments/train_modelnet.py:98-108, train_shapenet.py:101-134) and their
restatements in examples/train_*_like.py -- an eager step of ~124 launches through Python, autograd and ctypes, ``loss.item()``
and an arg-max read back per step (a synchronise each), and for ShapeNet predictions and labels copied to the host per batch
for ``calc_shape_IoU``.  Nothing here is a new kernel: the step is one graph replay, the loss trace a 4-byte copy, the metrics
one eager ``dc_eval_metrics`` launch per step (csrc/eval.hip, the launch of ``DeviceEvaluator``) on the logits of the training
forward, i.e. BEFORE the step's update, as in the reference.

    train = DeviceLoader(DeviceDataset.from_dataset(train_set, device), 32, shuffle=True, drop_last=True, transform=aug, seed=1)
    trainer = DeviceTrainer(model, train, optimizer, task="classification")
    for epoch in range(epochs):
        res = trainer.run_epoch(epoch)          # res["loss"], res["accuracy"], res["balanced_accuracy"], res["losses"], ...
        scheduler.step()

There is no CPU path: the model, the loader and every buffer live on the HIP device.
"""
import numpy as np
import torch

from ._lib import lib
from .evaluate import MAX_CLASSES, part_tables, reduce_metrics
from .graph_step import GraphedTrainStep
from .utils import calc_loss

__all__ = ["DeviceTrainer", "reduce_epoch", "epoch_indices"]


def _plain_ce(out, y):
    return calc_loss(out, y, smoothing=False)


def epoch_indices(loader, epoch=None):
    """Dataset index of the cloud of every result row of `epoch` on the loader's rank, in step order: int64 [steps * batch]."""
    batches = loader.batch_indices(epoch)
    return np.asarray([i for b in batches for i in b], dtype=np.int64)


def reduce_epoch(losses, batch_size, hit, cnt, ignored, iou=None, label=None, indices=None):
    """The host side of an epoch, on numpy arrays: per-step losses (fp32 [steps]) and the integer counts of the metric
    launches -> the result dict of ``DeviceTrainer.run_epoch``.  ``loss`` accumulates ``float(losses[i]) * batch_size`` in
    Python floats in step order and divides by the cloud count -- the examples' ``total += float(loss) * data.num_graphs;
    total / count``; everything else is ``evaluate.reduce_metrics`` (fp64)."""
    losses = np.asarray(losses, dtype=np.float32).reshape(-1)
    steps, bs = int(losses.shape[0]), int(batch_size)
    total, count = 0.0, 0
    for v in losses:
        total += float(v) * bs
        count += bs
    out = dict(loss=total / count if count else float("nan"), losses=losses, steps=steps, clouds=count)
    if indices is not None:
        out["indices"] = np.asarray(indices, dtype=np.int64)
    out.update(reduce_metrics(hit, cnt, ignored, iou, label))
    return out


def _named_state(optimizer):
    """[(parameter, key, tensor)] of every optimizer state tensor, in the order of ``graph_step._optimizer_tensors``."""
    state = optimizer.state
    return [(p, k, v) for g in optimizer.param_groups for p in g["params"] for k, v in state.get(p, {}).items() if torch.is_tensor(v)]


class DeviceTrainer:
    """Whole training epochs on the device.  `loader`: a ``DeviceLoader`` with ``drop_last=True`` over a store of equal-size
    clouds; `task`: "classification" (one label per cloud, the batch scored as one cloud) or "segmentation" (one label per
    point, one workgroup of the metric kernel per cloud, part IoU per shape when the store has categories; `class_choice` picks
    the parts as ``evaluate.part_tables`` / ``DeviceEvaluator`` do).  `loss_fn`: ``utils.calc_loss`` by default, without label
    smoothing for segmentation -- the reference's two uses.  `reducer`, `warmup`: handed to ``GraphedTrainStep``.

    The capture leaves no trace on the training state.  ``GraphedTrainStep``'s warm-up steps are real updates on the sample batch;
    every parameter and buffer of the model (``num_batches_tracked`` included) and every optimizer state tensor is copied aside
    before the capture and copied back IN PLACE after it -- same tensor objects, same addresses, so the graph stays valid; the
    writes bump the tensors' version counters, so the plane and coefficient caches follow.  Where the optimizer had no state
    yet, the state tensors the warm-up created are zeroed in place: a zero ``momentum_buffer`` gives the first update of
    torch's lazily created one, zero counters and moments are Adam's initial state (``deltaconv_amd.optim`` and torch's
    optimizers alike).  ``SGD`` with ``dampening != 0`` and no state raises ``ValueError``: its first update is not the one of a
    zero buffer.  NOTHING ELSE is restored: the offset of torch's device generator moves (the warm-up's Dropout draws), and so
    does whatever else a forward pass of the model changes outside its parameters and buffers.

    Learning rate: a ``deltaconv_amd.optim`` optimizer reads it from device scalars that every replay refreshes, so a scheduler
    step between epochs takes effect.  Any other optimizer has its rates baked into the capture: ``run_epoch`` raises
    ``ValueError`` when a group's rate is no longer the captured one.

    Train mode: a model in eval mode is put in train mode (``model.train()``) for the capture and for every epoch and gets the
    modes of all its modules back afterwards; a model already in train mode is taken as it is, module by module (a Dropout or
    BatchNorm module the caller put in eval mode stays there).  The captured step holds the modes of the capture.

    With a `reducer` the metrics and losses are those of this rank's share (no cross-rank reduction)."""

    def __init__(self, model, loader, optimizer, task="classification", loss_fn=None, class_choice=None, reducer=None, warmup=3):
        if task not in ("segmentation", "classification"):
            raise ValueError(f"DeviceTrainer: task must be 'segmentation' or 'classification', got {task!r}")
        if not loader.drop_last:
            raise ValueError("DeviceTrainer: the loader must have drop_last=True (the captured step replays one batch shape; a "
                             "short last batch has no place in it)")
        if len(loader) == 0:
            raise ValueError(f"DeviceTrainer: the loader has no full batch ({loader.share} clouds on this rank, batch_size "
                             f"{loader.batch_size})")
        store = loader.store
        if not np.all(store.sizes == store.sizes[0]):
            raise ValueError("DeviceTrainer: the clouds of the store must all have the same size (any cloud can land in any slot "
                             f"of the captured batch, which holds its cloud offsets); sizes range {int(store.sizes.min())} .. "
                             f"{int(store.sizes.max())}")
        self.seg = task == "segmentation"
        if self.seg and store.y_point is None:
            raise ValueError("DeviceTrainer: segmentation needs a store with one label per point")
        if not self.seg and store.y_cloud is None:
            raise ValueError("DeviceTrainer: classification needs a store with one label per cloud")
        if optimizer is None:
            raise ValueError("DeviceTrainer: an optimizer is required (its update is part of the captured step)")
        had_state = bool(_named_state(optimizer))
        if not had_state and isinstance(optimizer, torch.optim.SGD) and any(g.get("dampening", 0) != 0 for g in optimizer.param_groups):
            raise ValueError("DeviceTrainer: SGD with dampening != 0 and no state yet -- its first update (buf = grad) is not the "
                             "update of a zero momentum buffer, which is what the capture's warm-up would leave behind; run one "
                             "step first or use dampening=0")
        self.model, self.loader, self.store, self.optimizer, self.task = model, loader, store, optimizer, task
        self.loss_fn = loss_fn if loss_fn is not None else (_plain_ce if self.seg else calc_loss)
        self.batch_size, self.steps = loader.batch_size, len(loader)
        dev = store.device
        self.has_parts = self.seg and store.category is not None
        if self.has_parts:
            first = int(store.category[0].argmax()) if class_choice else None      # one host read, here and never again
            start, count = part_tables(class_choice, first)
            if store.category.shape[1] > len(start):
                raise ValueError(f"DeviceTrainer: {store.category.shape[1]} categories, the part tables hold {len(start)}")
            self.part_start = torch.tensor(start, dtype=torch.int32).to(dev)
            self.part_count = torch.tensor(count, dtype=torch.int32).to(dev)
        self._cls_ptr = None if self.seg else torch.tensor([0, self.batch_size], dtype=torch.int32).to(dev)
        self.losses = self.hit = self.cnt = self.ignored = self.iou = None
        self._rows = None

        modes = self._enter_train()
        try:
            saved = self._snapshot()
            self.step = GraphedTrainStep(model, self.loss_fn, loader.static_batch(), optimizer=optimizer, warmup=warmup,
                                         reducer=reducer)
            self._restore(saved)
        finally:
            self._leave_train(modes)
        # rates a replay cannot follow: those of an optimizer without device learning-rate scalars
        self._baked_lr = None if hasattr(optimizer, "sync_lr") else [g["lr"] for g in optimizer.param_groups]

    # ---- train mode ---------------------------------------------------------------------------------------------------------
    def _enter_train(self):
        modes = [(m, m.training) for m in self.model.modules()]
        if not self.model.training:
            self.model.train()
        return modes

    @staticmethod
    def _leave_train(modes):
        for m, was in modes:
            m.training = was

    # ---- the capture leaves no trace ----------------------------------------------------------------------------------------
    def _model_tensors(self):
        return list(self.model.parameters()) + list(self.model.buffers())

    @torch.no_grad()
    def _snapshot(self):
        return ([t.detach().clone() for t in self._model_tensors()],
                {(id(p), k): v.detach().clone() for p, k, v in _named_state(self.optimizer)})

    @torch.no_grad()
    def _restore(self, saved):
        tensors, state = saved
        for t, old in zip(self._model_tensors(), tensors):
            t.copy_(old)
        for p, k, v in _named_state(self.optimizer):
            old = state.get((id(p), k))
            if old is None:
                v.zero_()                       # created by the warm-up: the initial state is zero
            else:
                v.copy_(old)                    # (a counter shared by the parameters of a group gets the same value from each)

    # ---- buffers, made at the first epoch (the class count is the width of the logits) ----------------------------------------
    def _alloc(self):
        logits = self.step.out
        if logits.dim() != 2 or logits.dtype != torch.float32 or logits.stride(1) != 1:
            raise TypeError("DeviceTrainer: the model must return contiguous fp32 logits [rows, classes]")
        P, B, S = int(logits.shape[1]), self.batch_size, self.steps
        if not 1 <= P <= MAX_CLASSES:
            raise ValueError(f"DeviceTrainer: {P} classes, dc_eval_metrics takes 1 .. {MAX_CLASSES}")
        want = int(self.store.sizes[0]) * B if self.seg else B
        if logits.shape[0] != want:
            raise ValueError(f"DeviceTrainer: {logits.shape[0]} rows of logits for {want} labels -- one row per point "
                             "(segmentation) / per cloud (classification)")
        dev = self.store.device
        groups = S * B if self.seg else S                       # one row of counts per workgroup of the metric kernel
        self.P = P
        self.losses = torch.zeros(S, dtype=torch.float32, device=dev)
        self.hit = torch.zeros(groups, P, dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(groups, P, dtype=torch.int32, device=dev)
        self.ignored = torch.zeros(groups, dtype=torch.int32, device=dev)
        self.iou = torch.zeros(groups, dtype=torch.float64, device=dev) if self.has_parts else None
        per = B if self.seg else 1
        cut = lambda t, i: None if t is None else t[i * per:(i + 1) * per]
        # the views of step i, made once: no slicing between the replays
        self._rows = [(self.losses[i], cut(self.iou, i), cut(self.hit, i), cut(self.cnt, i), cut(self.ignored, i)) for i in range(S)]

    def _metrics(self, i):
        """One launch on the logits the replay left in ``step.out``, into the rows of step i."""
        s, logits = self.step.static, self.step.out
        _, iou, hit, cnt, ignored = self._rows[i]
        if self.seg:
            cat = s.category if self.has_parts else None
            lib.call("dc_eval_metrics", logits, logits.stride(0), None, s.y, s.ptr, self.batch_size, logits.shape[0], self.P, cat,
                     0 if cat is None else cat.shape[1], self.part_start if self.has_parts else None,
                     self.part_count if self.has_parts else None, None, iou, hit, cnt, ignored)
        else:
            lib.call("dc_eval_metrics", logits, logits.stride(0), None, s.y, self._cls_ptr, 1, self.batch_size, self.P, None, 0,
                     None, None, None, None, hit, cnt, ignored)

    def run_epoch(self, epoch=None):
        """One epoch of the loader (``loader.set_epoch(epoch)`` first when `epoch` is given; otherwise its current one) through
        the captured step.  No host read inside the loop, one synchronise at the end.  Returns ``loss`` (the mean over the
        clouds, accumulated as the examples do), ``losses`` (numpy fp32, one per step), ``steps``, ``clouds``, ``indices`` (the
        dataset index of every result row's cloud, step by step), ``accuracy``, ``balanced_accuracy``, ``ignored`` (rows whose
        label lies outside the classes) and, for a segmentation store with categories, ``mean_iou``, ``ious`` and ``label``
        (per cloud, in the order of ``indices``)."""
        if self._baked_lr is not None:
            now = [g["lr"] for g in self.optimizer.param_groups]
            if len(now) != len(self._baked_lr) or any(float(a) != float(b) for a, b in zip(now, self._baked_lr)):
                raise ValueError(f"DeviceTrainer: the learning rates changed since the capture ({self._baked_lr} -> {now}) and "
                                 f"{type(self.optimizer).__name__} has them baked into the captured update; use a "
                                 "deltaconv_amd.optim optimizer (device learning-rate scalars) or build a new DeviceTrainer")
        loader, step = self.loader, self.step
        if epoch is not None:
            loader.set_epoch(epoch)
        epoch = loader.epoch
        modes = self._enter_train()
        try:
            if self.losses is None:
                self._alloc()
            for t in (self.losses, self.hit, self.cnt, self.ignored, self.iou):
                if t is not None:
                    t.zero_()
            with torch.no_grad():
                for i, _ in enumerate(loader.into(step.static)):
                    self._rows[i][0].copy_(step())
                    self._metrics(i)
        finally:
            self._leave_train(modes)
        return self._results(epoch)

    def _results(self, epoch):
        """The one synchronise of the epoch: the result tensors to the host, reduced there."""
        indices = epoch_indices(self.loader, epoch)
        label = None
        if self.has_parts:
            label = self.store.category[torch.from_numpy(indices).to(self.store.device)].max(dim=1)[1]
        torch.cuda.synchronize(self.store.device)
        pull = lambda t: None if t is None else t.cpu().numpy()
        return reduce_epoch(pull(self.losses), self.batch_size, pull(self.hit), pull(self.cnt), pull(self.ignored), pull(self.iou),
                            pull(label), indices)

    # ---- stop and resume ----------------------------------------------------------------------------------------------------
    def _loader_settings(self):
        ld = self.loader
        return dict(seed=ld.seed, shuffle=bool(ld.shuffle), batch_size=ld.batch_size, rank=ld.rank, world=ld.world)

    def state_dict(self):
        """Everything an epoch depends on besides the scheduler (the caller's): copies of the model's and the optimizer's
        ``state_dict``, the loader's next epoch and its settings, the process seed (``torch.initial_seed()``: the key of the
        row-block dropout streams) and the device generator's state."""
        copy = lambda v: v.detach().clone() if torch.is_tensor(v) else v
        opt = self.optimizer.state_dict()
        opt = dict(state={i: {k: copy(v) for k, v in st.items()} for i, st in opt["state"].items()},
                   param_groups=[dict(g, params=list(g["params"])) for g in opt["param_groups"]])
        return dict(model={k: copy(v) for k, v in self.model.state_dict().items()}, optimizer=opt, epoch=int(self.loader.epoch),
                    loader=self._loader_settings(), initial_seed=int(torch.initial_seed()),
                    cuda_rng_state=torch.cuda.get_rng_state(self.store.device))

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Continue from ``state_dict()`` of another trainer: model and optimizer state VALUES copied in place into the tensors
        the captured step holds (``optimizer.load_state_dict`` would replace them, and ``GraphedTrainStep`` then refuses to
        replay), the groups' hyper-parameters taken from `sd`, the loader's epoch set, the device generator's state restored.
        Raises ``ValueError`` when the loader's settings or the process seed are not the saved ones."""
        mine = self._loader_settings()
        if dict(sd["loader"]) != mine:
            raise ValueError(f"DeviceTrainer.load_state_dict: saved with loader settings {dict(sd['loader'])}, this loader has {mine}")
        if int(sd["initial_seed"]) != int(torch.initial_seed()):
            raise ValueError(f"DeviceTrainer.load_state_dict: saved under torch.manual_seed({int(sd['initial_seed'])}), this process "
                             f"runs under {int(torch.initial_seed())} (the dropout streams are keyed by it)")
        own = self.model.state_dict()
        if set(own) != set(sd["model"]):
            raise ValueError("DeviceTrainer.load_state_dict: the model's keys differ from the saved ones: "
                             f"{sorted(set(own) ^ set(sd['model']))[:6]}")
        opt, saved = self.optimizer, sd["optimizer"]
        groups = saved["param_groups"]
        if len(groups) != len(opt.param_groups) or any(len(g["params"]) != len(h["params"]) for g, h in zip(groups, opt.param_groups)):
            raise ValueError("DeviceTrainer.load_state_dict: the optimizer's parameter groups differ from the saved ones")
        by_index = {i: p for g, h in zip(groups, opt.param_groups) for i, p in zip(g["params"], h["params"])}
        for i, st in saved["state"].items():                    # checked before anything is written
            cur = opt.state.get(by_index[i], {})
            for k, v in st.items():
                if torch.is_tensor(v) and not torch.is_tensor(cur.get(k)):
                    raise ValueError(f"DeviceTrainer.load_state_dict: saved optimizer state {k!r} of parameter {i} has no captured "
                                     "tensor to land in")
        for k, t in own.items():
            t.copy_(sd["model"][k])
        index_of = {id(p): i for i, p in by_index.items()}
        for p, k, v in _named_state(opt):
            old = saved["state"].get(index_of[id(p)], {}).get(k)
            if old is None:
                v.zero_()                       # saved before that state existed: its initial value
            else:
                v.copy_(old)
        for i, st in saved["state"].items():
            for k, v in st.items():
                if not torch.is_tensor(v):
                    opt.state[by_index[i]][k] = v
        for g, h in zip(groups, opt.param_groups):
            h.update({k: v for k, v in g.items() if k != "params"})
        self.loader.set_epoch(int(sd["epoch"]))
        torch.cuda.set_rng_state(sd["cuda_rng_state"].cpu(), self.store.device)
