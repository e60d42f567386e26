"""Device-side evaluation: the eval-mode forward captured once in a HIP graph (``GraphedEvalStep``) and the metrics of a
whole test pass -- vote sum, arg-max, per-class counts, part IoU per shape -- from ONE kernel launch per batch
(csrc/eval.hip: ``dc_eval_metrics``), with a single synchronise at the end of the pass (``DeviceEvaluator``).

What it replaces: the reference's test loops (experiments/utils.py:27-51, test_shapenet.py:71-112, the ``test`` functions
of train_modelnet.py / train_shapenet.py) -- an eager forward of a couple of hundred launches per batch, logits and labels
copied to the host per batch (a synchronise each), a Python loop over shapes and parts in numpy, and for multi-vote
testing ``[votes x shapes x points x 50]`` logits on the host.  The host forms stay where they were
(``utils.evaluate_votes``, ``utils.calc_shape_IoU``); they are the reference the device form is tested against.

    test = DeviceLoader(DeviceDataset.from_dataset(test_set, device), 16,
                        transform=[T.RandomScale((2 / 3, 3 / 2)), T.RandomTranslateGlobal(0.2)], seed=1)
    result = DeviceEvaluator(model, test, task="segmentation", num_votes=10).run()
    result["mean_iou"], result["accuracy"], result["balanced_accuracy"]

There is no CPU path: the model, the loader and every buffer live on the HIP device.
"""
import os

import numpy as np
import torch

from . import _ops
from ._lib import lib
from .nn import fused
from .utils import SHAPENET_INDEX_START, SHAPENET_SEG_NUM

__all__ = ["GraphedEvalStep", "DeviceEvaluator", "part_tables", "reduce_metrics", "MAX_CLASSES"]

_FLAG = "DEBUG_CLR_GRAPH_PACKET_CAPTURE"
MAX_CLASSES = 256          # csrc/eval_math.h: MAX_P


def part_tables(class_choice=None, first_label=None):
    """The parts of a shape of category k as ``(part_start[k], part_count[k])``, the way ``utils.calc_shape_IoU`` picks them:
    without ``class_choice`` the category's own range of the 50 ShapeNet part labels; with it (a one-category dataset whose
    labels start at 0) the range ``0 .. seg_num[first_label] - 1`` for EVERY shape, `first_label` being the category of the
    first shape of the set (calc_shape_IoU reads ``label[0]``)."""
    if not class_choice:
        return list(SHAPENET_INDEX_START), list(SHAPENET_SEG_NUM)
    if first_label is None or not 0 <= int(first_label) < len(SHAPENET_SEG_NUM):
        raise ValueError("part_tables: class_choice needs the category of the first shape, in [0, 16)")
    n = len(SHAPENET_SEG_NUM)
    return [0] * n, [SHAPENET_SEG_NUM[int(first_label)]] * n


def reduce_metrics(hit, cnt, ignored, iou=None, label=None):
    """Per-cloud (or per-batch) integer counts -> the scalar keys of ``utils.evaluate_votes``, in fp64 on the host.
    accuracy = hits / all rows (a row with a label outside the classes is a miss, as ``(true == pred).mean()`` has it);
    balanced_accuracy = the mean over the classes with cnt > 0 of hit / cnt."""
    h = np.asarray(hit, dtype=np.int64).sum(axis=0)
    c = np.asarray(cnt, dtype=np.int64).sum(axis=0)
    ign = int(np.asarray(ignored, dtype=np.int64).sum())
    rows = int(c.sum()) + ign
    seen = c > 0
    out = dict(accuracy=float(np.float64(int(h.sum())) / np.float64(rows)) if rows else float("nan"),
               balanced_accuracy=float(np.mean(h[seen] / c[seen])) if seen.any() else float("nan"), ignored=ign)
    if iou is not None:
        ious = [float(v) for v in np.asarray(iou, dtype=np.float64)]
        out.update(ious=ious, mean_iou=float(np.mean(ious)))
        if label is not None:
            out["label"] = np.asarray(label)
    return out


class GraphedEvalStep:
    """The eval-mode, no-grad forward of `model` on a batch of fixed shape, captured once and replayed with one host call.

    A replay uses the model's CURRENT parameters and running statistics, also when a ``GraphedTrainStep`` replay changed
    them through raw pointers: the two caches that are keyed by tensor versions -- the folded BatchNorm coefficients
    (``fused.eval_coeffs``) and the bf16 weight planes -- are invalidated in front of the capture, so ``dc_bn_eval_coeffs``
    and the plane cut (``dc_presplit_weights``) are nodes of the graph and run again in every replay.  The graph holds the
    plane buffers and their tables by raw address: ``planes_snapshot()`` is kept for its lifetime."""

    def __init__(self, model, sample_batch, warmup=1):
        if os.environ.get(_FLAG, "1") != "0":
            raise RuntimeError(f"GraphedEvalStep needs {_FLAG}=0 in the environment before the HIP runtime "
                               "starts (import deltaconv_amd before the first torch.cuda call, or export it)")
        self.model, self.static, self.warmup = model, sample_batch, int(warmup)
        was_training = model.training
        model.eval()
        try:
            self._capture()
        finally:
            model.train(was_training)

    @torch.no_grad()
    def _capture(self):
        if hasattr(self.static, "pos") and hasattr(self.static, "batch"):
            from .models.deltanet_base import _ptr_info
            _ptr_info(self.static)              # cloud offsets of the static batch: a host read, never inside the capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):           # warm-up outside the capture: allocator, and the weights register their planes
            for _ in range(self.warmup):
                self.model(self.static)
            fused.presplit_begin()              # weights registered by the warm-up join the one-launch table the capture cuts from
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        fused.invalidate_eval_coeffs()          # both caches stale: the capture computes coefficients and planes itself
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self.model(self.static).detach()
        torch.cuda.synchronize()
        self._planes_keepalive = fused.planes_snapshot()
        fused.invalidate_eval_coeffs()          # no eager pass may pick up a tensor that only a replay fills

    def load(self, batch):
        """Copy a new batch (same shapes) into the captured inputs: one launch (``dc_copy_many``)."""
        s = self.static
        if batch is s:
            return
        pairs = []
        for name in ("pos", "norm", "x", "y", "category"):
            dst, src = getattr(s, name, None), getattr(batch, name, None)
            if dst is not None:
                assert src is not None and src.shape == dst.shape, f"batch.{name}: static shape {tuple(dst.shape)}"
                pairs.append((src, dst))
        _ops.copy_many(pairs)

    def step(self, batch=None):
        """Load `batch` if given, replay, return the logits (``.out``: the same tensor every time, overwritten by the next
        replay)."""
        if batch is not None:
            self.load(batch)
        self.graph.replay()
        return self.out

    __call__ = step


class DeviceEvaluator:
    """A whole test pass on the device.  `loader`: a ``DeviceLoader`` with ``shuffle=False``; `task`: "segmentation" (labels
    per point, one workgroup of the metric kernel per cloud, part IoU when the store has categories) or "classification"
    (labels per cloud, the batch as one cloud).

    ``run()`` iterates the loader `num_votes` times -- vote v is the loader's next epoch exactly as iterating it would be, so
    its transforms redraw per vote.  Full batches are assembled in place in front of a ``GraphedEvalStep`` replay
    (``graphed=True``; needs equal-size clouds), a shorter last batch runs eagerly, both through ``dc_eval_metrics``.  With
    ``num_votes > 1`` the logits of the votes are summed in ONE ``[rows of the set, classes]`` fp32 device buffer, in vote
    order like the host's ``acc += stacked`` -- 4 * rows * classes bytes: the ShapeNet test split at 2 048 points and 50 parts
    is 2 874 * 2 048 * 50 * 4 = 1.2 GB.  The metrics of the last vote's launches land in per-cloud rows of dataset-sized
    result tensors; ONE synchronise at the end brings them to the host, where they are reduced in fp64.

    Returns the keys of ``utils.evaluate_votes``: ``accuracy``, ``balanced_accuracy`` (the mean over the classes with
    cnt > 0 of hit / cnt), ``ignored`` (rows whose label lies outside the classes), with categories ``mean_iou``, ``ious``
    and ``label``, with `keep_pred` ``pred`` and ``true`` ([clouds, points] for equal-size clouds, flat otherwise).
    `class_choice` picks the parts as ``calc_shape_IoU`` does (``part_tables``).

    ``propagate_to`` (segmentation only): the store the loader's clouds were sampled from -- a ``DeviceDataset`` with ``y_point``
    or a ``DeviceMeshDataset`` with ``y_vert``, the same clouds in the same order.  The k = ``propagate_k`` nearest sampled points
    of every target row are found once, here (``Propagator``: csrc/interp.hip).  On the LAST vote, after a batch's metric launch,
    the batch's vote sums (one vote: its logits) are interpolated to the target rows of its clouds and scored against the
    target's labels by a second ``dc_eval_metrics`` launch.  ``run()`` then returns the keys above at TARGET resolution plus
    ``"sampled"``: the same keys at the sampled points, exactly what it returns without ``propagate_to`` (with `keep_pred` the
    target-resolution ``pred`` and ``true`` are flat, one entry per target row in store order).  Still one synchronise
    per pass; inference only (no autograd through the interpolation).  ``propagate_to=None``: nothing changes, down to the
    launch list."""

    def __init__(self, model, loader, task="segmentation", num_votes=1, class_choice=None, graphed=True, keep_pred=False,
                 propagate_to=None, propagate_k=3):
        if task not in ("segmentation", "classification"):
            raise ValueError(f"DeviceEvaluator: task must be 'segmentation' or 'classification', got {task!r}")
        if loader.shuffle:
            raise ValueError("DeviceEvaluator: the loader must not shuffle (every vote has to see the clouds in the same rows)")
        if num_votes < 1:
            raise ValueError("DeviceEvaluator: num_votes >= 1")
        store = loader.store
        self.seg = task == "segmentation"
        if self.seg and store.y_point is None:
            raise ValueError("DeviceEvaluator: segmentation needs a store with one label per point")
        if not self.seg and store.y_cloud is None:
            raise ValueError("DeviceEvaluator: classification needs a store with one label per cloud")
        self.model, self.loader, self.store = model, loader, store
        self.num_votes, self.keep_pred = int(num_votes), bool(keep_pred)
        self.share = loader.rank_share(0)                       # shuffle=False: the same clouds in the same order, every epoch
        sizes = store.sizes[self.share] if self.seg else np.ones(len(self.share), dtype=np.int64)
        self.row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)    # first result row of every cloud
        self.sizes = sizes
        bs, n = loader.batch_size, len(self.share)
        self.n_batches = len(loader)
        self.groups = n if self.seg else self.n_batches         # one row of counts per workgroup of the metric kernel
        dev = store.device
        self.has_parts = self.seg and store.category is not None
        if self.has_parts:
            first = None
            if class_choice:
                first = int(store.category[int(self.share[0])].argmax()) if n else 0       # one host read, here and never again
            start, count = part_tables(class_choice, first)
            if store.category.shape[1] > len(start):
                raise ValueError(f"DeviceEvaluator: {store.category.shape[1]} categories, the part tables hold {len(start)}")
            self.part_start = torch.tensor(start, dtype=torch.int32).to(dev)
            self.part_count = torch.tensor(count, dtype=torch.int32).to(dev)
        full = n // bs
        self.step = None
        if graphed and full > 0:
            fs = store.sizes[self.share[:full * bs]].reshape(full, bs)
            if not np.all(fs == fs[0, 0]):       # (ragged clouds inside a batch pool through host-read offsets: not capturable)
                raise ValueError("DeviceEvaluator: graphed=True replays one captured batch shape -- the clouds of the full batches "
                                 "must all have the same cloud sizes; pass graphed=False for ragged sets")
            self.step = GraphedEvalStep(model, loader.static_batch())
        self._cls_ptr = {}
        self.hit = self.cnt = self.ignored = self.iou = self.pred = self.votes = None
        self.prop = self.full = None
        if propagate_to is not None:
            from .propagate import Propagator, target_view
            if not self.seg:
                raise ValueError("DeviceEvaluator: propagate_to is for segmentation (labels per point)")
            if loader.world != 1:
                raise ValueError("DeviceEvaluator: propagate_to needs the whole set on one rank (a batch is a contiguous range of "
                                 "the store's clouds)")
            self.full_y = target_view(propagate_to)[3]
            if self.full_y is None:
                raise ValueError("DeviceEvaluator: propagate_to must carry one label per point (y_point) or per vertex (y_vert)")
            self.prop = Propagator(store, propagate_to, k=propagate_k)

    # ---- buffers, made at the first batch (the class count is the width of the logits) ------------------------------------
    def _alloc(self, P):
        if not 1 <= P <= MAX_CLASSES:
            raise ValueError(f"DeviceEvaluator: {P} classes, dc_eval_metrics takes 1 .. {MAX_CLASSES}")
        dev, rows = self.store.device, int(self.row_off[-1])
        self.P = P
        self.hit = torch.zeros(self.groups, P, dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(self.groups, P, dtype=torch.int32, device=dev)
        self.ignored = torch.zeros(self.groups, dtype=torch.int32, device=dev)
        self.iou = torch.zeros(self.groups, dtype=torch.float64, device=dev) if self.has_parts else None
        self.pred = torch.zeros(rows, dtype=torch.int64, device=dev) if self.keep_pred else None
        self.votes = torch.zeros(rows, P, dtype=torch.float32, device=dev) if self.num_votes > 1 else None
        if self.prop is not None:                               # the same result rows at target resolution
            trows = int(self.prop.toff[-1])
            self.full = dict(hit=torch.zeros_like(self.hit), cnt=torch.zeros_like(self.cnt), ignored=torch.zeros_like(self.ignored),
                             iou=None if self.iou is None else torch.zeros_like(self.iou),
                             pred=torch.zeros(trows, dtype=torch.int64, device=dev) if self.keep_pred else None)

    def _metrics(self, i, batch, logits, last=False):
        """One launch: batch i of the pass (its clouds start at cloud i * batch_size of the share).  With ``propagate_to``, on the
        last vote, two more: the interpolation to the target rows of the batch's clouds and their metrics."""
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise TypeError("DeviceEvaluator: the model must return fp32 logits [rows, classes]")
        if self.hit is None:
            self._alloc(int(logits.shape[1]))
        P, B = self.P, batch.num_graphs
        assert logits.shape[1] == P
        c0 = i * self.loader.batch_size
        r0, r1 = int(self.row_off[c0]), int(self.row_off[c0 + B])
        assert logits.shape[0] == r1 - r0, "DeviceEvaluator: one row of logits per point (segmentation) / cloud (classification)"
        if logits.stride(1) != 1:
            logits = logits.contiguous()
        votes = None if self.votes is None else self.votes[r0:r1]
        pred = None if self.pred is None else self.pred[r0:r1]
        if self.seg:
            cat = batch.category if self.has_parts else None
            lib.call("dc_eval_metrics", logits, logits.stride(0), votes, batch.y, batch.ptr, B, r1 - r0, P, cat,
                     0 if cat is None else cat.shape[1], self.part_start if self.has_parts else None,
                     self.part_count if self.has_parts else None, pred, None if self.iou is None else self.iou[c0:c0 + B],
                     self.hit[c0:c0 + B], self.cnt[c0:c0 + B], self.ignored[c0:c0 + B])
            if self.prop is not None and last:
                _, _, tptr32, (t0, t1), _ = self.prop.cloud_range((c0, c0 + B))
                if t1 > t0:
                    up = self.prop.apply(logits if votes is None else votes, (c0, c0 + B))
                    f = self.full
                    lib.call("dc_eval_metrics", up, up.stride(0), None, self.full_y[t0:t1], tptr32, B, t1 - t0, P, cat,
                             0 if cat is None else cat.shape[1], self.part_start if self.has_parts else None,
                             self.part_count if self.has_parts else None, None if f["pred"] is None else f["pred"][t0:t1],
                             None if f["iou"] is None else f["iou"][c0:c0 + B], f["hit"][c0:c0 + B], f["cnt"][c0:c0 + B],
                             f["ignored"][c0:c0 + B])
        else:
            ptr = self._cls_ptr.get(B)
            if ptr is None:
                ptr = self._cls_ptr[B] = torch.tensor([0, B], dtype=torch.int32).to(self.store.device)
            lib.call("dc_eval_metrics", logits, logits.stride(0), votes, batch.y, ptr, 1, B, P, None, 0, None, None, pred, None,
                     self.hit[i:i + 1], self.cnt[i:i + 1], self.ignored[i:i + 1])

    @torch.no_grad()
    def run(self):
        model = self.model
        was_training = model.training
        model.eval()
        try:
            if self.votes is not None:
                self.votes.zero_()
            for vote in range(self.num_votes):
                it = self.loader.into(self.step.static, fresh_tail=True) if self.step is not None else iter(self.loader)
                for i, batch in enumerate(it):
                    graphed = self.step is not None and batch is self.step.static
                    self._metrics(i, batch, self.step.step() if graphed else model(batch), last=vote == self.num_votes - 1)
        finally:
            model.train(was_training)
        return self._results()

    def _results(self):
        """The one synchronise of the pass: the result tensors to the host, reduced there in fp64."""
        if self.hit is None:
            raise ValueError("DeviceEvaluator: the loader yields no batch")
        store, label = self.store, None
        share_dev = torch.from_numpy(np.ascontiguousarray(self.share)).to(store.device)
        if self.has_parts:
            label = store.category[share_dev].max(dim=1)[1]
        pull = lambda t: None if t is None else t.cpu().numpy()
        hit, cnt, ign, iou, label = pull(self.hit), pull(self.cnt), pull(self.ignored), pull(self.iou), pull(label)
        out = reduce_metrics(hit, cnt, ign, iou, label)
        if self.full is not None:
            f = self.full
            top = reduce_metrics(pull(f["hit"]), pull(f["cnt"]), pull(f["ignored"]), pull(f["iou"]), label)
            if self.keep_pred:
                top.update(pred=pull(f["pred"]), true=pull(self.full_y))
        if self.keep_pred:
            pred = pull(self.pred)
            if self.seg:
                lo = np.concatenate([[0], np.cumsum(store.sizes)])
                y_all = pull(store.y_point)
                true = np.concatenate([y_all[lo[c]:lo[c + 1]] for c in self.share]) if len(self.share) else y_all[:0]
                if len(self.sizes) and np.all(self.sizes == self.sizes[0]):
                    pred, true = pred.reshape(len(self.sizes), -1), true.reshape(len(self.sizes), -1)
            else:
                true = pull(store.y_cloud[share_dev])
            out.update(pred=pred, true=true)
        if self.full is not None:
            top["sampled"] = out
            return top
        return out
