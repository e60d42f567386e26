"""Device-side evaluation on the MI355X (deltaconv_amd/evaluate.py, csrc/eval.hip: dc_eval_metrics): the metric kernel
against numpy (arg-max and counts exactly, IoU within 1e-12 of ``calc_shape_IoU``), the vote sum bit for bit, the captured
eval forward against the eager one (also after the parameters moved under it), and ``DeviceEvaluator`` against
``utils.evaluate_votes`` iterating an identically configured ``DeviceLoader``.

Status when written: no MI355X slot was available, so NONE of these tests has run on the device yet; what ran is the host
side (tests/test_eval_host.py: the kernel's per-row and per-cloud code built by g++) and the evaluator's bookkeeping against
``evaluate_votes`` with both kernels replaced by numpy stand-ins on the CPU.  The replay == eager comparisons are
``torch.equal`` as the same launches run; should a launch turn out to differ, name it here and bound the difference by the
eager pass's own repeat-to-repeat difference."""
import numpy as np
import pytest
import torch

import deltaconv_amd as dc
import deltaconv_amd.transforms as T
from deltaconv_amd._lib import lib
from deltaconv_amd.evaluate import DeviceEvaluator, GraphedEvalStep, part_tables
from deltaconv_amd.loader import DeviceDataset, DeviceLoader
from deltaconv_amd.utils import calc_loss, calc_shape_IoU, evaluate_votes
from tests import batch_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 5, 63, 64, 65, 256, 257, 700] * 2          # 16 clouds: below / at / above a wave, a slab and several slabs
GUARD = 5


def _guarded(n, dtype, fill):
    """A buffer of n elements followed by GUARD sentinel elements: (the view handed to the kernel, the whole buffer)."""
    whole = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[:n], whole


def _launch(logits, y, ptr, P, votes=None, category=None, want_iou=True):
    B, nt = ptr.numel() - 1, logits.shape[0]
    start, count = part_tables()
    ps, pc = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (start, count))
    bufs = dict(pred=_guarded(nt, torch.int64, -9), iou=_guarded(B, torch.float64, -9.0), hit=_guarded(B * P, torch.int32, -9),
                cnt=_guarded(B * P, torch.int32, -9), ignored=_guarded(B, torch.int32, -9))
    lib.call("dc_eval_metrics", logits, logits.stride(0), votes, y, ptr, B, nt, P, category,
             0 if category is None else category.shape[1], ps if category is not None else None,
             pc if category is not None else None, bufs["pred"][0], bufs["iou"][0] if want_iou else None, bufs["hit"][0],
             bufs["cnt"][0], bufs["ignored"][0])
    torch.cuda.synchronize()
    for name, (view, whole) in bufs.items():
        assert bool((whole[view.numel():] == -9).all()), f"guard elements after {name} were written"
    if not want_iou:
        assert bool((bufs["iou"][1] == -9.0).all())
    out = {k: v[0].cpu().numpy() for k, v in bufs.items()}
    out["hit"], out["cnt"] = out["hit"].reshape(B, P), out["cnt"].reshape(B, P)
    return out


def _case(P, seed, strided):
    rng = np.random.default_rng(seed)
    nt = sum(SIZES)
    logits = rng.integers(0, 3, size=(nt, P)).astype(np.float32)               # three values: ties in almost every row
    logits[rng.integers(0, nt)] = np.nan                                        # one row all NaN
    logits[rng.integers(0, nt), P // 2] = np.nan
    y = rng.integers(0, P, size=nt)
    bad = rng.choice(nt, size=6, replace=False)
    y[bad[:3]], y[bad[3:]] = -1, P                                              # a few labels outside the classes
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    dev_logits = torch.from_numpy(logits).to(DEV)
    if strided:
        wide = torch.full((nt, P + 3), float("inf"), device=DEV)               # the gap holds values that would win
        wide[:, :P] = dev_logits
        dev_logits = wide[:, :P]
        assert dev_logits.stride(0) == P + 3
    return logits, y, ptr, dev_logits, torch.from_numpy(y).to(DEV), torch.from_numpy(ptr).to(DEV)


def _iou_all_classes(pred, y, P):
    per = []
    for k in range(P):
        p, g = pred == k, y == k
        u = np.sum(p | g)
        per.append(1.0 if u == 0 else np.sum(p & g) / float(u))
    return np.mean(per)


# ---- 1. the kernel against numpy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("P", [1, 2, 50, 65, 200])
def test_metrics_kernel_equals_numpy(P, strided):
    logits, y, ptr, d_logits, d_y, d_ptr = _case(P, 10 + P, strided)
    B = len(SIZES)
    cat = None
    if P == 50:                                                                 # the ShapeNet tables, all 16 categories present
        cat = torch.zeros(B, 16, device=DEV)
        cat[torch.arange(B), torch.arange(B) % 16] = 1
    got = _launch(d_logits, d_y, d_ptr, P, category=cat)
    pred = np.argmax(logits, axis=1)
    assert np.array_equal(got["pred"], pred)
    worst = 0.0
    for b in range(B):
        lo, hi = ptr[b], ptr[b + 1]
        yb, pb = y[lo:hi], pred[lo:hi]
        ok = (yb >= 0) & (yb < P)
        assert np.array_equal(got["cnt"][b], np.bincount(yb[ok], minlength=P)), b
        assert np.array_equal(got["hit"][b], np.bincount(yb[ok][pb[ok] == yb[ok]], minlength=P)), b
        assert got["ignored"][b] == np.sum(~ok), b
        want = calc_shape_IoU(pb[None], yb[None], np.array([b % 16]), None)[0] if P == 50 else _iou_all_classes(pb, yb, P)
        worst = max(worst, abs(got["iou"][b] - want))
    print(f"P={P} strided={strided}: worst |iou - reference| = {worst:.3e}")
    assert worst <= 1e-12
    assert int(got["ignored"].sum()) == 6
    if P == 50 and not strided:
        none = _launch(d_logits, d_y, d_ptr, P, category=None)                 # no category: all P classes
        for b in range(B):
            lo, hi = ptr[b], ptr[b + 1]
            assert abs(none["iou"][b] - _iou_all_classes(pred[lo:hi], y[lo:hi], P)) <= 1e-12
        for k in ("pred", "hit", "cnt", "ignored"):
            assert np.array_equal(none[k], got[k])
        skip = _launch(d_logits, d_y, d_ptr, P, category=cat, want_iou=False)  # iou = null: everything else as before
        for k in ("pred", "hit", "cnt", "ignored"):
            assert np.array_equal(skip[k], got[k])


def test_out_of_range_labels_move_nothing_else():
    P = 50
    logits, y, ptr, d_logits, d_y, d_ptr = _case(P, 3, False)
    clean = y.copy()
    bad = np.where((y < 0) | (y >= P))[0]
    got = _launch(d_logits, d_y, d_ptr, P)
    clean[bad] = 0
    ref = _launch(d_logits, torch.from_numpy(clean).to(DEV), d_ptr, P)
    pred = np.argmax(logits, axis=1)
    cloud_of = np.searchsorted(ptr, bad, side="right") - 1
    cnt, hit = ref["cnt"].copy(), ref["hit"].copy()
    for r, b in zip(bad, cloud_of):                                             # take the six rows out of class 0 again
        cnt[b, 0] -= 1
        hit[b, 0] -= int(pred[r] == 0)
    assert np.array_equal(got["cnt"], cnt) and np.array_equal(got["hit"], hit) and np.array_equal(got["pred"], ref["pred"])
    assert np.array_equal(got["ignored"], np.bincount(cloud_of, minlength=len(SIZES))) and int(ref["ignored"].sum()) == 0


def test_classification_is_the_batch_as_one_cloud_and_limits():
    rng = np.random.default_rng(1)
    logits = rng.integers(0, 3, size=(37, 40)).astype(np.float32)
    y = rng.integers(0, 40, size=37)
    ptr = torch.tensor([0, 37], dtype=torch.int32, device=DEV)
    got = _launch(torch.from_numpy(logits).to(DEV), torch.from_numpy(y).to(DEV), ptr, 40, want_iou=False)
    pred = np.argmax(logits, axis=1)
    assert np.array_equal(got["pred"], pred) and np.array_equal(got["cnt"][0], np.bincount(y, minlength=40))
    assert np.array_equal(got["hit"][0], np.bincount(y[pred == y], minlength=40)) and got["ignored"][0] == 0
    # offsets outside [0, Nt] are clamped, an empty cloud counts nothing
    odd = torch.tensor([0, 0, 20, 99], dtype=torch.int32, device=DEV)
    got = _launch(torch.from_numpy(logits).to(DEV), torch.from_numpy(y).to(DEV), odd, 40)
    assert got["cnt"][0].sum() == 0 and got["iou"][0] == 1.0 and got["cnt"][1].sum() == 20 and got["cnt"][2].sum() == 17
    # P above the limit: an error with a message, nothing launched
    big = torch.zeros(4, 257, device=DEV)
    with pytest.raises(RuntimeError, match="supported: 1 .. 256"):
        _launch(big, torch.zeros(4, dtype=torch.int64, device=DEV), torch.tensor([0, 4], dtype=torch.int32, device=DEV), 257)
    _launch(big[:, :256], torch.zeros(4, dtype=torch.int64, device=DEV), torch.tensor([0, 4], dtype=torch.int32, device=DEV), 256)


# ---- 2. votes and determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [50, 200])
def test_votes_are_the_fp32_sum_in_call_order(P):
    nt = sum(SIZES)
    g = torch.Generator().manual_seed(P)
    a, b, c = (torch.randn(nt, P, generator=g).to(DEV) * s for s in (1.0, 1e3, 1e-3))
    _, y, ptr, _, d_y, d_ptr = _case(P, 4, False)
    whole = torch.zeros(nt * P + GUARD, device=DEV)
    whole[nt * P:] = -9
    votes = whole[:nt * P].view(nt, P)
    for t in (a, b, c):
        got = _launch(t, d_y, d_ptr, P, votes=votes)
    assert bool((whole[nt * P:] == -9).all())
    want = a + b + c                                                            # (a + b) + c, one fp32 add per call
    assert torch.equal(votes, want)
    assert np.array_equal(got["pred"], np.argmax(want.cpu().numpy(), axis=1))
    # the counts follow the predictions from the votes, not from the last logits
    pred = got["pred"]
    lo, hi = ptr[7], ptr[8]
    ok = (y[lo:hi] >= 0) & (y[lo:hi] < P)
    assert np.array_equal(got["hit"][7], np.bincount(y[lo:hi][ok][pred[lo:hi][ok] == y[lo:hi][ok]], minlength=P))


def test_two_runs_give_the_same_bits():
    _, _, _, d_logits, d_y, d_ptr = _case(50, 8, False)
    cat = torch.zeros(len(SIZES), 16, device=DEV)
    cat[torch.arange(len(SIZES)), torch.arange(len(SIZES)) % 16] = 1
    one, two = (_launch(d_logits, d_y, d_ptr, 50, category=cat) for _ in range(2))
    for k in one:
        assert np.array_equal(one[k], two[k], equal_nan=True), k


# ---- 3. the captured eval forward -----------------------------------------------------------------------------------------------------
def _seg_items(n_clouds=10, points=256):
    start, count = part_tables()
    items = R.make_items(n_clouds, points)
    g = torch.Generator().manual_seed(6)
    for i, d in enumerate(items):
        k = (3 * i) % 16
        d.category = torch.zeros(1, 16)
        d.category[0, k] = 1
        d.y = torch.randint(start[k], start[k] + count[k], (points,), generator=g)
    return items


def _seg_model():
    torch.manual_seed(7)
    return dc.models.DeltaNetSegmentation(in_channels=3, num_classes=50, conv_channels=[16, 32], mlp_depth=1, embedding_size=64,
                                          num_neighbors=8, categorical_vector=True).to(DEV)


def _cls_model(num_classes=10):
    torch.manual_seed(8)
    return dc.models.DeltaNetClassification(in_channels=3, num_classes=num_classes, conv_channels=[16, 32], num_neighbors=8).to(DEV)


def _eager_eval(model, batch):
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(batch).clone()
    model.train(was)
    return out


@pytest.mark.parametrize("kind", ["segmentation", "classification"])
def test_replay_equals_the_eager_eval_forward_also_after_updates(kind):
    from deltaconv_amd.graph_step import GraphedTrainStep
    seg = kind == "segmentation"
    store = DeviceDataset.from_dataset(_seg_items(8) if seg else R.make_items(8, 256), DEV)
    loader = DeviceLoader(store, 4, drop_last=True)
    model = (_seg_model() if seg else _cls_model(40)).train()
    loss_fn = (lambda o, y: calc_loss(o, y, smoothing=False)) if seg else calc_loss
    step = GraphedEvalStep(model, loader.static_batch())
    assert model.training                                                       # what it was before construction
    other = loader.assemble([4, 5, 6, 7])
    for batch in (step.static, other):
        got = step.step(None if batch is step.static else batch).clone()
        assert got.shape == ((4 * 256, 50) if seg else (4, 40))
        assert torch.equal(got, _eager_eval(model, step.static)), "replay != eager eval forward on the same batch"
    assert model.training
    # an eager optimizer step moves parameters and running statistics (version bumps)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    before = step.out.clone()
    loss_fn(model(step.static), step.static.y).backward()
    opt.step()
    assert torch.equal(step.step().clone(), _eager_eval(model, step.static))
    assert not torch.equal(step.out, before)
    # a captured training step moves them through raw pointers (no version moves): no stale coefficients, no stale planes
    opt.zero_grad(set_to_none=True)
    train = GraphedTrainStep(model, loss_fn, loader.assemble([0, 1, 2, 3]), optimizer=opt, warmup=2)
    before = step.step().clone()
    train()
    assert torch.equal(step.step().clone(), _eager_eval(model, step.static))
    assert not torch.equal(step.out, before)
    train()
    assert torch.equal(_eager_eval(model, step.static), step.step())           # eager first, then the replay
    model.eval()
    assert not GraphedEvalStep(model, step.static, warmup=1).model.training


# ---- 4. the evaluator ----------------------------------------------------------------------------------------------------------------
_AUG = lambda: [T.RandomScale((2 / 3, 3 / 2)), T.RandomTranslateGlobal(0.2)]
_SHARED = {}


def _seg_setup():
    """Model, store and the host reference per vote count: computed once, shared, left unchanged."""
    if not _SHARED:
        store = DeviceDataset.from_dataset(_seg_items(10), DEV)
        model = _seg_model().eval()
        ref = {v: evaluate_votes(model, DeviceLoader(store, 4, transform=_AUG(), seed=3), num_votes=v) for v in (1, 3)}
        _SHARED.update(store=store, model=model, ref=ref)
    return _SHARED["store"], _SHARED["model"], _SHARED["ref"]


@pytest.mark.parametrize("votes", [1, 3])
def test_evaluator_equals_evaluate_votes(votes):
    store, model, ref = _seg_setup()
    want = ref[votes]
    res = {}
    for graphed in (True, False):
        loader = DeviceLoader(store, 4, transform=_AUG(), seed=3)               # two full batches and a short one
        ev = DeviceEvaluator(model, loader, "segmentation", num_votes=votes, graphed=graphed, keep_pred=True)
        assert (ev.step is not None) == graphed
        model.train()
        got = res[graphed] = ev.run()
        assert model.training and loader.epoch == votes                         # vote v was the loader's epoch v
        model.eval()
        for k in ("pred", "true", "label"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, graphed)
        for k in ("accuracy", "balanced_accuracy", "mean_iou"):
            print(f"votes={votes} graphed={graphed} {k}: {got[k]!r} vs {want[k]!r}")
            assert abs(got[k] - want[k]) <= 1e-12, (k, graphed)
        assert np.abs(np.asarray(got["ious"]) - np.asarray(want["ious"])).max() <= 1e-12 and got["ignored"] == 0
    for k in res[True]:
        assert np.array_equal(res[True][k], res[False][k]), f"graphed and eager evaluators differ in {k}"
    # the same evaluator again: the loader moves on to other epochs, the buffers start over
    again = ev.run()
    assert again["pred"].shape == want["pred"].shape and loader.epoch == 2 * votes


def test_evaluator_class_choice_and_refusals():
    store, model, _ = _seg_setup()
    loader = DeviceLoader(store, 4)
    plain = DeviceEvaluator(model, loader, graphed=False, keep_pred=True).run()
    ev = DeviceEvaluator(model, loader, class_choice="Airplane", graphed=False, keep_pred=True)
    got = ev.run()
    assert np.array_equal(got["pred"], plain["pred"])
    want = calc_shape_IoU(got["pred"], got["true"], got["label"], "Airplane")
    assert np.abs(np.asarray(got["ious"]) - np.asarray(want)).max() <= 1e-12
    with pytest.raises(ValueError, match="shuffle"):
        DeviceEvaluator(model, DeviceLoader(store, 4, shuffle=True))
    with pytest.raises(ValueError, match="one label per cloud"):
        DeviceEvaluator(model, loader, task="classification")
    ragged = DeviceDataset.from_dataset(_seg_items(8)[:4] + _seg_items(8, 128)[4:], DEV)
    with pytest.raises(ValueError, match="same cloud sizes"):
        DeviceEvaluator(model, DeviceLoader(ragged, 2), graphed=True)


@pytest.mark.parametrize("votes", [1, 3])
def test_classification_evaluator(votes):
    items = R.make_items(10, 256)
    for i, d in enumerate(items):
        d.y = torch.tensor([(7 * i) % 10])
    store = DeviceDataset.from_dataset(items, DEV)
    model = _cls_model(10).eval()
    mk = lambda: DeviceLoader(store, 4, transform=R.RECIPES["modelnet"](), seed=5)
    acc, loader = None, mk()
    with torch.no_grad():
        for _ in range(votes):
            logits = torch.cat([model(b) for b in loader]).cpu().numpy()
            acc = logits if acc is None else acc + logits
    pred, true = np.argmax(acc, axis=1), np.array([(7 * i) % 10 for i in range(10)])
    want_acc = float((pred == true).mean())
    want_bal = float(np.mean([(pred[true == c] == c).mean() for c in np.unique(true)]))
    out = {}
    for graphed in (True, False):
        got = out[graphed] = DeviceEvaluator(model, mk(), "classification", num_votes=votes, graphed=graphed, keep_pred=True).run()
        assert np.array_equal(got["pred"], pred) and np.array_equal(got["true"], true)
        assert abs(got["accuracy"] - want_acc) <= 1e-12 and abs(got["balanced_accuracy"] - want_bal) <= 1e-12
        assert "mean_iou" not in got and got["ignored"] == 0
    assert all(np.array_equal(out[True][k], out[False][k]) for k in out[True])
