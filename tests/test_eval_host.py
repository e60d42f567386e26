"""Host side of the device evaluation (deltaconv_amd/evaluate.py, csrc/eval.hip), without a GPU: a g++ build of
csrc/eval_math.h (tests/hostcheck_eval) -- the row arg-max against ``np.argmax`` (indices equal), the per-cloud counters and
IoU fold against ``utils.calc_shape_IoU`` (<= 1e-12, the bound tests/test_utils.py holds that function to) -- the part-table
translation with and without ``class_choice``, the fp64 reduction of the counts against the formulas of
``utils.evaluate_votes``, and the entry point's argument errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from deltaconv_amd.evaluate import MAX_CLASSES, part_tables, reduce_metrics
from deltaconv_amd.utils import SHAPENET_INDEX_START, SHAPENET_SEG_NUM, calc_shape_IoU
from tests.helpers import ROOT

HE_DIR = os.path.join(ROOT, "tests", "hostcheck_eval")
P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def he():
    subprocess.run(["make", "-s", "-C", HE_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HE_DIR, "libhostcheck_eval.so"))
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    lib.he_argmax.argtypes = [vp, i64, ci, i64, vp]
    lib.he_argmax.restype = None
    lib.he_cloud_iou.argtypes = [vp, vp, i64, ci, ci, ci, vp, vp, vp]
    lib.he_cloud_iou.restype = ctypes.c_double
    lib.he_max_p.restype = ci
    return lib


def _argmax(he, rows, ld=None):
    r, p = rows.shape
    buf = rows
    if ld is not None:                       # rows at a stride, the gap filled with values that would win
        buf = np.full((r, ld), np.inf, dtype=np.float32)
        buf[:, :p] = rows
    buf = np.ascontiguousarray(buf)
    out = np.full(r, -7, dtype=np.int64)
    he.he_argmax(P(buf), r, p, buf.shape[1], P(out))
    return out


# ---- the arg-max rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 2, 3, 50, 65, 256])
def test_argmax_is_numpys_on_ties_nans_and_infinities(he, p):
    rng = np.random.default_rng(p)
    rows = [rng.integers(0, 3, size=(400, p)).astype(np.float32) - 1,          # three values: ties in almost every row
            np.zeros((3, p), dtype=np.float32), np.full((2, p), -np.inf, dtype=np.float32),
            np.full((2, p), np.inf, dtype=np.float32), np.full((2, p), np.nan, dtype=np.float32)]
    special = rng.standard_normal((40, p)).astype(np.float32)
    for i in range(40):                                                         # NaN first / middle / last, +-inf, mixed
        where = [0, p // 2, p - 1, int(rng.integers(0, p))][i % 4]
        kind = (i // 4) % 5
        if kind == 0:
            special[i, where] = np.nan
        elif kind == 1:
            special[i, where] = np.nan
            special[i, int(rng.integers(0, p))] = np.nan                       # two NaNs: the first wins
        elif kind == 2:
            special[i, where] = np.inf
            special[i, int(rng.integers(0, p))] = np.inf
        elif kind == 3:
            special[i, where] = -np.inf
        else:
            special[i, where] = np.nan
            special[i, int(rng.integers(0, p))] = np.inf                       # a NaN beats +inf wherever it stands
    rows = np.concatenate(rows + [special])
    want = np.argmax(rows, axis=1)
    assert np.array_equal(_argmax(he, rows), want)
    assert np.array_equal(_argmax(he, rows, ld=p + 3), want)
    assert np.array_equal(_argmax(he, -rows), np.argmax(-rows, axis=1))


# ---- counters and the IoU fold ------------------------------------------------------------------------------------------------
def _cloud(he, pred, y, p, start, count):
    hit, cnt, ign = np.full(p, -1, dtype=np.int32), np.full(p, -1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
    pred, y = np.ascontiguousarray(pred, dtype=np.int64), np.ascontiguousarray(y, dtype=np.int64)
    iou = he.he_cloud_iou(P(pred), P(y), pred.shape[0], p, start, count, P(hit), P(cnt), P(ign))
    return iou, hit, cnt, int(ign[0])


@pytest.mark.parametrize("cat", range(16))
def test_iou_fold_is_calc_shape_iou(he, cat):
    """Random predictions and labels per category; in half of the shapes one part is in neither (union 0 -> 1), predictions
    stray into other categories' parts as a half-trained network's do."""
    rng = np.random.default_rng(100 + cat)
    start, count = part_tables()
    s0, n = start[cat], count[cat]
    worst = 0.0
    for shape in range(12):
        npts = [1, 7, 300, 2048][shape % 4]
        parts = np.arange(s0, s0 + n)
        if shape % 2 and n > 1:
            parts = np.delete(parts, rng.integers(0, n))                        # a part absent from labels and predictions
        y = rng.choice(parts, size=npts)
        pred = np.where(rng.random(npts) < 0.6, y, rng.choice(parts, size=npts))
        if shape % 3 == 0:
            other = np.setdiff1d(np.arange(50), np.arange(s0, s0 + n))
            stray = rng.random(npts) < 0.1
            pred = np.where(stray, rng.choice(other, size=npts), pred)
        want = calc_shape_IoU(pred[None], y[None], np.array([cat]), None)[0]
        got, hit, cnt, ign = _cloud(he, pred, y, 50, s0, n)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12, (cat, shape, got, want)
        assert ign == 0 and np.array_equal(cnt, np.bincount(y, minlength=50))
        assert np.array_equal(hit, np.bincount(y[pred == y], minlength=50))
    print(f"category {cat}: worst |iou - calc_shape_IoU| = {worst:.3e}")


def test_labels_outside_the_classes_are_ignored_and_index_nothing(he):
    rng = np.random.default_rng(5)
    y = rng.integers(0, 6, size=500)
    pred = rng.integers(0, 6, size=500)
    base = _cloud(he, pred, y, 6, 0, 6)
    bad = y.copy()
    bad[[3, 77, 499]] = [-1, 6, 2 ** 40]
    keep = np.ones(500, dtype=bool)
    keep[[3, 77, 499]] = False
    iou, hit, cnt, ign = _cloud(he, pred, bad, 6, 0, 6)
    assert ign == 3
    assert np.array_equal(cnt, np.bincount(y[keep], minlength=6)) and np.array_equal(hit, np.bincount(y[keep][pred[keep] == y[keep]], minlength=6))
    # the ignored rows still predict something: they stay in the unions, as (pred == part) | (seg == part) has them
    want = np.mean([1.0 if not np.any((pred == k) | (bad == k)) else np.sum((pred == k) & (bad == k)) / np.sum((pred == k) | (bad == k))
                    for k in range(6)])
    assert abs(iou - want) <= 1e-12 and base[3] == 0
    # parts outside [0, P) have an empty union; an empty part list has no mean
    assert _cloud(he, pred, y, 6, 4, 5)[0] == pytest.approx((_cloud(he, pred, y, 6, 4, 2)[0] * 2 + 3) / 5, abs=1e-15)
    assert _cloud(he, pred, y, 6, -2, 2)[0] == 1.0 and _cloud(he, pred, y, 6, 100, 3)[0] == 1.0
    assert np.isnan(_cloud(he, pred, y, 6, 0, 0)[0])


def test_all_classes_fold_without_categories(he):
    """No category: the parts are all P classes (P = 200: numpy sums pairwise, the fold in order -- within 1e-12)."""
    rng = np.random.default_rng(9)
    for p in (1, 2, 50, 200):
        y = rng.integers(0, p, size=3000)
        pred = np.where(rng.random(3000) < 0.5, y, rng.integers(0, p, size=3000))
        want = np.mean([1.0 if not np.any((pred == k) | (y == k)) else np.sum((pred == k) & (y == k)) / float(np.sum((pred == k) | (y == k)))
                        for k in range(p)])
        assert abs(_cloud(he, pred, y, p, 0, p)[0] - want) <= 1e-12


# ---- part tables ------------------------------------------------------------------------------------------------------------------
def test_part_tables_with_and_without_class_choice(he):
    start, count = part_tables()
    assert start == list(SHAPENET_INDEX_START) and count == list(SHAPENET_SEG_NUM) and sum(count) == 50
    assert all(start[k + 1] == start[k] + count[k] for k in range(15))
    assert part_tables(None) == part_tables("") == (start, count)
    rng = np.random.default_rng(2)
    for cat in range(16):
        s, c = part_tables("Chair", cat)
        assert s == [0] * 16 and c == [SHAPENET_SEG_NUM[cat]] * 16
        # a one-category set, labels from 0: calc_shape_IoU reads label[0] for every shape
        n = SHAPENET_SEG_NUM[cat]
        y = rng.integers(0, n, size=(3, 256))
        pred = rng.integers(0, n, size=(3, 256))
        want = calc_shape_IoU(pred, y, np.full(3, cat), "Chair")
        for i in range(3):
            assert abs(_cloud(he, pred[i], y[i], 50, s[cat], c[cat])[0] - want[i]) <= 1e-12
    with pytest.raises(ValueError, match="first shape"):
        part_tables("Chair")
    with pytest.raises(ValueError, match="first shape"):
        part_tables("Chair", 16)


# ---- the reduction of the counts ---------------------------------------------------------------------------------------------------
def test_reduce_metrics_is_the_host_formula():
    rng = np.random.default_rng(4)
    true = rng.integers(0, 50, size=(10, 256))
    true[true == 13] = 12                                                       # a class nobody has
    pred = np.where(rng.random((10, 256)) < 0.7, true, rng.integers(0, 50, size=(10, 256)))
    hit = np.stack([np.bincount(t[p == t], minlength=50) for p, t in zip(pred, true)])
    cnt = np.stack([np.bincount(t, minlength=50) for t in true])
    iou = rng.random(10)
    out = reduce_metrics(hit, cnt, np.zeros(10, dtype=np.int32), iou, np.arange(10))
    ft, fp = true.flatten(), pred.flatten()
    assert out["accuracy"] == float((ft == fp).mean())
    assert abs(out["balanced_accuracy"] - float(np.mean([(fp[ft == c] == c).mean() for c in np.unique(ft)]))) <= 1e-15
    assert out["ious"] == list(iou) and out["mean_iou"] == float(np.mean(list(iou))) and out["ignored"] == 0
    assert np.array_equal(out["label"], np.arange(10))
    # ignored rows are misses in the accuracy and belong to no class
    out2 = reduce_metrics(hit, cnt, np.full(10, 2))
    assert out2["accuracy"] == float(np.float64(hit.sum()) / (cnt.sum() + 20)) and out2["ignored"] == 20
    assert out2["balanced_accuracy"] == out["balanced_accuracy"] and "mean_iou" not in out2


# ---- the entry point, as far as it goes without a device ----------------------------------------------------------------------------
def test_entry_point_argument_errors(he):
    from deltaconv_amd._lib import lib
    assert he.he_max_p() == MAX_CLASSES == 256
    fn = lib.raw("dc_eval_metrics")
    rest = (None, 0) + (None,) * 8                                               # category, Cc, tables, outputs, stream
    assert fn(None, 0, None, None, None, 0, 0, 50, None, 0, None, None, None, None, None, None, None, None) == 0          # B = 0
    rc = fn(None, 0, None, None, None, 1, 0, MAX_CLASSES + 1, None, 0, None, None, None, None, None, None, None, None)
    assert rc == -1 and "257" in lib.last_error() and "256" in lib.last_error()
    assert fn(None, 0, None, None, None, 1, 0, 0, *rest) == -1 and "P = 0" in lib.last_error()
    assert fn(None, 50, None, None, None, 1, 0, 50, *rest) == -1 and "null" in lib.last_error()


def test_graphed_eval_step_refuses_to_run_with_packet_capture_on(monkeypatch):
    """The same runtime-flag precondition as GraphedTrainStep, checked before anything touches the GPU."""
    from deltaconv_amd.evaluate import GraphedEvalStep
    monkeypatch.setenv("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "1")
    with pytest.raises(RuntimeError, match="DEBUG_CLR_GRAPH_PACKET_CAPTURE"):
        GraphedEvalStep(None, None)


def test_evaluator_refuses_what_it_cannot_run():
    from deltaconv_amd.evaluate import DeviceEvaluator
    from deltaconv_amd.loader import DeviceLoader

    class _Store:
        y_point, y_cloud, category, device = None, None, None, "cpu"
        sizes = np.full(8, 16, dtype=np.int64)
        norm = None

        def __len__(self):
            return 8

    with pytest.raises(ValueError, match="shuffle"):
        DeviceEvaluator(None, DeviceLoader(_Store(), 4, shuffle=True))
    with pytest.raises(ValueError, match="one label per point"):
        DeviceEvaluator(None, DeviceLoader(_Store(), 4))
    with pytest.raises(ValueError, match="one label per cloud"):
        DeviceEvaluator(None, DeviceLoader(_Store(), 4), task="classification")
    with pytest.raises(ValueError, match="task must be"):
        DeviceEvaluator(None, DeviceLoader(_Store(), 4), task="detection")
    with pytest.raises(ValueError, match="num_votes"):
        DeviceEvaluator(None, DeviceLoader(_Store(), 4), num_votes=0)
