"""The propagation stage on the MI355X (csrc/interp.hip: ``dc_knn_cross``, ``dc_knn_interpolate``; ``geometry.knn_cross`` /
``knn_interpolate``; ``Propagator``; ``DeviceEvaluator(propagate_to=...)``) against the numpy restatement of csrc/interp_math.h
(tests/interp_restate.py, itself held to a g++ build of that header and to fp64 by tests/test_interp_host.py): neighbours,
distances and interpolated rows bit for bit.  Cloud sizes sit on the kernels' seams: the 256 queries of a workgroup (1, 256,
257, 700), the 2048 reference points of an LDS tile (1, 5, 2048, 2049), reference clouds below k, empty clouds; channel counts
around the 4-channel groups (1, 3, 50, 64, 65) on the 16-byte and on the scalar path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import interp_restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
# (query points, reference points) of the pairs of the one ragged call: several workgroups x several tiles, a tile exactly, fewer
# reference points than k, one point each, an empty query cloud, an empty reference cloud
PAIRS = [(700, 2049), (257, 2048), (256, 5), (1, 1), (0, 300), (40, 0)]
KS = (1, 3, 8, 16)


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def clouds():
    """-> (query [Nq,3], qptr, ref [Nr,3], rptr) of PAIRS: uniform in the unit cube; pair 0 has 40 duplicated reference points and
    one query equal to a reference point."""
    rng = np.random.default_rng(0)
    qptr = np.concatenate([[0], np.cumsum([p[0] for p in PAIRS])]).astype(np.int64)
    rptr = np.concatenate([[0], np.cumsum([p[1] for p in PAIRS])]).astype(np.int64)
    qry, ref = rng.random((qptr[-1], 3), dtype=np.float32), rng.random((rptr[-1], 3), dtype=np.float32)
    ref[100:140] = ref[0:40]
    qry[5] = ref[17]
    return qry, qptr, ref, rptr


@functools.lru_cache(maxsize=None)
def restated(k):
    """The restated search of the ragged call, computed once per k and shared."""
    qry, qptr, ref, rptr = clouds()
    return R.knn_cross_batched(qry, qptr, ref, rptr, k)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(rows, cols, dtype, fill):
    whole = torch.full((GUARD + rows * cols + GUARD,), fill, dtype=dtype, device=DEV)
    return whole[GUARD:GUARD + rows * cols].view(rows, cols), whole


def guards_intact(whole, n, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def search(k, pairs=None):
    """dc_knn_cross over the pairs `pairs` (default: all in one call) into guarded buffers -> (idx, d2) as numpy."""
    from deltaconv_amd._lib import lib
    qry, qptr, ref, rptr = clouds()
    nq = int(qptr[-1])
    (idx, iw), (d2, dw) = guarded(nq, k, torch.int32, -9), guarded(nq, k, torch.float32, -9.0)
    dq, dr, dqp, drp = dev(qry), dev(ref), dev(qptr), dev(rptr)
    for lo, hi in ([(0, len(PAIRS))] if pairs is None else pairs):
        mq = int((qptr[lo + 1:hi + 1] - qptr[lo:hi]).max())
        lib.call("dc_knn_cross", dq, dqp[lo:hi + 1], dr, drp[lo:hi + 1], hi - lo, mq, k, idx, d2)
    torch.cuda.synchronize()
    assert guards_intact(iw, nq * k, -9) and guards_intact(dw, nq * k, -9.0), "guard words around idx / d2 were written"
    return idx.cpu().numpy(), d2.cpu().numpy()


# ---- 1. the search --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_ragged_search_equals_the_restatement_bitwise(k):
    idx, d2 = search(k)
    widx, wd2 = restated(k)
    assert np.array_equal(idx, widx), np.argwhere(idx != widx)[:5]
    assert np.array_equal(bits(d2), bits(wd2))
    qry, qptr, ref, rptr = clouds()
    assert idx[5, 0] == 17 and d2[5, 0] == 0.0                                  # the query that IS a reference point (lower of 17 / 117)
    if k > 1:
        assert idx[5, 1] == 117 and d2[5, 1] == 0.0                             # its duplicate: the tie goes to the lower index
    rows = slice(qptr[2], qptr[3])                                              # 5 reference points: the first min(k, 5) slots
    assert (idx[rows, :min(k, 5)] >= 0).all() and (idx[rows, 5:] == -1).all() and np.isinf(d2[rows, 5:]).all()
    rows = slice(qptr[5], qptr[6])                                              # the empty reference cloud
    assert (idx[rows] == -1).all() and np.isinf(d2[rows]).all()
    # the same pairs one call each, and a second run: the same bits
    one = search(k, pairs=[(b, b + 1) for b in range(len(PAIRS))])
    again = search(k)
    for other in (one, again):
        assert np.array_equal(other[0], idx) and np.array_equal(bits(other[1]), bits(d2))


def test_a_nan_coordinate_is_never_picked_on_the_device():
    from deltaconv_amd.geometry import knn_cross
    rng = np.random.default_rng(3)
    ref, qry = rng.random((300, 3), dtype=np.float32), rng.random((260, 3), dtype=np.float32)
    ref[7, 1], ref[250, 0], qry[3, 2] = np.nan, np.nan, np.nan
    idx, d2 = knn_cross(dev(qry), dev(ref), 8)
    widx, wd2 = R.knn_cross(qry, ref, 8)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(bits(d2), bits(wd2))
    assert not np.isin(widx, [7, 250]).any() and (widx[3] == -1).all() and (np.delete(widx, 3, axis=0) >= 0).all()


# ---- 2. the interpolation --------------------------------------------------------------------------------------------------------
def laid_out(x, vec):
    """x [n,C] on the device with a leading dimension above C: 16-byte aligned rows (vec) or an odd leading dimension on a base
    one float off alignment (the scalar path).  The gaps hold NaN."""
    n, c = x.shape
    ld = (c + 4) // 4 * 4 if vec else (c + 1) | 1
    whole = torch.full((n * ld + 8,), float("nan"), device=DEV)
    off = 0 if vec else 1
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + n * ld].view(n, ld)[:, :c]
    view.copy_(dev(x))
    return view, ld


@pytest.mark.parametrize("vec", [True, False], ids=["vec16", "scalar"])
@pytest.mark.parametrize("c", [1, 3, 50, 64, 65])
def test_interpolation_equals_the_restatement_bitwise(c, vec):
    from deltaconv_amd._lib import lib
    qry, qptr, ref, rptr = clouds()
    nq = int(qptr[-1])
    x = (np.random.default_rng(c).standard_normal((int(rptr[-1]), c)) * 10).astype(np.float32)
    dx, ldx = laid_out(x, vec)
    mq = max(p[0] for p in PAIRS)
    for k in (3, 1, 16):
        idx, d2 = restated(k)
        want = R.interpolate_batched(x, qptr, rptr, idx, d2)
        ldo = (c + 4) // 4 * 4 if vec else (c + 1) | 1
        whole = torch.full((GUARD + nq * ldo + GUARD,), -9.0, device=DEV)
        start = GUARD if vec else GUARD + 1                                     # GUARD floats = 32 bytes: aligned / one float off
        out = whole[start:start + (nq - 1) * ldo + c].as_strided((nq, c), (ldo, 1))
        assert (out.data_ptr() % 16 == 0) == vec and (dx.data_ptr() % 16 == 0) == vec
        dqp, drp, didx, dd2 = dev(qptr), dev(rptr), dev(idx), dev(d2)
        lib.call("dc_knn_interpolate", dx, ldx, c, dqp, drp, len(PAIRS), mq, k, didx, dd2, out, ldo)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out), bits(want)), (c, vec, k)
        full = whole.cpu().numpy()
        # the same pairs one call each, and a second run of the one call: the same bits, guards and gaps included
        whole.fill_(-9.0)
        for b in range(len(PAIRS)):
            lib.call("dc_knn_interpolate", dx, ldx, c, dqp[b:b + 2], drp[b:b + 2], 1, PAIRS[b][0], k, didx, dd2, out, ldo)
        torch.cuda.synchronize()
        assert np.array_equal(bits(whole), bits(full)), ("one call per pair", c, vec, k)
        whole.fill_(-9.0)
        lib.call("dc_knn_interpolate", dx, ldx, c, dqp, drp, len(PAIRS), mq, k, didx, dd2, out, ldo)
        torch.cuda.synchronize()
        assert np.array_equal(bits(whole), bits(full)), ("second run", c, vec, k)
        touched = np.zeros(full.shape[0], dtype=bool)
        for r in range(nq):
            touched[start + r * ldo:start + r * ldo + c] = True
        assert (full[~touched] == -9.0).all(), "floats between the rows or around the output were written"
        if k == 1:                                                              # an exact gather
            rows = np.concatenate([rptr[b] + idx[qptr[b]:qptr[b + 1], 0] for b in range(len(PAIRS))])
            live = np.concatenate([idx[qptr[b]:qptr[b + 1], 0] >= 0 for b in range(len(PAIRS))])
            got = out.cpu().numpy()
            assert np.array_equal(bits(got[live]), bits(x[rows[live]])) and not got[~live].any()


def test_interpolate_rows_reads_a_strided_x_as_the_tensor_it_is():
    """A channel slice with a non-unit stride is copied before the launch, also when it has ONE row (no row stride to tell by);
    one channel has no channel stride and goes in as it is."""
    from deltaconv_amd.geometry.interpolate import interpolate_rows
    t = torch.arange(24, dtype=torch.float32, device=DEV).view(3, 8)
    idx, d2 = torch.zeros((5, 1), dtype=torch.int32, device=DEV), torch.full((5, 1), 0.25, device=DEV)
    ptr = lambda n: torch.tensor([0, n], dtype=torch.int64, device=DEV)
    one_row = t[:1, ::2]                                                        # [1,4], strides (8, 2)
    got = interpolate_rows(one_row, ptr(5), ptr(1), idx, d2, 5)
    assert torch.equal(got, one_row.expand(5, 4)), got
    idx[:, 0] = torch.tensor([2, 0, 1, 1, 2], dtype=torch.int32)
    rows = t[:, ::2]                                                            # [3,4], strides (8, 2)
    assert torch.equal(interpolate_rows(rows, ptr(5), ptr(3), idx, d2, 5), rows[idx[:, 0].long()])
    one_channel = t[:, 3::8]                                                    # [3,1], strides (8, 8): rows 8 apart, no copy needed
    assert one_channel.shape == (3, 1) and one_channel.stride(1) != 1
    assert torch.equal(interpolate_rows(one_channel, ptr(5), ptr(3), idx, d2, 5), one_channel[idx[:, 0].long()])


# ---- 3. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_dc_err_arg_without_a_launch():
    from deltaconv_amd._lib import lib
    qry, qptr, ref, rptr = clouds()
    dq, dr, dqp, drp = dev(qry), dev(ref), dev(qptr), dev(rptr)
    nq, b = int(qptr[-1]), len(PAIRS)
    idx = torch.full((nq, 16), -9, dtype=torch.int32, device=DEV)
    d2 = torch.full((nq, 16), -9.0, device=DEV)
    x, out = torch.ones(int(rptr[-1]), 4, device=DEV), torch.full((nq, 4), -9.0, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    cross, interp = lib.raw("dc_knn_cross"), lib.raw("dc_knn_interpolate")

    def call_cross(B=b, k=3, q=dq, r=dr, i=idx, d=d2, qp=dqp, mq=700):
        return cross(vp(q), vp(qp), vp(r), vp(drp), B, mq, k, vp(i), vp(d), None)

    def call_interp(B=b, k=3, xx=x, o=out, i=idx, C=4, ldx=4, ldo=4):
        return interp(vp(xx), ldx, C, vp(dqp), vp(drp), B, 700, k, vp(i), vp(d2), vp(o), ldo, None)

    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(q=None), "null"),
                    (dict(r=None), "null"), (dict(i=None), "null"), (dict(d=None), "null"), (dict(qp=None), "null"),
                    (dict(mq=-1), "max_query_cloud")):
        assert call_cross(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    for kw, msg in ((dict(k=0), "k = 0"), (dict(k=17), "k = 17"), (dict(B=65536), "65535"), (dict(xx=None), "null"),
                    (dict(o=None), "null"), (dict(i=None), "null"), (dict(C=0), "C = 0"), (dict(ldx=3), "ldx"), (dict(ldo=3), "ldo")):
        assert call_interp(**kw) == -1 and msg in lib.last_error(), (kw, lib.last_error())
    assert call_cross(B=0) == 0 and call_interp(B=0) == 0 and call_cross(B=0, q=None, r=None) == 0
    torch.cuda.synchronize()
    assert bool((idx == -9).all()) and bool((d2 == -9).all()) and bool((out == -9).all())


# ---- 4. the tensor-level interface ---------------------------------------------------------------------------------------------------
def test_knn_interpolate_equals_the_restatement_with_batch_vectors_and_with_ptr():
    import deltaconv
    from deltaconv_amd.geometry import knn_cross, knn_interpolate
    assert deltaconv.geometry.knn_interpolate is knn_interpolate
    qry, qptr, ref, rptr = clouds()
    sel = [0, 1, 2, 3]                                                          # a batch vector cannot name an empty cloud
    q = np.concatenate([qry[qptr[b]:qptr[b + 1]] for b in sel])
    r = np.concatenate([ref[rptr[b]:rptr[b + 1]] for b in sel])
    qp = np.concatenate([[0], np.cumsum([PAIRS[b][0] for b in sel])])
    rp = np.concatenate([[0], np.cumsum([PAIRS[b][1] for b in sel])])
    bq, br = np.repeat(np.arange(4), np.diff(qp)), np.repeat(np.arange(4), np.diff(rp))
    x = np.random.default_rng(9).standard_normal((r.shape[0], 50)).astype(np.float32)
    want = R.knn_interpolate(x, r, q, 3, ptr_x=rp, ptr_y=qp)
    a = knn_interpolate(dev(x), dev(r), dev(q), dev(br), dev(bq))                # PyG's argument order, k = 3 by default
    b = knn_interpolate(dev(x), dev(r), dev(q), k=3, ptr_x=dev(rp), ptr_y=dev(qp))
    assert a.shape == (q.shape[0], 50) and a.dtype == torch.float32
    assert np.array_equal(bits(a), bits(want)) and torch.equal(a, b)
    one = knn_interpolate(dev(x[:5]), dev(r[:5]), dev(q[:300]), k=8)             # neither: one cloud pair
    assert np.array_equal(bits(one), bits(R.knn_interpolate(x[:5], r[:5], q[:300], 8)))
    idx, d2 = knn_cross(dev(q), dev(r), 3, batch_query=dev(bq), batch_ref=dev(br))
    widx, wd2 = R.knn_cross_batched(q, qp, r, rp, 3)
    assert np.array_equal(idx.cpu().numpy(), widx) and np.array_equal(bits(d2), bits(wd2))
    with pytest.raises(ValueError, match="4 query clouds but 3 reference clouds"):
        knn_cross(dev(q), dev(r), 3, ptr_query=dev(qp), ptr_ref=dev(rp[:-1]))
    with pytest.raises(ValueError, match="outside"):
        knn_cross(dev(q), dev(r), 17)
    # inference only: a graph is never cut silently
    xg = dev(x).requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference-only"):
        knn_interpolate(xg, dev(r), dev(q), dev(br), dev(bq))
    with torch.no_grad():
        assert torch.equal(knn_interpolate(xg, dev(r), dev(q), dev(br), dev(bq)), a)
    with pytest.raises(RuntimeError, match="HIP device"):
        knn_interpolate(torch.from_numpy(x), dev(r), dev(q))


# ---- 5. Propagator and DeviceEvaluator ---------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """Logits that are a fixed elementwise function of the batch's positions: the same bits whatever batch a cloud lands in."""

    def __init__(self, classes=50):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.register_buffer("w", torch.randn(3, classes, generator=g) * 3)

    def forward(self, batch):
        p = batch.pos
        return torch.sin(p[:, 0:1] * self.w[0] + torch.cos(p[:, 1:2] * self.w[1]) + p[:, 2:3] * self.w[2])


def _aug():
    import deltaconv_amd.transforms as T
    return [T.RandomScale((2 / 3, 3 / 2)), T.RandomTranslateGlobal(0.2)]


def _seg_items(n_clouds=6, points=300):
    from deltaconv_amd.evaluate import part_tables
    from tests.batch_restate import make_items
    start, count = part_tables()
    items = make_items(n_clouds, points)
    g = torch.Generator().manual_seed(6)
    for i, d in enumerate(items):
        k = (3 * i) % 16
        d.category = torch.zeros(1, 16)
        d.category[0, k] = 1
        d.y = torch.randint(start[k], start[k] + count[k], (points,), generator=g)
    return items


def _host_scores(pred, true, label, sizes):
    """accuracy / balanced accuracy / part IoU the way ``utils.evaluate_votes`` forms them, clouds of any sizes."""
    from deltaconv_amd.utils import calc_shape_IoU
    off = np.concatenate([[0], np.cumsum(sizes)])
    classes = np.unique(true)
    ious = [calc_shape_IoU(pred[None, off[c]:off[c + 1]], true[None, off[c]:off[c + 1]], label[c:c + 1], None)[0]
            for c in range(len(sizes))]
    return dict(accuracy=float((true == pred).mean()),
                balanced_accuracy=float(np.mean([(pred[true == c] == c).mean() for c in classes])), ious=ious,
                mean_iou=float(np.mean(ious)))


def _host_reference(model, store, votes, k, tpos, tptr, ty):
    """The host pass: the loader's epochs 0 .. votes-1, logits summed in fp32 in vote order, the restated interpolation of the sums
    to the target rows, arg-max, ``calc_shape_IoU``."""
    from deltaconv_amd.loader import DeviceLoader
    loader = DeviceLoader(store, 4, transform=_aug(), seed=3)
    acc = None
    with torch.no_grad():
        for _ in range(votes):
            logits = torch.cat([model(b) for b in loader]).cpu().numpy()
            acc = logits if acc is None else acc + logits
    sptr = store.ptr.cpu().numpy()
    idx, d2 = R.knn_cross_batched(tpos, tptr, store.pos.cpu().numpy(), sptr, k)
    up = R.interpolate_batched(acc, tptr, sptr, idx, d2)
    label = store.category.cpu().numpy().argmax(axis=1)
    return up, _host_scores(np.argmax(up, axis=1), ty, label, np.diff(tptr)), idx, d2


def _same(got, want):
    for key in ("accuracy", "balanced_accuracy", "mean_iou"):
        assert abs(got[key] - want[key]) <= 1e-12, (key, got[key], want[key])
    assert np.abs(np.asarray(got["ious"]) - np.asarray(want["ious"])).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def seg_stores():
    from deltaconv_amd.loader import DeviceDataset
    full = DeviceDataset.from_dataset(_seg_items(), DEV)
    return full, full.geodesic_subsample(128, seed=1)


@pytest.mark.parametrize("votes", [1, 3])
def test_evaluator_scores_the_interpolated_votes_at_target_resolution(votes):
    from deltaconv_amd import DeviceEvaluator, DeviceLoader, Propagator
    full, sampled = seg_stores()
    model = _Stub().to(DEV).eval()
    tpos, tptr, ty = full.pos.cpu().numpy(), full.ptr.cpu().numpy(), full.y_point.cpu().numpy()
    up, want, idx, d2 = _host_reference(model, sampled, votes, 3, tpos, tptr, ty)
    mk = lambda: DeviceLoader(sampled, 4, transform=_aug(), seed=3)             # a full batch and a short one
    ev = DeviceEvaluator(model, mk(), "segmentation", num_votes=votes, graphed=False, keep_pred=True, propagate_to=full)
    got = ev.run()
    assert np.array_equal(ev.prop.idx.cpu().numpy(), idx) and np.array_equal(bits(ev.prop.d2), bits(d2))
    assert np.array_equal(got["pred"], np.argmax(up, axis=1)) and np.array_equal(got["true"], ty) and got["ignored"] == 0
    _same(got, want)
    # "sampled": exactly what a run without propagate_to returns
    plain = DeviceEvaluator(model, mk(), "segmentation", num_votes=votes, graphed=False, keep_pred=True).run()
    assert set(got["sampled"]) == set(plain) and "sampled" not in plain
    for key in plain:
        assert np.array_equal(got["sampled"][key], plain[key]), key
    # Propagator.apply on the vote sums = the restated rows, bit for bit; a range of clouds = those rows
    prop = Propagator(sampled, full, k=3)
    sums = ev.votes if votes > 1 else torch.cat([model(b) for b in mk()])
    assert np.array_equal(bits(prop.apply(sums)), bits(up))
    s0, s1 = int(sampled.ptr[2]), int(sampled.ptr[5])
    assert np.array_equal(bits(prop.apply(sums[s0:s1], (2, 5))), bits(up[tptr[2]:tptr[5]]))
    # the target is the sampled store itself, k = 1: every point finds itself and both sets of keys are identical
    same = DeviceEvaluator(model, mk(), "segmentation", num_votes=votes, graphed=False, keep_pred=True, propagate_to=sampled,
                           propagate_k=1).run()
    for key in plain:
        assert np.array_equal(np.asarray(same[key]).reshape(-1), np.asarray(same["sampled"][key]).reshape(-1)), key
        assert np.array_equal(same["sampled"][key], plain[key]), key


def test_label_transfer_and_refusals():
    from deltaconv_amd import DeviceEvaluator, DeviceLoader, Propagator
    from deltaconv_amd.loader import DeviceDataset
    from tests.batch_restate import make_items
    full, sampled = seg_stores()
    prop = Propagator(sampled, full, k=1)
    idx, _ = R.knn_cross_batched(full.pos.cpu().numpy(), full.ptr.cpu().numpy(), sampled.pos.cpu().numpy(), sampled.ptr.cpu().numpy(), 1)
    rows = np.repeat(sampled.ptr.cpu().numpy()[:-1], full.sizes) + idx[:, 0]
    assert np.array_equal(prop.labels(sampled.y_point).cpu().numpy(), sampled.y_point.cpu().numpy()[rows])
    t0, t1, s0, s1 = int(full.ptr[1]), int(full.ptr[3]), int(sampled.ptr[1]), int(sampled.ptr[3])
    assert torch.equal(prop.labels(sampled.y_point[s0:s1], (1, 3)), prop.labels(sampled.y_point)[t0:t1])
    # the sampled points are points of the full cloud: each of them finds itself, so the transfer reproduces its label there
    assert float((prop.labels(sampled.y_point) == full.y_point).float().mean()) >= 128 / 300
    model = _Stub().to(DEV).eval()
    bare = DeviceDataset(full.pos, full.ptr, full.sizes)
    with pytest.raises(ValueError, match="per vertex"):
        DeviceEvaluator(model, DeviceLoader(sampled, 4), graphed=False, propagate_to=bare)
    with pytest.raises(ValueError, match="source clouds"):
        Propagator(sampled, DeviceDataset.from_dataset(make_items(5, 64), DEV))
    with pytest.raises(ValueError, match="outside"):
        Propagator(sampled, full, k=17)


def test_evaluator_with_a_mesh_target_scores_the_vertices():
    from deltaconv_amd import DeviceEvaluator, DeviceLoader, DeviceMeshDataset
    from deltaconv_amd.data import synthetic_mesh
    from deltaconv_amd.datasets import Data
    items = []
    for i, f in enumerate((63, 200, 64)):
        pos, face, y = synthetic_mesh(f, 20 + i, labels=True)
        items.append(Data(pos=pos, face=face, y=y % 4, category=torch.eye(16)[0]))              # category 0: parts 0 .. 3
    meshes = DeviceMeshDataset.from_dataset(items, DEV)
    sampled = meshes.sample_points(128, include_labels=True, seed=1)
    assert sampled.category is not None and sampled.y_point is not None
    model = _Stub().to(DEV).eval()
    tpos, tptr, ty = meshes.vert.cpu().numpy(), meshes.vptr.cpu().numpy(), meshes.y_vert.cpu().numpy()
    up, want, _, _ = _host_reference(model, sampled, 1, 3, tpos, tptr, ty)
    got = DeviceEvaluator(model, DeviceLoader(sampled, 4, transform=_aug(), seed=3), num_votes=1, graphed=False, keep_pred=True,
                          propagate_to=meshes).run()
    assert got["pred"].shape == (tpos.shape[0],) and np.array_equal(got["pred"], np.argmax(up, axis=1))
    assert np.array_equal(got["true"], ty)
    _same(got, want)
    assert got["sampled"]["pred"].shape == (3, 128)
