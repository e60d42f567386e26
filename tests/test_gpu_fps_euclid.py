"""``geometry.fps`` / ``fps_levels`` (csrc/fps_euclid.hip behind ``dc_fps_batch``) and ``DeltaNetMultiscale*(sampling="fps")`` on the
MI355X.  Every comparison is an equality: the device picks against the numpy restatement (tests/fps_euclid_restate.py) on every
case of tests/fps_euclid_cases.py, a ragged batch against the per-cloud calls, every larger kernel instance against the one the
cloud's size picks, a captured call replayed on new positions against the eager call; the model with ``sampling="fps"`` against
``sampling="prefix"`` on clouds whose rows are in pick order, and its captured training step against the eager one."""
import numpy as np
import pytest
import torch

from tests import fps_euclid_cases as C
from deltaconv_amd.data import Batch, synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
INSTANCE_SIZES = (64, 1024, 2048, 4096, 8192, C.CAP)           # the largest cloud of every kernel instance


def on_device(c):
    pos = torch.from_numpy(np.concatenate(c["clouds"])).to(DEV)
    ptr = torch.from_numpy(C.ptr_of(c)).to(DEV)
    start = None if c["start"] is None else torch.tensor(c["start"], dtype=torch.int32, device=DEV)
    return pos, ptr, start


def wanted(c):
    ptr = C.ptr_of(c)
    rows = np.concatenate([ptr[b] + picks for b, picks in enumerate(C.expected(c))])
    optr = np.concatenate([[0], np.cumsum([p.size for p in C.expected(c)])])
    return torch.from_numpy(rows), torch.from_numpy(optr)


def info_of(sizes):
    from deltaconv_amd.geometry.graph import PtrInfo
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    return PtrInfo(ptr, len(sizes), int(max(sizes)), int(min(sizes)))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_device_picks_equal_the_restatement(name):
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.geometry.fps import FPS_EUCLID_MAX_POINTS
    assert FPS_EUCLID_MAX_POINTS == C.CAP
    c = C.BY_NAME[name]
    pos, ptr, start = on_device(c)
    rows, optr = fps(pos, ptr=ptr, ratio=c["ratio"], n_samples=c["n_samples"], start=start)
    want_rows, want_optr = wanted(c)
    assert rows.dtype == torch.int64 and optr.dtype == torch.int64
    assert torch.equal(optr.cpu(), want_optr) and torch.equal(rows.cpu(), want_rows)


def test_the_ragged_batch_equals_the_per_cloud_calls_and_the_batch_vector_form():
    from deltaconv_amd.geometry import fps
    c = C.BY_NAME["ragged"]
    pos, ptr, _ = on_device(c)
    rows, optr = fps(pos, ptr=ptr, ratio=3)
    host_ptr = C.ptr_of(c)
    parts = [fps(pos[host_ptr[b]:host_ptr[b + 1]], ratio=3)[0] + int(host_ptr[b]) for b in range(len(c["clouds"]))]
    assert torch.equal(rows, torch.cat(parts))
    batch = torch.repeat_interleave(torch.arange(len(c["clouds"]), device=DEV), ptr[1:] - ptr[:-1])
    rows_b, optr_b = fps(pos, batch=batch, ratio=3)
    assert torch.equal(rows_b, rows) and torch.equal(optr_b, optr)
    out = torch.full_like(rows, -7)
    assert fps(pos, ptr_info=info_of(C.RAGGED_SIZES), ratio=3, out=out)[0] is out and torch.equal(out, rows)


@pytest.mark.parametrize("name", ["n1", "n65", "ragged", "nan_and_inf_rows", "lattice_8x8x8", "nonzero_starts"])
def test_a_larger_kernel_instance_gives_the_same_rows(name):
    from deltaconv_amd.geometry.fps import fps_launch
    c = C.BY_NAME[name]
    pos, ptr, start = on_device(c)
    want_rows, want_optr = wanted(c)
    most = max(p.size for p in C.expected(c))
    largest = max(p.shape[0] for p in c["clouds"])
    for max_cloud in [s for s in INSTANCE_SIZES if s >= largest]:
        rows = fps_launch(pos, ptr, want_optr.to(DEV), len(c["clouds"]), max_cloud, most, int(want_optr[-1]), start)
        assert torch.equal(rows.cpu(), want_rows), max_cloud


def test_a_pick_index_past_the_cloud_gets_minus_one():
    from deltaconv_amd.geometry.fps import fps_launch
    pos = torch.from_numpy(C.normal(5, 7)).to(DEV)
    ptr, optr = torch.tensor([0, 7], device=DEV), torch.tensor([0, 10], device=DEV)
    rows = fps_launch(pos, ptr, optr, 1, 7, 10, 10)
    from tests import fps_euclid_restate as R
    assert rows[:7].tolist() == R.sample(pos.cpu().numpy(), 7).tolist() and rows[7:].tolist() == [-1, -1, -1]


def test_a_captured_call_replays_on_positions_written_in_place():
    from deltaconv_amd.geometry import fps
    sizes = (300, 300, 300)
    info = info_of(sizes)
    first = torch.from_numpy(np.concatenate([C.normal(200 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    second = torch.from_numpy(np.concatenate([C.normal(210 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    pos = first.clone()
    start = torch.tensor([0, 299, 7], dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fps(pos, ptr_info=info, ratio=4, start=start)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows, optr = fps(pos, ptr_info=info, ratio=4, start=start)
    for new in (second, first):
        pos.copy_(new)
        graph.replay()
        want, want_optr = fps(new, ptr_info=info, ratio=4, start=start)
        assert torch.equal(rows, want) and torch.equal(optr, want_optr)
    assert not torch.equal(fps(first, ptr_info=info, ratio=4, start=start)[0], fps(second, ptr_info=info, ratio=4, start=start)[0])


def test_the_argument_errors_raise():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import fps
    pos = torch.from_numpy(C.normal(1, 40)).to(DEV)
    ptr = torch.tensor([0, 40], device=DEV)
    rows = torch.zeros(10, dtype=torch.int64, device=DEV)
    raw = lib.raw("dc_fps_batch")
    args = lambda **kw: tuple({**dict(pos=pos.data_ptr(), ptr=ptr.data_ptr(), optr=ptr.data_ptr(), B=1, max_cloud=40, max_samples=10,
                                     start=None, rows=rows.data_ptr(), stream=None), **kw}.values())
    for bad in (dict(pos=None), dict(ptr=None), dict(optr=None), dict(rows=None), dict(B=-1), dict(max_cloud=C.CAP + 1),
                dict(max_samples=-1)):
        assert raw(*args(**bad)) == -1 and "dc_fps_batch" in lib.last_error(), bad
    assert raw(*args(B=0)) == 0
    for kw in (dict(ratio=0), dict(ratio=2.5), dict(), dict(ratio=2, n_samples=4), dict(n_samples=41), dict(n_samples=0),
               dict(ratio=2, ptr=ptr, batch=torch.zeros(40, dtype=torch.long, device=DEV)), dict(ratio=2, ptr=torch.tensor([0, 0, 40])),
               dict(ratio=2, ptr=torch.tensor([0, 41])), dict(ratio=2, start=torch.zeros(1, dtype=torch.int32)),
               dict(ratio=2, start=torch.zeros(2, dtype=torch.int32, device=DEV)), dict(ratio=2, out=torch.zeros(20, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            fps(pos, **kw)
    for bad_pos in (pos.double(), pos.reshape(-1), pos[:, :2], pos.cpu()):
        with pytest.raises(ValueError):
            fps(bad_pos, ratio=2)
    with pytest.raises(ValueError, match="16384"):
        fps(torch.zeros(C.CAP + 1, 3, device=DEV), n_samples=4)
    with pytest.raises(RuntimeError, match="requires grad"):
        fps(pos.clone().requires_grad_(), ratio=2)
    with torch.no_grad():
        assert fps(pos.clone().requires_grad_(), ratio=2)[0].shape == (20,)


# ---- the levels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(512, 512, 512, 512), C.RAGGED_SIZES[1:]])
def test_fps_levels_is_prefix_levels_with_sampled_rows(sizes):
    from deltaconv_amd.geometry import fps, fps_levels, prefix_levels
    info = info_of(sizes)
    pos = torch.from_numpy(np.concatenate([C.normal(400 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    ratios = (4, 2, 3)
    got, want = fps_levels(pos, info, ratios), prefix_levels(info, ratios)
    assert len(got) == len(want) == 4 and got[0][0] is None
    for (_, gp, gi), (_, wp, wi) in zip(got, want):
        assert torch.equal(gp, wp) and torch.equal(gi[0], wi[0]) and tuple(gi[1:]) == tuple(wi[1:]) and gi.min_cloud == wi.min_cloud
    rows1, optr1 = fps(pos, ptr_info=info, ratio=4)
    assert torch.equal(got[1][0], rows1) and torch.equal(got[1][1], optr1)
    for rows, ptr, _ in got[2:]:
        o1, o = optr1.tolist(), ptr.tolist()
        assert torch.equal(rows, torch.cat([rows1[o1[b]:o1[b] + o[b + 1] - o[b]] for b in range(len(sizes))]))
    assert [lvl[0] for lvl in fps_levels(pos, info, ())] == [None]
    start = torch.tensor([n - 1 for n in sizes], dtype=torch.int32, device=DEV)
    assert torch.equal(fps_levels(pos, info, ratios, start=start)[1][0], fps(pos, ptr_info=info, ratio=4, start=start)[0])


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
B, N, CLASSES = 4, 512, 6
CFG = dict(enc_channels=((16, 16), (32,), (32,)), dec_channels=(32, 16), ratios=(4, 2), num_neighbors=16, k_down=8, k_up=3)


def make(sampling, seed=1):
    import deltaconv_amd as dc
    torch.manual_seed(seed)
    model = dc.models.DeltaNetMultiscaleSegmentation(3, CLASSES, sampling=sampling, **CFG).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return model


def rows_of(data, rows):
    return Batch(data.pos[rows].contiguous(), data.batch, data.norm[rows].contiguous(), None, data.y[rows].contiguous(), None, B)


def in_pick_order(seed):
    """A batch whose rows are, per cloud, in Euclidean pick order from row 0 (a full ordering: ratio = 1)."""
    from deltaconv_amd.geometry import fps
    data = synthetic_batch(B, N, seed=seed, num_classes=CLASSES, per_point_labels=True).to(DEV)
    rows, _ = fps(data.pos.contiguous(), ptr_info=info_of((N,) * B), ratio=1)
    assert torch.equal(torch.sort(rows).values, torch.arange(B * N, device=DEV))
    return rows_of(data, rows)


def shuffled(data, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.cat([b * N + torch.randperm(N, generator=g) for b in range(B)]).to(DEV)
    return rows_of(data, rows)


def step(model, data):
    from deltaconv_amd.utils import calc_loss
    for p in model.parameters():
        p.grad = None
    logits = model(data)
    calc_loss(logits, data.y, smoothing=False).backward()
    return logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def ordered():
    return in_pick_order(90)


def test_on_rows_in_pick_order_fps_and_prefix_sampling_agree_bitwise(ordered):
    la, ga = step(make("fps"), ordered)
    lb, gb = step(make("prefix"), ordered)
    assert la.shape == (B * N, CLASSES) and bool(torch.isfinite(la).all()) and ga.keys() == gb.keys() and len(ga) > 10
    assert torch.equal(la, lb)
    for name in ga:
        assert torch.equal(ga[name], gb[name]), name


def test_on_shuffled_rows_they_do_not_and_two_runs_give_the_same_bits(ordered):
    data = shuffled(ordered, 3)
    la, ga = step(make("fps"), data)
    lb, _ = step(make("prefix"), data)
    assert not torch.equal(la, lb) and float((la - lb).abs().max()) > 1e-4
    lc, gc = step(make("fps"), data)
    assert torch.equal(la, lc) and all(torch.equal(ga[n], gc[n]) for n in ga)


def test_the_captured_training_step_with_fps_sampling_matches_eager():
    from deltaconv_amd.graph_step import GraphedTrainStep
    from deltaconv_amd.utils import calc_loss
    loss_fn = lambda out, y: calc_loss(out, y, smoothing=False)
    batches = [synthetic_batch(B, N, seed=95 + i, num_classes=CLASSES, per_point_labels=True).to(DEV) for i in range(3)]

    def build():
        m = make("fps", seed=5)
        return m, torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)

    def eager_step(m, opt, b):
        for p in m.parameters():
            p.grad = None
        loss = loss_fn(m(b), b.y)
        loss.backward()
        opt.step()
        return float(loss)

    m1, o1 = build()
    for _ in range(3):
        eager_step(m1, o1, batches[0])                                          # = the warm-up steps of the capture (its default)
    ref_losses = [eager_step(m1, o1, b) for b in (batches[1], batches[2])]
    m2, o2 = build()
    graphed = GraphedTrainStep(m2, loss_fn, synthetic_batch(B, N, seed=95, num_classes=CLASSES, per_point_labels=True).to(DEV),
                               optimizer=o2)
    losses = [float(graphed(b)) for b in (batches[1], batches[2])]
    assert losses == ref_losses
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for key in sd1:
        assert torch.equal(sd1[key], sd2[key]), key
