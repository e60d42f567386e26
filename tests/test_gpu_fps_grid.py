"""``geometry.fps(method="grid")`` (csrc/fps_grid.hip behind ``dc_fps_grid``), ``fps_levels`` / ``DeltaNetMultiscale*`` / ``fps_subsample``
through it, on the MI355X.  Every comparison is ``torch.equal``: rows, offsets AND stats against the numpy restatement
(tests/fps_grid_restate.py) on every case of tests/fps_grid_cases.py at three targets -- the stats are the populations of the
boxes, so a kernel that ignores the box rule fails them -- and the rows against the register kernel (``method="brute"``)."""
import numpy as np
import pytest
import torch

from tests import fps_grid_cases as C
from tests import fps_grid_restate as R
from deltaconv_amd.data import synthetic_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def on_device(c):
    pos = torch.from_numpy(np.concatenate(c["clouds"])).to(DEV)
    ptr = torch.from_numpy(C.ptr_of(c)).to(DEV)
    start = None if c["start"] is None else torch.tensor(c["start"], dtype=torch.int32, device=DEV)
    return pos, ptr, start


def wanted(c, target):
    ptr, exp = C.ptr_of(c), C.expected(c, target)
    rows = np.concatenate([ptr[b] + picks for b, (picks, _) in enumerate(exp)])
    optr = np.concatenate([[0], np.cumsum([picks.size for picks, _ in exp])])
    return torch.from_numpy(rows), torch.from_numpy(optr), torch.from_numpy(np.stack([s for _, s in exp]))


def info_of(sizes):
    from deltaconv_amd.geometry.graph import PtrInfo
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)
    return PtrInfo(ptr, len(sizes), int(max(sizes)), int(min(sizes)))


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_device_rows_and_stats_equal_the_restatement_and_the_register_kernel(name):
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.geometry.fps import FPS_GRID_MAX_POINTS
    assert FPS_GRID_MAX_POINTS == R.CAP
    c = C.BY_NAME[name]
    pos, ptr, start = on_device(c)
    brute, brute_optr = fps(pos, ptr=ptr, ratio=c["ratio"], n_samples=c["n_samples"], start=start, method="brute")
    for target in C.TARGETS:
        rows, optr, stats = fps(pos, ptr=ptr, ratio=c["ratio"], n_samples=c["n_samples"], start=start, method="grid",
                                grid_target=target, stats=True)
        want_rows, want_optr, want_stats = wanted(c, target)
        assert rows.dtype == torch.int64 and optr.dtype == torch.int64 and stats.dtype == torch.int64
        assert torch.equal(optr.cpu(), want_optr) and torch.equal(rows.cpu(), want_rows), target
        assert torch.equal(stats.cpu(), want_stats), (target, stats.tolist(), want_stats.tolist())
        assert torch.equal(rows, brute) and torch.equal(optr, brute_optr), target


def test_a_cloud_above_the_old_cap_equals_the_restatement():
    from deltaconv_amd.geometry import fps
    pos, picks, _, history = C.big_sphere()
    m = 2500                                              # FPS is greedy: the first m picks are the m-pick sample
    rows, optr, stats = fps(torch.from_numpy(pos).to(DEV), n_samples=m, method="grid", stats=True)
    assert optr.tolist() == [0, m] and torch.equal(rows.cpu(), torch.from_numpy(picks[:m]))
    assert torch.equal(stats.cpu(), torch.from_numpy(history[m - 2])[None])
    assert int(stats[0, 0]) < pos.shape[0] * (m - 1) // 10


@pytest.mark.parametrize("target", (0.5, None, 1.0))
def test_a_cloud_at_the_cap_equals_the_restatement(target):
    """The largest tables (2 n cells at target 0.5) and the largest first pass."""
    from deltaconv_amd.geometry import fps
    pos = C.sphere(490, R.CAP)
    pos[::7] *= np.float32(0.5)                           # two shells: the cells are not all on one surface
    m, s = 64, 12345
    want, want_stats = R.sample(pos, m, s, R.DEFAULT_TARGET if target is None else target)
    rows, optr, stats = fps(torch.from_numpy(pos).to(DEV), n_samples=m, start=torch.tensor([s], dtype=torch.int32, device=DEV),
                            method="grid", grid_target=target, stats=True)
    assert torch.equal(rows.cpu(), torch.from_numpy(want)) and torch.equal(stats.cpu(), torch.from_numpy(want_stats)[None])


def test_the_ragged_batch_equals_the_per_cloud_calls_and_the_three_forms_agree():
    from deltaconv_amd.geometry import fps
    c = C.BY_NAME["ragged"]
    pos, ptr, _ = on_device(c)
    rows, optr, stats = fps(pos, ptr=ptr, ratio=3, method="grid", stats=True)
    host_ptr = C.ptr_of(c)
    parts = [fps(pos[host_ptr[b]:host_ptr[b + 1]], ratio=3, method="grid", stats=True) for b in range(len(c["clouds"]))]
    assert torch.equal(rows, torch.cat([p[0] + int(host_ptr[b]) for b, p in enumerate(parts)]))
    assert torch.equal(stats, torch.cat([p[2] for p in parts]))
    batch = torch.repeat_interleave(torch.arange(len(c["clouds"]), device=DEV), ptr[1:] - ptr[:-1])
    rows_b, optr_b = fps(pos, batch=batch, ratio=3, method="grid")
    assert torch.equal(rows_b, rows) and torch.equal(optr_b, optr)
    out = torch.full_like(rows, -7)
    from tests.fps_euclid_cases import RAGGED_SIZES
    got = fps(pos, ptr_info=info_of(RAGGED_SIZES), ratio=3, out=out, method="grid")
    assert got[0] is out and torch.equal(out, rows) and torch.equal(got[1], optr)


@pytest.mark.parametrize("name", ["sphere_3000", "lattice_8x8x8", "heavy_cell_300_of_2000", "ragged_with_specials"])
def test_a_second_run_gives_the_same_rows_and_stats(name):
    from deltaconv_amd.geometry import fps
    c = C.BY_NAME[name]
    pos, ptr, start = on_device(c)
    a = fps(pos, ptr=ptr, ratio=c["ratio"], start=start, method="grid", stats=True)
    b = fps(pos, ptr=ptr, ratio=c["ratio"], start=start, method="grid", stats=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_switch_names_the_method_where_the_call_names_none():
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.geometry.fps import FPS_METHOD
    pos = torch.from_numpy(C.sphere(1, 20000)).to(DEV)
    old = FPS_METHOD[0]
    try:
        FPS_METHOD[0] = "grid"
        rows, _ = fps(pos, n_samples=8)
        FPS_METHOD[0] = "brute"
        with pytest.raises(ValueError, match="16384"):
            fps(pos, n_samples=8)
    finally:
        FPS_METHOD[0] = old
    assert torch.equal(rows, fps(pos, n_samples=8, method="grid")[0])


def test_a_pick_index_past_the_cloud_gets_minus_one_and_a_cloud_above_max_cloud_is_not_sampled():
    from deltaconv_amd.geometry.fps import fps_grid_launch
    from tests import fps_euclid_restate as E
    pos = torch.from_numpy(np.concatenate([C.normal(5, 7), C.normal(6, 50)])).to(DEV)
    ptr, optr = torch.tensor([0, 7, 57], device=DEV), torch.tensor([0, 10, 14], device=DEV)
    rows, stats = fps_grid_launch(pos, ptr, optr, 2, 50, 10, 14, stats=True)
    assert rows[:7].tolist() == E.sample(pos[:7].cpu().numpy(), 7).tolist() and rows[7:10].tolist() == [-1, -1, -1]
    assert rows[10:].tolist() == (7 + E.sample(pos[7:].cpu().numpy(), 4)).tolist()
    small, small_stats = fps_grid_launch(pos, ptr, optr, 2, 7, 10, 14, stats=True)      # max_cloud = 7: the second cloud claims more
    assert torch.equal(small[:10], rows[:10]) and small[10:].tolist() == [-1] * 4
    assert torch.equal(small_stats[0], stats[0]) and small_stats[1].tolist() == [0, 0]


def test_a_captured_call_replays_on_positions_written_in_place():
    from deltaconv_amd.geometry import fps
    sizes = (300, 300, 300)
    info = info_of(sizes)
    first = torch.from_numpy(np.concatenate([C.normal(200 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    second = torch.from_numpy(np.concatenate([C.normal(210 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    pos = first.clone()
    start = torch.tensor([0, 299, 7], dtype=torch.int32, device=DEV)
    call = lambda p: fps(p, ptr_info=info, ratio=4, start=start, method="grid", stats=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(pos)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows, optr, stats = call(pos)
    for new in (second, first):
        pos.copy_(new)
        graph.replay()
        want = call(new)
        assert torch.equal(rows, want[0]) and torch.equal(optr, want[1]) and torch.equal(stats, want[2])
    assert not torch.equal(call(first)[0], call(second)[0])


def test_the_argument_errors_raise():
    from deltaconv_amd._lib import lib
    from deltaconv_amd.geometry import fps, fps_levels
    pos = torch.from_numpy(C.normal(1, 40)).to(DEV)
    ptr = torch.tensor([0, 40], device=DEV)
    rows = torch.zeros(10, dtype=torch.int64, device=DEV)
    need = int(lib.raw("dc_fps_grid_workspace_bytes")(40, 1))
    assert need > 0 and lib.raw("dc_fps_grid_workspace_bytes")(-1, 1) == 0 and lib.raw("dc_fps_grid_workspace_bytes")(40, -1) == 0
    work = torch.zeros(need // 8 + 4, dtype=torch.int64, device=DEV)
    raw = lib.raw("dc_fps_grid")
    args = lambda **kw: tuple({**dict(pos=pos.data_ptr(), ptr=ptr.data_ptr(), optr=ptr.data_ptr(), B=1, max_cloud=40, max_samples=10,
                                     start=None, target=1.0, rows=rows.data_ptr(), stats=None, workspace=work.data_ptr(),
                                     workspace_bytes=need, stream=None), **kw}.values())
    for bad in (dict(pos=None), dict(ptr=None), dict(optr=None), dict(rows=None), dict(workspace=None), dict(B=-1),
                dict(max_cloud=R.CAP + 1), dict(max_cloud=-1), dict(max_samples=-1), dict(target=0.0), dict(target=-1.0),
                dict(target=float("inf")), dict(target=float("nan")), dict(workspace=work.data_ptr() + 8),
                dict(workspace_bytes=need - 16), dict(workspace_bytes=0)):
        assert raw(*args(**bad)) == -1 and "dc_fps_grid" in lib.last_error(), bad
    assert raw(*args(B=0)) == 0 and raw(*args(max_samples=0)) == 0
    for kw in (dict(ratio=2, method="cells"), dict(ratio=2, method="brute", grid_target=1.0), dict(ratio=2, method="brute", stats=True),
               dict(ratio=2, method="grid", grid_target=0.0), dict(ratio=2, method="grid", grid_target=float("inf")),
               dict(ratio=0, method="grid"), dict(n_samples=41, method="grid"),
               dict(ratio=2, method="grid", start=torch.zeros(2, dtype=torch.int32, device=DEV))):
        with pytest.raises(ValueError):
            fps(pos, **kw)
    with pytest.raises(ValueError, match=str(R.CAP)):
        fps(torch.zeros(R.CAP + 1, 3, device=DEV), n_samples=4, method="grid")
    with pytest.raises(ValueError):
        fps_levels(pos, info_of((40,)), (2,), method="brute", grid_target=2.0)
    with pytest.raises(ValueError):
        fps_levels(pos, info_of((40,)), (2,), method="cells")


def test_the_default_path_is_unchanged():
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.geometry.fps import FPS_METHOD
    assert FPS_METHOD[0] == "brute"
    with pytest.raises(ValueError, match="16384"):
        fps(torch.zeros(16385, 3, device=DEV), n_samples=4)
    pos = torch.from_numpy(C.normal(3, 500)).to(DEV)
    assert torch.equal(fps(pos, ratio=4)[0], fps(pos, ratio=4, method="brute")[0])


# ---- the levels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(512, 512, 512, 512), (65, 1025, 300, 2049)])
def test_fps_levels_with_the_grid_equals_brute_force(sizes):
    from deltaconv_amd.geometry import fps_levels
    info = info_of(sizes)
    pos = torch.from_numpy(np.concatenate([C.normal(400 + b, n) for b, n in enumerate(sizes)])).to(DEV)
    start = torch.tensor([n - 1 for n in sizes], dtype=torch.int32, device=DEV)
    for st in (None, start):
        got, want = fps_levels(pos, info, (4, 2, 3), start=st, method="grid", grid_target=2.0), fps_levels(pos, info, (4, 2, 3), start=st, method="brute")
        assert len(got) == len(want) == 4 and got[0][0] is None
        for (gr, gp, gi), (wr, wp, wi) in zip(got[1:], want[1:]):
            assert torch.equal(gr, wr) and torch.equal(gp, wp) and tuple(gi[1:]) == tuple(wi[1:])


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
B, N, CLASSES = 4, 512, 6
CFG = dict(enc_channels=((16, 16), (32,), (32,)), dec_channels=(32, 16), ratios=(4, 2), num_neighbors=16, k_down=8, k_up=3)


def make(fps_method, seed=1):
    import deltaconv_amd as dc
    torch.manual_seed(seed)
    model = dc.models.DeltaNetMultiscaleSegmentation(3, CLASSES, sampling="fps", fps_method=fps_method, **CFG).to(DEV).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.eval()
    return model


def step(model, data):
    from deltaconv_amd.utils import calc_loss
    for p in model.parameters():
        p.grad = None
    logits = model(data)
    calc_loss(logits, data.y, smoothing=False).backward()
    return logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def test_the_model_with_the_grid_sampler_equals_the_register_kernel_bitwise():
    data = synthetic_batch(B, N, seed=90, num_classes=CLASSES, per_point_labels=True).to(DEV)
    la, ga = step(make("grid"), data)
    lb, gb = step(make("brute"), data)
    assert la.shape == (B * N, CLASSES) and bool(torch.isfinite(la).all()) and ga.keys() == gb.keys() and len(ga) > 10
    assert torch.equal(la, lb)
    for name in ga:
        assert torch.equal(ga[name], gb[name]), name


def test_the_captured_training_step_with_the_grid_sampler_matches_eager():
    from deltaconv_amd.graph_step import GraphedTrainStep
    from deltaconv_amd.utils import calc_loss
    loss_fn = lambda out, y: calc_loss(out, y, smoothing=False)
    batches = [synthetic_batch(B, N, seed=95 + i, num_classes=CLASSES, per_point_labels=True).to(DEV) for i in range(3)]

    def build():
        m = make("grid", seed=5)
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


# ---- the store ---------------------------------------------------------------------------------------------------------------------------
def test_fps_subsample_is_the_store_built_by_hand_and_propagates_back():
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.loader import DeviceDataset
    from deltaconv_amd.propagate import Propagator
    sizes = np.array([700, 20000, 333], dtype=np.int64)
    pos = torch.from_numpy(np.concatenate([C.sphere(500 + i, int(n)) for i, n in enumerate(sizes)])).to(DEV)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)])).to(DEV)
    y = torch.arange(pos.shape[0], device=DEV) % 11
    store = DeviceDataset(pos, ptr, sizes, None, pos * 2.0, y, torch.arange(3, device=DEV), None)
    m, starts = 256, [5, 19999, 0]
    sub = store.fps_subsample(m, start=starts, method="grid")
    rows, optr = fps(pos, ptr=ptr, n_samples=m, start=torch.tensor(starts, dtype=torch.int32, device=DEV), method="grid")
    assert torch.equal(sub.source_rows, rows) and torch.equal(sub.ptr, optr) and sub.sizes.tolist() == [m] * 3
    assert torch.equal(sub.pos, pos[rows]) and torch.equal(sub.x, pos[rows] * 2.0) and torch.equal(sub.y_point, y[rows])
    assert sub.norm is None and torch.equal(sub.y_cloud, store.y_cloud)
    assert rows[optr[:-1]].tolist() == (ptr[:-1] + torch.tensor(starts, device=DEV)).tolist()
    seeded = store.fps_subsample(m, seed=3, method="grid")
    assert torch.equal(seeded.source_rows, store.fps_subsample(m, seed=3, method="grid").source_rows)
    # the way back: every picked row of the parent gets its own label through the k = 1 transfer
    back = Propagator(sub, store, k=1).labels(sub.y_point)
    assert back.shape == y.shape and torch.equal(back[rows], y[rows])
    with pytest.raises(ValueError, match="cloud 2"):
        store.fps_subsample(334, method="grid")
    with pytest.raises(ValueError, match="16384"):
        store.fps_subsample(m, start=starts, method="brute")
    with pytest.raises(ValueError):
        store.fps_subsample(m, start=[0, 0], method="grid")
