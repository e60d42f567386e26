"""Host side of exact farthest-point sampling on a cell grid (csrc/fps_grid_math.h), without a GPU: a g++ build of the header
(tests/hostcheck_fps_grid) equals the numpy restatement (tests/fps_grid_restate.py) in picks AND stats on every case of
tests/fps_grid_cases.py at three targets; both equal brute force (dcfpse::sample / tests/fps_euclid_restate.py); the property the
proof rests on holds on sampled (pick, point outside the box) pairs; and the box rule prunes.  Every assertion is an equality or
an inequality the header derives; the pruning bound (one tenth of brute force's updates) is the issue's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fps_euclid_restate as E
from tests import fps_grid_cases as C
from tests import fps_grid_restate as R
from tests import knn_grid_restate as K
from tests.helpers import ROOT

HG_DIR = os.path.join(ROOT, "tests", "hostcheck_fps_grid")
P = lambda a: ctypes.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def hg():
    subprocess.run(["make", "-s", "-C", HG_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HG_DIR, "libhostcheck_fps_grid.so"))
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    lib.hg_max_points.argtypes, lib.hg_max_points.restype = [], i32
    lib.hg_block_cells.argtypes, lib.hg_block_cells.restype = [], i32
    lib.hg_default_target.argtypes, lib.hg_default_target.restype = [], f32
    lib.hg_sample.argtypes, lib.hg_sample.restype = [vp, i64, i32, i32, f32, vp, vp], ctypes.c_int
    lib.hg_sample_brute.argtypes, lib.hg_sample_brute.restype = [vp, i64, i32, i32, vp], ctypes.c_int
    lib.hg_key_md.argtypes, lib.hg_key_md.restype = [vp, vp, i64, vp, vp], None
    return lib


def host_sample(hg, pos, m, start, target):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    picks, stats = np.full(m, -7, np.int32), np.full(2, -7, np.int64)
    assert hg.hg_sample(P(pos), pos.shape[0], m, start, target, P(picks), P(stats)) == 0
    return picks.astype(np.int64), stats


def host_brute(hg, pos, m, start):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    picks = np.full(m, -7, np.int32)
    assert hg.hg_sample_brute(P(pos), pos.shape[0], m, start, P(picks)) == 0
    return picks.astype(np.int64)


def test_the_cap_is_declared_the_same_everywhere(hg):
    from deltaconv_amd.geometry.fps import FPS_GRID_MAX_POINTS, FPS_GRID_TARGET
    hdr = open(os.path.join(ROOT, "include", "deltaconv_hip.h")).read()
    declared = re.findall(r"#define DC_FPS_GRID_MAX_POINTS \((\d+)\)", hdr)
    assert len(declared) == 1                                                          # declared once
    assert int(declared[0]) == hg.hg_max_points() == FPS_GRID_MAX_POINTS == R.CAP and R.CAP >= 262144
    assert hg.hg_default_target() == FPS_GRID_TARGET == R.DEFAULT_TARGET
    # the block keys of a cloud at the cap, 2 n cells, fill 64 KiB of LDS
    assert -(-2 * R.CAP // hg.hg_block_cells()) * 8 <= 64 * 1024


def test_the_cases_hit_the_grids_they_are_named_for():
    cells = lambda name, t=1.0: K.grid_of(C.BY_NAME[name]["clouds"][0], t)
    assert cells("cells_64")["cells"] == 64 and cells("cells_65")["cells"] == 65
    for name in ("n1", "coincident_50", "no_finite_point"):
        assert cells(name)["cells"] == 1 and cells(name, 0.5)["cells"] == 1             # nothing to divide
    G = cells("zero_extent_two_axes")
    assert G["g"][1] == G["g"][2] == 1 and G["g"][0] > 64
    G = cells("short_rows_2000")
    assert 1 < G["g"][0] < 32 and G["cells"] > 256                                       # several x-runs in one block of 64 cells
    pos = C.BY_NAME["heavy_cell_300_of_2000"]["clouds"][0]
    G = cells("heavy_cell_300_of_2000")
    ids = K.cells(G, pos) @ np.array([1, G["g"][0], G["g"][0] * G["g"][1]])
    assert np.bincount(ids).max() >= 300 and G["cells"] > 64                             # more than one wave pass over a cell
    G = cells("sphere_scaled_1e-17")
    assert G["cells"] > 64 and float(K.bound2(G["g"].max(), G["min_h"])) == 0.0          # bound2 below B2_MIN: no pruning
    for name in C.NAMES:
        for pos in C.BY_NAME[name]["clouds"]:
            assert K.grid_of(pos, C.ONE_CELL)["cells"] == 1
            assert pos.shape[0] <= 16384


@pytest.mark.parametrize("target", C.TARGETS)
@pytest.mark.parametrize("name", C.NAMES)
def test_host_build_equals_the_restatement_and_brute_force(hg, name, target):
    c = C.BY_NAME[name]
    for b, (pos, (want, wstats)) in enumerate(zip(c["clouds"], C.expected(c, target))):
        m, s = C.picks_of(c, b), C.start_of(c, b)
        got, stats = host_sample(hg, pos, m, s, target)
        assert np.array_equal(got, want), (name, b)
        assert np.array_equal(stats, wstats), (name, b, stats, wstats)
        assert np.array_equal(want, E.sample(pos, m, s)), (name, b)                      # restatement == brute restatement
        assert np.array_equal(got, host_brute(hg, pos, m, s)), (name, b)                 # host build == dcfpse::sample
        assert np.unique(got).size == got.size and got.min() >= 0 and got.max() < pos.shape[0]


@pytest.mark.parametrize("name", C.NAMES)
def test_stats_at_the_one_cell_target_are_brute_force(name):
    """One cell: every updating pick (finite, not the last) visits every finite point and that one cell."""
    c = C.BY_NAME[name]
    for b, (pos, (picks, stats)) in enumerate(zip(c["clouds"], C.expected(c, C.ONE_CELL))):
        finite = np.isfinite(pos).all(1)
        updating = int(finite[picks[:-1]].sum())
        assert stats.tolist() == [int(finite.sum()) * updating, updating], (name, b)


@pytest.mark.parametrize("target", (0.5, 1.0))
@pytest.mark.parametrize("name", C.NAMES)
def test_outside_the_box_the_computed_distance_is_at_least_the_bound_and_the_bound_at_least_D(name, target):
    """What the proof rests on, on sampled (pick, point outside the box) pairs: computed d2 >= bound2(R) >= D."""
    c = C.BY_NAME[name]
    rng = np.random.default_rng(7)
    for b, pos in enumerate(c["clouds"]):
        trace = []
        R.sample(pos, C.picks_of(c, b), C.start_of(c, b), target, trace=trace)
        finite = np.isfinite(pos).all(1)
        for cur, rad, D, G, inside in trace[:: max(1, len(trace) // 40)]:
            outside = np.nonzero(finite & ~inside)[0]
            if outside.size == 0:
                continue
            assert rad >= 1 or D == 0
            b2 = K.bound2(rad, G["min_h"])
            assert b2 >= D, (name, b, cur, rad)
            rows = rng.choice(outside, min(outside.size, 64), replace=False)
            assert (E.dist2(pos[rows], pos[cur]) >= b2).all(), (name, b, cur, rad)


def test_the_box_rule_prunes():
    """A sphere of 20 000 points sampled to 5 000: below one tenth of brute force's n (m - 1) updates at the default target."""
    pos, picks, stats, history = C.big_sphere()
    n, m = pos.shape[0], picks.size
    print("share of brute force's updates:", stats[0] / (n * (m - 1)), "points a pick:", stats[0] / (m - 1))
    assert 0 < stats[0] < n * (m - 1) / 10
    assert len(history) == m - 1 and np.array_equal(history[-1], stats)


def test_a_pick_index_past_the_cloud_gets_minus_one(hg):
    pos = C.normal(5, 7)
    for target in C.TARGETS:
        got, stats = host_sample(hg, pos, 10, 3, target)
        assert np.array_equal(got[:7], E.sample(pos, 7, 3)) and got[7:].tolist() == [-1, -1, -1]
        assert np.array_equal(stats, R.sample(pos, 7, 3, target)[1])
    got, stats = host_sample(hg, np.zeros((0, 3), np.float32), 3, 0, 1.0)
    assert got.tolist() == [-1, -1, -1] and stats.tolist() == [0, 0]


def test_the_md_inside_a_key(hg):
    md = np.array([-2.0, -1.0, -0.5, 0.0, 1e-45, 1e-38, 1.0, 3e38, np.inf], np.float32)
    ids = np.arange(md.size, dtype=np.int32)
    out, live = np.zeros(md.size, np.float32), np.zeros(md.size, np.int32)
    hg.hg_key_md(P(md), P(ids), md.size, P(out), P(live))
    assert np.array_equal(out.view(np.uint32), md.view(np.uint32)) and live.tolist() == (md >= 0).astype(int).tolist()


def test_fps_refuses_bad_methods_on_the_host():
    import torch
    from deltaconv_amd.geometry import fps
    from deltaconv_amd.geometry.fps import FPS_METHOD
    assert FPS_METHOD[0] in ("brute", "grid")
    with pytest.raises(ValueError, match="HIP device"):
        fps(torch.zeros(8, 3), ratio=2, method="grid")


def test_the_model_takes_an_fps_method():
    from deltaconv_amd.models.deltanet_multiscale import DeltaNetMultiscaleBase, DeltaNetMultiscaleSegmentation
    kw = dict(enc_channels=((8,), (8,)), dec_channels=(8,), ratios=(2,))
    assert DeltaNetMultiscaleBase(3, sampling="fps", **kw).fps_method is None
    assert DeltaNetMultiscaleBase(3, sampling="fps", fps_method="grid", **kw).fps_method == "grid"
    assert DeltaNetMultiscaleSegmentation(3, 4, sampling="fps", fps_method="grid", **kw).deltanet_base.fps_method == "grid"
    for cls, args in ((DeltaNetMultiscaleBase, (3,)), (DeltaNetMultiscaleSegmentation, (3, 4))):
        with pytest.raises(ValueError, match="fps_method"):
            cls(*args, sampling="fps", fps_method="cells", **kw)
