"""Host side of Euclidean farthest-point sampling (csrc/fps_euclid_math.h), without a GPU: a g++ build of the header
(tests/hostcheck_fps_euclid) equals the numpy restatement (tests/fps_euclid_restate.py) on every case of tests/fps_euclid_cases.py,
and the properties ``geometry.prefix_levels`` / ``fps_levels`` rest on.  Everything is an equality except the fp64 property, whose
factor 1 - 12u is derived in the header (worst ratio observed: 1.0 on every case -- the fp32 maximum was the fp64 maximum)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import fps_euclid_cases as C
from tests import fps_euclid_restate as R
from tests.helpers import ROOT

HF_DIR = os.path.join(ROOT, "tests", "hostcheck_fps_euclid")
P = lambda a: ctypes.c_void_p(a.ctypes.data)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hf():
    subprocess.run(["make", "-s", "-C", HF_DIR], check=True)
    lib = ctypes.CDLL(os.path.join(HF_DIR, "libhostcheck_fps_euclid.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.hf_max_points.argtypes, lib.hf_max_points.restype = [], i32
    lib.hf_sample.argtypes, lib.hf_sample.restype = [vp, i64, i32, i32, vp], ctypes.c_int
    lib.hf_keys.argtypes, lib.hf_keys.restype = [vp, vp, i64, vp], None
    return lib


def host_sample(hf, pos, m, start=0):
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    picks = np.full(m, -7, np.int32)
    assert hf.hf_sample(P(pos), pos.shape[0], m, start, P(picks)) == 0
    return picks.astype(np.int64)


def test_the_cap_is_declared_the_same_everywhere(hf):
    from deltaconv_amd.geometry.fps import FPS_EUCLID_MAX_POINTS
    hdr = open(os.path.join(ROOT, "include", "deltaconv_hip.h")).read()
    declared = int(re.search(r"#define DC_FPS_EUCLID_MAX_POINTS \((\d+)\)", hdr).group(1))
    assert declared == hf.hf_max_points() == FPS_EUCLID_MAX_POINTS == C.CAP and declared >= 8192


@pytest.mark.parametrize("name", C.NAMES)
def test_host_build_equals_the_restatement(hf, name):
    c = C.BY_NAME[name]
    for b, (pos, want) in enumerate(zip(c["clouds"], C.expected(c))):
        got = host_sample(hf, pos, C.picks_of(c, b), C.start_of(c, b))
        assert np.array_equal(got, want), (name, b)
        assert got[0] == C.start_of(c, b) and np.unique(got).size == got.size              # pairwise distinct
        assert got.min() >= 0 and got.max() < pos.shape[0]


def test_the_selection_key_orders_by_md_then_lowest_id(hf):
    md = np.array([-2.0, -1.0, -0.5, 0.0, 1e-45, 1e-38, 1.0, 1.0, 3e38, np.inf, np.inf], np.float32)
    ids = np.array([5, 9, 4, 3, 2, 1, 8, 7, 6, 11, 10], np.int32)
    keys = np.zeros(md.size, np.uint64)
    hf.hf_keys(P(md), P(ids), md.size, P(keys))
    want = sorted(range(md.size), key=lambda i: (float(md[i]), -int(ids[i])))
    assert list(np.argsort(keys, kind="stable")) == want and np.unique(keys).size == keys.size
    assert int(np.argmax(keys)) == 10                                                   # of the two +inf the lower id


def test_non_finite_points_come_last_in_ascending_id(hf):
    c = C.BY_NAME["nan_and_inf_rows"]
    got = host_sample(hf, c["clouds"][0], 200)
    assert got[-2:].tolist() == [17, 90] and sorted(got.tolist()) == list(range(200))
    for name in ("start_at_the_nan_row", "start_at_the_inf_row"):                       # a non-finite start lowers nothing
        c = C.BY_NAME[name]
        got = host_sample(hf, c["clouds"][0], 200, c["start"][0])
        other = 90 if c["start"][0] == 17 else 17
        assert got[0] == c["start"][0] and got[1] == 0 and got[-1] == other


def test_a_pick_index_past_the_cloud_gets_minus_one(hf):
    pos = C.normal(5, 7)
    got = host_sample(hf, pos, 10)
    assert np.array_equal(got[:7], R.sample(pos, 7)) and got[7:].tolist() == [-1, -1, -1]


@pytest.mark.parametrize("name", ["n65", "n1025", "ragged", "coincident_295_of_1000", "lattice_8x8x8", "nan_and_inf_rows",
                                  "nonzero_starts"])
def test_reordering_into_pick_order_gives_the_identity_prefix(hf, name):
    """What the model relies on: rows re-ordered so that the picks come first, in pick order, sample to 0, 1, ..., m - 1."""
    c = C.BY_NAME[name]
    for b, (pos, picks) in enumerate(zip(c["clouds"], C.expected(c))):
        rest = np.setdiff1d(np.arange(pos.shape[0]), picks)
        order = np.concatenate([picks, np.random.default_rng(b).permutation(rest)])
        got = host_sample(hf, pos[order], picks.size, 0)
        assert np.array_equal(got, np.arange(picks.size)), (name, b)


@pytest.mark.parametrize("name", ["n1025", "coincident_295_of_1000", "lattice_8x8x8", "nan_and_inf_rows", "ratio_1"])
def test_the_first_picks_of_a_sample_are_the_smaller_sample(hf, name):
    c = C.BY_NAME[name]
    pos, picks = c["clouds"][0], C.expected(c)[0]
    for m in sorted({1, 2, picks.size // 3, picks.size - 1} - {0}):
        assert np.array_equal(host_sample(hf, pos, m, C.start_of(c, 0)), picks[:m]), (name, m)


@pytest.mark.parametrize("name", C.TIE_FREE)
def test_permuting_the_rows_keeps_the_set_of_picked_points(hf, name):
    c = C.BY_NAME[name]
    pos, picks = c["clouds"][0], C.expected(c)[0]
    assert C.start_of(c, 0) == 0
    perm = np.concatenate([[0], 1 + np.random.default_rng(9).permutation(pos.shape[0] - 1)])      # row 0 stays the start
    got = host_sample(hf, pos[perm], picks.size, 0)
    assert np.array_equal(perm[got], picks)                                             # the same points, even in the same order


def fp64_ratio(pos, picks):
    """min over the picks j >= 1 of md64(pick_j) / max_i md64(i), i over the finite unpicked points (1.0 where that maximum is 0)."""
    p = pos.astype(np.float64)
    md = np.full(p.shape[0], np.inf)
    taken = np.zeros(p.shape[0], bool)
    worst = 1.0
    for j in range(1, picks.size):
        c = picks[j - 1]
        taken[c] = True
        d = p - p[c]
        md = np.minimum(md, (d * d).sum(1))
        top = md[~taken].max()
        assert md[picks[j]] >= (1 - 12 * U) * top, (j, md[picks[j]], top)
        if top > 0:
            worst = min(worst, md[picks[j]] / top)
    return worst


def test_every_pick_is_within_the_fp64_bound_of_the_farthest_point(hf):
    worst = {}
    for c in C.CASES:
        if not all(np.isfinite(pos).all() for pos in c["clouds"]):
            continue
        for b, pos in enumerate(c["clouds"]):
            picks = host_sample(hf, pos, C.picks_of(c, b), C.start_of(c, b))
            worst[(c["name"], b)] = fp64_ratio(pos, picks)
    print("worst md64(pick) / max md64:", min(worst.values()), min(worst, key=worst.get))
    assert min(worst.values()) >= 1 - 12 * U


def info_of(sizes):
    from deltaconv_amd.geometry.graph import PtrInfo
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    return PtrInfo(ptr, len(sizes), int(max(sizes)), int(min(sizes)))


@pytest.mark.parametrize("sizes", [(512, 512, 512, 512), (1, 65, 1025, 300, 2049), (130,), (7, 7, 8)])
@pytest.mark.parametrize("ratios", [(4, 2), (3,), (1, 3, 4)])
def test_the_output_sizes_are_those_of_prefix_levels(sizes, ratios):
    """The host half of ``fps_levels == prefix_levels`` in ptr and info: the offsets ``fps`` derives for a ratio are the offsets of
    the prefix hierarchy, level by level (the rows need the device: tests/test_gpu_fps_euclid.py)."""
    from deltaconv_amd.geometry import prefix_levels
    from deltaconv_amd.geometry.fps import coarse_offsets, coarse_sizes
    levels = prefix_levels(info_of(sizes), ratios)
    assert len(levels) == len(ratios) + 1
    for (_, fptr, finfo), (rows, cptr, cinfo), r in zip(levels[:-1], levels[1:], ratios):
        optr, total = coarse_offsets(fptr, len(sizes), r, finfo[2], finfo.min_cloud)
        assert optr.dtype == torch.int64 and torch.equal(optr, cptr) and total == rows.numel() == int(cptr[-1])
        assert coarse_sizes(r, finfo[2], finfo.min_cloud) == (cinfo[2], cinfo.min_cloud)


def test_fps_refuses_what_the_host_can_see():
    from deltaconv_amd.geometry import fps
    with pytest.raises(ValueError, match="HIP device"):
        fps(torch.zeros(8, 3), ratio=2)
    with pytest.raises(ValueError, match="HIP device"):
        fps(np.zeros((8, 3), np.float32), ratio=2)


def test_the_model_refuses_an_unknown_sampling():
    from deltaconv_amd.models.deltanet_multiscale import DeltaNetMultiscaleBase, DeltaNetMultiscaleSegmentation
    kw = dict(enc_channels=((8,), (8,)), dec_channels=(8,), ratios=(2,))
    assert DeltaNetMultiscaleBase(3, **kw).sampling == "prefix" and DeltaNetMultiscaleBase(3, sampling="fps", **kw).sampling == "fps"
    assert DeltaNetMultiscaleSegmentation(3, 4, sampling="fps", **kw).deltanet_base.sampling == "fps"
    for cls, args in ((DeltaNetMultiscaleBase, (3,)), (DeltaNetMultiscaleSegmentation, (3, 4))):
        with pytest.raises(ValueError, match="sampling"):
            cls(*args, sampling="random", **kw)
