"""Greedy farthest-point sampling is prefix-stable: the first m picks of an n-point sample are the m-point sample from the same
start point.  ``geodesic_subsample`` writes its rows in pick order, so the first ``ceil(n / r)`` rows of a stored cloud ARE its
coarser FPS sample -- the assumption ``geometry.prefix_levels`` and ``models.DeltaNetMultiscaleBase`` rest on.  Host library,
no GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import ROOT


@pytest.fixture(scope="module")
def fps():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "deltaconv_amd", "csrc_host")], check=True)
    from deltaconv_amd.geometry.fps import geodesic_fps
    return geodesic_fps


@pytest.mark.parametrize("points,seed", [(300, 3), (1000, 3), (2048, 11)])
def test_the_first_m_picks_are_the_m_point_sample(fps, points, seed):
    rng = np.random.default_rng(points)
    nrm = rng.standard_normal((points, 3))
    pos = nrm / np.linalg.norm(nrm, axis=1, keepdims=True) * (1 + 0.1 * rng.random((points, 1)))     # a bumpy sphere
    half = fps(pos, points // 2, seed=seed)
    assert len(set(half.tolist())) == points // 2
    for m in (points // 8, points // 4, 1):
        assert np.array_equal(half[:m], np.atleast_1d(fps(pos, m, seed=seed))), m
