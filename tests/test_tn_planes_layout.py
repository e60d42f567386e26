"""The LDS plane image of csrc/gemm_tn_planes.hip, lane by lane on the CPU (tools/tn_planes_layout_sim.py): every ds_write_b128 of
the staging threads and every ds_read_b128 of the MFMA fragments is conflict-free under the LDS bank rules for all four tile
shapes, the stores fill the image exactly once and every fragment lane reads its own column and k-octet."""
import importlib.util
import os

import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tn_planes_layout_sim.py")
_spec = importlib.util.spec_from_file_location("tn_planes_layout_sim", _PATH)
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)


@pytest.mark.parametrize("bm,bn", sim.TILES)
def test_plane_image_is_conflict_free(bm, bn):
    stores, reads = sim.check(bm, bn)
    assert stores == 1 and reads == 1


def test_the_model_sees_conflicts():
    """Negative control: without the row swap the 8 lanes of a store group share four slots of the 128-byte window; without the
    slot swizzle the 16 lanes of a read group share four slots of the bank row."""
    import numpy as np
    lanes = np.arange(64)
    plain_store = (4 * (lanes % 32)) * sim.ROWB + (lanes // 32) * 16
    assert sim.multiplicity(plain_store, sim.WRITE_GROUPS, 32) == 8
    no_row_swap = (4 * (lanes % 32)) * sim.ROWB + (((lanes // 32) ^ (lanes % 4)) * 16)
    assert sim.multiplicity(no_row_swap, sim.WRITE_GROUPS, 32) == 2
    plain_read = (lanes % 32) * sim.ROWB + (lanes // 32) * 16
    assert sim.multiplicity(plain_read, sim.READ_GROUPS, 64) == 4
