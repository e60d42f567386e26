"""The activation ring of csrc/gemm.hip's LDS-DMA loop, lane by lane on the CPU (tools/gemm_dma_layout_sim.py): the DMA lanes
map one-to-one onto the (row, chunk) slots of a ring buffer for 64- and 128-row tiles, every row is fetched as one whole
128-byte line, every fragment lane reads its own row and chunk, and every fragment ds_read_b128 (all four tile shapes, both
k-steps, both lane halves, both chunks of a k-step) is conflict-free under the LDS bank rules."""
import importlib.util
import os

import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gemm_dma_layout_sim.py")
_spec = importlib.util.spec_from_file_location("gemm_dma_layout_sim", _PATH)
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)


@pytest.mark.parametrize("bm,bn", sim.TILES)
def test_ring_reads_are_conflict_free(bm, bn):
    assert sim.check(bm, bn) == 1
    assert len(sim.read_accesses(bm, bn)) == 4 * (bm // 64) * 2 * 2        # waves x fragments x k-steps x chunks of a lane


@pytest.mark.parametrize("bm", [64, 128])
def test_dma_lanes_are_a_bijection_onto_the_tile(bm):
    slots, payload = set(), set()
    pieces = sim.dma_accesses(bm)
    assert len(pieces) == bm // 8                                           # 1 KiB = 8 rows each
    for addr, what, _ in pieces:
        slots.update(int(a) for a in addr)
        payload.update(what)
    assert slots == set(range(0, bm * sim.ROWB, 16))
    assert payload == {(r, c) for r in range(bm) for c in range(8)}


def test_the_model_sees_conflicts():
    """Negative controls: unswizzled rows put the 16 lanes of a read group on two slots (8-way), and the plain swizzle by
    r & 7 leaves rows r and r + 8 on one slot (2-way).  Both still pass the data-flow checks: only the banks differ."""
    assert sim.check(128, 128, swz=lambda r: 0) == 8
    assert sim.check(128, 128, swz=lambda r: r & 7) == 2
