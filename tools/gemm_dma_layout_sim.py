"""Lane-level model (numpy) of the activation ring of csrc/gemm.hip (plain products over pre-split weight planes): where every
lane of every LDS-DMA piece (buffer_load_dwordx4 ... lds) puts its 16 bytes and what every lane of every fragment
ds_read_b128 fetches, checked against the LDS bank rules of CDNA4 before any GPU time is spent (same rules and lane groups as
tools/tn_planes_layout_sim.py):

  LDS-DMA piece:  one wave instruction writes 64 x 16 bytes contiguously from a wave-uniform base: lane l -> base + 16 l;
                  the SOURCE address is per lane
  ds_read_b128:   four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32 for the upper half-wave),
                  bank = (addr / 4) % 64  (a 256-byte bank row of sixteen 16-byte slots)
  lanes of a group conflict when they touch the same bank at different addresses; equal addresses broadcast.

Ring buffer: [BM rows][32 floats = eight 16-byte chunks], no padding.  Chunk position cp of row r holds global chunk
cp ^ ((r >> 1) & 7); a fragment lane that wants chunk c of row r reads position c ^ ((r >> 1) & 7).  Piece `it` of wave w
covers rows 32 it + 8 w .. + 7, lane l = row (l >> 3) of those, position l & 7.

    python tools/gemm_dma_layout_sim.py        # prints the worst read multiplicity per tile shape
"""
import numpy as np

ROWB = 128
TILES = [(128, 128), (128, 64), (64, 128), (64, 64)]
_G = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = _G + [[l + 32 for l in g] for g in _G]


def swizzle(row):
    return (row >> 1) & 7


def dma_accesses(bm, swz=swizzle):
    """One entry per LDS-DMA instruction: (LDS byte addresses[64], payload[64] = (row, global chunk), source byte offsets[64] in a
    tile stored with 128-byte rows)."""
    out = []
    for it in range(bm // 32):
        for wave in range(4):
            base = (it * 32 + wave * 8) * ROWB
            addr, what, src = [], [], []
            for lane in range(64):
                row, cp = it * 32 + wave * 8 + (lane >> 3), lane & 7
                addr.append(base + 16 * lane)
                what.append((row, cp ^ swz(row)))
                src.append(row * ROWB + (cp ^ swz(row)) * 16)
            out.append((np.array(addr), what, np.array(src)))
    return out


def read_accesses(bm, bn, swz=swizzle):
    """One entry per fragment ds_read_b128 of a wave: (addresses[64], wanted[64] = (row, chunk)).  A k-step ks reads the two
    chunks 4 ks + 2 lh and 4 ks + 2 lh + 1 of the lane's row (lh = lane half); waves sharing a wave row repeat the reads."""
    out = []
    for wave in range(4):
        wm0 = (wave >> 1) * (bm // 2)
        for i in range(bm // 64):
            for ks in range(2):
                for half in range(2):
                    addr, want = [], []
                    for lane in range(64):
                        li, lh = lane & 31, lane >> 5
                        row, c = wm0 + 32 * i + li, 4 * ks + 2 * lh + half
                        addr.append(row * ROWB + ((c ^ swz(row)) * 16))
                        want.append((row, c))
                    out.append((np.array(addr), want))
    return out


def multiplicity(addr, groups, banks=64):
    """Worst number of distinct addresses on one bank within a lane group (1 = conflict-free) for 16-byte accesses."""
    worst = 1
    for g in groups:
        per_bank = {}
        for a in {int(x) for x in addr[g]}:
            for d in range(4):
                per_bank.setdefault((a // 4 + d) % banks, set()).add(a)
        worst = max(worst, max(len(v) for v in per_bank.values()))
    return worst


def check(bm, bn, swz=swizzle):
    """-> worst read multiplicity; asserts that the pieces fill the buffer exactly once (a bijection lane -> (row, chunk)), that
    the 8 lanes of a row fetch one whole 128-byte line, and that every fragment lane reads its own row and chunk."""
    image = {}
    for addr, what, src in dma_accesses(bm, swz):
        assert np.array_equal(addr, addr[0] + 16 * np.arange(64)) and addr[0] % 1024 == 0, "a piece is 1 KiB from a wave-uniform base"
        for a, w in zip(addr, what):
            assert 0 <= a < bm * ROWB and int(a) not in image, "piece outside the buffer or on top of another"
            image[int(a)] = w
        for r8 in range(8):
            line = src[8 * r8:8 * r8 + 8]
            assert len({int(s) // ROWB for s in line}) == 1 and sorted(int(s) % ROWB for s in line) == list(range(0, ROWB, 16)), \
                "the 8 lanes of a row read one whole line"
    assert len(image) == bm * 8 and len(set(image.values())) == bm * 8, "the pieces are a bijection onto the tile"
    worst = 1
    for addr, want in read_accesses(bm, bn, swz):
        for a, w in zip(addr, want):
            assert image[int(a)] == w, "a fragment read returns another row / chunk"
        worst = max(worst, multiplicity(addr, READ_GROUPS))
    return worst


def main():
    for bm, bn in TILES:
        print(f"tile {bm:3d} x {bn:3d}: ring 3 x {bm * ROWB // 1024} KB  ds_read_b128 worst {check(bm, bn)}-way")


if __name__ == "__main__":
    main()
