"""Lane-level model (numpy) of the LDS plane image of csrc/gemm_tn_planes.hip: the byte address of every lane of every
ds_write_b128 (plane stores of the staging threads) and ds_read_b128 (MFMA fragment reads), checked against the LDS bank
rules of CDNA4 before any GPU time is spent:

  ds_write_b128: serviced in 8 groups of 8 contiguous lanes, bank = (addr / 4) % 32  (a 128-byte window of eight 16-byte slots)
  ds_read_b128:  four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32 for the upper half-wave),
                 bank = (addr / 4) % 64  (a 256-byte bank row of sixteen 16-byte slots)
  lanes of a group conflict when they touch the same bank at different addresses; equal addresses broadcast.

Image: [plane][BM columns of A, then BN columns of B][64 bytes = 32 k as bf16].  Column c of an operand lives in row
c ^ ((c >> 4) & 1), its k-octet s (k = 8 s .. 8 s + 7) in 16-byte slot s ^ ((c >> 2) & 3).  The model also replays the data
flow: what a staging thread stores for (operand, column, octet) is what the MFMA lane of that column and octet reads.

    python tools/tn_planes_layout_sim.py        # prints the worst multiplicity per access kind and tile shape
"""
import numpy as np

ROWB = 64
TILES = [(128, 128), (128, 64), (64, 128), (64, 64)]
WRITE_GROUPS = [list(range(8 * g, 8 * g + 8)) for g in range(8)]
_G = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = _G + [[l + 32 for l in g] for g in _G]


def image_offset(col_base, c, octet):
    """Byte offset inside one plane of (column c of the operand whose columns start at row col_base, k-octet)."""
    return (col_base + (c ^ ((c >> 4) & 1))) * ROWB + ((octet ^ ((c >> 2) & 3)) * 16)


def store_accesses(bm, bn):
    """One entry per ds_write_b128 instruction of a staging wave: (addresses[64], payload[64] = (operand, column, octet))."""
    pl = (bm + bn) * ROWB
    out = []
    for wave in range(4):
        if wave * 64 >= bm + bn:
            continue                                        # no staging role
        is_a = wave * 64 < bm
        bc = bm if is_a else bn
        for e in range(4):
            for plane in range(3):
                addr, what = [], []
                for lane in range(64):
                    u = wave * 64 + lane - (0 if is_a else bm)
                    cq, q = u % (bc // 4), u // (bc // 4)
                    c = 4 * cq + e
                    addr.append(plane * pl + image_offset(0 if is_a else bm, c, q))
                    what.append((plane, 0 if is_a else 1, c, q))
                out.append((np.array(addr), what))
    return out


def read_accesses(bm, bn):
    """One entry per ds_read_b128 instruction of a wave: (addresses[64], wanted[64] = (plane, operand, column, octet))."""
    pl = (bm + bn) * ROWB
    out = []
    for wave in range(4):
        for op, (w0, bc, base) in enumerate((((wave >> 1) * (bm // 2), bm, 0), ((wave & 1) * (bn // 2), bn, bm))):
            for frag in range(bc // 64):
                for ks in range(2):
                    for plane in range(3):
                        addr, want = [], []
                        for lane in range(64):
                            li, lh = lane & 31, lane >> 5
                            c = w0 + 32 * frag + li
                            addr.append(plane * pl + image_offset(base, c, 2 * ks + lh))
                            want.append((plane, op, c, 2 * ks + lh))
                        out.append((np.array(addr), want))
    return out


def multiplicity(addr, groups, banks):
    """Worst number of distinct addresses on one bank within a lane group (1 = conflict-free) for 16-byte accesses."""
    worst = 1
    for g in groups:
        per_bank = {}
        for a in {int(x) for x in addr[g]}:
            for d in range(4):
                per_bank.setdefault((a // 4 + d) % banks, set()).add(a)
        worst = max(worst, max(len(v) for v in per_bank.values()))
    return worst


def check(bm, bn):
    """-> (worst store multiplicity, worst read multiplicity); asserts the data flow."""
    stores, reads = store_accesses(bm, bn), read_accesses(bm, bn)
    image = {}
    for addr, what in stores:
        for a, w in zip(addr, what):
            assert a % 16 == 0 and 0 <= a < 3 * (bm + bn) * ROWB and int(a) not in image, "store outside the image or twice"
            image[int(a)] = w
    assert len(image) == 3 * (bm + bn) * 4, "the stores must fill every slot of the image"
    for addr, want in reads:
        for a, w in zip(addr, want):
            assert image[int(a)] == w, "a fragment read returns another column / octet"
    return (max(multiplicity(a, WRITE_GROUPS, 32) for a, _ in stores), max(multiplicity(a, READ_GROUPS, 64) for a, _ in reads))


def main():
    for bm, bn in TILES:
        ws, rd = check(bm, bn)
        print(f"tile {bm:3d} x {bn:3d}: LDS {3 * (bm + bn) * ROWB // 1024} KB  ds_write_b128 worst {ws}-way  ds_read_b128 worst {rd}-way")


if __name__ == "__main__":
    main()
