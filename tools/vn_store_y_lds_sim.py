"""Lane-level model (numpy) of the LDS reads of the combined store of csrc/gemm.hip (EPI_VNSTATS with store_y): every wave
re-reads its staged WM x WN tile (row stride WN floats), a lane taking the row pair (2 rp, 2 rp + 1) and eight staged columns
with four ds_read_b128, checked against the LDS bank rule of CDNA4:

  ds_read_b128:  four 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+32 for the upper half-wave),
                 bank = (addr / 4) % 64  (a 256-byte bank row of sixteen 16-byte slots)
  lanes of a group conflict when they touch the same bank at different addresses.

`swap`: odd row pairs read the two 16-byte halves of their eight columns in the opposite order (what the kernel does).
The model also checks that the four reads of all lanes cover the wave's tile exactly once.

    python tools/vn_store_y_lds_sim.py
"""
import numpy as np

_G = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_GROUPS = _G + [[l + 32 for l in g] for g in _G]
WAVE_TILES = [(64, 64), (64, 32), (32, 64), (32, 32)]       # (WM, WN) of the 128x128, 128x64, 64x128, 64x64 tiles


def reads(wm, wn, swap):
    """One entry per ds_read_b128 instruction of a wave: byte addresses [64] inside the wave's staging area."""
    pl = wn // 8
    out = []
    for it in range(wm * wn // 16 // 64):
        idx = it * 64 + np.arange(64)
        rp, c8 = idx // pl, (idx % pl) * 8
        odd = (rp & 1) * (1 if swap else 0)
        first = (2 * rp) * wn + c8 + 4 * odd
        second = first + np.where(odd == 1, -4, 4)
        for base in (first, first + wn, second, second + wn):      # u row, v row of either half
            out.append(4 * base)
    return out


def multiplicity(addr):
    worst = 1
    for g in READ_GROUPS:
        per_bank = {}
        for a in {int(x) for x in addr[g]}:
            for d in range(4):
                per_bank.setdefault((a // 4 + d) % 64, set()).add(a)
        worst = max(worst, max(len(v) for v in per_bank.values()))
    return worst


def main():
    for wm, wn in WAVE_TILES:
        line = f"wave tile {wm} x {wn}:"
        for swap in (False, True):
            rd = reads(wm, wn, swap)
            seen = sorted(int(a) for r in rd for a in r)
            assert seen == list(range(0, 4 * wm * wn, 16)), "the reads must cover the staged tile exactly once"
            line += f"  {'halves swapped on odd row pairs' if swap else 'plain'}: worst {max(multiplicity(a) for a in rd)}-way"
        print(line)


if __name__ == "__main__":
    main()
