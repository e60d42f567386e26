"""Same-process A/B of the weight-gradient kernels per shape: gemm_kernel path (switch 12 = 1) against the plane-image kernel
forced onto every whole tile (12 = 2), plain and BatchNorm-prologue forms, interleaved rounds, median / min of the per-call time
(product + ordered slab sum).  The plan rule tn_planes_faster() of csrc/gemm.hip is read off this table.

    python tools/tn_planes_ab.py [--rounds 7] [--calls 20]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deltaconv_amd._lib import lib

SHAPES = [  # (R, M, N, prologue): the C2 step's launches, then per-rank and C3..C5 ones
    (32768, 1024, 512, 0), (32768, 1024, 448, 0), (65536, 256, 256, 0), (32768, 256, 512, 1), (32768, 256, 256, 1),
    (65536, 128, 128, 0), (32768, 128, 256, 1), (32768, 128, 128, 1), (32768, 64, 256, 1), (32768, 64, 128, 1), (32768, 64, 64, 1),
    (65536, 64, 64, 0), (8192, 128, 64, 0), (8192, 256, 256, 0), (4096, 1024, 512, 0), (131072, 128, 128, 0), (32768, 64, 1024, 0), (32768, 1024, 64, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    opt = lib.raw("dc_set_option")
    dev = "cuda"
    print(f"{'R':>7} {'M':>5} {'N':>5} pro   gemm_kernel us (min)   planes us (min)   ratio")
    for r, m, n, pro in SHAPES:
        g = torch.Generator().manual_seed(r + m + n)
        a, b = torch.randn(r, m, generator=g).to(dev), torch.randn(r, n, generator=g).to(dev)
        h = torch.randn(r, m, generator=g).to(dev)
        coefs = (torch.rand(5 * m, generator=g) + 0.5).to(dev)
        c = torch.empty(m, n, device=dev)
        nb = lib.raw("dc_gemm_tn_workspace_bytes")(r, m, n)
        ws = torch.empty((nb + 3) // 4, device=dev)

        def call():
            if pro:
                lib.call("dc_linear_bn_backward_weight", a, m, h, m, coefs, 0.2, b, n, r, m, n, c, n, 0, ws, ws.numel() * 4)
            else:
                lib.call("dc_gemm_tn", a, m, b, n, r, m, n, c, n, 0, ws, ws.numel() * 4)
        times = {1: [], 2: []}
        for rnd in range(args.rounds + 1):
            for sw in (1, 2):
                opt(12, sw)
                call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    call()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[sw].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        opt(12, 0)
        t1, t2 = statistics.median(times[1]), statistics.median(times[2])
        print(f"{r:7d} {m:5d} {n:5d} {pro:3d}   {t1:8.1f} ({min(times[1]):7.1f})   {t2:8.1f} ({min(times[2]):7.1f})   {t2 / t1:.3f}")


if __name__ == "__main__":
    main()
