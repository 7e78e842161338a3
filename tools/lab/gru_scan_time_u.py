#!/usr/bin/env python
"""The two BiGRU scans alone (forward over a precomputed projection, back-propagation through time) at hidden size 32 and 64 on the SR
trunk's geometry (N 48, 16 x 64), both scan axes -- us per launch, hipEvents around 30 back-to-back launches.
    python tools/lab/gru_scan_time_u.py [--hidden 32 64]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64])
args = ap.parse_args()
dev = "cuda"
N, H, W = 48, 16, 64
P = N * H * W


def timed(fn, reps=30):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


print("| hidden | kernel | axis 0 (T 64, 768 sequences) us | axis 1 (T 16, 3072 sequences) us |\n|---|---|---|---|")
for U in args.hidden:
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g).to(dev)
    gi, whh, bhh, dh = R(P, 6 * U), R(2, 3 * U, U) / U ** 0.5, R(2, 3 * U), R(P, 2 * U)
    h, gates = torch.empty(P, 2 * U, device=dev), torch.empty(P, 8 * U, device=dev)
    dgi, dgh = torch.empty(P, 6 * U, device=dev), torch.empty(P, 6 * U, device=dev)
    fwd = lambda ax: K.bigru_fwd(gi, whh, bhh, N, H, W, ax, h, gates, hidden=U)
    bwd = lambda ax: K.bigru_bwd(gates, h, dh, None, whh, N, H, W, ax, dgi, dgh, hidden=U)
    print(f"| {U} | forward scan (bigru_fwd) | {timed(lambda: fwd(0)):.1f} | {timed(lambda: fwd(1)):.1f} |")
    fwd(0)
    print(f"| {U} | back-propagation through time (bigru_bwd) | {timed(lambda: bwd(0)):.1f} | {timed(lambda: bwd(1)):.1f} |")
