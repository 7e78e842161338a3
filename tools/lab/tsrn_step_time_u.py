#!/usr/bin/env python
"""One TSRNTrainStep step (TSRN, STN + mask, bs 48, 16 x 64 -> 32 x 128) at hidden_units 32 and 64 -- ms per step, hipEvents around 20 steps
after 5 warm-up steps, under the step's default arithmetic policy.
    python tools/lab/tsrn_step_time_u.py [--hidden 32 64] [--bs 48]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd.interfaces.super_resolution import TSRNTrainStep  # noqa: E402
from tpgsr_amd.model import tsrn  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", type=int, nargs="+", default=[32, 64])
ap.add_argument("--bs", type=int, default=48)
args = ap.parse_args()
dev = "cuda"
lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1))
print("| hidden_units | precision | ms per step |\n|---|---|---|")
for U in args.hidden:
    torch.manual_seed(0)
    net = tsrn.TSRN(STN=True, mask=True, hidden_units=U).to(dev).train()
    ts = TSRNTrainStep(net)
    for _ in range(5):
        ts.step(lr, hr)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        loss = ts.step(lr, hr)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    print(f"| {U} | {ts.precision} | {e0.elapsed_time(e1) / 20:.3f} |")
