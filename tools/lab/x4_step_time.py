#!/usr/bin/env python
"""One C3 step (TPGSRTrainStep: TSRN_TL + CRNN teacher + student, stu_iter 1, STN, LR 16 x 64) at scale_factor 4 (SR 64 x 256, two
up-sampling stages) next to the same step at scale_factor 2 (SR 32 x 128): ms per step and the launches one step makes, per arithmetic
policy.  hipEvents around `--steps` steps after `--warmup` steps; the two scales alternate `--rounds` times in one process (best of the
rounds, all rounds printed: their spread is the noise of the number).
    python tools/lab/x4_step_time.py [--bs 48] [--precision x2 x3] [--out profiles/x4_step_time.md]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import TPGSRTrainStep  # noqa: E402
from tpgsr_amd.model import tsrn  # noqa: E402
from tpgsr_amd.model.crnn import crnn  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--precision", nargs="+", default=["x2", "x3"])
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
args = ap.parse_args()
dev = "cuda"
SCALES = (2, 4)
data = {s: tuple(t.to(dev) for t in synthetic_batch(args.bs, 1, scale=s)) for s in SCALES}


def build(scale, precision):
    torch.manual_seed(0)
    net = tsrn.TSRN_TL(scale_factor=scale, width=64 * scale, height=16 * scale, STN=True, mask=True).to(dev).train()
    stu, teacher = crnn.CRNN(32, 1, 37, 256).to(dev).train(), crnn.CRNN(32, 1, 37, 256).to(dev).eval()
    return TPGSRTrainStep([net], [stu], teacher, stu_iter=1, precision=precision)


def count_launches(ts, scale):
    """launches of one step: every op of every plan replayed + every launch made outside a plan"""
    n = [0]
    run, launch = K.Plan.run, K._launch

    def plan_run(self):
        n[0] += sum(1 for op in self.ops if op[1] is not None)
        return run(self)

    def direct(name, *a):
        if K._REC is None:
            n[0] += 1
        return launch(name, *a)
    K.Plan.run, K._launch = plan_run, direct
    try:
        ts.step(*data[scale])
    finally:
        K.Plan.run, K._launch = run, launch
    torch.cuda.synchronize()
    return n[0]


def timed(ts, scale):
    lr, hr = data[scale]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        loss = ts.step(lr, hr)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    return e0.elapsed_time(e1) / args.steps


lines = ["| step | precision | bs | scale | SR grid | ms per step: best (rounds) | launches per step | x4 / x2 |", "|---|---|---|---|---|---|---|---|"]
for precision in args.precision:
    steps = {s: build(s, precision) for s in SCALES}
    for s, ts in steps.items():
        for _ in range(args.warmup):
            ts.step(*data[s])
    torch.cuda.synchronize()
    ms = {s: [] for s in SCALES}
    for _ in range(args.rounds):
        for s, ts in steps.items():
            ms[s].append(timed(ts, s))
    for s, ts in steps.items():
        ratio = f"{min(ms[4]) / min(ms[2]):.2f}" if s == 4 else ""
        lines.append(f"| C3 | {ts.precision} | {args.bs} | x{s} | {16 * s} x {64 * s} | {min(ms[s]):.3f} ({', '.join('%.3f' % v for v in ms[s])}) | "
                     f"{count_launches(ts, s)} | {ratio} |")
    del steps
print("\n".join(lines), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
