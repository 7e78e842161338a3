#!/usr/bin/env python
"""One SRTrainStep step with a prior-free baseline (`--arch srres | rdn | vdsr`: bs 48, 16 x 64 -> 32 x 128, the backbone's own image
criterion and channel count): ms per step RECORDED (engine_functional.PlainSREngine's plans) against OPERATOR BY OPERATOR through autograd
(TPGSR_SR_RECORD=0), and the launches one step makes.  hipEvents around `--steps` steps after `--warmup` steps; the two modes alternate
`--rounds` times in one process (the spread between rounds is printed).
    python tools/lab/plain_step_time.py [--arch srres rdn] [--bs 48] [--precision x3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import SRTrainStep  # noqa: E402
from tpgsr_amd.model import rdn, srresnet, vdsr  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

MAKE = {"srres": (lambda: srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True), dict(image_crit="mse")),
        "rdn": (lambda: rdn.RDN(scale_factor=2), dict(image_crit="l1", channels=3)),
        "vdsr": (lambda: vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False), dict(image_crit="mse", channels=3))}

ap = argparse.ArgumentParser()
ap.add_argument("--arch", nargs="+", default=["srres", "rdn"], choices=sorted(MAKE))
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--precision", default="x3")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
dev = "cuda"
lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1))


def build(arch, record):
    torch.manual_seed(0)
    make, kw = MAKE[arch]
    net = make().to(dev).train()
    net._engine().record = record
    return SRTrainStep(net, precision=args.precision, **kw)


def count_launches(ts):
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
        ts.step(lr, hr)
    finally:
        K.Plan.run, K._launch = run, launch
    torch.cuda.synchronize()
    return n[0]


def timed(ts):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        loss = ts.step(lr, hr)
    e1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    return e0.elapsed_time(e1) / args.steps


print("| arch | precision | bs | mode | ms per step (rounds) | launches per step |\n|---|---|---|---|---|---|")
for arch in args.arch:
    steps = {"recorded": build(arch, True), "operator by operator": build(arch, False)}
    for ts in steps.values():
        for _ in range(args.warmup):
            ts.step(lr, hr)
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, ts in steps.items():
            ms[k].append(timed(ts))
    for k, ts in steps.items():
        print(f"| {arch} | {ts.precision} | {args.bs} | {k} | {min(ms[k]):.3f} ({', '.join('%.3f' % v for v in ms[k])}) | {count_launches(ts)} |", flush=True)
