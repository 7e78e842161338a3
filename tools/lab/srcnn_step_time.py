#!/usr/bin/env python
"""`--arch srcnn`: what the direct 5x5 narrow-output kernels buy for conv3, against the matrix-core route on the same commit, bs 48,
LR 16 x 64:
  (a) conv3 alone (32 -> 3 with bias on the HR grid, forward + both gradients), the direct kernels of functional.conv2d_narrow5x5
      against the matrix-core route, at HR 32 x 128 (x2) and 64 x 256 (x4);
  (b) the whole SRTrainStep(SRCNN(s), image_crit="mse", channels=3) at x2 and x4, recorded plans, under both forms of conv3.
hipEvents around `--steps` iterations after `--warmup`; the forms alternate `--rounds` times in one process, best, every round and the
spread printed.  The rule for functional.NARROW5_DEFAULT_FORM (the project's, from profiles/edsr_step_time.md): "narrow" is the default
only where it is lower than "matrix" by more than the spread (max - min over the rounds) of the matrix form's own runs, on the whole
step at both factors -- the verdict column.
    python tools/lab/srcnn_step_time.py [--bs 48] [--precision x2] [--out profiles/srcnn_step_time.md]"""
import argparse
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import functional as Fh, kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import SRTrainStep  # noqa: E402
from tpgsr_amd.model import srcnn  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--precision", default="x2", help="arithmetic policy (the train steps default to x2)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the tables to this file")
args = ap.parse_args()
dev = "cuda"
lines = []


def emit(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


def alternate(fns):
    """fns: name -> callable; -> name -> ms of every round (the candidates alternate inside a round)"""
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return ms


def cell(v):
    return f"{min(v):.3f} ({', '.join('%.3f' % t for t in v)})"


def row(head, ms):
    """the narrow form against the matrix form: lower by more than the matrix form's own spread?"""
    spread = max(ms["matrix"]) - min(ms["matrix"])
    won = min(ms["matrix"]) - min(ms["narrow"]) > spread
    emit(f"| {head} | {cell(ms['narrow'])} | {cell(ms['matrix'])} | {min(ms['matrix']) / min(ms['narrow']):.3f} | {spread:.3f} | "
         f"{'narrow' if won else 'matrix'} |")
    return won


emit(f"bs {args.bs}, LR 16 x 64, policy {args.precision}, {args.steps} iterations after {args.warmup}, {args.rounds} alternating rounds; "
     "ms: best (rounds)")
emit()
emit("(a) conv3 alone, 32 -> 3 with bias, forward + data gradient + weight and bias gradient, operator by operator (the matrix form packs "
     "its weight per call, as everywhere in the functional layer)")
emit()
emit("| HR grid | narrow | matrix | matrix / narrow | spread of matrix (ms) | lower by more than the spread |\n|---|---|---|---|---|---|")
tail_won = []
with K.policy(args.precision):
    g = torch.Generator().manual_seed(16)
    for s in (2, 4):
        xt = torch.randn(args.bs, 16 * s, 64 * s, 32, generator=g).to(dev).requires_grad_(True)
        wt = (torch.randn(3, 32, 5, 5, generator=g) / 28.0).to(dev).requires_grad_(True)
        bt = torch.randn(3, generator=g).to(dev).requires_grad_(True)
        gt = torch.randn(args.bs, 16 * s, 64 * s, 3, generator=g).to(dev)

        def tail(form):
            def fn():
                xt.grad = wt.grad = bt.grad = None
                Fh.conv2d_narrow5x5(xt, wt, bt, form=form).backward(gt)
            return fn
        tail_won.append(row(f"{16 * s} x {64 * s}", alternate({f: tail(f) for f in Fh.NARROW_FORMS})))
        del xt, gt
    torch.cuda.empty_cache()

emit()
emit("(b) SRTrainStep(SRCNN(s), image_crit=\"mse\", channels=3), recorded plans")
emit()
emit("| network | narrow | matrix | matrix / narrow | spread of matrix (ms) | lower by more than the spread |\n|---|---|---|---|---|---|")
step_won = []
for s in (2, 4):
    lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1, scale=s))

    def step(form):
        torch.manual_seed(0)
        net = srcnn.SRCNN(scale_factor=s).to(dev).train()
        net.set_tail_form(form)
        ts = SRTrainStep(net, precision=args.precision, image_crit="mse", channels=3)
        return lambda: ts.step(lr, hr)
    ms = alternate({f: step(f) for f in Fh.NARROW_FORMS})
    step_won.append(row(f"SRCNN x{s}, 16 x 64 -> {16 * s} x {64 * s}", ms))
    del ms
    gc.collect()                  # (module <-> engine reference cycle)
    torch.cuda.empty_cache()
emit()
emit(f"the whole step, narrow lower than matrix by more than its spread at (x2, x4): {tuple(step_won)}")
emit(f"conv3 alone, narrow lower than matrix by more than its spread at (32 x 128, 64 x 256): {tuple(tail_won)}")
emit(f"functional.NARROW5_DEFAULT_FORM = {Fh.NARROW5_DEFAULT_FORM!r}")

if args.out:
    with open(args.out, "w") as f:
        f.write("# SRCNN: the direct 5x5 narrow-output tail against the matrix-core route (tools/lab/srcnn_step_time.py)\n\n"
                + "\n".join(lines) + "\n")
