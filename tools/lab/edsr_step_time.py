#!/usr/bin/env python
"""`--arch edsr`: what the two switches of the network buy, each against the other form on the same commit, bs 48, LR 16 x 64:
  (a) one _Residual_Block (256 channels) alone, operator by operator -- forward, and forward + backward -- the fused form of
      functional.res_block against the composed one (the block works on the LR grid in both networks);
  (b) conv_output alone (256 -> 3 on the HR grid, forward + both gradients), the direct kernels of functional.conv2d_narrow against the
      matrix-core route, at HR 32 x 128 (x2) and 64 x 256 (x4);
  (c) the whole SRTrainStep(EDSR(s), image_crit="l1", channels=3) at x2 and x4, recorded plans: both switches off (composed, matrix), each
      on its own, both on; and the peak device memory of the step with both on.
hipEvents around `--steps` iterations after `--warmup`; the forms alternate `--rounds` times in one process, best, every round and the
spread printed.  The rule for functional.RES_DEFAULT_FORM / NARROW_DEFAULT_FORM: a form is the default only where it is faster than the
other by more than the spread (max - min over the rounds) of the other's own runs, at both factors -- the verdict column.
    python tools/lab/edsr_step_time.py [--bs 48] [--nb 32] [--precision x2] [--out profiles/edsr_step_time.md]"""
import argparse
import gc
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import functional as Fh, kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import SRTrainStep  # noqa: E402
from tpgsr_amd.model import edsr  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--nb", type=int, default=32)
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


def row(head, ms, new, base):
    """the new form against its baseline: faster by more than the baseline's own spread?"""
    spread = max(ms[base]) - min(ms[base])
    won = min(ms[base]) - min(ms[new]) > spread
    emit(f"| {head} | {cell(ms[new])} | {cell(ms[base])} | {min(ms[base]) / min(ms[new]):.3f} | {spread:.3f} | {new if won else base} |")
    return won


emit(f"bs {args.bs}, LR 16 x 64, {args.nb} residual blocks, policy {args.precision}, {args.steps} iterations after {args.warmup}, {args.rounds} "
     "alternating rounds; ms: best (rounds)")
emit()
emit("(a) _Residual_Block (256 channels) alone, operator by operator (weights packed per call, as everywhere in the functional layer)")
emit()
emit("| pass | fused | composed | composed / fused | spread of composed (ms) | lower by more than the spread |\n|---|---|---|---|---|---|")
with K.policy(args.precision):
    g = torch.Generator().manual_seed(16)
    x = torch.randn(args.bs, 16, 64, 256, generator=g).to(dev).requires_grad_(True)
    ws = [(torch.randn(256, 256, 3, 3, generator=g) / 48.0).to(dev).requires_grad_(True) for _ in range(2)]
    gy = torch.randn(args.bs, 16, 64, 256, generator=g).to(dev)

    def blk_fwd(form):
        def fn():
            with torch.no_grad():
                Fh.res_block(x, ws[0], ws[1], form=form)
        return fn

    def blk_fwd_bwd(form):
        def fn():
            x.grad = ws[0].grad = ws[1].grad = None
            Fh.res_block(x, ws[0], ws[1], form=form).backward(gy)
        return fn
    row("forward", alternate({f: blk_fwd(f) for f in Fh.RES_FORMS}), "fused", "composed")
    row("forward + backward", alternate({f: blk_fwd_bwd(f) for f in Fh.RES_FORMS}), "fused", "composed")
    del x, gy

    emit()
    emit("(b) conv_output alone, 256 -> 3, forward + data gradient + weight gradient")
    emit()
    emit("| HR grid | narrow | matrix | matrix / narrow | spread of matrix (ms) | lower by more than the spread |\n|---|---|---|---|---|---|")
    tail_won = []
    for s in (2, 4):
        xt = torch.randn(args.bs, 16 * s, 64 * s, 256, generator=g).to(dev).requires_grad_(True)
        wt = (torch.randn(3, 256, 3, 3, generator=g) / 48.0).to(dev).requires_grad_(True)
        gt = torch.randn(args.bs, 16 * s, 64 * s, 3, generator=g).to(dev)

        def tail(form):
            def fn():
                xt.grad = wt.grad = None
                Fh.conv2d_narrow(xt, wt, form=form).backward(gt)
            return fn
        tail_won.append(row(f"{16 * s} x {64 * s}", alternate({f: tail(f) for f in Fh.NARROW_FORMS}), "narrow", "matrix"))
        del xt, gt
    torch.cuda.empty_cache()

emit()
emit(f"(c) SRTrainStep(EDSR(s, n_resblocks={args.nb}), image_crit=\"l1\", channels=3), recorded plans")
emit()
CONFIGS = {"both off": ("composed", "matrix"), "block fused": ("fused", "matrix"), "tail narrow": ("composed", "narrow"), "both on": ("fused", "narrow")}
emit("| network | " + " | ".join(f"{k} ({a}, {b})" for k, (a, b) in CONFIGS.items()) + " | spread of both off (ms) | peak memory, both on (GB) |")
emit("|---|---|---|---|---|---|---|")
step_won = {"block fused": [], "tail narrow": [], "both on": []}
for s in (2, 4):
    lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1, scale=s))

    def step(cfg):
        torch.manual_seed(0)
        net = edsr.EDSR(scale_factor=s, n_resblocks=args.nb).to(dev).train()
        net.set_form(cfg[0])
        net.set_tail_form(cfg[1])
        ts = SRTrainStep(net, precision=args.precision, image_crit="l1", channels=3)
        return lambda: ts.step(lr, hr)
    # peak memory of one step object alone, before the others exist
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    fn = step(CONFIGS["both on"])
    fn()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base_mem) / 1e9
    del fn
    gc.collect()                  # (module <-> engine reference cycle)
    torch.cuda.empty_cache()
    ms = alternate({k: step(c) for k, c in CONFIGS.items()})
    spread = max(ms["both off"]) - min(ms["both off"])
    for k in step_won:
        step_won[k].append(min(ms["both off"]) - min(ms[k]) > spread)
    emit(f"| EDSR x{s}, 16 x 64 -> {16 * s} x {64 * s} | " + " | ".join(cell(ms[k]) for k in CONFIGS) + f" | {spread:.3f} | {peak:.2f} |")
    del ms
    gc.collect()
    torch.cuda.empty_cache()
emit()
emit("faster than both off by more than its spread at (x2, x4): " + ", ".join(f"{k} {tuple(v)}" for k, v in step_won.items()))
emit(f"conv_output alone, narrow faster than matrix at (32 x 128, 64 x 256): {tuple(tail_won)}")
emit(f"functional.RES_DEFAULT_FORM = {Fh.RES_DEFAULT_FORM!r}, functional.NARROW_DEFAULT_FORM = {Fh.NARROW_DEFAULT_FORM!r}")

if args.out:
    with open(args.out, "w") as f:
        f.write("# EDSR: the fused residual block and the narrow-output tail against the existing routes (tools/lab/edsr_step_time.py)\n\n"
                + "\n".join(lines) + "\n")
