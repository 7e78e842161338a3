#!/usr/bin/env python
"""`--arch lapsrn`: what the sub-pixel form of ConvTranspose2d(64, 64, 4, 2, 1) buys over the zero-dilated form (functional.conv_transpose2d_k4s2's
`form` argument), bs 48:
  (a) the layer alone -- forward + data gradient + weight gradient -- at 16 x 64 and 32 x 128 (the two stages of LapSRN x4);
  (b) the whole SRTrainStep(LapSRN, image_crit="l1_charbonnier", channels=3) at x2 and x4 with each form (this script hands the op the
      form for the 64 -> 64 layers while a step runs, i.e. while its plans are recorded; the product has no such switch).
hipEvents around `--steps` iterations after `--warmup`; the two forms alternate `--rounds` times in one process, best and spread printed.
    python tools/lab/lapsrn_step_time.py [--bs 48] [--precision x2] [--out profiles/lapsrn_step_time.md]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import functional as Fh, kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import SRTrainStep  # noqa: E402
from tpgsr_amd.model import lapsrn  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--precision", default="x2", help="arithmetic policy (the train steps default to x2)")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the tables to this file")
args = ap.parse_args()
dev = "cuda"
FORMS = ("subpixel", "dilated")
OP = Fh.conv_transpose2d_k4s2
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
    """fns: form -> callable; -> form -> ms of every round (the forms alternate inside a round)"""
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return ms


def row(head, ms):
    best = {k: min(v) for k, v in ms.items()}
    spread = max(max(v) - min(v) for v in ms.values())
    cells = " | ".join(f"{best[k]:.3f} ({', '.join('%.3f' % t for t in ms[k])})" for k in FORMS)
    emit(f"| {head} | {cells} | {best['dilated'] / best['subpixel']:.2f} | {spread:.3f} |")


emit(f"bs {args.bs}, policy {args.precision}, {args.steps} iterations after {args.warmup}, {args.rounds} alternating rounds; ms: best (rounds)")
emit()
emit("(a) ConvTranspose2d(64, 64, 4, 2, 1) alone: forward + data gradient + weight gradient")
emit()
emit("| input | sub-pixel | zero-dilated | dilated / sub-pixel | spread (ms) |\n|---|---|---|---|---|")
with K.policy(args.precision):
    for H, W in ((16, 64), (32, 128)):
        g = torch.Generator().manual_seed(H)
        x = torch.randn(args.bs, H, W, 64, generator=g).to(dev).requires_grad_(True)
        w = (torch.randn(64, 64, 4, 4, generator=g) / 16).to(dev).requires_grad_(True)
        gy = torch.randn(args.bs, 2 * H, 2 * W, 64, generator=g).to(dev)

        def layer(form):
            def fn():
                x.grad = w.grad = None
                Fh.conv_transpose2d_k4s2(x, w, form).backward(gy)
            return fn
        row(f"{args.bs} x {H} x {W} x 64", alternate({f: layer(f) for f in FORMS}))

emit()
emit("(b) SRTrainStep(LapSRN, image_crit=\"l1_charbonnier\", channels=3), recorded plans")
emit()
emit("| network | sub-pixel | zero-dilated | dilated / sub-pixel | spread (ms) |\n|---|---|---|---|---|")
for s in (2, 4):
    lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1, scale=s))

    def step(form):
        torch.manual_seed(0)
        net = lapsrn.LapSRN(scale_factor=s).to(dev).train()
        ts = SRTrainStep(net, precision=args.precision, image_crit="l1_charbonnier", channels=3)

        def fn():
            Fh.conv_transpose2d_k4s2 = lambda x, w, f=None: OP(x, w, form if w.shape[0] == 64 else f)
            try:
                ts.step(lr, hr)
            finally:
                Fh.conv_transpose2d_k4s2 = OP
        return fn
    row(f"LapSRN x{s}, 16 x 64 -> {16 * s} x {64 * s}", alternate({f: step(f) for f in FORMS}))

if args.out:
    with open(args.out, "w") as f:
        f.write("# LapSRN: sub-pixel against zero-dilated transposed convolution (tools/lab/lapsrn_step_time.py)\n\n" + "\n".join(lines) + "\n")
