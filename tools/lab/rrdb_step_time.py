#!/usr/bin/env python
"""`--arch esrgan`: what the in-place form of the residual dense block (functional.dense_block: one concatenation buffer the convolutions
read and write in place, csrc/dense.hip between them) buys over the composed form (fork / cat / conv2d / leaky_relu, as model/rdn.py
composes its blocks), bs 48, LR 16 x 64:
  (a) one ResidualDenseBlock_5C(64, 32) alone, operator by operator -- forward, and forward + backward (the block works on the LR grid in
      both networks, so this table is the same for x2 and x4);
  (b) the whole SRTrainStep(RRDBNet(nb), image_crit="l1", channels=3) at x2 and x4 with each form (RRDBNet.set_form), recorded plans.
hipEvents around `--steps` iterations after `--warmup`; the two forms alternate `--rounds` times in one process, best, every round and the
spread printed.  The rule for functional.DENSE_DEFAULT_FORM: in place if its whole-step time is lower than the composed form's by more than
the spread (max - min over the rounds) of the composed form's own runs -- the verdict column.
    python tools/lab/rrdb_step_time.py [--bs 48] [--nb 23] [--precision x2] [--out profiles/rrdb_step_time.md]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import functional as Fh, kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import SRTrainStep  # noqa: E402
from tpgsr_amd.model import esrgan  # noqa: E402
from tpgsr_amd.utils.synthetic import synthetic_batch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--nb", type=int, default=23)
ap.add_argument("--precision", default="x2", help="arithmetic policy (the train steps default to x2)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the tables to this file")
args = ap.parse_args()
dev = "cuda"
FORMS = ("inplace", "composed")
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
    spread = max(ms["composed"]) - min(ms["composed"])
    gain = best["composed"] - best["inplace"]
    verdict = "in place" if gain > spread else "composed"
    cells = " | ".join(f"{best[k]:.3f} ({', '.join('%.3f' % t for t in ms[k])})" for k in FORMS)
    emit(f"| {head} | {cells} | {best['composed'] / best['inplace']:.3f} | {spread:.3f} | {verdict} |")
    return verdict


HEAD = "| in place | composed | composed / in place | spread of composed (ms) | lower by more than the spread |\n|---|---|---|---|---|---|"
emit(f"bs {args.bs}, LR 16 x 64, nb {args.nb}, policy {args.precision}, {args.steps} iterations after {args.warmup}, {args.rounds} alternating "
     "rounds; ms: best (rounds)")
emit()
emit("(a) ResidualDenseBlock_5C(64, 32) alone, operator by operator (weights packed per call, as everywhere in the functional layer)")
emit()
emit("| pass " + HEAD)
with K.policy(args.precision):
    g = torch.Generator().manual_seed(16)
    x = torch.randn(args.bs, 16, 64, 64, generator=g).to(dev).requires_grad_(True)
    ws = [(torch.randn(32 if k < 4 else 64, 64 + 32 * k, 3, 3, generator=g) / (3 * (64 + 32 * k) ** 0.5)).to(dev).requires_grad_(True) for k in range(5)]
    bs = [(0.1 * torch.randn(32 if k < 4 else 64, generator=g)).to(dev).requires_grad_(True) for k in range(5)]
    gy = torch.randn(args.bs, 16, 64, 64, generator=g).to(dev)

    def fwd(form):
        def fn():
            with torch.no_grad():
                Fh.dense_block(x, ws, bs, form=form)
        return fn

    def fwd_bwd(form):
        def fn():
            x.grad = None
            for t in ws + bs:
                t.grad = None
            Fh.dense_block(x, ws, bs, form=form).backward(gy)
        return fn
    row("forward", alternate({f: fwd(f) for f in FORMS}))
    row("forward + backward", alternate({f: fwd_bwd(f) for f in FORMS}))

emit()
emit(f"(b) SRTrainStep(RRDBNet(nb={args.nb}), image_crit=\"l1\", channels=3), recorded plans")
emit()
emit("| network " + HEAD)
verdicts = []
for s in (2, 4):
    lr, hr = (t.to(dev) for t in synthetic_batch(args.bs, 1, scale=s))

    def step(form):
        torch.manual_seed(0)
        net = esrgan.RRDBNet(scale_factor=s, nb=args.nb).to(dev).train()
        net.set_form(form)
        ts = SRTrainStep(net, precision=args.precision, image_crit="l1", channels=3)
        return lambda: ts.step(lr, hr)
    verdicts.append(row(f"RRDBNet x{s}, 16 x 64 -> {16 * s} x {64 * s}", alternate({f: step(f) for f in FORMS})))
    torch.cuda.empty_cache()
emit()
emit("whole-step verdicts: " + ", ".join(verdicts) + f"; functional.DENSE_DEFAULT_FORM = {Fh.DENSE_DEFAULT_FORM!r}")

if args.out:
    with open(args.out, "w") as f:
        f.write("# RRDBNet: the dense block in place against composed (tools/lab/rrdb_step_time.py)\n\n" + "\n".join(lines) + "\n")
