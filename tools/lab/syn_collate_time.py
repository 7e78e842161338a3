#!/usr/bin/env python
"""One `--syn` batch (HR-only images -> images_hr, images_lr) two ways, ms per batch:
  A  AlignCollateSyn: one upload of the source pixels, the first resize (w // s, h // s) on the device (tpgsr_resize_ragged)
  B  what there was before it: Pillow's `image.resize((w // s, h // s), Image.BICUBIC)` per image on the host, then AlignCollate on the pairs
hipEvents around `--steps` batches after `--warmup` batches, and the wall clock around the same loop (the host's share is the point of B:
it belongs to this machine's CPUs); the two cases alternate `--rounds` times in one process (best and all rounds printed).  Also the kernel
launches, the host-to-device copies and the bytes uploaded per batch, and a bitwise comparison of the two results.
    python tools/lab/syn_collate_time.py [--bs 48] [--scale 2] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import data, kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--bs", type=int, default=48)
ap.add_argument("--scale", type=int, default=2)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
from PIL import Image  # noqa: E402

rng = np.random.default_rng(3)
s = args.scale
batch = [rng.integers(0, 256, (int(rng.integers(6, 70)), int(rng.integers(8, 260)), 3), dtype=np.uint8) for _ in range(args.bs)]
words = [f"w{i}" for i in range(args.bs)]
syn, real = data.AlignCollateSyn(down_sample_scale=s), data.AlignCollate(down_sample_scale=s)


def case_a():
    hr, lr, _, _ = syn(list(zip(batch, words)))
    return hr, lr


def case_b():
    small = [np.asarray(Image.fromarray(im).resize((im.shape[1] // s, im.shape[0] // s), Image.BICUBIC)) for im in batch]
    hr, lr, _ = real(list(zip(batch, small, words)))
    return hr, lr


def counted(fn):
    """(kernel launches, host-to-device copies, bytes uploaded) of one batch"""
    n, up, copies = [0], [0], [0]
    launch, to = K._launch, torch.Tensor.to

    def direct(name, *a):
        n[0] += 2 if name == "tpgsr_resize_ragged" else 2 + a[7]          # tpgsr_resize_normalize: horizontal, vertical [, mask]
        return launch(name, *a)

    def upload(self, *a, **kw):
        out = to(self, *a, **kw)
        if out.is_cuda and not self.is_cuda:
            up[0] += self.numel() * self.element_size()
            copies[0] += 1
        return out
    K._launch, torch.Tensor.to = direct, upload
    try:
        fn()
    finally:
        K._launch, torch.Tensor.to = launch, to
    torch.cuda.synchronize()
    return n[0], copies[0], up[0]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps, (time.perf_counter() - t0) * 1e3 / args.steps


cases = {"A AlignCollateSyn": case_a, "B Pillow per image + AlignCollate": case_b}
(hr_a, lr_a), (hr_b, lr_b) = case_a(), case_b()
assert torch.equal(hr_a, hr_b) and torch.equal(lr_a, lr_b), "the two paths differ"
for fn in cases.values():
    for _ in range(args.warmup):
        fn()
ev, wall = {k: [] for k in cases}, {k: [] for k in cases}
for _ in range(args.rounds):
    for k, fn in cases.items():
        e, w = timed(fn)
        ev[k].append(e)
        wall[k].append(w)
rows = []
print("| case | bs | s | hipEvent ms per batch (rounds) | wall ms per batch (rounds) | kernel launches | uploads | bytes uploaded |\n|---|---|---|---|---|---|---|---|")
for k, fn in cases.items():
    n, copies, up = counted(fn)
    rows.append(dict(case=k, bs=args.bs, scale=s, event_ms=ev[k], wall_ms=wall[k], launches=n, uploads=copies, bytes_uploaded=up))
    print(f"| {k} | {args.bs} | {s} | {min(ev[k]):.3f} ({', '.join('%.3f' % v for v in ev[k])}) | {min(wall[k]):.3f} "
          f"({', '.join('%.3f' % v for v in wall[k])}) | {n} | {copies} | {up} |", flush=True)
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/lab/syn_collate_time.py", device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup,
                       host_cpus=len(os.sched_getaffinity(0)), bitwise_equal=True, rows=rows), f, indent=1)
