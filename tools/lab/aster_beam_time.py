#!/usr/bin/env python
"""The ASTER decode two ways, ms per decode on one GPU:
  greedy  AttentionRecognitionHead.sample()                  N decoder rows
  beam    AttentionRecognitionHead.beam_search(., B, eos)    N * B decoder rows, the reference evaluator's decode (B = 5)
for the decoder alone (random encoder features) and for the whole `TextSREvaluator.recognize` ASTER pass (parse_aster_data, rectification,
encoder, decode, strings).  hipEvents around `--steps` decodes after `--warmup`; the cases alternate `--rounds` times in one process (best
and all rounds printed).  Also the C-ABI launches per decode and the bytes a B-fold copy of the encoder features and their projection
would have cost against tpgsr_aster_attention_rows, which reads one copy per image.
    python tools/lab/aster_beam_time.py [--n 48] [--len 100] [--beam 5] [--json out.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tpgsr_amd import kernels as K  # noqa: E402
from tpgsr_amd.interfaces.super_resolution import TextSREvaluator  # noqa: E402
from tpgsr_amd.model.recognizer import RecognizerBuilder  # noqa: E402
from tpgsr_amd.utils.metrics import get_vocabulary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=48)
ap.add_argument("--len", type=int, default=100)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

voc = get_vocabulary("all")
C, eos, dev = len(voc), voc.index("EOS"), "cuda"
torch.manual_seed(0)
nets = {}
for name, width in (("greedy", 0), ("beam", args.beam)):
    net = RecognizerBuilder(arch="ResNet_ASTER", rec_num_classes=C, max_len_labels=args.len, eos=eos, beam_width=width)
    if nets:
        net.load_state_dict(nets["greedy"].state_dict())
    nets[name] = net.to(dev).eval()
T, D, A = 25, 512, 512
feats = torch.randn(args.n, T, D, device=dev)
lr = torch.rand(args.n, 4, 16, 64, device=dev)
evals = {k: TextSREvaluator([], [None], recognizer=n) for k, n in nets.items()}
cases = {
    "decoder greedy": lambda: nets["greedy"].decoder.sample([feats, None, None]),
    f"decoder beam B={args.beam}": lambda: nets["beam"].decoder.beam_search(feats, args.beam, eos),
    "evaluator greedy": lambda: evals["greedy"].recognize(lr),
    f"evaluator beam B={args.beam}": lambda: evals["beam"].recognize(lr),
}


def launches(fn):
    n, launch = [0], K._launch

    def counting(name, *a):
        n[0] += 1
        return launch(name, *a)
    K._launch = counting
    try:
        fn()
    finally:
        K._launch = launch
    torch.cuda.synchronize()
    return n[0]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.steps


for fn in cases.values():
    for _ in range(args.warmup):
        fn()
ms = {k: [] for k in cases}
for _ in range(args.rounds):
    for k, fn in cases.items():
        ms[k].append(timed(fn))
rows = []
print(f"N {args.n}, L {args.len}, C {C}, T {T}, {torch.cuda.get_device_name(0)}\n")
print("| case | decoder rows | ms per decode, best (rounds) | C-ABI launches per decode |\n|---|---|---|---|")
for k, fn in cases.items():
    n = launches(fn)
    r = args.n * (args.beam if "beam" in k else 1)
    rows.append(dict(case=k, rows=r, ms=ms[k], launches=n))
    print(f"| {k} | {r} | {min(ms[k]):.3f} ({', '.join('%.3f' % v for v in ms[k])}) | {n} |", flush=True)
best = {k: min(v) for k, v in ms.items()}
kd, ke = f"decoder beam B={args.beam}", f"evaluator beam B={args.beam}"
per_image = (T * D + T * A) * 4                                # feats + xproj of one image, bytes
copy_bytes = args.n * (args.beam - 1) * per_image              # what B - 1 more copies would add to memory ...
read_bytes = args.n * args.beam * per_image * args.len         # ... and what the attention reads per decode either way (L steps, R rows)
print(f"\nbeam / greedy: decoder {best[kd] / best['decoder greedy']:.2f}x, evaluator {best[ke] / best['evaluator greedy']:.2f}x "
      f"({args.beam}x the decoder rows)")
print(f"x / xproj kept once per image: {args.n * per_image} bytes resident; a {args.beam}-fold copy would write and keep {copy_bytes} more "
      f"bytes per decode ({copy_bytes / 2 ** 20:.2f} MiB); the attention kernel reads {read_bytes / 2 ** 20:.1f} MiB per decode either way, "
      f"from {args.n} distinct row blocks instead of {args.n * args.beam}")
if args.json:
    with open(args.json, "w") as f:
        json.dump(dict(tool="tools/lab/aster_beam_time.py", device=torch.cuda.get_device_name(0), n=args.n, len=args.len, beam=args.beam,
                       steps=args.steps, warmup=args.warmup, rows=rows, copy_bytes=copy_bytes), f, indent=1)
