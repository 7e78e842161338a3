#!/usr/bin/env python
"""Fixtures for `--arch srcnn` (reference model/srcnn.py:109-145 SRCNN, constructed by interfaces/base.py:332-334 with nn.MSELoss and
trained through the `else:` branch of the loop, interfaces/super_resolution.py:409-424, on three channels) at scale_factor 2 and 4,
generated from the GENUINE reference's module (imported at run time through oracle/ref_import.py; build container only).

SRCNN has no depth argument (nb = None, as LapSRN).  Weights by recipe (`generic_recipe` of make_golden_next.py, seeds in `SEEDS`) and
inputs by `synthetic_batch(n, seed, scale=s)`: the tests rebuild both, only results are stored.  Every stored forward result is first
compared with this file's own float64 restatement of the network (`srcnn_forward`, plain torch.nn.functional -- the tests import it as
their float64 reference where no fixture is stored), and the reference's float32 run has to stay within a QUARTER of every bound
tests/test_srcnn_gpu.py applies, measured against float64 (`BOUNDS` and the skeletons of golden_plain_arch.py; the train fixture here is
golden_plain_arch.train_fixture with nn.MSELoss in place of nn.L1Loss); a seed set that does not raises OverMargin: choose another and
commit it here.  SR images are stored for the first `N_STORE[scale]` samples of a batch.

    python tests/golden/make_golden_srcnn.py     # rewrites tests/golden/srcnn_x{2,4}.npz, train_srcnn_x{2,4}.npz, srcnn_layouts.json"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from golden_plain_arch import (BOUNDS, Recipe, _p64, _quarter, _rel, _within, eval_fixture, model_fixture, save_pair, ssim64,  # noqa: E402,F401
                               to64)      # (ssim64 -- over the reference's float32-built taps -- and to64 are re-exported for the tests)
from make_golden_next import generic_recipe, grad_summary  # noqa: E402

SCALES = (2, 4)
CHANNELS = 3                                                     # `--arch srcnn` runs without --mask: three planes
# scale -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch): sets that hold the quarter margin
SEEDS = {2: (286, 705, 715, 296), 4: (287, 706, 716, 297)}
N, N_SMALL, SMALL_HW = 4, 2, (12, 40)
N_STORE = {2: 4, 4: 2}                                            # samples of the 16x64 batch whose SR image is stored
# the evaluator batch (N = 6): weight seeds of the network (per scale) and of the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_SEEDS = 6, {2: 725, 4: 726, "rec": 60}
EVAL_DATA_SEEDS = range(500, 564)


def srcnn_forward(p, x, scale, nb=None):
    """the network restated over torch.nn.functional in the dtype of `p` / `x` (p: a dict of tensors keyed like the state_dict)"""
    h = F.interpolate(x, scale_factor=scale)
    h = F.relu(F.conv2d(h, p["conv1.weight"], p["conv1.bias"], padding=4))
    h = F.relu(F.conv2d(h, p["conv2.weight"], p["conv2.bias"]))
    return F.conv2d(h, p["conv3.weight"], p["conv3.bias"], padding=2)


RECIPE = Recipe(build=lambda R, s, nb: R.srcnn.SRCNN(scale_factor=s), forward=srcnn_forward, channels=CHANNELS, n={None: N}, n_store=N_STORE,
                n_small=N_SMALL, small_hw=SMALL_HW, eval_n=EVAL_N, eval_nb=None, eval_seeds=EVAL_SEEDS, eval_data_seeds=EVAL_DATA_SEEDS)


def _bare(d):
    """golden_plain_arch prefixes its keys with the depth: a depth-less backbone stores them bare (tests/plain_arch_common.py `_pre`)"""
    return {k[len("nbNone_"):] if k.startswith("nbNone_") else k: v for k, v in d.items()}


def train_fixture(s, R, O):
    """two steps of the reference loop body (:409-424): nn.MSELoss()(model(lr[:, :3]), hr[:, :3]).mean() * 100, clip 0.25, Adam(lr 1e-3,
    betas (0.5, 0.999)) over model.parameters() -- and the same two steps in float64 over the restatement, under the quarter margin"""
    dseed, wseed, _, _ = SEEDS[s]
    C = CHANNELS
    lr, hr = O.synthetic_batch(N, dseed, scale=s)
    net = R.srcnn.SRCNN(scale_factor=s)
    sd = generic_recipe(net.state_dict(), wseed)
    net.load_state_dict(sd)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = torch.nn.MSELoss()
    p64 = _p64(sd, ())
    opt64 = torch.optim.Adam(list(p64.values()), lr=1e-3, betas=(0.5, 0.999))
    loss_l, gn_l = [], []
    for step in range(2):
        sr = net(lr[:, :C, ...])
        loss = crit(sr, hr[:, :C, ...]).mean() * 100
        opt.zero_grad()
        loss.backward()
        if step == 0:
            gs = grad_summary(net)
            sr0 = sr.detach().numpy()[:N_STORE[s]]
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        sr64 = srcnn_forward(p64, lr[:, :C].double(), s)
        loss64 = ((sr64 - hr[:, :C].double()) ** 2).mean() * 100
        opt64.zero_grad()
        loss64.backward()
        gn64 = torch.nn.utils.clip_grad_norm_(list(p64.values()), 0.25)
        opt64.step()
        _quarter(abs(loss.item() - loss64.item()) / loss64.item(), BOUNDS["loss" if step == 0 else "loss2"], f"x{s} loss, step {step}")
        if step == 0:
            _quarter(abs(float(gn) - float(gn64)) / float(gn64), BOUNDS["gnorm"], f"x{s} clip norm")
            _within(_rel(sr.detach(), sr64.detach()), RECIPE.fwd_tol, f"x{s} sr_step0")
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  x{s} step {step}: loss {loss.item():.6f} (float64 {loss64.item():.6f})  clip norm {float(gn):.5f} (float64 {float(gn64):.5f})")
    return dict(loss=np.array(loss_l), gnorm=np.array(gn_l), sr_step0=sr0, sr_grad_names=gs[0], sr_grad_norms=gs[1], sr_grad_heads=gs[2],
                seeds=np.array([dseed, wseed]))


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    torch.manual_seed(0)
    layouts = {}
    for s in SCALES:
        net = R.srcnn.SRCNN(scale_factor=s)
        layouts[f"x{s}"] = [(k, list(v.shape)) for k, v in net.state_dict().items()]
        assert sum(v.numel() for v in net.state_dict().values()) == 20099 and len(net.state_dict()) == 6
        model = _bare(model_fixture(RECIPE, None, s, SEEDS[s], R, O))      # raises OverMargin where the seed set does not hold the margin
        model.update(eval_fixture(RECIPE, s, R, O))
        save_pair(HERE, "srcnn", s, model, train_fixture(s, R, O))
    json.dump(layouts, open(os.path.join(HERE, "srcnn_layouts.json"), "w"), indent=0)
    print("srcnn_x*.npz, train_srcnn_x*.npz, srcnn_layouts.json written")


if __name__ == "__main__":
    main()
