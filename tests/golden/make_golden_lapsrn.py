#!/usr/bin/env python
"""Fixtures for `--arch lapsrn` (reference model/lapsrn.py LapSRN / L1_Charbonnier_loss, constructed by interfaces/base.py:351-353 and
trained through the `else:` branch of the loop, interfaces/super_resolution.py:409-424) at scale_factor 2 and 4, generated from the
GENUINE reference's module (imported at run time through oracle/ref_import.py; build container only).

Weights by recipe (`generic_recipe` of make_golden_next.py, seeds in `SEEDS`) and inputs by `synthetic_batch(n, seed, scale=s)`: the tests
rebuild both, only results are stored.  Every stored forward result is first compared with this file's own float64 restatement of the
network (`lapsrn_forward`, plain torch.nn.functional -- the tests import it as their float64 reference where no fixture is stored).  The x4
images (64 x 256) are stored for the first `N_STORE[4]` samples of the N = 4 batch.

    python tests/golden/make_golden_lapsrn.py     # rewrites tests/golden/lapsrn_x{2,4}.npz, train_lapsrn_x{2,4}.npz, lapsrn_layouts.json"""
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

from golden_plain_arch import Recipe, eval_fixture, save_pair, to64  # noqa: E402
from golden_plain_arch import ssim64 as _ssim64  # noqa: E402
from make_golden_next import generic_recipe, grad_summary  # noqa: E402

SCALES = (2, 4)
CHANNELS = 3                                                     # `--arch lapsrn` runs without --mask: three planes
# scale -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch)
SEEDS = {2: (84, 503, 513, 94), 4: (85, 504, 514, 95)}
N, N_SMALL, SMALL_HW = 4, 2, (12, 40)
N_STORE = {2: 4, 4: 2}                                            # samples of the 16x64 batch whose SR image is stored
EPS, SLOPE = 1e-6, 0.2
# the evaluator batch (N = 6): weight seeds of the network (per scale) and of the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_SEEDS = 6, {2: 523, 4: 524, "rec": 60}
EVAL_DATA_SEEDS = range(300, 364)


def lapsrn_forward(p, x, scale):
    """the network restated over torch.nn.functional in the dtype of `p` / `x` (p: a dict of tensors keyed like the state_dict)"""
    def stage(k, h):
        for i in range(0, 20, 2):
            h = F.leaky_relu(F.conv2d(h, p[f"{k}.0.cov_block.{i}.weight"], padding=1), SLOPE)
        return F.leaky_relu(F.conv_transpose2d(h, p[f"{k}.0.cov_block.20.weight"], stride=2, padding=1), SLOPE)

    f1 = stage("convt_F1", F.leaky_relu(F.conv2d(x, p["conv_input.weight"], padding=1), SLOPE))
    hr2 = F.conv_transpose2d(x, p["convt_I1.weight"], stride=2, padding=1) + F.conv2d(f1, p["convt_R1.weight"], padding=1)
    if scale == 2:
        return hr2
    f2 = stage("convt_F2", f1)
    return F.conv_transpose2d(hr2, p["convt_I2.weight"], stride=2, padding=1) + F.conv2d(f2, p["convt_R2.weight"], padding=1)


def charbonnier(sr, hr):
    d = sr - hr
    return torch.sqrt(d * d + EPS).sum()


def ssim64(img1, img2, window_size=11):
    """golden_plain_arch.ssim64 over taps built in float64 and rounded to float32 afterwards (oracle.tpgsr_oracle.ssim keeps a float32 window)"""
    return _ssim64(img1, img2, window_size, taps=torch.float64)


def _close(a, b, what, tol=2e-5):
    e = float((a.double() - b.double()).abs().max()) / max(1.0, float(b.double().abs().max()))
    assert e <= tol, f"{what}: reference vs float64 restatement differ by {e:.2e}"
    return e


def trained_names(scale):
    """parameters the factor's forward reaches (the second stage exists at x2 too, without gradient)"""
    return lambda k: scale == 4 or not k.startswith(("convt_I2", "convt_R2", "convt_F2"))


def model_fixture(s, R, O):
    dseed, wseed, gseed, sseed = SEEDS[s]
    lr = O.synthetic_batch(N, dseed, scale=s)[0][:, :CHANNELS].contiguous()
    lr_s = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW, scale=s)[0][:, :CHANNELS].contiguous()
    ref = R.lapsrn.LapSRN(scale_factor=s, width=128, height=32, STN=False)
    sd = generic_recipe(ref.state_dict(), wseed)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    with torch.no_grad():
        ys = ref(lr_s)
        _close(ys, lapsrn_forward(to64(sd), lr_s.double(), s), f"x{s} eval 12x40")
    ref.train()
    y = ref(lr)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    (y * gy).sum().backward()
    p64 = to64(sd)
    for v in p64.values():
        v.requires_grad_(True)
    y64 = lapsrn_forward(p64, lr.double(), s)
    _close(y.detach(), y64.detach(), f"x{s} train")
    (y64 * gy.double()).sum().backward()
    live = trained_names(s)
    gmax = max(float(q.grad.double().norm()) for k, q in ref.named_parameters() if live(k))
    for k, q in ref.named_parameters():
        if not live(k):
            assert q.grad is None and p64[k].grad is None, k
            continue
        d = float((q.grad.double() - p64[k].grad).norm())
        # (float32 against float64 through up to 23 LeakyReLU kinks: a pre-activation within rounding of zero changes a whole gradient element)
        assert d <= 1e-2 * max(float(p64[k].grad.norm()), 1e-3 * gmax), (s, k, d, float(p64[k].grad.norm()), gmax)
    names, norms, heads = grad_summary(ref)
    print(f"x{s}: y {tuple(y.shape)}, {len(names)} parameters, |y| max {float(y.abs().max()):.3f}")
    out = dict(y=y.detach().numpy()[:N_STORE[s]], y_small=ys.numpy(), grad_names=names, grad_norms=norms, grad_heads=heads,
               seeds=np.array([dseed, wseed, gseed, sseed]))
    out.update(eval_fixture(RECIPE, s, R, O))
    return out


def train_fixture(s, R, O):
    """two steps of the reference loop body (:409-424): L1_Charbonnier_loss(model(lr[:, :3]), hr[:, :3]).mean() * 100, clip 0.25, Adam"""
    dseed, wseed, _, _ = SEEDS[s]
    lr, hr = O.synthetic_batch(N, dseed, scale=s)
    net = R.lapsrn.LapSRN(scale_factor=s, width=128, height=32, STN=False)
    net.load_state_dict(generic_recipe(net.state_dict(), wseed))
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = R.lapsrn.L1_Charbonnier_loss()
    loss_l, gn_l = [], []
    for step in range(2):
        sr = net(lr[:, :CHANNELS, ...])
        loss = crit(sr, hr[:, :CHANNELS, ...]).mean() * 100
        assert abs(loss.item() - 100 * charbonnier(sr.detach().double(), hr[:, :CHANNELS].double()).item()) < 1e-5 * loss.item()
        opt.zero_grad()
        loss.backward()
        if step == 0:
            gs = grad_summary(net)
            sr0 = sr.detach().numpy()[:N_STORE[s]]
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  x{s} step {step}: loss {loss.item():.6f}  clip norm {float(gn):.5f}")
    return dict(loss=np.array(loss_l), gnorm=np.array(gn_l), sr_step0=sr0, sr_grad_names=gs[0], sr_grad_norms=gs[1], sr_grad_heads=gs[2],
                seeds=np.array([dseed, wseed]))


# the evaluator batch: golden_plain_arch.eval_fixture under this file's own forward tolerance (_close) and without the metric margin
RECIPE = Recipe(build=lambda R, s, nb: R.lapsrn.LapSRN(scale_factor=s, width=128, height=32, STN=False),
                forward=lambda p, x, s, nb: lapsrn_forward(p, x, s), channels=CHANNELS, n={None: N}, n_store=N_STORE, n_small=N_SMALL,
                small_hw=SMALL_HW, eval_n=EVAL_N, eval_nb=None, eval_seeds=EVAL_SEEDS, eval_data_seeds=EVAL_DATA_SEEDS, fwd_tol=2e-5,
                metric_margin=False)


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    from model import lapsrn as r_lapsrn      # (the reference's, on sys.path now)
    R.lapsrn = r_lapsrn
    torch.manual_seed(0)
    layouts = {}
    for s in SCALES:
        net = R.lapsrn.LapSRN(scale_factor=s)
        layouts[f"x{s}"] = [(k, list(v.shape)) for k, v in net.state_dict().items()]
        tent = torch.tensor([0.25, 0.75, 0.75, 0.25])
        assert all(torch.equal(v, torch.outer(tent, tent).expand_as(v)) for k, v in net.state_dict().items() if k.startswith("convt_I") or k.endswith(".20.weight"))
        save_pair(HERE, "lapsrn", s, model_fixture(s, R, O), train_fixture(s, R, O))
    json.dump(layouts, open(os.path.join(HERE, "lapsrn_layouts.json"), "w"), indent=0)
    print("lapsrn_x*.npz, train_lapsrn_x*.npz, lapsrn_layouts.json written")


if __name__ == "__main__":
    main()
