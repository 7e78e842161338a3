#!/usr/bin/env python
"""Fixtures for `--arch esrgan` (reference model/esrgan.py RRDBNet, constructed by interfaces/base.py:342-344 with nn.L1Loss and trained
through the `else:` branch of the loop, interfaces/super_resolution.py:409-424) at scale_factor 2 and 4, generated from the GENUINE
reference's module (imported at run time through oracle/ref_import.py; build container only).

Two depths per factor: nb = 23 (the default trunk) on N = 2 samples and nb = 2 on N = 4.  Weights by recipe (`generic_recipe` of
make_golden_next.py, seeds in `SEEDS`) and inputs by `synthetic_batch(n, seed, scale=s)`: the tests rebuild both, only results are stored.
Every stored forward result is first compared with this file's own float64 restatement of the network (`rrdb_forward`, plain
torch.nn.functional -- the tests import it as their float64 reference where no fixture is stored), and the reference's float32 run has to
stay within a QUARTER of every bound tests/test_rrdb_gpu.py applies, measured against float64 (`BOUNDS`).  SR images are stored for the
first `N_STORE[scale]` samples of a batch.

    python tests/golden/make_golden_rrdb.py     # rewrites tests/golden/rrdb_x{2,4}.npz, train_rrdb_x{2,4}.npz, rrdb_layouts.json"""
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

from make_golden_lapsrn import to64  # noqa: E402,F401  (re-exported for the tests)
from make_golden_next import generic_recipe, grad_summary  # noqa: E402


def ssim_window():
    """the 11 x 11 taps as the reference builds them (utils/ssim_psnr.py:18-27 gaussian / create_window): the Gaussian from Python floats into
    a float32 tensor, normalised and multiplied out IN FLOAT32.  They sum to 1 - 6.9e-8; taps built in float64 and rounded afterwards sum to
    1 - 6.2e-9, and on these batches that alone moves the mean SSIM by 1.1e-7 (x2) / 2.1e-8 (x4): main() asserts the taps against the
    reference's own"""
    import math
    g = torch.Tensor([math.exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float()


def ssim64(img1, img2):
    """utils/ssim_psnr.py SSIM(window_size=11, size_average=True) in the dtype of its inputs over the reference's float32 taps"""
    a, b = img1[:, :3], img2[:, :3]
    ch = a.shape[1]
    w = ssim_window().to(a.dtype).expand(ch, 1, 11, 11).contiguous()
    mu1, mu2 = F.conv2d(a, w, padding=5, groups=ch), F.conv2d(b, w, padding=5, groups=ch)
    s11 = F.conv2d(a * a, w, padding=5, groups=ch) - mu1 * mu1
    s22 = F.conv2d(b * b, w, padding=5, groups=ch) - mu2 * mu2
    s12 = F.conv2d(a * b, w, padding=5, groups=ch) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))).mean()

SCALES = (2, 4)
DEPTHS = (23, 2)
CHANNELS = 3                                                     # `--arch esrgan` runs without --mask: three planes
N = {23: 2, 2: 4}                                                # batch size per depth
# (nb, scale) -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch).  (2, 2): the first set tried, (88, 507, 517,
# 98), puts a pre-activation within float32 rounding of a LeakyReLU kink -- the reference's own float32 gradient of one weight is then 1.9e-3
# from float64, over a quarter of the 5e-3 bound -- so the next set is used; the assertions below hold every set to the quarter margin
SEEDS = {(23, 2): (86, 505, 515, 96), (23, 4): (87, 506, 516, 97), (2, 2): (98, 517, 527, 108), (2, 4): (89, 508, 518, 99)}
N_SMALL, SMALL_HW = 1, (12, 40)
N_STORE = {2: 2, 4: 1}                                            # samples of a 16x64 batch whose SR image is stored
SLOPE, RES_SCALE = 0.2, 0.2
# the bounds of tests/test_rrdb_gpu.py (those of tests/test_lapsrn_gpu.py for the same quantities)
BOUNDS = dict(fwd=1e-4, grad=5e-3, head=0.1, loss=3e-4, gnorm=3e-3, loss2=2e-2, dpsnr=1e-5, dssim=1e-7)
# the evaluator batch (N = 6, nb = EVAL_NB): weight seeds of the network (per scale) and of the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_NB, EVAL_SEEDS = 6, 2, {2: 525, 4: 526, "rec": 60}
EVAL_DATA_SEEDS = range(300, 364)


def rrdb_forward(p, x, scale, nb):
    """the network restated over torch.nn.functional in the dtype of `p` / `x` (p: a dict of tensors keyed like the state_dict)"""
    def conv(name, h):
        return F.conv2d(h, p[name + ".weight"], p[name + ".bias"], padding=1)

    def rdb(name, h):
        feats = [h]
        for k in range(1, 5):
            feats.append(F.leaky_relu(conv(f"{name}.conv{k}", torch.cat(feats, 1)), SLOPE))
        return conv(f"{name}.conv5", torch.cat(feats, 1)) * RES_SCALE + h

    fea = conv("conv_first", x)
    h = fea
    for i in range(nb):
        o = h
        for j in (1, 2, 3):
            o = rdb(f"RRDB_trunk.{i}.RDB{j}", o)
        h = o * RES_SCALE + h
    fea = fea + conv("trunk_conv", h)
    for i in range({2: 1, 4: 2}[scale]):
        fea = F.leaky_relu(conv(f"upconv{i + 1}", F.interpolate(fea, scale_factor=2, mode="nearest")), SLOPE)
    return conv("conv_last", F.leaky_relu(conv("HRconv", fea), SLOPE))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(1.0, float(b.double().abs().max()))


def _quarter(err, bound, what):
    assert err <= 0.25 * bound, f"{what}: the reference's float32 run is {err:.2e} from float64, more than a quarter of the bound {bound:.0e}"
    return err


def _grad_errors(net32, p64):
    """the per-parameter rule of check_param_grads (tests/test_tl_cascade_gpu.py), float32 reference against float64"""
    n64 = {k: float(v.grad.norm()) for k, v in p64.items()}
    gmax = max(n64.values())
    en = eh = 0.0
    worst = None
    for k, q in net32.named_parameters():
        g32, g64 = q.grad.double(), p64[k].grad
        e = abs(float(g32.norm()) - n64[k]) / max(n64[k], 1e-3 * gmax)
        if e > en:
            en, worst = e, k
        sc = max(n64[k], 1e-3 * gmax) / np.sqrt(g64.numel())
        eh = max(eh, float((g32.reshape(-1)[:8] - g64.reshape(-1)[:8]).abs().max()) / sc)
    print(f"  worst parameter-gradient norm: {worst} {en:.2e} (|g| {n64[worst]:.3e}, largest {gmax:.3e})")
    return en, eh


def model_fixture(nb, s, R, O):
    dseed, wseed, gseed, sseed = SEEDS[(nb, s)]
    n = N[nb]
    lr = O.synthetic_batch(n, dseed, scale=s)[0][:, :CHANNELS].contiguous()
    lr_s = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW, scale=s)[0][:, :CHANNELS].contiguous()
    ref = R.esrgan.RRDBNet(scale_factor=s, nb=nb)
    sd = generic_recipe(ref.state_dict(), wseed)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    with torch.no_grad():
        ys = ref(lr_s)
        _quarter(_rel(ys, rrdb_forward(to64(sd), lr_s.double(), s, nb)), BOUNDS["fwd"], f"nb {nb} x{s} eval 12x40")
    ref.train()
    y = ref(lr)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    (y * gy).sum().backward()
    p64 = to64(sd)
    for v in p64.values():
        v.requires_grad_(True)
    y64 = rrdb_forward(p64, lr.double(), s, nb)
    e = _quarter(_rel(y.detach(), y64.detach()), BOUNDS["fwd"], f"nb {nb} x{s} train")
    (y64 * gy.double()).sum().backward()
    en, eh = _grad_errors(ref, p64)
    _quarter(en, BOUNDS["grad"], f"nb {nb} x{s} parameter-gradient norms")
    _quarter(eh, BOUNDS["head"], f"nb {nb} x{s} parameter-gradient heads")
    names, norms, heads = grad_summary(ref)
    print(f"nb {nb} x{s}: y {tuple(y.shape)}, {len(names)} parameters, |y| max {float(y.abs().max()):.3f}; float32 against float64: forward "
          f"{e:.2e}, gradient norms {en:.2e}, heads {eh:.2e}")
    pre = f"nb{nb}_"
    return {pre + "y": y.detach().numpy()[:N_STORE[s]], pre + "y_small": ys.numpy(), pre + "grad_names": names, pre + "grad_norms": norms,
            pre + "grad_heads": heads, pre + "seeds": np.array([dseed, wseed, gseed, sseed])}


def train_fixture(nb, s, R, O):
    """two steps of the reference loop body (:409-424): nn.L1Loss()(model(lr[:, :3]), hr[:, :3]).mean() * 100, clip 0.25, Adam(lr 1e-3,
    betas (0.5, 0.999)) -- and the same two steps in float64 over the restatement"""
    dseed, wseed, _, _ = SEEDS[(nb, s)]
    lr, hr = O.synthetic_batch(N[nb], dseed, scale=s)
    net = R.esrgan.RRDBNet(scale_factor=s, nb=nb)
    sd = generic_recipe(net.state_dict(), wseed)
    net.load_state_dict(sd)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = torch.nn.L1Loss()
    p64 = {k: v.requires_grad_(True) for k, v in to64(sd).items()}
    opt64 = torch.optim.Adam(list(p64.values()), lr=1e-3, betas=(0.5, 0.999))
    loss_l, gn_l = [], []
    for step in range(2):
        sr = net(lr[:, :CHANNELS, ...])
        loss = crit(sr, hr[:, :CHANNELS, ...]).mean() * 100
        opt.zero_grad()
        loss.backward()
        if step == 0:
            gs = grad_summary(net)
            sr0 = sr.detach().numpy()[:N_STORE[s]]
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        sr64 = rrdb_forward(p64, lr[:, :CHANNELS].double(), s, nb)
        loss64 = (sr64 - hr[:, :CHANNELS].double()).abs().mean() * 100
        opt64.zero_grad()
        loss64.backward()
        gn64 = torch.nn.utils.clip_grad_norm_(list(p64.values()), 0.25)
        opt64.step()
        _quarter(abs(loss.item() - loss64.item()) / loss64.item(), BOUNDS["loss" if step == 0 else "loss2"], f"nb {nb} x{s} loss, step {step}")
        if step == 0:
            _quarter(abs(float(gn) - float(gn64)) / float(gn64), BOUNDS["gnorm"], f"nb {nb} x{s} clip norm")
            _quarter(_rel(sr.detach(), sr64.detach()), BOUNDS["fwd"], f"nb {nb} x{s} sr_step0")
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  nb {nb} x{s} step {step}: loss {loss.item():.6f} (float64 {loss64.item():.6f})  clip norm {float(gn):.5f} (float64 {float(gn64):.5f})")
    pre = f"nb{nb}_"
    return {pre + "loss": np.array(loss_l), pre + "gnorm": np.array(gn_l), pre + "sr_step0": sr0, pre + "sr_grad_names": gs[0],
            pre + "sr_grad_norms": gs[1], pre + "sr_grad_heads": gs[2], pre + "seeds": np.array([dseed, wseed])}


def eval_fixture(s, R, O):
    """the evaluator batch of a factor: the first data seed at which the recogniser's float32 and float64 arg-max agree at every time step
    for LR, HR and the SR image; the expected strings = the oracle's CRNN forward + greedy decode on the reference SR image"""
    sd_r = O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"])
    r32, r64 = O.as_params(sd_r, False), O.as_params(to64(sd_r), False)
    ref = R.esrgan.RRDBNet(scale_factor=s, nb=EVAL_NB)
    sd = generic_recipe(ref.state_dict(), EVAL_SEEDS[s])
    ref.load_state_dict(sd, strict=True)
    ref.eval()

    def logits(img, p):
        return O.crnn_forward(p, O.parse_crnn_data(img[:, :3]), training=False)

    with torch.no_grad():
        for seed in EVAL_DATA_SEEDS:
            lr, hr = O.synthetic_batch(EVAL_N, seed, scale=s)
            sr = ref(lr[:, :CHANNELS])
            sr64 = rrdb_forward(to64(sd), lr[:, :CHANNELS].double(), s, EVAL_NB)
            _quarter(_rel(sr, sr64), BOUNDS["fwd"], f"evaluator x{s} SR")
            # the metrics of the reference's float32 image against those of the float64 image, both computed in float64: a batch on which
            # the reference's own rounding uses up more than a quarter of the evaluator test's metric bounds is no fixture for them
            hr64 = hr[:, :CHANNELS].double()
            dp = abs(float(O.calculate_psnr(sr.double(), hr64)) - float(O.calculate_psnr(sr64, hr64)))
            ds = abs(float(ssim64(sr.double(), hr64)) - float(ssim64(sr64, hr64)))
            if dp > 0.25 * BOUNDS["dpsnr"] or ds > 0.25 * BOUNDS["dssim"]:
                print(f"  evaluator batch x{s} seed {seed}: the float32 reference image moves PSNR by {dp:.2e} dB, SSIM by {ds:.2e}, next seed")
                continue
            res, ok = {}, True
            for k, img in (("lr", lr), ("hr", hr), ("sr", sr)):
                l32, l64 = logits(img, r32), logits(img.double(), r64)
                if not torch.equal(l32.argmax(-1), l64.argmax(-1)):
                    ok = False
                    break
                res[k] = O.get_string_crnn(l32)
            if not ok:
                print(f"  evaluator batch x{s} seed {seed}: float32 / float64 arg-max differ, next seed")
                continue
            print(f"evaluator batch x{s}: data seed {seed}", res)
            return dict(eval_seed=np.array(seed), eval_lr=np.array(res["lr"]), eval_hr=np.array(res["hr"]), eval_sr=np.array(res["sr"]))
    raise RuntimeError("no evaluator batch with agreeing float32 / float64 arg-max among the candidate seeds")


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    from model import esrgan as r_esrgan      # (the reference's, on sys.path now)
    R.esrgan = r_esrgan
    assert torch.equal(R.ssim_psnr.create_window(11, 1)[0, 0], ssim_window()), "ssim_window() is not the reference's window"
    torch.manual_seed(0)
    layouts = {}
    for s in SCALES:
        model, train = {}, {}
        for nb in DEPTHS:
            net = R.esrgan.RRDBNet(scale_factor=s, nb=nb)
            layouts[f"x{s}_nb{nb}"] = [(k, list(v.shape)) for k, v in net.state_dict().items()]
            model.update(model_fixture(nb, s, R, O))
            train.update(train_fixture(nb, s, R, O))
        model.update(eval_fixture(s, R, O))
        np.savez_compressed(os.path.join(HERE, f"rrdb_x{s}.npz"), **model)
        np.savez_compressed(os.path.join(HERE, f"train_rrdb_x{s}.npz"), **train)
        for f in (f"rrdb_x{s}.npz", f"train_rrdb_x{s}.npz"):
            assert os.path.getsize(os.path.join(HERE, f)) < 700 * 1024, f
    json.dump(layouts, open(os.path.join(HERE, "rrdb_layouts.json"), "w"), indent=0)
    print("rrdb_x*.npz, train_rrdb_x*.npz, rrdb_layouts.json written")


if __name__ == "__main__":
    main()
