#!/usr/bin/env python
"""Fixtures for the PRIOR-FREE baselines (`--arch srres | rdn | vdsr`, reference model/{srresnet,rdn,vdsr}.py SRResNet / RDN / VDSR, the
`else:` branch of the train loop, interfaces/super_resolution.py:409-424) and for the prior-free evaluation pass (:770-793), generated from
the GENUINE reference's modules (imported at run time through oracle/ref_import.py; build container only).

Weights by recipe (`generic_recipe` of make_golden_next.py, seeds in `SEEDS`) and inputs by `synthetic_batch(n, seed)`: the tests rebuild
both, only results are stored.  Every stored forward result is first compared with this file's own float64 restatement of the network
(`plain_forward`, plain torch.nn.functional -- the tests import it as their float64 reference where no fixture is stored).

    python tests/golden/make_golden_plain.py      # rewrites tests/golden/plain_<name>.npz, train_plain_<name>.npz, plain_layouts.json,
                                                  # plain_eval.json"""
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

from make_golden_next import generic_recipe, grad_summary  # noqa: E402

BACKBONES = ("srres", "rdn", "vdsr")
CRIT = {"srres": "mse", "rdn": "l1", "vdsr": "mse"}              # interfaces/base.py:332-347
CHANNELS = {"srres": 4, "rdn": 3, "vdsr": 3}                      # interfaces/super_resolution.py:410-413 (srres: mask=True)
# backbone -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch)
SEEDS = {"srres": (81, 500, 510, 91), "rdn": (82, 501, 511, 92), "vdsr": (83, 502, 512, 93)}
N, N_SMALL, SMALL_HW = 4, 2, (12, 40)
# the evaluator batch (N = 6): weight seeds of srres / tsrn.TSRN / rdn / the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_SEEDS = 6, dict(srres=520, tsrn=521, rdn=522, rec=60)
EVAL_CHANNELS = dict(srres=None, tsrn=None, bicubic=None, rdn=3)      # the evaluator's channels= (rdn: the RGB prefix, HR cut alike)
EVAL_DATA_SEEDS = range(200, 264)


def build_reference(name, R):
    if name == "srres":
        return R.srresnet.SRResNet(scale_factor=2, width=128, height=32, STN=False, mask=True)
    if name == "rdn":
        return R.rdn.RDN(scale_factor=2)
    return R.vdsr.VDSR(scale_factor=2, width=128, height=32, STN=False)


def _bn(p, k, x, training):
    return F.batch_norm(x, p[k + ".running_mean"], p[k + ".running_var"], p[k + ".weight"], p[k + ".bias"], training, 0.1, 1e-5)


def _conv(p, k, x, pad):
    return F.conv2d(x, p[k + ".weight"], p.get(k + ".bias"), padding=pad)


def plain_forward(name, p, x, training):
    """the three networks restated over torch.nn.functional, in the dtype of `p` / `x` (a dict of tensors keyed like the state_dict;
    training=True updates the running statistics in `p` in place, like nn.BatchNorm2d)"""
    if name == "srres":
        b1 = F.prelu(_conv(p, "block1.0", x, 4), p["block1.1.weight"])
        b = b1
        for i in range(2, 7):
            r = F.prelu(_bn(p, f"block{i}.bn1", _conv(p, f"block{i}.conv1", b, 1), training), p[f"block{i}.prelu.weight"])
            b = b + _bn(p, f"block{i}.bn2", _conv(p, f"block{i}.conv2", r, 1), training)
        b7 = _bn(p, "block7.1", _conv(p, "block7.0", b, 1), training)
        u = F.prelu(F.pixel_shuffle(_conv(p, "block8.0.conv", b1 + b7, 1), 2), p["block8.0.prelu.weight"])
        return torch.tanh(_conv(p, "block8.1", u, 4))
    if name == "rdn":
        def rdb(k, h):
            out = h
            for j in range(6):
                out = torch.cat((out, F.relu(_conv(p, f"{k}.dense_layers.{j}.conv", out, 1))), 1)
            return _conv(p, f"{k}.conv_1x1", out, 0) + h
        f_ = _conv(p, "conv1", x, 1)
        f1 = rdb("RDB1", _conv(p, "conv2", f_, 1))
        f2 = rdb("RDB2", f1)
        f3 = rdb("RDB3", f2)
        fgf = _conv(p, "GFF_3x3", _conv(p, "GFF_1x1", torch.cat((f1, f2, f3), 1), 0), 1)
        return _conv(p, "conv3", F.pixel_shuffle(_conv(p, "conv_up", fgf + f_, 1), 2), 1)
    assert name == "vdsr"
    h = F.interpolate(x, scale_factor=2)
    out = F.relu(_conv(p, "input", h, 1))
    for j in range(6):
        out = F.relu(_conv(p, f"residual_layer.{j}.conv", out, 1)) + out
    return _conv(p, "output", out, 1) + h


def to64(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def _close(a, b, what, tol=2e-5):
    e = float((a.double() - b.double()).abs().max()) / max(1.0, float(b.double().abs().max()))
    assert e <= tol, f"{what}: reference vs float64 restatement differ by {e:.2e}"
    return e


def running_cat(sd):
    rs = [v.reshape(-1).float() for k, v in sd.items() if "running_" in k]
    return torch.cat(rs).numpy() if rs else np.zeros(1, dtype=np.float32)


def model_fixture(name, R, O):
    dseed, wseed, gseed, sseed = SEEDS[name]
    C = CHANNELS[name]
    lr = O.synthetic_batch(N, dseed)[0][:, :C].contiguous()
    lr_s = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW)[0][:, :C].contiguous()
    ref = build_reference(name, R)
    sd = generic_recipe(ref.state_dict(), wseed)
    out = {}
    # eval mode: 16x64 and the 12x40 tile-edge case
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    with torch.no_grad():
        ye, ys = ref(lr), ref(lr_s)
        _close(ye, plain_forward(name, to64(sd), lr.double(), False), f"{name} eval")
        _close(ys, plain_forward(name, to64(sd), lr_s.double(), False), f"{name} eval 12x40")
    out.update(y_eval=ye.numpy(), y_small=ys.numpy())
    # train mode: forward, every parameter gradient for a fixed upstream gradient, running buffers
    ref.load_state_dict(sd, strict=True)
    ref.train()
    y = ref(lr)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    (y * gy).sum().backward()
    p64 = to64(sd)
    for k, v in p64.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
    y64 = plain_forward(name, p64, lr.double(), True)
    _close(y.detach(), y64.detach(), f"{name} train")
    (y64 * gy.double()).sum().backward()
    gmax = max(float(q.grad.double().norm()) for q in ref.parameters())
    for k, q in ref.named_parameters():
        d = float((q.grad.double() - p64[k].grad).norm())
        # (float32 against float64 through up to 19 ReLU kinks: a pre-activation within rounding of zero flips a whole gradient element;
        #  measured 2.2e-3 for rdn's deepest dense layer, 1e-4 class elsewhere)
        assert d <= 1e-2 * max(float(p64[k].grad.norm()), 1e-3 * gmax), (name, k, d, float(p64[k].grad.norm()), gmax)
    _close(torch.tensor(running_cat(ref.state_dict())), torch.tensor(running_cat(p64)), f"{name} running buffers")
    names, norms, heads = grad_summary(ref)
    out.update(y=y.detach().numpy(), grad_names=names, grad_norms=norms, grad_heads=heads, running_cat=running_cat(ref.state_dict()),
               seeds=np.array([dseed, wseed, gseed, sseed]))
    print(f"{name}: y {tuple(y.shape)}, {len(names)} parameters, |y| max {float(y.abs().max()):.3f}")
    return out


def train_fixture(name, R, O):
    """two steps of the reference loop body (:409-424): criterion(model(lr[:, :C]), hr[:, :C]).mean() * 100, clip 0.25, Adam"""
    dseed, wseed, _, _ = SEEDS[name]
    C = CHANNELS[name]
    lr, hr = O.synthetic_batch(N, dseed)
    net = build_reference(name, R)
    net.load_state_dict(generic_recipe(net.state_dict(), wseed))
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = torch.nn.MSELoss() if CRIT[name] == "mse" else torch.nn.L1Loss()
    loss_l, gn_l = [], []
    for step in range(2):
        sr = net(lr[:, :C, ...])
        loss = crit(sr, hr[:, :C, ...]).mean() * 100
        opt.zero_grad()
        loss.backward()
        if step == 0:
            gs = grad_summary(net)
            sr0 = sr.detach().numpy()
        gn = torch.nn.utils.clip_grad_norm_(net.parameters(), 0.25)
        opt.step()
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  {name} step {step}: loss {loss.item():.6f}  clip norm {float(gn):.5f}")
    return dict(loss=np.array(loss_l), gnorm=np.array(gn_l), sr_step0=sr0, sr_grad_names=gs[0], sr_grad_norms=gs[1], sr_grad_heads=gs[2],
                seeds=np.array([dseed, wseed]))


def eval_models(R, O):
    """name -> (float32 SR function, float64 SR function) of the evaluator cases"""
    ref = build_reference("srres", R)
    sd = generic_recipe(ref.state_dict(), EVAL_SEEDS["srres"])
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    sd_t = O.recipe_state_dict(O.tsrn_spec(STN=False, mask=True), EVAL_SEEDS["tsrn"])
    ref_rdn = build_reference("rdn", R)
    sd_rdn = generic_recipe(ref_rdn.state_dict(), EVAL_SEEDS["rdn"])
    ref_rdn.load_state_dict(sd_rdn, strict=True)
    ref_rdn.eval()
    bic = R.bicubic.BICUBIC(scale_factor=2)
    return {
        "srres": (lambda lr: ref(lr), lambda lr: plain_forward("srres", to64(sd), lr.double(), False)),
        "tsrn": (lambda lr: O.tsrn_forward(O.as_params(sd_t, False), lr, training=False, stn=False),
                 lambda lr: O.tsrn_forward(O.as_params(to64(sd_t), False), lr.double(), training=False, stn=False)),
        "rdn": (lambda lr: ref_rdn(lr[:, :3, ...]), lambda lr: plain_forward("rdn", to64(sd_rdn), lr[:, :3].double(), False)),
        "bicubic": (lambda lr: bic(lr), lambda lr: F.interpolate(lr.double(), scale_factor=2, mode="bicubic", align_corners=True)),
    }


def eval_fixture(R, O):
    """the evaluator batch: the first data seed at which the recogniser's float32 and float64 arg-max agree at every time step for LR, HR
    and the SR image of every case; the expected strings = the oracle's CRNN forward + greedy decode on the reference SR image"""
    sd_r = O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"])
    r32, r64 = O.as_params(sd_r, False), O.as_params(to64(sd_r), False)
    models = eval_models(R, O)

    def logits(img, p):
        return O.crnn_forward(p, O.parse_crnn_data(img[:, :3]), training=False)

    with torch.no_grad():
        for seed in EVAL_DATA_SEEDS:
            lr, hr = O.synthetic_batch(EVAL_N, seed)
            imgs = {"lr": lr, "hr": hr}
            for k, (f32, f64) in models.items():
                sr = f32(lr)
                _close(sr, f64(lr), f"evaluator {k} SR")
                imgs["sr_" + k] = sr
            res, ok = {}, True
            for k, img in imgs.items():
                l32, l64 = logits(img, r32), logits(img.double(), r64)
                if not torch.equal(l32.argmax(-1), l64.argmax(-1)):
                    ok = False
                    break
                res[k] = O.get_string_crnn(l32)
            if not ok:
                print(f"  evaluator batch seed {seed}: float32 / float64 arg-max differ, next seed")
                continue
            out = dict(data_seed=seed, n=EVAL_N, weight_seeds=EVAL_SEEDS, strings=res, psnr={}, ssim={})
            for k in models:
                out["psnr"][k] = float(R.ssim_psnr.calculate_psnr(imgs["sr_" + k], hr))
                out["ssim"][k] = float(R.ssim_psnr.SSIM()(imgs["sr_" + k], hr))
                assert abs(out["psnr"][k] - float(O.calculate_psnr(imgs["sr_" + k].double(), hr.double()))) < 1e-4
                assert abs(out["ssim"][k] - float(O.ssim(imgs["sr_" + k], hr))) < 1e-5
            print(f"evaluator batch: data seed {seed}", res)
            return out
    raise RuntimeError("no evaluator batch with agreeing float32 / float64 arg-max among the candidate seeds")


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    from model import bicubic as r_bicubic, rdn as r_rdn, srresnet as r_srresnet, vdsr as r_vdsr      # (the reference's, on sys.path now)
    R.rdn, R.srresnet, R.vdsr, R.bicubic = r_rdn, r_srresnet, r_vdsr, r_bicubic
    torch.manual_seed(0)
    layouts = {}
    for name in BACKBONES:
        layouts[name] = [(k, list(v.shape)) for k, v in build_reference(name, R).state_dict().items()]
        np.savez_compressed(os.path.join(HERE, f"plain_{name}.npz"), **model_fixture(name, R, O))
        np.savez_compressed(os.path.join(HERE, f"train_plain_{name}.npz"), **train_fixture(name, R, O))
    json.dump(layouts, open(os.path.join(HERE, "plain_layouts.json"), "w"), indent=0)
    json.dump(eval_fixture(R, O), open(os.path.join(HERE, "plain_eval.json"), "w"), indent=1)
    print("plain_*.npz, train_plain_*.npz, plain_layouts.json, plain_eval.json written")


if __name__ == "__main__":
    main()
