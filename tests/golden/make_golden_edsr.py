#!/usr/bin/env python
"""Fixtures for `--arch edsr` (reference model/edsr.py EDSR, constructed by interfaces/base.py:348-350 with nn.L1Loss and trained through
the `else:` branch of the loop, interfaces/super_resolution.py:409-424) at scale_factor 2 and 4, generated from the GENUINE reference's
module (imported at run time through oracle/ref_import.py; build container only).

Two depths per factor: the reference's 32 residual blocks on N = 2 samples and 2 blocks on N = 4 (the reference has no depth argument: the
shallow network is the reference's with `net.residual` replaced by its first two blocks).  Weights by recipe (`generic_recipe` of
make_golden_next.py, seeds in `SEEDS` -- the four frozen MeanShift tensors included, as a checkpoint would set them) and inputs by
`synthetic_batch(n, seed, scale=s)`: the tests rebuild both, only results are stored (no 160 MB of weights).  Every stored forward result
is first compared with this file's own float64 restatement of the network (`edsr_forward`, plain torch.nn.functional -- the tests import it
as their float64 reference where no fixture is stored), and the reference's float32 run has to stay within a QUARTER of every bound
tests/test_edsr_gpu.py applies, measured against float64 (`BOUNDS`); a seed set that does not is replaced by the next one (every seed moved
up by 1000) and the count of sets tried is printed.  SR images are stored for the first `N_STORE[scale]` samples of a batch.

    python tests/golden/make_golden_edsr.py     # rewrites tests/golden/edsr_x{2,4}.npz, train_edsr_x{2,4}.npz, edsr_layouts.json"""
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
from make_golden_rrdb import ssim64, ssim_window  # noqa: E402,F401

SCALES = (2, 4)
DEPTHS = (32, 2)
CHANNELS = 3                                                     # `--arch edsr` runs without --mask: three planes
N = {32: 2, 2: 4}                                                # batch size per depth
# (depth, scale) -> (data seed, weight seed, upstream-gradient seed, data seed of the 12x40 batch): the first set of each that holds the
# quarter margin (main() prints how many were tried)
SEEDS = {(32, 2): (186, 605, 615, 196), (32, 4): (187, 606, 616, 197), (2, 2): (188, 607, 617, 198), (2, 4): (189, 608, 618, 199)}
N_SMALL, SMALL_HW = 1, (12, 40)
N_STORE = {2: 2, 4: 1}                                            # samples of a 16x64 batch whose SR image is stored
RES_SCALE = 0.1
FROZEN = ("sub_mean.weight", "sub_mean.bias", "add_mean.weight", "add_mean.bias")
# the bounds of tests/test_edsr_gpu.py (those of tests/test_rrdb_gpu.py for the same quantities)
BOUNDS = dict(fwd=1e-4, grad=5e-3, head=0.1, loss=3e-4, gnorm=3e-3, loss2=2e-2, dpsnr=1e-5, dssim=1e-7)
# the evaluator batch (N = 6, depth EVAL_NB): weight seeds of the network (per scale) and of the CRNN recogniser; the data seed is CHOSEN below
EVAL_N, EVAL_NB, EVAL_SEEDS = 6, 2, {2: 625, 4: 626, "rec": 60}
EVAL_DATA_SEEDS = range(400, 464)


def edsr_forward(p, x, scale, nb):
    """the network restated over torch.nn.functional in the dtype of `p` / `x` (p: a dict of tensors keyed like the state_dict)"""
    def conv(name, h):
        return F.conv2d(h, p[name + ".weight"], None, padding=1)

    out = conv("conv_input", F.conv2d(x, p["sub_mean.weight"], p["sub_mean.bias"]))
    skip = out
    for i in range(nb):
        r = conv(f"residual.{i}.conv2", F.relu(conv(f"residual.{i}.conv1", out)))
        out = r * torch.tensor(RES_SCALE, dtype=torch.float32).to(r.dtype) + out       # (`output *= 0.1`: the float32 value of 0.1)
    out = conv("conv_mid", out) + skip
    for i in range({2: 1, 4: 2}[scale]):
        out = F.pixel_shuffle(conv(f"upscale.{2 * i}", out), 2)
    return F.conv2d(conv("conv_output", out), p["add_mean.weight"], p["add_mean.bias"])


def build_reference(R, scale, nb):
    """the reference's EDSR; nb < 32: its trunk cut to the first nb blocks at run time"""
    net = R.edsr.EDSR(scale_factor=scale)
    if nb != 32:
        net.residual = torch.nn.Sequential(*list(net.residual)[:nb])
    return net


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(1.0, float(b.double().abs().max()))


class OverMargin(AssertionError):
    pass


def _quarter(err, bound, what):
    if not err <= 0.25 * bound:
        raise OverMargin(f"{what}: the reference's float32 run is {err:.2e} from float64, more than a quarter of the bound {bound:.0e}")
    return err


def _grad_errors(net32, p64):
    """the per-parameter rule of check_param_grads (tests/test_tl_cascade_gpu.py), float32 reference against float64; frozen tensors have
    no gradient on either side"""
    n64 = {k: float(v.grad.norm()) for k, v in p64.items() if v.grad is not None}
    gmax = max(n64.values())
    en = eh = 0.0
    worst = None
    for k, q in net32.named_parameters():
        if k in FROZEN:
            assert q.grad is None and p64[k].grad is None, k
            continue
        g32, g64 = q.grad.double(), p64[k].grad
        e = abs(float(g32.norm()) - n64[k]) / max(n64[k], 1e-3 * gmax)
        if e > en:
            en, worst = e, k
        sc = max(n64[k], 1e-3 * gmax) / np.sqrt(g64.numel())
        eh = max(eh, float((g32.reshape(-1)[:8] - g64.reshape(-1)[:8]).abs().max()) / sc)
    print(f"  worst parameter-gradient norm: {worst} {en:.2e} (|g| {n64[worst]:.3e}, largest {gmax:.3e})")
    return en, eh


def _p64(sd):
    p = to64(sd)
    for k, v in p.items():
        if k not in FROZEN:
            v.requires_grad_(True)
    return p


def model_fixture(nb, s, seeds, R, O):
    dseed, wseed, gseed, sseed = seeds
    n = N[nb]
    lr = O.synthetic_batch(n, dseed, scale=s)[0][:, :CHANNELS].contiguous()
    lr_s = O.synthetic_batch(N_SMALL, sseed, lr_hw=SMALL_HW, scale=s)[0][:, :CHANNELS].contiguous()
    ref = build_reference(R, s, nb)
    sd = generic_recipe(ref.state_dict(), wseed)
    ref.load_state_dict(sd, strict=True)
    assert [k for k, q in ref.named_parameters() if not q.requires_grad] == list(FROZEN)
    ref.eval()
    with torch.no_grad():
        ys = ref(lr_s)
        _quarter(_rel(ys, edsr_forward(to64(sd), lr_s.double(), s, nb)), BOUNDS["fwd"], f"nb {nb} x{s} eval 12x40")
    ref.train()
    y = ref(lr)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(gseed))
    (y * gy).sum().backward()
    p64 = _p64(sd)
    y64 = edsr_forward(p64, lr.double(), s, nb)
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


def train_fixture(nb, s, seeds, R, O):
    """two steps of the reference loop body (:409-424): nn.L1Loss()(model(lr[:, :3]), hr[:, :3]).mean() * 100, clip 0.25, Adam(lr 1e-3,
    betas (0.5, 0.999)) over model.parameters() -- and the same two steps in float64 over the restatement"""
    dseed, wseed, _, _ = seeds
    lr, hr = O.synthetic_batch(N[nb], dseed, scale=s)
    net = build_reference(R, s, nb)
    sd = generic_recipe(net.state_dict(), wseed)
    net.load_state_dict(sd)
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.5, 0.999))
    crit = torch.nn.L1Loss()
    p64 = _p64(sd)
    train64 = [v for k, v in p64.items() if k not in FROZEN]
    opt64 = torch.optim.Adam(train64, lr=1e-3, betas=(0.5, 0.999))
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
        sr64 = edsr_forward(p64, lr[:, :CHANNELS].double(), s, nb)
        loss64 = (sr64 - hr[:, :CHANNELS].double()).abs().mean() * 100
        opt64.zero_grad()
        loss64.backward()
        gn64 = torch.nn.utils.clip_grad_norm_(train64, 0.25)
        opt64.step()
        _quarter(abs(loss.item() - loss64.item()) / loss64.item(), BOUNDS["loss" if step == 0 else "loss2"], f"nb {nb} x{s} loss, step {step}")
        if step == 0:
            _quarter(abs(float(gn) - float(gn64)) / float(gn64), BOUNDS["gnorm"], f"nb {nb} x{s} clip norm")
            _quarter(_rel(sr.detach(), sr64.detach()), BOUNDS["fwd"], f"nb {nb} x{s} sr_step0")
        loss_l.append(loss.item())
        gn_l.append(float(gn))
        print(f"  nb {nb} x{s} step {step}: loss {loss.item():.6f} (float64 {loss64.item():.6f})  clip norm {float(gn):.5f} (float64 {float(gn64):.5f})")
    for k in FROZEN:                                               # torch.optim.Adam skips parameters without a gradient
        assert torch.equal(net.state_dict()[k], sd[k]), k
    pre = f"nb{nb}_"
    return {pre + "loss": np.array(loss_l), pre + "gnorm": np.array(gn_l), pre + "sr_step0": sr0, pre + "sr_grad_names": gs[0],
            pre + "sr_grad_norms": gs[1], pre + "sr_grad_heads": gs[2], pre + "seeds": np.array([dseed, wseed])}


def eval_fixture(s, R, O):
    """the evaluator batch of a factor: the first data seed at which the recogniser's float32 and float64 arg-max agree at every time step
    for LR, HR and the SR image; the expected strings = the oracle's CRNN forward + greedy decode on the reference SR image"""
    sd_r = O.recipe_state_dict(O.crnn_spec(), EVAL_SEEDS["rec"])
    r32, r64 = O.as_params(sd_r, False), O.as_params(to64(sd_r), False)
    ref = build_reference(R, s, EVAL_NB)
    sd = generic_recipe(ref.state_dict(), EVAL_SEEDS[s])
    ref.load_state_dict(sd, strict=True)
    ref.eval()

    def logits(img, p):
        return O.crnn_forward(p, O.parse_crnn_data(img[:, :3]), training=False)

    with torch.no_grad():
        for tried, seed in enumerate(EVAL_DATA_SEEDS, 1):
            lr, hr = O.synthetic_batch(EVAL_N, seed, scale=s)
            sr = ref(lr[:, :CHANNELS])
            sr64 = edsr_forward(to64(sd), lr[:, :CHANNELS].double(), s, EVAL_NB)
            _quarter(_rel(sr, sr64), BOUNDS["fwd"], f"evaluator x{s} SR")
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
            print(f"evaluator batch x{s}: data seed {seed} ({tried} tried; float32 image moves PSNR by {dp:.2e} dB, SSIM by {ds:.2e})", res)
            return dict(eval_seed=np.array(seed), eval_lr=np.array(res["lr"]), eval_hr=np.array(res["hr"]), eval_sr=np.array(res["sr"]))
    raise RuntimeError("no evaluator batch with agreeing float32 / float64 arg-max among the candidate seeds")


def fixtures_with_margin(nb, s, R, O, max_sets=8):
    """model + train fixture of the first seed set (SEEDS[(nb, s)] moved up by 1000 per attempt) that holds the quarter margin"""
    for tried in range(max_sets):
        seeds = tuple(v + 1000 * tried for v in SEEDS[(nb, s)])
        try:
            m, t = model_fixture(nb, s, seeds, R, O), train_fixture(nb, s, seeds, R, O)
        except OverMargin as e:
            print(f"  nb {nb} x{s} seed set {seeds}: {e}; next set")
            continue
        print(f"nb {nb} x{s}: seed set {seeds} holds the margin ({tried + 1} tried)")
        if tried:
            print(f"  ** SEEDS[({nb}, {s})] in this file must read {seeds} **")
        return m, t, seeds
    raise RuntimeError(f"nb {nb} x{s}: no seed set within the quarter margin among {max_sets}")


def main():
    import types
    import warnings
    warnings.filterwarnings("ignore")
    from oracle import ref_import, tpgsr_oracle as O
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    R = ref_import.load()
    from model import edsr as r_edsr      # (the reference's, on sys.path now)
    R.edsr = r_edsr
    assert torch.equal(R.ssim_psnr.create_window(11, 1)[0, 0], ssim_window()), "ssim_window() is not the reference's window"
    torch.manual_seed(0)
    layouts = {}
    moved = {}
    for s in SCALES:
        model, train = {}, {}
        for nb in DEPTHS:
            net = build_reference(R, s, nb)
            layouts[f"x{s}_nb{nb}"] = [(k, list(v.shape)) for k, v in net.state_dict().items()]
            layouts[f"x{s}_nb{nb}_frozen"] = [k for k, q in net.named_parameters() if not q.requires_grad]
            m, t, seeds = fixtures_with_margin(nb, s, R, O)
            if seeds != SEEDS[(nb, s)]:
                moved[(nb, s)] = seeds
            model.update(m)
            train.update(t)
        model.update(eval_fixture(s, R, O))
        np.savez_compressed(os.path.join(HERE, f"edsr_x{s}.npz"), **model)
        np.savez_compressed(os.path.join(HERE, f"train_edsr_x{s}.npz"), **train)
        for f in (f"edsr_x{s}.npz", f"train_edsr_x{s}.npz"):
            assert os.path.getsize(os.path.join(HERE, f)) < 700 * 1024, f
    json.dump(layouts, open(os.path.join(HERE, "edsr_layouts.json"), "w"), indent=0)
    assert not moved, f"update SEEDS to {moved} and run again: the tests rebuild weights and inputs from SEEDS"
    print("edsr_x*.npz, train_edsr_x*.npz, edsr_layouts.json written")


if __name__ == "__main__":
    main()
